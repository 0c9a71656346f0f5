#!/usr/bin/env python3
"""What the device Gauss-Seidel smoother costs on one MI355X: 3-D Poisson Q1 at --cells per direction (default 128), --levels GMG
levels (default 4), everything in one process, b and x resident in HBM.

  setup        seconds of numerical_setup with Richardson(Jacobi, 10, 2/3) pre = post (the headline configuration) and with
               SymGaussSeidelSmoother(1) pre = post (level sets + triangle tables of both directions on every smoothed level)
  schedule     sets, largest set, launches and one-set launches per level and direction (gmg_get_gs_schedule)
  forward      per level: median ms of one application of GaussSeidelSmoother(1, 1.0, :forward) as a preconditioner
               (gmg_precond_apply = ldiv!: copy of r, the triangular solve, x = dx, r -= A dx) and of one y = A x of the same level;
               their difference estimates the triangular solve alone (the copy and the update are two element-wise launches)
  vcycle / cg  median ms of one V-cycle (the GMG as a preconditioner, maxiter = 1) and of one CG solve (rtol 1e-6, maxiter 20, rhs
               of u = x1 + x2), with iteration counts, for both smoother choices

  --ordering   the visiting order of every Gauss-Seidel smoother above: natural (default) or multicolor (gmg_set_gs_ordering)
  --ab         (with --ordering multicolor) the kernel A/B on level 0: one forward triangular solve + x update through gs_wide_kernel
               (option gs_wide = 1) and through gs_sets_kernel (gs_wide = 0) on the same tables, alternating, timed by the library's
               HIP events around exactly those launches (gmg_profile_enable / gmg_get_kernel_stats) and by the host clock around
               the whole pass; at omega = 0.9 both forms make the update launch (the kernels alone), at omega = 1 the new one folds it

Every figure: one warm-up call, then --reps calls each between two device synchronisations; median, minimum and maximum are kept.

    python tools/gs_timing.py [--cells 128] [--levels 4] [--reps 10] [--ordering natural] [--ab] [--out profiles/gs_timing.json]
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ordering", choices=("natural", "multicolor"), default="natural")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    if not torch.cuda.is_available():
        sys.exit("gs_timing.py measures on the GPU: no device visible")
    pkg = entry.import_package()
    S, po, abi = pkg.solvers, pkg.poisson, pkg.abi
    nc, nlev = (a.cells,) * 3, a.levels
    H = po.build_hierarchy(nc, nlev, 1)
    A = H["mats"][0]
    bd = torch.from_numpy(po.dirichlet_lift_rhs(nc, 1)).cuda()
    xd = torch.zeros_like(bd)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def runs(fn):
        fn()                                                  # warm-up: code objects, work vectors
        return _stats([timed(fn) for _ in range(a.reps)])

    def gmg(sm, **kw):
        return S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=[sm] * (nlev - 1),
                                 post_smoothers=[sm] * (nlev - 1), maxiter=1, mode="preconditioner", **kw)

    smoothers = dict(jacobi_10_10=lambda: S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0),
                     sym_gauss_seidel_1=lambda: S.SymGaussSeidelSmoother(1, 1.0, a.ordering))
    out = dict(ordering=a.ordering, cells=a.cells, levels=nlev, dofs=[int(M.shape[0]) for M in H["mats"]], reps=a.reps, setup_s={}, vcycle_ms={}, cg={})
    for name, make in smoothers.items():
        g = gmg(make())
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(g, A), A)
        torch.cuda.synchronize()
        out["setup_s"][name] = time.perf_counter() - t0
        out.setdefault("device_bytes", {})[name] = ns.device_bytes()
        if name == "sym_gauss_seidel_1":
            out["schedule"] = [dict(level=l, forward=ns.gs_schedule(l, True), backward=ns.gs_schedule(l, False),
                                    ncolors=ns.gs_ordering(l)["ncolors"]) for l in range(nlev - 1)]

        def vcycle():
            S.solve_(xd, ns, bd)

        out["vcycle_ms"][name] = runs(vcycle)
        ns.close()
        solver = S.CGSolver(gmg(make()), maxiter=20, atol=1e-14, rtol=1e-6)
        ks = S.numerical_setup(S.symbolic_setup(solver, A), A)

        def cg():
            xd.zero_()
            S.solve_(xd, ks, bd)

        out["cg"][name] = dict(ms=runs(cg), iters=int(solver.log.num_iters), flag=int(solver.log.flag))
        ks.P_ns.close()
    # one forward pass per level, next to one mat-vec of the level
    ns = S.numerical_setup(S.symbolic_setup(gmg(S.GaussSeidelSmoother(1, 1.0, "forward", a.ordering)), A), A)
    out["forward"] = []
    for l in range(nlev - 1):
        n = ns.sizes[l]
        r = torch.from_numpy(np.random.default_rng(l).uniform(-1.0, 1.0, n)).cuda()
        dx, y = torch.zeros_like(r), torch.zeros_like(r)
        p = runs(lambda: ns.precond(l, r, dx))
        m = runs(lambda: ns.op_apply(l, abi.OP_A, r, y))
        out["forward"].append(dict(level=l, rows=n, pass_ms=p, matvec_ms=m, triangular_solve_ms_estimate=p["median"] - m["median"],
                                   launches=ns.gs_schedule(l, True)["nlaunches"]))
    ns.close()
    if a.ab:
        out["ab_level0"] = {}
        for omega in (0.9, 1.0):
            ns = S.numerical_setup(S.symbolic_setup(gmg(S.GaussSeidelSmoother(1, omega, "forward", a.ordering)), A), A)
            n = ns.sizes[0]
            r = torch.from_numpy(np.random.default_rng(0).uniform(-1.0, 1.0, n)).cuda()
            dx = torch.zeros_like(r)
            ev, wall, launches = {1: [], 0: []}, {1: [], 0: []}, {}
            for rep in range(a.reps + 1):                     # (the first round is the warm-up)
                for wide in (1, 0):
                    ns.set_option("gs_wide", wide)
                    ns.profile(0)
                    w = timed(lambda: ns.precond(0, r, dx))
                    st = ns.kernel_stats()
                    ns.profile(0, False)
                    launches[wide] = st["launches"]
                    if rep:
                        ev[wide].append(st["total_ms"]); wall[wide].append(w)
            out["ab_level0"]["omega_%g" % omega] = {name: dict(solve_and_update_event_ms=_stats(ev[wide]), pass_wall_ms=_stats(wall[wide]),
                                                               launches=launches[wide])
                                                    for name, wide in (("gs_wide_kernel", 1), ("gs_sets_kernel", 0))}
            ns.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
