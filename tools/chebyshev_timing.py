#!/usr/bin/env python3
"""What the ChebyshevSmoother buys on one MI355X against the stock Richardson(PatchSolver, 10, 0.2), everything in one process, vectors
resident in HBM.

  config3   3-D Poisson Q2 at --cells per direction (default 128), --levels GMG levels (default 5), vertex-star patches on every
            level, FGMRES(5) to rtol 1e-6 on the Dirichlet-lift rhs -- the solver bench.py builds for its config-3 leg -- with
            Richardson(patch, 10, 0.2) and with Chebyshev(patch, d), d = 3, 4, 5, default interval: outer iterations, ms per solve,
            seconds of numerical_setup with the estimate and (d = 4, lambda_max given) without it
  sweep     level 0 of the same hierarchy: ms of one smoothing pass (gmg_smooth) divided by its patch sweeps, per variant -- a
            Chebyshev sweep is a Richardson patch sweep plus one more vector read and write (d)
  stokes    (--stokes-cells, default 256; 0 skips) the velocity GMG of config 5 -- vector Q2 + grad-div (alpha = 1e3), vertex-star patch
            smoothers, patch-corrected prolongation, maxiter 4 -- as the preconditioner of FGMRES(5) on the velocity block alone, rtol
            1e-6, random rhs: iterations and ms per solve for the same variants

The variants alternate inside every round; one warm-up round, then --reps rounds (default 5), each solve between two device
synchronisations; medians, minima and maxima are kept.

    python tools/chebyshev_timing.py [--cells 128] [--levels 5] [--stokes-cells 256] [--stokes-levels 5] [--reps 5]
                                     [--out profiles/chebyshev_timing.md]
Prints one JSON object and writes the table file."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEGREES = (3, 4, 5)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--stokes-cells", type=int, default=256)
    ap.add_argument("--stokes-levels", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chebyshev_timing.md"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    if not torch.cuda.is_available():
        sys.exit("chebyshev_timing.py measures on the GPU: no device visible")
    pkg = entry.import_package()
    S, po = pkg.solvers, pkg.poisson

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def alternate(fns):
        """{name: fn} -> {name: stats of ms}: one warm-up round, then a.reps rounds with the variants in turn"""
        ms = {k: [] for k in fns}
        for rep in range(a.reps + 1):
            for k, fn in fns.items():
                t = timed(fn)
                if rep:
                    ms[k].append(t)
        return {k: _stats(v) for k, v in ms.items()}

    def variants(patch_solvers, given):
        """name -> (smoothers per level, patch sweeps per pass); given: the lambda_max of the variant that runs no estimate"""
        out = {"richardson_10": ([S.RichardsonSmoother(M, 10, 0.2) for M in patch_solvers], 10)}
        for d in DEGREES:
            out["chebyshev_%d" % d] = ([S.ChebyshevSmoother(M, d) for M in patch_solvers], d)
        out["chebyshev_4_given"] = ([S.ChebyshevSmoother(M, 4, lambda_max=given) for M in patch_solvers], 4)
        return out

    out = dict(reps=a.reps)
    # ---------------------------------------------------------------- config 3
    nc, nlev, order = (a.cells,) * 3, a.levels, 2
    H = po.build_hierarchy(nc, nlev, order, stream_min_rows=1000000)
    Ms = [S.PatchSolver(*po.vertex_star_patches(H["ncells"][l], order)) for l in range(nlev - 1)]
    bd = torch.from_numpy(po.dirichlet_lift_rhs(nc, order)).cuda()
    xd = torch.zeros_like(bd)
    c3 = dict(cells=a.cells, levels=nlev, dofs=[int(M.shape[0]) for M in H["mats"]], setup_s={}, lambda_est={}, iters={}, sweeps_per_pass={})
    handles, solves, passes = {}, {}, {}
    n0 = int(H["mats"][0].shape[0])
    rs = torch.from_numpy(np.random.default_rng(0).uniform(-1.0, 1.0, n0)).cuda()
    xs, rw = torch.zeros_like(rs), torch.zeros_like(rs)
    for name, (sm, sweeps) in variants(Ms, 8.8).items():
        gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1)
        solver = S.FGMRESSolver(5, gmg, maxiter=20, atol=1e-14, rtol=1e-6)
        t0 = time.perf_counter()
        ns = S.numerical_setup(S.symbolic_setup(solver, H["mats"][0]), H["mats"][0])
        torch.cuda.synchronize()
        c3["setup_s"][name] = time.perf_counter() - t0
        c3["sweeps_per_pass"][name] = sweeps
        if name.startswith("chebyshev"):
            c3["lambda_est"][name] = [ns.P_ns.chebyshev_info(l)["lambda_est"] for l in range(nlev - 1)]
        handles[name] = (ns, solver)

        def solve(ns=ns):
            xd.zero_()
            S.solve_(xd, ns, bd)

        def one_pass(ns=ns):
            xs.zero_(); rw.copy_(rs)
            ns.P_ns.smooth(0, xs, rw)

        solves[name], passes[name] = solve, one_pass
    c3["solve_ms"] = alternate(solves)
    for name, (ns, solver) in handles.items():
        c3["iters"][name] = int(solver.log.num_iters)
    c3["pass_ms"] = alternate(passes)
    c3["copy_ms"] = alternate(dict(copy=lambda: (xs.zero_(), rw.copy_(rs))))["copy"]      # what one_pass spends outside the library
    c3["sweep_us"] = {k: 1e3 * (v["median"] - c3["copy_ms"]["median"]) / c3["sweeps_per_pass"][k] for k, v in c3["pass_ms"].items()}
    c3["signature_level0"] = {k: ns.P_ns.sweep_signature(0) for k, (ns, _s) in handles.items()}
    for ns, _s in handles.values():
        ns.P_ns.close()
    out["config3"] = c3
    # ---------------------------------------------------------------- the velocity GMG of config 5
    if a.stokes_cells > 0:
        st = importlib.import_module(pkg.__name__ + ".stokes")
        n, nl, alpha = a.stokes_cells, a.stokes_levels, 1.0e3
        fast = n >= 8 and not (n & (n - 1))
        Hv = st.velocity_hierarchy_fast(n, nl, alpha) if fast else st.velocity_hierarchy(n, nl, alpha)
        Ms = [S.PatchSolver(pp, pd) for pp, pd in Hv["star_patches"]]
        nv = int(Hv["mats"][0].shape[0])
        bv = torch.from_numpy(po.random_rhs(nv)).cuda()
        xv = torch.zeros_like(bv)
        c5 = dict(cells=n, levels=nl, dofs=[int(M.shape[0]) for M in Hv["mats"]], setup_s={}, lambda_est={}, iters={})
        handles, solves = {}, {}
        for name, (sm, _sweeps) in variants(Ms, 4.4).items():
            interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
                      for l in range(nl - 1)]
            gmg = S.GMGLinearSolver(Hv["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm,
                                    coarsest_solver=S.LUSolver(), maxiter=4, mode="preconditioner")
            solver = S.FGMRESSolver(5, gmg, maxiter=50, atol=1e-14, rtol=1e-6)
            t0 = time.perf_counter()
            ns = S.numerical_setup(S.symbolic_setup(solver, Hv["mats"][0]), Hv["mats"][0])
            torch.cuda.synchronize()
            c5["setup_s"][name] = time.perf_counter() - t0
            if name.startswith("chebyshev"):
                c5["lambda_est"][name] = [ns.P_ns.chebyshev_info(l)["lambda_est"] for l in range(nl - 1)]
            handles[name] = (ns, solver)

            def solve(ns=ns):
                xv.zero_()
                S.solve_(xv, ns, bv)

            solves[name] = solve
        c5["solve_ms"] = alternate(solves)
        for name, (ns, solver) in handles.items():
            c5["iters"][name] = int(solver.log.num_iters)
            ns.P_ns.close()
        out["stokes_velocity"] = c5
    # ---------------------------------------------------------------- the table file
    lines = ["# ChebyshevSmoother against Richardson(PatchSolver, 10, 0.2) on one MI355X", "",
             "Written by `tools/chebyshev_timing.py`; medians of %d alternating rounds after one warm-up round (min .. max in brackets)." % a.reps, ""]

    def table(title, c, with_sweeps):
        lines.extend(["## " + title, "", "dofs per level: %s" % c["dofs"], "",
                      "| smoother (pre = post) | outer iterations | ms per solve | setup s |" + (" ms per pass (level 0) | us per patch sweep |" if with_sweeps else ""),
                      "|---|---|---|---|" + ("---|---|" if with_sweeps else "")])
        for k, v in c["solve_ms"].items():
            row = "| %s | %d | %.2f (%.2f .. %.2f) | %.2f |" % (k, c["iters"][k], v["median"], v["min"], v["max"], c["setup_s"][k])
            if with_sweeps:
                row += " %.3f | %.1f |" % (c["pass_ms"][k]["median"], c["sweep_us"][k])
            lines.append(row)
        lines.extend(["", "lambda_est per level: %s" % json.dumps(c["lambda_est"]), ""])

    table("config 3: Q2 %d^3, %d levels, FGMRES(5), rtol 1e-6" % (a.cells, nlev), c3, True)
    lines.extend(["`chebyshev_4_given` passes lambda_max = 8.8 (4.4 on the 2-D velocity block): its setup runs no power iteration.  A pass is one gmg_smooth call on level 0 "
                  "(x = 0, a copy of r: %.3f ms, subtracted before the division by the sweeps).  Level-0 signatures: %s" %
                  (c3["copy_ms"]["median"], json.dumps(c3["signature_level0"])), ""])
    if "stokes_velocity" in out:
        c5 = out["stokes_velocity"]
        table("velocity GMG of config 5: Stokes %d^2, %d levels, GMG(maxiter 4) inside FGMRES(5), rtol 1e-6, random rhs" % (c5["cells"], c5["levels"]), c5, False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
