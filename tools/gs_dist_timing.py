#!/usr/bin/env python3
"""What the Gauss-Seidel smoother costs on a partitioned hierarchy, on one MI355X: 3-D Poisson Q1 at --cells per direction (default
64), --levels GMG levels (default 4), SymGaussSeidelSmoother(1) in the multicolour order pre = post, one process.

  distributed   the partition of --ranks ranks (default 8) folded onto the one GPU (partition.fold_ranks), every halo exchange and
                all-reduce through RCCL (transport rccl_loopback): rank-block sweeps on the partitioned levels
  single        the same global problem on a handle without a communicator: global sweeps (the path that existed before)
  vcycle / cg   median ms of one V-cycle (the GMG as a preconditioner) and of one CG solve (rtol 1e-6, maxiter 30), the two
                handles ALTERNATING call by call, with minimum and maximum; the iteration counts differ by construction
  pack_ab       option gs_pack_fused 0 against 1 on level 0 of the distributed handle, alternating: one symmetric pass
                (gmg_smooth on device vectors, two directions) between two device synchronisations, per direction = half of it.
                Two configurations in which the pass makes an update launch at all: multicolour at omega = 1.2, natural at omega = 1
                (multicolour at omega = 1 folds the update into gs_wide_kernel: the option has nothing to switch there)

    python tools/gs_dist_timing.py [--cells 64] [--levels 4] [--ranks 8] [--reps 20] [--out profiles/gs_dist_timing.json]
Prints one JSON object."""
import argparse
import ctypes as C
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
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--transport", default="rccl_loopback")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    pkg = entry.import_package()
    import importlib
    S, po, abi = pkg.solvers, pkg.poisson, pkg.abi
    pa, mg = (importlib.import_module(pkg.__name__ + "." + m) for m in ("partition", "multigpu"))
    nc, nlev, W = (a.cells,) * 3, a.levels, a.ranks
    grid = pa.rank_grid(W, 3)
    t0 = time.perf_counter()
    F = pa.fold_ranks([pa.build_local_hierarchy(nc, nlev, grid, r, 1, None, None, None, "jacobi") for r in range(W)])
    H = po.build_hierarchy(nc, nlev, 1)
    t_host = time.perf_counter() - t0
    if not torch.cuda.is_available():
        sys.exit("gs_dist_timing.py measures on the GPU: no device visible (the hierarchies were built in %.1f s)" % t_host)
    A = H["mats"][0]
    b = po.dirichlet_lift_rhs(nc, 1)
    gid = F["levels"][0].own_gid

    def sync_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def alternating(fns):
        for f in fns.values():
            f()                                               # warm-up: code objects, work vectors
        t = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, f in fns.items():
                t[k].append(sync_ms(f))
        return {k: _stats(v) for k, v in t.items()}

    sym = lambda ordering="multicolor", omega=1.0: S.SymGaussSeidelSmoother(1, omega, ordering)
    out = dict(cells=a.cells, levels=nlev, ranks=W, transport=a.transport, reps=a.reps, dofs=[int(M.shape[0]) for M in H["mats"]])
    # ---- the two handles
    gd = mg.DistributedGMG(nc, nlev, 0, 2, device_id=0, transport=a.transport, local_hierarchy=F, cells_global=nc, smoother=sym())
    gmg1 = lambda: S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=[sym()] * (nlev - 1),
                                     post_smoothers=[sym()] * (nlev - 1), maxiter=1, mode="preconditioner")
    ns1 = S.numerical_setup(S.symbolic_setup(gmg1(), A), A)
    cg1 = S.CGSolver(gmg1(), maxiter=30, atol=1e-14, rtol=1e-6)
    ks1 = S.numerical_setup(S.symbolic_setup(cg1, A), A)
    out["schedule"] = dict(distributed=[dict(level=l, forward=gd.gs_schedule(l, True), ncolors=gd.gs_ordering(l)["ncolors"]) for l in range(nlev - 1)],
                           single=[dict(level=l, forward=ns1.gs_schedule(l, True), ncolors=ns1.gs_ordering(l)["ncolors"]) for l in range(nlev - 1)])
    out["halo_level0"] = gd.halo_info(0)
    bd, b1 = torch.from_numpy(np.ascontiguousarray(b[gid])).cuda(), torch.from_numpy(b).cuda()
    xd, x1 = torch.zeros_like(bd), torch.zeros_like(b1)
    out["vcycle_ms"] = alternating(dict(distributed=lambda: gd.apply(bd, xd), single=lambda: S.solve_(x1, ns1, b1)))
    logs = {}

    def cg_d():
        xd.zero_()
        logs["d"] = gd.cg_solve(bd, xd, maxiter=30, atol=1e-14, rtol=1e-6)

    def cg_1():
        x1.zero_()
        S.solve_(x1, ks1, b1)

    out["cg_ms"] = alternating(dict(distributed=cg_d, single=cg_1))
    out["cg_iters"] = dict(distributed=int(logs["d"].num_iters), single=int(cg1.log.num_iters))
    xs = x1.cpu().numpy()
    out["cg_solutions_rel_diff"] = float(np.linalg.norm(xd.cpu().numpy() - xs[gid]) / np.linalg.norm(xs))
    out["vcycle_ms_per_cg_iteration"] = {k: out["cg_ms"][k]["median"] / out["cg_iters"][k] for k in ("distributed", "single")}
    gd.close(); ns1.close(); ks1.P_ns.close()
    # ---- gs_pack_fused 0 against 1
    out["pack_ab"] = {}
    n0 = F["levels"][0].n_own
    rng = np.random.default_rng(0)
    for name, ordering, omega in (("multicolor_omega_1.2", "multicolor", 1.2), ("natural_omega_1", "natural", 1.0)):
        g = mg.DistributedGMG(nc, nlev, 0, 2, device_id=0, transport=a.transport, local_hierarchy=F, cells_global=nc, smoother=sym(ordering, omega))
        r0 = torch.from_numpy(rng.uniform(-1.0, 1.0, n0)).cuda()
        res = {}

        def one_pass(fused):
            abi.check(g.h, g._lib.gmg_set_option(g.h, b"gs_pack_fused", float(fused)))
            x, r = torch.zeros_like(r0), r0.clone()
            ms = sync_ms(lambda: abi.check(g.h, g._lib.gmg_smooth(g.h, 0, abi.PRE, C.c_void_p(x.data_ptr()), C.c_void_p(r.data_ptr()), abi.MEM_DEVICE)))
            res[fused] = (x, r)
            return ms

        t = {1: [], 0: []}
        for rep in range(a.reps + 1):                         # (the first round is the warm-up)
            for fused in (1, 0):
                ms = one_pass(fused)
                if rep:
                    t[fused].append(ms)
        same = bool(torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]))
        out["pack_ab"][name] = dict(pass_ms={"gs_pack_fused_%d" % k: _stats(v) for k, v in t.items()},
                                    per_direction_ms={"gs_pack_fused_%d" % k: float(np.median(v)) / 2 for k, v in t.items()},
                                    same_bits=same, pack_fused_level=bool(g.halo_info(0)["pack_fused"]), schedule=g.gs_schedule(0, True))
        g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
