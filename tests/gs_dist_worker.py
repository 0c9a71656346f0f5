"""Worker of tests/test_gpu_gs_true_ranks.py: TWO true ranks as threads of this process (tests/thread_ranks.py, host transport), each
with a handle of its own on the one GPU, CG + GMG with SymGaussSeidelSmoother(1) pre = post on the structured Poisson hierarchy.

    python tests/gs_dist_worker.py OUT.npz CXxCYx.. NLEV ORDERING REP_FROM SUB_FROM SUB_RANKS [OPTIONS as JSON]      (0 = not set)

Writes per rank r: x_r (the rank's owned part of the CG solution), hist_r, iters_r, for every level l the global ids the rank owns
(gid_l_r; empty where it holds nothing of the level), and sx_r / sr_r: one symmetric pass (niter 2, omega 1.2) of level 0's smoother
through gmg_smooth on the owned part of two seeded global vectors."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

WORLD = 2
SMOOTH = (2, 1.2)                                            # niter, omega of the level-0 pass


def seeded(n):
    rng = np.random.default_rng(5)
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


def main():
    import thread_ranks
    out, cells, nlev, ordering = sys.argv[1], tuple(int(c) for c in sys.argv[2].split("x")), int(sys.argv[3]), sys.argv[4]
    rep, sub_from, sub_ranks = (int(a) or None for a in sys.argv[5:8])
    options = __import__("json").loads(sys.argv[8]) if len(sys.argv) > 8 else None
    results = {}

    def body(rank):
        import importlib
        import torch
        pkg = entry.import_package()
        pa, mg = (importlib.import_module(pkg.__name__ + "." + m) for m in ("partition", "multigpu"))
        S, po, abi = pkg.solvers, pkg.poisson, pkg.abi
        grid = pa.rank_grid(WORLD, len(cells))
        per_rank = tuple(c // g for c, g in zip(cells, grid))
        torch.cuda.set_device(0)
        g = mg.DistributedGMG(per_rank, nlev, rank, WORLD, device_id=0, transport="host", group=None, rep_from=rep,
                              smoother=S.SymGaussSeidelSmoother(1, 1.0, ordering), sub_from=sub_from, sub_ranks=sub_ranks, options=options)
        lv = g.local["levels"]
        gid = lv[0].own_gid
        b = po.dirichlet_lift_rhs(cells, 1)[gid]
        x = np.zeros(g.n_own)
        log = g.cg_solve(b, x, maxiter=100, atol=1e-14, rtol=1e-8)
        res = dict(x=x, hist=np.asarray(log.residuals[: log.num_iters + 1]), iters=np.int64(log.num_iters))
        for l, L in enumerate(lv):
            res["gid_%d" % l] = np.zeros(0, dtype=np.int64) if L is None else np.asarray(L.own_gid, dtype=np.int64)
        # one pass of level 0 with another niter / omega: every rank resets its smoother and sets up again (a collective)
        abi.check(g.h, g._lib.gmg_set_smoother_gauss_seidel(g.h, 0, abi.PRE_AND_POST, SMOOTH[0], SMOOTH[1], abi.GS_SYMMETRIC))
        abi.check(g.h, g._lib.gmg_setup(g.h))
        x0, r0 = seeded(int(np.prod([c - 1 for c in cells])))
        sx, sr = np.ascontiguousarray(x0[gid]), np.ascontiguousarray(r0[gid])
        abi.check(g.h, g._lib.gmg_smooth(g.h, 0, abi.PRE, C.c_void_p(sx.ctypes.data), C.c_void_p(sr.ctypes.data), abi.MEM_HOST))
        res.update(sx=sx, sr=sr)
        g.close()
        results[rank] = res

    thread_ranks.run(WORLD, body)
    np.savez(out, **{"%s_%d" % (k, r): v for r, res in results.items() for k, v in res.items()})


if __name__ == "__main__":
    main()
