"""Worker of tests/test_gpu_chebyshev_distributed.py::test_two_true_ranks: TWO true ranks as threads of this process
(tests/thread_ranks.py, host transport), each with a handle of its own on the one GPU, CG + GMG with ChebyshevSmoother(Jacobi, DEGREE)
and the default estimate pre = post on the structured Q1 Poisson hierarchy.

    python tests/cheb_dist_worker.py OUT.npz CXxCYx.. NLEV

Writes per rank r: x_r (the rank's owned part of the CG solution), hist_r, iters_r, for every level l the global ids the rank owns
(gid_l_r), lest_r (lambda_est of every smoothed level), and sx_r / sr_r: one pass of level 0 with the GIVEN bounds BOUNDS through
gmg_smooth on the owned part of two seeded global vectors."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

WORLD = 2
DEGREE = 3
# the own x own streams pinned to SELL-64 (rows sum in storage order), as tests/test_gpu_gs_true_ranks.py pins them: a rank's matrix and
# the folded one then round their row sums alike
OPTIONS = dict(pattern=0, vdict=0, idx16=0, opattern=0, sell_maxpad=1.0e6)
BOUNDS = (0.2, 2.0)                                          # lambda_min, lambda_max of the level-0 pass (Jacobi on Q1: the spectrum lies in (0, 2))


def seeded(n):
    rng = np.random.default_rng(5)
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


def given_pass(abi, g, gid, ncells):
    """level 0 gets ChebyshevSmoother(Jacobi, DEGREE, lambda_min, lambda_max = BOUNDS) and a fresh setup (a collective); one pass"""
    abi.check(g.h, g._lib.gmg_set_smoother_jacobi(g.h, 0, abi.PRE_AND_POST, 1, 1.0))
    abi.check(g.h, g._lib.gmg_set_smoother_chebyshev(g.h, 0, abi.PRE_AND_POST, DEGREE, BOUNDS[0], BOUNDS[1], 10, 10.0, 1.1))
    abi.check(g.h, g._lib.gmg_setup(g.h))
    x0, r0 = seeded(ncells)
    sx, sr = np.ascontiguousarray(x0[gid]), np.ascontiguousarray(r0[gid])
    abi.check(g.h, g._lib.gmg_smooth(g.h, 0, abi.PRE, C.c_void_p(sx.ctypes.data), C.c_void_p(sr.ctypes.data), abi.MEM_HOST))
    return sx, sr


def main():
    import thread_ranks
    out, cells, nlev = sys.argv[1], tuple(int(c) for c in sys.argv[2].split("x")), int(sys.argv[3])
    results = {}

    def body(rank):
        import importlib
        import torch
        pkg = entry.import_package()
        pa, mg = (importlib.import_module(pkg.__name__ + "." + m) for m in ("partition", "multigpu"))
        po, abi = pkg.poisson, pkg.abi
        grid = pa.rank_grid(WORLD, len(cells))
        per_rank = tuple(c // g for c, g in zip(cells, grid))
        torch.cuda.set_device(0)
        g = mg.DistributedGMG(per_rank, nlev, rank, WORLD, device_id=0, transport="host", group=None, chebyshev=dict(degree=DEGREE), options=OPTIONS)
        lv = g.local["levels"]
        gid = lv[0].own_gid
        b = po.dirichlet_lift_rhs(cells, 1)[gid]
        x = np.zeros(g.n_own)
        log = g.cg_solve(b, x, maxiter=100, atol=1e-14, rtol=1e-8)
        res = dict(x=x, hist=np.asarray(log.residuals[: log.num_iters + 1]), iters=np.int64(log.num_iters),
                   lest=np.array([g.chebyshev_info(l)["lambda_est"] for l in range(nlev - 1)]))
        for l, L in enumerate(lv):
            res["gid_%d" % l] = np.asarray(L.own_gid, dtype=np.int64)
        sx, sr = given_pass(abi, g, gid, int(np.prod([c - 1 for c in cells])))
        res.update(sx=sx, sr=sr)
        g.close()
        results[rank] = res

    thread_ranks.run(WORLD, body)
    np.savez(out, **{"%s_%d" % (k, r): v for r, res in results.items() for k, v in res.items()})


if __name__ == "__main__":
    main()
