"""The Gauss-Seidel smoother between TRUE ranks: two ranks as threads of one child process (tests/gs_dist_worker.py over
tests/thread_ranks.py, host transport, a handle per rank on the one GPU) against the W = 2 partition folded onto one rank
(host loopback, reductions rank by rank: gmg_comm_set_loopback_rows) and against the numpy twin with reference (b) per level (tests/gs_dist_reference.py)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gs_dist_reference as gd
import gs_dist_worker as gw
import gs_reference as gr
import halo_edge_problems as he
from conftest import rel_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _mods(pkg):
    m = lambda n: importlib.import_module(pkg.__name__ + "." + n)
    return m("partition"), m("multigpu"), m("solvers"), m("abi")


def _worker(tmp_path, cells, nlev, ordering, rep=0, sub_from=0, sub_ranks=0, options=None):
    out = os.path.join(str(tmp_path), "ranks.npz")
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "gs_dist_worker.py"), out, "x".join(map(str, cells)), str(nlev), ordering,
                        str(rep), str(sub_from), str(sub_ranks)] + ([__import__("json").dumps(options)] if options else []), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return np.load(out)


_RUNS = {}
LAYOUTS = {"default": None, "sell": dict(pattern=0, vdict=0, idx16=0, opattern=0, sell_maxpad=1.0e6)}


def _two_ranks_and_folded(pkg, po, tmp_path_factory, ordering, layout="default"):
    """the two-rank run of the worker and the W = 2 folded run of the same problem, once per ordering"""
    key, options = (ordering, layout), LAYOUTS[layout]
    if key in _RUNS:
        return _RUNS[key]
    import ctypes as C
    pa, mg, sv, abi = _mods(pkg)
    cells, nlev = (16, 16, 16), 3
    v = _worker(tmp_path_factory.mktemp("ranks_" + ordering), cells, nlev, ordering, options=options)
    grid = pa.rank_grid(2, 3)
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, None, None, "jacobi") for r in range(2)])
    gid = F["levels"][0].own_gid
    assert np.array_equal(gid, np.concatenate([v["gid_0_0"], v["gid_0_1"]]))
    g = mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport="host_loopback", local_hierarchy=F, cells_global=cells,
                          smoother=sv.SymGaussSeidelSmoother(1, 1.0, ordering), loopback_rows=[v["gid_0_0"].size, v["gid_0_1"].size], options=options)
    try:
        b = po.dirichlet_lift_rhs(cells, 1)[gid]
        x = np.zeros(g.n_own)
        log = g.cg_solve(b, x, maxiter=100, atol=1e-14, rtol=1e-8)
        hist = np.asarray(log.residuals[: log.num_iters + 1])
        abi.check(g.h, g._lib.gmg_set_smoother_gauss_seidel(g.h, 0, abi.PRE_AND_POST, gw.SMOOTH[0], gw.SMOOTH[1], abi.GS_SYMMETRIC))
        abi.check(g.h, g._lib.gmg_setup(g.h))
        x0, r0 = gw.seeded(int(np.prod([c - 1 for c in cells])))
        sx, sr = np.ascontiguousarray(x0[gid]), np.ascontiguousarray(r0[gid])
        abi.check(g.h, g._lib.gmg_smooth(g.h, 0, abi.PRE, C.c_void_p(sx.ctypes.data), C.c_void_p(sr.ctypes.data), abi.MEM_HOST))
    finally:
        g.close()
    _RUNS[key] = (v, dict(x=x, hist=hist, iters=int(log.num_iters), sx=sx, sr=sr))
    return _RUNS[key]


@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_pass_between_two_true_ranks_is_bitwise_the_folded_run(pkg, po, tmp_path_factory, ordering):
    """One symmetric pass (niter 2, omega 1.2) of level 0 -- triangular solves on each rank's own block, dx exchanged between the two
    handles, r -= A dx -- gives on every rank the bits of its rows of the W = 2 folded run; the CG + GMG solve takes the same number
    of iterations on both ranks and in the folded run, with one history on both ranks."""
    v, f = _two_ranks_and_folded(pkg, po, tmp_path_factory, ordering)
    rx, rr = np.concatenate([v["sx_0"], v["sx_1"]]), np.concatenate([v["sr_0"], v["sr_1"]])
    assert np.array_equal(he.bits(rx), he.bits(f["sx"])) and np.array_equal(he.bits(rr), he.bits(f["sr"]))
    assert int(v["iters_0"]) == int(v["iters_1"]) == f["iters"] and np.array_equal(he.bits(v["hist_0"]), he.bits(v["hist_1"]))


@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_solve_between_two_true_ranks_is_bitwise_the_folded_run(pkg, po, tmp_path_factory, ordering, layout="sell"):
    """x and history of the CG + GMG solve bit for bit the W = 2 folded run.

    Two things make the bits equal, and both runs get them alike.  (1) The folded handle is told the two ranks' row counts
    (loopback_rows -> gmg_comm_set_loopback_rows): every dot product and norm of CG is reduced rank by rank and the sums are added in
    rank order, as the two ranks' all-reduce does; without it the folded handle makes ONE reduction over the stacked rows.  (2) The
    own x own streams are pinned to SELL-64, whose rows sum in storage order (the pin of tests/test_gpu_halo_edges.py): the
    structure-exploiting layouts are chosen per matrix, and a rank's matrix and the folded one get forms whose row sums round
    differently.  Measured on an MI355X, 5 iterations in every run: with (1) and (2) x and the history are equal bit for bit; with (1)
    alone x differs by 1.2e-16 relative and the history by 9.2e-17 r0 (multicolour 1.0e-16, 1.6e-18 r0); with neither by 1.0e-16 and
    5.1e-18 r0.  The smoothing passes of level 0 are bitwise equal in the default layout too (the test above)."""
    v, f = _two_ranks_and_folded(pkg, po, tmp_path_factory, ordering, layout)
    xr = np.concatenate([v["x_0"], v["x_1"]])
    n = min(v["hist_0"].size, f["hist"].size)
    print(ordering, layout, "iterations", int(v["iters_0"]), f["iters"], "x rel", rel_err(xr, f["x"]),
          "history max difference / r0", float(np.max(np.abs(v["hist_0"][:n] - f["hist"][:n]) / f["hist"][0])))
    assert np.array_equal(he.bits(v["hist_0"]), he.bits(f["hist"])), "history differs from the folded run"
    assert np.array_equal(he.bits(xr), he.bits(f["x"])), "x differs from the folded run"


@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
def test_redistributed_subset(pkg, po, tmp_path, ordering):
    """Levels 0 on two ranks, level 1 on the first rank alone (sub_from = 1, sub_ranks = 1 of 2: one block, global sweeps there),
    level 2 replicated: iteration count of the numpy twin with reference (b) per level, history <= 1e-8 r0 per entry, x <= 1e-10."""
    cells, nlev, rep = (16, 16), 3, 2
    v = _worker(tmp_path, cells, nlev, ordering, rep=rep, sub_from=1, sub_ranks=1)
    assert v["gid_1_1"].size == 0 and v["gid_1_0"].size == 7 * 7               # level 1 lives on rank 0 alone
    H = po.build_hierarchy(cells, nlev, 1)
    gids = [np.concatenate([v["gid_0_0"], v["gid_0_1"]]), v["gid_1_0"], np.arange(H["mats"][2].shape[0])]
    blocks = [gd.blocks_of([v["gid_0_0"].size, v["gid_0_1"].size]), None, None]
    levels = [type("L", (), dict(own_gid=q)) for q in gids]
    mats, Ps, Rs = gd.folded_hierarchy(H, levels)
    w = lambda Ms: [he._po_csr(po, M) for M in Ms]
    sms = [gd.BlockGS(1, 1.0, "symmetric", ordering, blocks[l]) for l in range(nlev - 1)]
    G = gr.GMG(w(mats), w(Ps), w(Rs), sms, sms)
    b = po.dirichlet_lift_rhs(cells, 1)[gids[0]]
    xo, nit, hist = gr.cg(mats[0], b, Pl=G.solve, maxiter=100, atol=1e-14, rtol=1e-8)
    x = np.concatenate([v["x_0"], v["x_1"]])
    print(ordering, "iterations", int(v["iters_0"]), "reference", nit, "x rel", rel_err(x, xo))
    assert hist[-1] / hist[0] < 1e-8
    assert int(v["iters_0"]) == int(v["iters_1"]) == nit
    assert np.all(np.abs(v["hist_0"][: nit + 1] - hist) <= 1e-8 * hist[0])
    assert rel_err(x, xo) <= 1e-10


def test_loopback_rows_are_checked(pkg):
    """gmg_comm_set_loopback_rows: one count per virtual rank; a rank but the last with an odd count is refused (the next rank's part of
    a folded vector would lose the alignment that a rank's own vector has, and with it the form of the dot kernel)"""
    pa, mg, sv, abi = _mods(pkg)
    cells, nlev = (16, 16, 16), 3
    grid = pa.rank_grid(2, 3)
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, None, None, "jacobi") for r in range(2)])
    n = F["levels"][0].n_own
    for rows, code, text in (([n - 1801, 1801][::-1], abi.ERR_UNSUPPORTED, "odd number of rows"), ([n], abi.ERR_INVALID, "one row count per virtual rank"),
                             ([-2, n + 2], abi.ERR_INVALID, "negative row count")):
        with pytest.raises(abi.GmgError, match=text) as e:
            mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport="host_loopback", local_hierarchy=F, cells_global=cells,
                              loopback_rows=rows)
        assert e.value.code == code
    with pytest.raises(ValueError, match="loopback transports"):
        mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport="host", local_hierarchy=F, cells_global=cells, loopback_rows=[n // 2, n - n // 2])
