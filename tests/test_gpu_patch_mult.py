"""MultiplicativePatchSmoother on the device (csrc/pmult.inc.hpp, kernels.hpp patch_mult_*) against its numpy twin
(tests/patch_mult_reference.py).

1. whole passes, bit for bit: x and r of gmg_smooth, z of gmg_precond_apply, and within TOL_KERNEL of the LAPACK reference; the level
   layout pinned to SELL-64 (operator_edge_problems.CONFIGS["sell"]: r -= A dx sums every row in its stored order)
2. the one-launch pass: the same bits, the profiled launch counts
3. setter, signature, refresh
4. solves: the twin's iteration counts, x within TOL_KERNEL
5. errors, none of which runs a sweep"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import fullsize_reference as fr
import gs_reference as gr
import numpy_twin as nt
import operator_edge_problems as oe
import patch_edge_problems as pe
import patch_mult_reference as pm
from conftest import max_rel

pytestmark = pytest.mark.gpu

TOL_KERNEL = fr.TOL_KERNEL
SELL = dict(oe.CONFIGS["sell"])
ONE_LAUNCH_OFF = dict(SELL, pmult_one_launch=0)              # one launch per colour and direction
ONE_LAUNCH_ON = dict(SELL, pmult_one_launch=2)               # the whole pass as one launch of one workgroup


def _raw(po, M):
    return po.CSR(M.shape, M.indptr, M.indices, M.data)


def _opts(**kw):
    return dict(SELL, **kw)


def _setup(S, po, c, pre, post=None, options=None, **kw):
    post = pre if post is None else post
    kw.setdefault("maxiter", 1)
    gmg = S.GMGLinearSolver([_raw(po, c.A), _raw(po, c.Ac)], [_raw(po, c.P)], [_raw(po, c.R)], pre_smoothers=[pre], post_smoothers=[post],
                            options=SELL if options is None else options, **kw)
    return S.numerical_setup(S.symbolic_setup(gmg, gmg.smatrices[0]), gmg.smatrices[0])


_CASES = {}


def _case(po, hierarchy, key):
    """-> namespace(A, Ac, P, R, n, pp, pd, pivot, blocks, x0, r0): the fine level of a two-level hierarchy and its patch table"""
    if key in _CASES:
        return _CASES[key]
    if isinstance(key, tuple) and not isinstance(key[0], str):
        H = hierarchy(key, 2, 2)
        A = gr.csr(H["mats"][0].to_scipy())
        pp, pd = po.vertex_star_patches(key, 2)
        rng = np.random.default_rng([23, A.shape[0]])
        c = types.SimpleNamespace(A=A, Ac=gr.csr(H["mats"][1].to_scipy()), P=gr.csr(H["prolongations"][0].to_scipy()),
                                  R=gr.csr(H["restrictions"][0].to_scipy()), n=A.shape[0], pp=pp, pd=pd, pivot=True, blocks=None,
                                  x0=rng.uniform(-1, 1, A.shape[0]), r0=rng.uniform(-1, 1, A.shape[0]))
    else:
        e = pe.case(*key)
        H = pe.two_level(e.A, e.agg)
        c = types.SimpleNamespace(A=gr.csr(e.A), Ac=gr.csr(H["mats"][1]), P=gr.csr(H["prolongations"][0]), R=gr.csr(H["restrictions"][0]),
                                  n=e.N, pp=e.pp, pd=e.pd, pivot=e.pivot, blocks=e.blocks, x0=e.x0, r0=e.r)
    _CASES[key] = c
    return c


@functools.lru_cache(maxsize=None)
def _inverses(key, lapack=False, factors=False):
    c = _CASES[key]
    if factors:
        return [pm.factor_inverse(*f) for f in _factors(key)]
    return pm.inverses(c.A, c.pp, c.pd, c.pivot, c.blocks, lapack)


@functools.lru_cache(maxsize=None)
def _factors(key):
    """lu!(block) of every patch as LAPACK leaves it: (LU, 1-based ipiv)"""
    c = _CASES[key]
    blocks = c.blocks if c.blocks is not None else pe.blocks_of(c.A, c.pp, c.pd)
    out = []
    for B in blocks:
        if B.shape[0] == 0:
            out.append((np.zeros((0, 0)), np.zeros(0, dtype=np.int32)))
            continue
        lu, piv = sla.lu_factor(B)
        out.append((lu, (piv + 1).astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def _greedy(key):
    c = _CASES[key]
    return pm.greedy_coloring(c.A, c.pp, c.pd)[0]


def _solver(S, c, key=None, source="level"):
    cls = S.PatchSolver if c.pivot else S.BlockJacobiSolver
    if source == "factors":
        f = _factors(key)
        return cls(c.pp, c.pd, factors=pe.pack_colmajor([q[0] for q in f]), pivots=np.concatenate([q[1] for q in f]))
    if c.blocks is not None:
        return cls(c.pp, c.pd, patch_mats=pe.pack_colmajor(c.blocks))
    return cls(c.pp, c.pd)


def _twin_pass(key, niter, omega, type_, color, x0, r0, **inv):
    c = _CASES[key]
    x, r = x0.copy(), r0.copy()
    pm.smooth(c.A, _inverses(key, **inv), c.pp, c.pd, _greedy(key) if color is None else color, niter, omega, type_, x, r)
    return x, r


def _device_pass(ns, which, x0, r0):
    x, r = x0.copy(), r0.copy()
    ns.smooth(0, x, r, which)
    return x, r


def _check_pass(ns, pkg, key, which, niter, omega, type_, color=None, what="", **inv):
    """x, r of gmg_smooth from x0 != 0 and from x = 0, z of gmg_precond_apply: the twin's bits; and the LAPACK reference within TOL_KERNEL"""
    c = _CASES[key]
    zero = np.zeros(c.n)
    for x0 in (c.x0, zero):
        x, r = _device_pass(ns, which, x0, c.r0)
        xt, rt = _twin_pass(key, niter, omega, type_, color, x0, c.r0, **inv)
        assert np.array_equal(x, xt), (what, type_, niter, omega, "x", max_rel(x, xt))
        assert np.array_equal(r, rt), (what, type_, niter, omega, "r", max_rel(r, rt))
    z = np.full(c.n, np.nan)
    ns.precond(0, c.r0, z, which)
    assert np.array_equal(z, xt), (what, "z", max_rel(z, xt))   # (xt: the twin's pass from x = 0)
    if not inv.get("factors"):
        xl, rl = _twin_pass(key, niter, omega, type_, color, c.x0, c.r0, lapack=True)
        x, r = _device_pass(ns, which, c.x0, c.r0)
        ex, er = max_rel(x, xl), max_rel(r, rl)
        print("%s %s niter %d omega %.1f: against LAPACK inverses max_rel x %.2e r %.2e" % (what, type_, niter, omega, ex, er))
        assert ex <= TOL_KERNEL and er <= TOL_KERNEL, (what, ex, er)


SLOTS = (("forward", 1, 1.0), ("backward", 2, 0.7), ("symmetric", 1, 0.7), ("symmetric", 2, 1.0))   # (type, niter, omega): pre, post


def _both_slots(S, po, pkg, hierarchy, key, options=None, source="level", coloring="greedy", what=""):
    c = _case(po, hierarchy, key)
    color = None if isinstance(coloring, str) else coloring
    inv = dict(factors=True) if source == "factors" else {}
    for pre_s, post_s in (SLOTS[:2], SLOTS[2:]):
        pre = S.MultiplicativePatchSmoother(_solver(S, c, key, source), pre_s[1], pre_s[2], pre_s[0], coloring)
        post = S.MultiplicativePatchSmoother(_solver(S, c, key, source), post_s[1], post_s[2], post_s[0], coloring)
        ns = _setup(S, po, c, pre, post, options)
        try:
            for which, s in ((pkg.abi.PRE, pre_s), (pkg.abi.POST, post_s)):
                _check_pass(ns, pkg, key, which, s[1], s[2], s[0], color, what or str(key), **inv)
            nc, got = ns.patch_coloring(0, "post")
            want = _greedy(key) if color is None else color
            assert np.array_equal(got, want) and nc == int(want.max()) + 1
            d = {"forward": "F", "backward": "B", "symmetric": "F+B"}
            tag = "F+B" if pre_s[0] != post_s[0] else d[pre_s[0]]
            assert ns.sweep_signature(0).endswith(" pmult=%s/%d" % (tag, nc)), ns.sweep_signature(0)
        finally:
            ns.close()


# ---------------------------------------------------------------- 1. whole passes
def test_passes_q2_2d(S, po, pkg, hierarchy):
    """Q2 (6, 6): 49 patches (not a multiple of 4) of 1 to 9 dofs, truncated at the boundary; 4 colours; as one launch and per colour"""
    c = _case(po, hierarchy, (6, 6))
    assert c.pp.size - 1 == 49 and np.diff(c.pp).max() == 9 and np.diff(c.pp).min() == 1 and _greedy((6, 6)).max() == 3
    _both_slots(S, po, pkg, hierarchy, (6, 6), options=ONE_LAUNCH_ON, what="q2 6x6 one launch")
    _both_slots(S, po, pkg, hierarchy, (6, 6), options=ONE_LAUNCH_OFF, what="q2 6x6 per colour")


@pytest.mark.parametrize("dedup", (1, 0))
def test_passes_q2_3d(S, po, pkg, hierarchy, dedup):
    """Q2 (4, 4, 4): 125 patches of up to 27 dofs, 8 colours; de-duplicated blocks or the plain store: the same bits"""
    c = _case(po, hierarchy, (4, 4, 4))
    assert c.pp.size - 1 == 125 and np.diff(c.pp).max() == 27 and _greedy((4, 4, 4)).max() == 7
    for one in (0, 2):
        _both_slots(S, po, pkg, hierarchy, (4, 4, 4), options=_opts(patch_dedup=dedup, pmult_one_launch=one), what="q2 4^3 dedup %d one launch %d" % (dedup, one))


@pytest.mark.parametrize("name,kind", (("wave63", "lu"), ("wave63", "nopivot"), ("wave64", "lu"), ("big", "nopivot"), ("dense", "lu"),
                                       ("dedup_ragged", "nopivot")))
def test_passes_ragged_families(S, po, pkg, hierarchy, name, kind):
    """patch_edge_problems: pivoting and non-pivoting blocks, caller patch_mats (`dense`), n_p in {0, 1, 63, 64, 65, 81, 125, 130},
    colours that hold one patch, de-duplicated blocks of ragged sizes"""
    key = (name, kind)
    c = _case(po, hierarchy, key)
    color = _greedy(key)
    assert np.bincount(color).min() == 1 or name == "dedup_ragged"
    if name == "big":
        assert set(np.diff(c.pp)) >= {0, 64, 65, 130}
    for options in ((ONE_LAUNCH_ON, ONE_LAUNCH_OFF) if name in ("wave63", "big") else (ONE_LAUNCH_ON if name == "dedup_ragged" else None,)):
        _both_slots(S, po, pkg, hierarchy, key, options=options, what="%s-%s%s" % (name, kind, "" if options is None else " one launch %d" % options["pmult_one_launch"]))


def test_passes_caller_factors(S, po, pkg, hierarchy):
    """the blocks handed over as lu! factors with LAPACK pivots: the inverse is ldiv!(F, I) on the host"""
    key = ("dense", "lu")
    _case(po, hierarchy, key)
    assert any(np.any(f[1] != np.arange(1, f[1].size + 1)) for f in _factors(key))
    _both_slots(S, po, pkg, hierarchy, key, options=ONE_LAUNCH_ON, source="factors", what="factors")


@pytest.mark.parametrize("kind", ("reversed", "own"))
def test_passes_given_coloring(S, po, pkg, hierarchy, kind):
    """a given valid colouring (the greedy colours in reverse) and every patch its own colour"""
    key = (6, 6)
    c = _case(po, hierarchy, key)
    g = _greedy(key)
    color = (g.max() - g).astype(np.int32) if kind == "reversed" else np.arange(c.pp.size - 1, dtype=np.int32)
    for options in (ONE_LAUNCH_ON, ONE_LAUNCH_OFF):
        _both_slots(S, po, pkg, hierarchy, key, options=options, coloring=color, what="given-" + kind)


# ---------------------------------------------------------------- 2. the one-launch pass
@pytest.mark.parametrize("key", ((6, 6), (4, 4, 4), ("big", "nopivot")))
def test_one_launch_same_bits_and_launch_counts(S, po, pkg, hierarchy, key):
    c = _case(po, hierarchy, key)
    sm = S.MultiplicativePatchSmoother(_solver(S, c, key), 1, 1.0, "forward")
    ns = _setup(S, po, c, sm)
    out = {}
    try:
        nc, color = ns.patch_coloring(0)
        for mode in (0, 2, 1):
            ns.set_option("pmult_one_launch", mode)
            ns.profile(0)
            x, r = _device_pass(ns, 0, c.x0, c.r0)
            out[mode] = (x, r, ns.kernel_stats()["launches"])
            ns.profile(0, False)
        ns.set_option("pmult_one_launch", 1)
        ns.set_option("pmult_one_launch_max", 0)
        off = _device_pass(ns, 0, c.x0, c.r0)
    finally:
        ns.close()
    for mode in (2, 1):
        assert np.array_equal(out[0][0], out[mode][0]) and np.array_equal(out[0][1], out[mode][1])
    assert np.array_equal(out[0][0], off[0]) and np.array_equal(out[0][1], off[1])
    sizes = np.diff(c.pp)
    # (one launch per colour for its patches of at most 64 dofs, one for its larger ones)
    launches = sum(int(np.any(sizes[color == q] > 64)) + int(np.any((sizes[color == q] > 0) & (sizes[color == q] <= 64))) for q in range(nc))
    print(key, "colours", nc, "launches per forward sweep", launches, "profiled", out[0][2], out[2][2])
    assert out[2][2] == 1 + 1 and out[0][2] == launches + 1
    if key != ("big", "nopivot"):
        assert out[0][2] - out[2][2] == nc - 1                # one launch per colour against one launch


# ---------------------------------------------------------------- 3. setter, signature, refresh
def test_coloring_is_the_host_functions(S, po, pkg, hierarchy):
    for key in ((4, 4, 4), ("wave63", "lu")):
        c = _case(po, hierarchy, key)
        ns = _setup(S, po, c, S.MultiplicativePatchSmoother(_solver(S, c, key), type="backward"))
        try:
            nc, color = ns.patch_coloring(0, "pre")
            hc, hn = S.patch_multicolor(_raw(po, c.A), c.pp, c.pd)
            assert nc == hn and np.array_equal(color, hc)
            assert ns.sweep_signature(0).endswith(" pmult=B/%d" % nc)
            assert ns.patch_coloring(0, "post")[0] == nc
        finally:
            ns.close()


@pytest.mark.parametrize("key", ((4, 4, 4), ("wave63", "lu")))
def test_value_refresh_is_bitwise_a_fresh_setup(S, po, pkg, hierarchy, key):
    c = _case(po, hierarchy, key)
    s = 1.0 + 0.5 * np.sin(2.0 * np.pi * np.arange(c.n) / c.n)
    A2 = gr.csr(sp.diags(s) @ c.A + sp.diags(0.5 * s * np.abs(c.A.diagonal())))
    assert np.array_equal(A2.indices, c.A.indices) and np.array_equal(A2.indptr, c.A.indptr)
    c2 = types.SimpleNamespace(**vars(c))
    c2.A = A2
    out = []
    for start in (c, c2):
        ns = _setup(S, po, start, S.MultiplicativePatchSmoother(_solver(S, c, key), 1, 1.0, "symmetric"))
        try:
            before = ns.patch_coloring(0)
            first = _device_pass(ns, 0, c.x0, c.r0)
            if start is c:
                S.numerical_setup_(ns, _raw(po, A2))
                after = ns.patch_coloring(0)
                assert before[0] == after[0] and np.array_equal(before[1], after[1])
            out.append(_device_pass(ns, 0, c.x0, c.r0) + (first,))
        finally:
            ns.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert not np.array_equal(out[0][2][0], out[0][0])        # (the new values changed the pass)


def test_a_matrix_gmg_set_matrix_streamed_gets_its_rows_back(S, po, pkg, hierarchy):
    """>= 20 000 rows with the default options: gmg_set_matrix keeps the level as a row stream; the setup of a multiplicative slot takes
    the rows back -- the same bits as with that conversion switched off"""
    nc = (72, 72)
    H = hierarchy(nc, 2, 2)
    n = H["mats"][0].shape[0]
    assert n == 143 * 143 and n >= 20000                      # (the row count from which gmg_set_matrix streams)
    pp, pd = po.vertex_star_patches(nc, 2)
    rng = np.random.default_rng(11)
    x0, r0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    out = []
    for options in (dict(), dict(eager=0)):
        sm = S.MultiplicativePatchSmoother(S.PatchSolver(pp, pd), 1, 1.0, "symmetric")
        gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=[sm], post_smoothers=[sm], options=options, maxiter=1)
        ns = S.numerical_setup(S.symbolic_setup(gmg, H["mats"][0]), H["mats"][0])
        try:
            out.append(_device_pass(ns, 0, x0, r0) + (ns.patch_coloring(0)[0],))
        finally:
            ns.close()
    assert out[0][2] == 4 and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.linalg.norm(out[0][1]) < 0.5 * np.linalg.norm(r0)


# ---------------------------------------------------------------- 4. solves
SOLVES = {
    "cg-q2-8x8-2lev": dict(nc=(8, 8), nlev=2, solver="cg", cycle="v", pre="forward", post="backward", rtol=1e-8),
    "cg-q2-16x16-3lev": dict(nc=(16, 16), nlev=3, solver="cg", cycle="v", pre="forward", post="backward", rtol=1e-8),
    "fgmres-q2-4x4x4-2lev": dict(nc=(4, 4, 4), nlev=2, solver="fgmres", cycle="v", pre="symmetric", post="symmetric", rtol=1e-8),
    "cg-q2-16x16-3lev-w": dict(nc=(16, 16), nlev=3, solver="cg", cycle="w", pre="symmetric", post="symmetric", rtol=1e-8),
    "fgmres-pl-q2-8x8-2lev": dict(nc=(8, 8), nlev=2, solver="fgmres_pl", cycle="v", pre="symmetric", post="symmetric", rtol=1e-6),
}


def _twin_solve(po, H, c, b):
    A = H["mats"][0].to_scipy().tocsr()
    tabs = [po.vertex_star_patches(cells, 2) for cells in H["ncells"][:-1]]
    pre = [pm.PMult(*t, type=c["pre"]) for t in tabs]
    post = [pm.PMult(*t, type=c["post"]) for t in tabs]
    G = gr.GMG(H["mats"], H["prolongations"], H["restrictions"], pre, post, cycle=c["cycle"])
    kw = dict(maxiter=100, atol=1e-14, rtol=c["rtol"])
    if c["solver"] == "cg":
        return nt.cg(A, b, Pl=G.solve, **kw)
    if c["solver"] == "fgmres":
        return nt.fgmres(A, b, Pr=G.solve, m=5, **kw)

    def Pl(v):
        x, r = np.zeros_like(v), v.copy()
        pre[0].smooth(G.pre_ns[0], x, r)
        return x

    class Left:
        def __matmul__(self, v):
            return Pl(A @ v)
    return nt.fgmres(Left(), Pl(b), Pr=G.solve, m=5, **kw)


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_solves(S, po, hierarchy, name):
    c = SOLVES[name]
    H = hierarchy(c["nc"], c["nlev"], 2)
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    tabs = [po.vertex_star_patches(cells, 2) for cells in H["ncells"][:-1]]
    pre = [S.MultiplicativePatchSmoother(S.PatchSolver(*t), type=c["pre"]) for t in tabs]
    post = pre if c["post"] == c["pre"] else [S.MultiplicativePatchSmoother(S.PatchSolver(*t), type=c["post"]) for t in tabs]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=pre, post_smoothers=post,
                            cycle_type=c["cycle"] + "_cycle", maxiter=1, options=SELL)
    kw = dict(maxiter=100, atol=1e-14, rtol=c["rtol"])
    if c["solver"] == "cg":
        solver = S.CGSolver(gmg, **kw)
    elif c["solver"] == "fgmres":
        solver = S.FGMRESSolver(5, gmg, **kw)
    else:
        solver = S.FGMRESSolver(5, gmg, Pl=S.LinearSolverFromSmoother(gmg.pre_smoothers[0]), **kw)
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    try:
        x = np.zeros(b.size)
        S.solve_(x, ns, b)
        sig = ns.P_ns.sweep_signature(0)
    finally:
        ns.P_ns.close()
    xo, nit, hist = _twin_solve(po, H, c, b)
    err = max_rel(x, xo)
    print(name, "iterations", solver.log.num_iters, "twin", nit, "max_rel x %.2e" % err, sig)
    assert hist[-1] / hist[0] < c["rtol"]
    assert solver.log.num_iters == nit and solver.log.flag == S.SOLVER_CONVERGED_RTOL
    assert err <= TOL_KERNEL
    assert " pmult=F+B/" in sig


def test_inside_a_block_solver(S, po, hierarchy):
    """BlockDiagonalSolver([GMG with the multiplicative smoother, LU]): the first block of one application is one cycle of the twin"""
    nc = (8, 8)
    H = hierarchy(nc, 2, 2)
    A = H["mats"][0]
    n = A.shape[0]
    t = po.vertex_star_patches(nc, 2)
    sm = [S.MultiplicativePatchSmoother(S.PatchSolver(*t))]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1, options=SELL)
    solver = S.BlockDiagonalSolver([gmg, S.LUSolver()])
    mat = [[A, None], [None, A]]
    ns = S.numerical_setup(S.symbolic_setup(solver, mat), mat)
    try:
        b = np.random.default_rng(2).uniform(-1, 1, 2 * n)
        x = np.zeros(2 * n)
        S.solve_(x, ns, b)
    finally:
        ns.close()
    G = gr.GMG(H["mats"], H["prolongations"], H["restrictions"], [pm.PMult(*t)])
    err = max_rel(x[:n], G.solve(b[:n]))
    print("block application: max_rel %.2e" % err)
    assert err <= TOL_KERNEL


# ---------------------------------------------------------------- 5. errors
def _q2_handle(S, po, hierarchy, sm=None, coloring="greedy"):
    c = _case(po, hierarchy, (6, 6))
    sm = sm or S.MultiplicativePatchSmoother(S.PatchSolver(c.pp, c.pd), coloring=coloring)
    return _setup(S, po, c, sm), c


def test_conflicting_coloring_is_refused_at_setup(S, po, pkg, hierarchy):
    abi = pkg.abi
    c = _case(po, hierarchy, (6, 6))
    bad = _greedy((6, 6)).copy()
    q, p = 3, 10                                              # two interior vertex stars next to each other (patch 3 + 7 = 10)
    assert pm.first_conflict(c.A, c.pp, c.pd, np.where(np.arange(49) == p, bad[q], bad)) == (q, p)
    bad[p] = bad[q]
    with pytest.raises(abi.GmgError) as e:
        _q2_handle(S, po, hierarchy, coloring=bad)
    msg = str(e.value)
    assert e.value.code == abi.ERR_INVALID and "level 0" in msg and "patches %d and %d" % (q, p) in msg


def test_setter_errors(S, po, pkg, hierarchy):
    abi = pkg.abi
    lib = abi.load()
    ns, c = _q2_handle(S, po, hierarchy, S.RichardsonSmoother(S.PatchSolver(*po.vertex_star_patches((6, 6), 2)), 1, 0.2))
    h = ns.h
    try:
        with pytest.raises(abi.GmgError) as e:
            ns.patch_coloring(0)
        assert e.value.code == abi.ERR_STATE
        for args in ((0, 1.0, abi.PMULT_FORWARD), (1, 0.0, abi.PMULT_FORWARD), (1, -1.0, abi.PMULT_SYMMETRIC), (1, 1.0, 3), (1, 1.0, -1)):
            assert lib.gmg_set_smoother_patch_multiplicative(h, 0, abi.PRE_AND_POST, *args) == abi.ERR_INVALID
        assert lib.gmg_set_smoother_patch_multiplicative(h, 0, 7, 1, 1.0, 0) == abi.ERR_INVALID
        assert lib.gmg_set_smoother_patch_multiplicative(h, 1, abi.PRE, 1, 1.0, 0) == abi.ERR_INVALID      # the coarsest level
        # colourings: a wrong length, a negative colour, an unknown kind, an array with kind 0
        col = np.zeros(49, dtype=np.int32)
        ptr = C.c_void_p(col.ctypes.data)
        assert lib.gmg_set_patch_coloring(h, 0, abi.PRE, 1, ptr, 48) == abi.ERR_INVALID
        assert lib.gmg_set_patch_coloring(h, 0, abi.PRE, 1, ptr, 50) == abi.ERR_INVALID
        assert lib.gmg_set_patch_coloring(h, 0, abi.PRE, 2, ptr, 49) == abi.ERR_INVALID
        assert lib.gmg_set_patch_coloring(h, 0, abi.PRE, 0, ptr, 49) == abi.ERR_INVALID
        col[5] = -1
        assert lib.gmg_set_patch_coloring(h, 0, abi.PRE, 1, ptr, 49) == abi.ERR_INVALID
        x, r = _device_pass(ns, 0, c.x0, c.r0)                # the refused calls left the handle as it was: still set up
        assert np.all(np.isfinite(x)) and " pmult=" not in ns.sweep_signature(0)
        # Chebyshev on the slot, and the slot on a Chebyshev slot
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.POST, 3, 0.0, 0.0, 10, 10.0, 1.1) == abi.OK
        assert lib.gmg_set_smoother_patch_multiplicative(h, 0, abi.POST, 1, 1.0, 0) == abi.ERR_UNSUPPORTED
        assert lib.gmg_set_smoother_patch_multiplicative(h, 0, abi.PRE, 1, 1.0, 0) == abi.OK
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.PRE, 3, 0.0, 0.0, 10, 10.0, 1.1) == abi.ERR_UNSUPPORTED
        # a slot without a patch smoother
        assert lib.gmg_set_smoother_jacobi(h, 0, abi.PRE_AND_POST, 2, 0.8) == abi.OK
        assert lib.gmg_set_smoother_patch_multiplicative(h, 0, abi.PRE, 1, 1.0, 0) == abi.ERR_STATE
        assert lib.gmg_set_patch_coloring(h, 0, abi.PRE, 0, None, 0) == abi.ERR_STATE
        assert lib.gmg_set_smoother_gauss_seidel(h, 0, abi.PRE, 1, 1.0, 0) == abi.OK
        assert lib.gmg_set_smoother_patch_multiplicative(h, 0, abi.PRE, 1, 1.0, 0) == abi.ERR_STATE
    finally:
        ns.close()
    h = C.c_void_p()
    abi.check(None, lib.gmg_create(C.byref(h), 2, 0))
    try:
        assert lib.gmg_set_smoother_patch_multiplicative(h, 0, abi.PRE_AND_POST, 1, 1.0, 0) == abi.ERR_STATE   # nothing assigned yet
    finally:
        lib.gmg_destroy(h)


def test_refused_at_setup(S, po, pkg, hierarchy):
    """patch_cols != patch_rows, a loopback communicator of 2, a streamed level: GMG_ERR_UNSUPPORTED naming the level, no sweep runs"""
    abi = pkg.abi
    c = _case(po, hierarchy, ("wave63", "nopivot"))
    sm = S.MultiplicativePatchSmoother(S.BlockJacobiSolver(c.pp, c.pd, patch_cols=pe.cols_reversed(c.pp, c.pd)))
    with pytest.raises(abi.GmgError) as e:
        _setup(S, po, c, sm)
    assert e.value.code == abi.ERR_UNSUPPORTED and "level 0" in str(e.value) and "patch_cols" in str(e.value)
    # a loopback communicator of 2
    ns, c = _q2_handle(S, po, hierarchy)
    xfn = abi.HOST_EXCHANGE_FN(lambda *a: None)
    rfn = abi.HOST_ALLREDUCE_FN(lambda *a: None)
    try:
        abi.check(ns.h, ns._lib.gmg_comm_init_host(ns.h, 0, 1, C.cast(xfn, C.c_void_p), C.cast(rfn, C.c_void_p), None))
        abi.check(ns.h, ns._lib.gmg_comm_set_loopback(ns.h, 2))
        with pytest.raises(abi.GmgError) as e:
            ns.setup()
        assert e.value.code == abi.ERR_UNSUPPORTED and "level 0" in str(e.value) and "communicator" in str(e.value)
    finally:
        ns.close()
    # a level streamed by the caller
    ns, c = _q2_handle(S, po, hierarchy)
    try:
        ptr, idx = c.A.indptr.astype(np.int64), c.A.indices.astype(np.int64)
        abi.check(ns.h, ns._lib.gmg_set_operator_rows(ns.h, 0, abi.OP_A, c.n, c.n, 0, c.n, C.c_void_p(ptr.ctypes.data), C.c_void_p(idx.ctypes.data),
                                                      C.c_void_p(c.A.data.ctypes.data), 0, 8))
        with pytest.raises(abi.GmgError) as e:
            ns.setup()
        assert e.value.code == abi.ERR_UNSUPPORTED and "level 0" in str(e.value) and "streamed" in str(e.value)
    finally:
        ns.close()
