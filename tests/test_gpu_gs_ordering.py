"""Visiting orders of the device Gauss-Seidel smoother (gmg_set_gs_ordering, csrc/gs.inc.hpp: the ordered schedule, gs_wide_kernel and
the folded x update) against the numpy restatement of tests/gs_ordering_reference.py on the families of tests/gs_edge_problems.py
and on level 0 of hierarchy((32,32,32), 3).

1. triangular solves in the multicolour, a random and the reversed order: BITWISE gs_reference.forward_rows / backward_rows on
   B = A[order, order]; the identity as a given order is the handle that never set one
2. gs_wide_kernel where it can go wrong: ragged last slice, slices of different widths, padded slots over a poisoned dx, chain-only and
   mixed plans
3. the folded x update: bits and launch counts (gmg_get_kernel_stats)      4. gmg_get_gs_schedule / gmg_get_gs_ordering
5. whole passes and the Krylov cases in the multicolour order              6. value refresh     7. errors"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp

import fullsize_reference as fr
import gs_edge_problems as ge
import gs_ordering_reference as go
import gs_reference as gr
import operator_edge_problems as oe
from conftest import max_rel, rel_err

pytestmark = pytest.mark.gpu

PLAIN_SELL = dict(pattern=0, vdict=0, idx16=0, opattern=0)   # a layout that stores explicit values: gmg_setup refreshes in place
LEVEL32 = "q1_3d-32"                                         # level 0 of hierarchy((32,32,32), 3): 29 791 rows, 8 colours of 3375 .. 4096 rows
ORDERS = ("multicolor", "random", "reversed")


@functools.lru_cache(maxsize=None)
def _case(name):
    if name != LEVEL32:
        return ge.case(name)
    A = ge._poisson_level((32, 32, 32), 3, 1, 0)
    n = A.shape[0]
    nH = oe.coarse_size(n)
    v = oe._rng(n, nH, 14).uniform(0.25, 1.0, n)             # (an aggregation, as gs_edge_problems does for its large family)
    P = sp.csr_matrix((v, (np.arange(n), np.arange(n) % nH)), shape=(n, nH))
    P.sort_indices()
    R = sp.csr_matrix(P.T)
    R.sort_indices()
    absum = lambda M: float(np.mean(np.abs(M).sum(axis=1))) or 1.0
    Ac = oe.coarse_matrix(nH, float(np.mean(np.abs(A.diagonal()))) * absum(P) * absum(R))
    rng = oe._rng(32, n, 13)
    return types.SimpleNamespace(name=name, A=A, P=P, R=R, Ac=Ac, n=n, nH=nH, x0=rng.uniform(-1, 1, n), r0=rng.uniform(-1, 1, n))


@functools.lru_cache(maxsize=None)
def _order(name, kind):
    """-> (order as the reference uses it, ordering argument of the device smoother)"""
    c = _case(name)
    if kind == "multicolor":
        return go.multicolor(c.A)[0], "multicolor"
    order = np.arange(c.n)[::-1].copy() if kind == "reversed" else oe._rng(c.n, 77, 5).permutation(c.n)
    return order, order


@functools.lru_cache(maxsize=None)
def _B(name, kind):
    return go.permuted(_case(name).A, _order(name, kind)[0])


def _csr(po, M):
    return po.CSR(M.shape, M.indptr, M.indices, M.data)      # raw: `shuffled` keeps its storage order


def _two_level(S, po, c, pre, post=None, scale=1.0, options=None):
    post = pre if post is None else post
    gmg = S.GMGLinearSolver([_csr(po, c.A * scale), _csr(po, c.Ac * scale)], [_csr(po, c.P)], [_csr(po, c.R)], pre_smoothers=[pre],
                            post_smoothers=[post], maxiter=1, mode="preconditioner", options=options)
    A = gmg.smatrices[0]
    return S.numerical_setup(S.symbolic_setup(gmg, A), A)


def _solves(S, po, pkg, name, kind, omega=1.0, poison=False):
    """one handle, forward smoother in front and backward smoother behind, both in the given order -> {forward: dx} from x = 0"""
    c = _case(name)
    arg = _order(name, kind)[1]
    ns = _two_level(S, po, c, S.GaussSeidelSmoother(1, omega, "forward", arg), S.GaussSeidelSmoother(1, omega, "backward", arg))
    out = {}
    try:
        for forward in (True, False):
            if poison:                                        # a pass over a NaN residual leaves NaN in every entry of the level's dx
                x, r = np.zeros(c.n), np.full(c.n, np.nan)
                ns.smooth(0, x, r, pkg.abi.PRE if forward else pkg.abi.POST)
                assert np.all(np.isnan(x))
            dx = np.full(c.n, np.nan)
            ns.precond(0, c.r0, dx, pkg.abi.PRE if forward else pkg.abi.POST)
            out[forward] = dx
        assert ns.sweep_signature(0).endswith(" gs=F+B")
    finally:
        ns.close()
    return out


def _reference(name, kind, forward, r):
    order = _order(name, kind)[0]
    return (go.forward if forward else go.backward)(_case(name).A, order, r, _B(name, kind))


# ---------------------------------------------------------------- 1. triangular solves, bitwise
@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("name", ge.FAMILIES)
def test_ordered_triangular_solves_are_bitwise_the_reference(S, po, pkg, name, kind):
    c = _case(name)
    got = _solves(S, po, pkg, name, kind)
    for forward in (True, False):
        ref = _reference(name, kind, forward, c.r0)
        assert np.array_equal(got[forward], ref), (name, kind, forward, max_rel(got[forward], ref))


@pytest.mark.parametrize("name", ["blocks", "q1_3d-1", "redblack", "shuffled"])
def test_the_identity_as_a_given_order_is_the_natural_order(S, po, name):
    c = _case(name)
    out = []
    for ordering in ("natural", np.arange(c.n)):
        ns = _two_level(S, po, c, S.SymGaussSeidelSmoother(2, 1.0, ordering), S.GaussSeidelSmoother(1, 0.9, "backward", ordering))
        try:
            x, r = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x, r, 0)
            x2, r2 = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x2, r2, 1)
            out.append((x, r, x2, r2, ns.gs_schedule(0, True), ns.gs_schedule(0, False), ns.sweep_signature(0)))
            o = ns.gs_ordering(0)
            assert (o["kind"], o["ncolors"]) == ("natural" if isinstance(ordering, str) else "given", 0)
            assert np.array_equal(o["order"], np.arange(c.n))
        finally:
            ns.close()
    for a, b in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(a, b)
    assert out[0][4:] == out[1][4:]


# ---------------------------------------------------------------- 2. the wide kernel where it can go wrong
@pytest.mark.parametrize("poison", [False, True], ids=["clean-dx", "nan-dx"])
def test_wide_kernel_on_ragged_slices_of_different_widths(S, po, pkg, poison):
    """3375 = 52 * 64 + 47 rows in the smallest colour: a ragged last slice and a part-filled last workgroup; boundary rows are
    shorter than interior ones, so slices differ in width and carry padded slots.  Backward, the padded slots of every set but the
    last gather dx[0] before row 0 (colour 0) is solved: over a poisoned dx the select must drop them."""
    c = _case(LEVEL32)
    sizes = np.bincount(go.multicolor(c.A)[1])
    assert c.n == 29791 and sizes.size == 8 and sizes.min() == 3375 and sizes.max() == 4096
    pattern, start = go.stored_pattern(_B(LEVEL32, "multicolor")), np.concatenate([[0], np.cumsum(sizes)])
    widths_differ = 0
    for tri in (sp.tril(pattern, -1), sp.triu(pattern, 1)):
        cnt = np.diff(tri.tocsr().indptr)
        slices = [[cnt[k:min(k + 64, start[q + 1])] for k in range(start[q], start[q + 1], 64)] for q in range(8)]
        assert any(s.max() != s.min() for w in slices for s in w)                     # padded slots, both ways
        widths_differ += sum(len({int(s.max()) for s in w}) > 1 for w in slices)
    assert widths_differ > 0                                                          # slices of one set with different widths
    got = _solves(S, po, pkg, LEVEL32, "multicolor", poison=poison)
    for forward in (True, False):
        ref = _reference(LEVEL32, "multicolor", forward, c.r0)
        assert np.array_equal(got[forward], ref), (forward, max_rel(got[forward], ref))


def test_plans_full_slices_chain_only_and_mixed(S, po, pkg):
    """redblack: two sets of 2048 rows, full slices only; q2_3d: 27 colours of 27 .. 512 rows, one chain launch; `blocks` reversed:
    the sets are the blocks reversed, chain and wide launches mixed.  Their solves are bitwise in test 1; here the plans."""
    for name, kind, want in (("redblack", "multicolor", dict(nsets=2, max_set_rows=2048, nlaunches=2, nwide=2)),
                             ("q2_3d", "multicolor", dict(nsets=27, max_set_rows=512, nlaunches=1, nwide=0)),
                             ("blocks", "reversed", dict(nsets=10, max_set_rows=2049, nlaunches=4, nwide=2))):
        c = _case(name)
        ns = _two_level(S, po, c, S.GaussSeidelSmoother(1, 1.0, "forward", _order(name, kind)[1]))
        try:
            assert ns.gs_schedule(0, True) == want, name
        finally:
            ns.close()
    sets = gr.level_sets(_B("blocks", "reversed"), True)
    assert tuple(np.bincount(sets)) == ge.BLOCK_SIZES[::-1] == (1, 5, 2049, 1025, 1024, 1023, 65, 64, 63, 1)
    sizes = np.bincount(go.multicolor(_case("q2_3d").A)[1])
    assert (sizes.min(), sizes.max()) == (27, 512)


# ---------------------------------------------------------------- 3. the folded update
def _forward_pass(S, po, name, kind, omega):
    """smooth of a forward smoother from x0 != 0, with gs_wide_kernel (1) and with the launches of the natural order (0) ->
    {gs_wide: (x, r, launches of the pass)}, schedule"""
    c = _case(name)
    ns = _two_level(S, po, c, S.GaussSeidelSmoother(1, omega, "forward", _order(name, kind)[1]))
    out = {}
    try:
        for wide in (1, 0):
            ns.set_option("gs_wide", wide)
            ns.profile(0)
            x, r = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x, r)
            out[wide] = (x, r, ns.kernel_stats()["launches"])
            ns.profile(0, False)
        sched = ns.gs_schedule(0, True)
    finally:
        ns.close()
    return out, sched


@pytest.mark.parametrize("name", ["redblack", LEVEL32])
def test_update_folds_into_the_wide_launches(S, po, name):
    c = _case(name)
    out, sched = _forward_pass(S, po, name, "multicolor", 1.0)
    assert sched["nlaunches"] == sched["nwide"] == (2 if name == "redblack" else 8)
    x, r, launches = out[1]
    assert np.array_equal(x, c.x0 + _reference(name, "multicolor", True, c.r0))
    assert launches == sched["nlaunches"]                     # no update launch
    assert out[0][2] == sched["nlaunches"] + 1                # the unfolded form: the same launches and the update
    assert np.array_equal(out[0][0], x) and np.array_equal(out[0][1], r)


def test_update_does_not_fold_at_omega_below_one_or_on_a_mixed_plan(S, po):
    for name, kind, omega in (("redblack", "multicolor", 0.9), (LEVEL32, "multicolor", 0.9), ("blocks", "reversed", 1.0)):
        c = _case(name)
        out, sched = _forward_pass(S, po, name, kind, omega)
        dx = omega * _reference(name, kind, True, c.r0)       # dx = w dx ; x += dx: one rounding each
        for wide in (1, 0):
            assert np.array_equal(out[wide][0], c.x0 + dx), (name, wide)
            assert out[wide][2] == sched["nlaunches"] + 1, (name, wide)
        assert np.array_equal(out[0][1], out[1][1])


def test_symmetric_pass_counts_both_directions(S, po):
    c = _case(LEVEL32)
    ns = _two_level(S, po, c, S.SymGaussSeidelSmoother(2, 1.0, "multicolor"), S.SymGaussSeidelSmoother(1, 1.2, "multicolor"))
    try:
        for which, want in ((0, 2 * (8 + 8)), (1, 8 + 1 + 8 + 1)):
            ns.profile(0)
            x, r = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x, r, which)
            assert ns.kernel_stats()["launches"] == want
    finally:
        ns.close()


# ---------------------------------------------------------------- 4. schedule and order
@pytest.mark.parametrize("name", ge.FAMILIES + (LEVEL32,))
def test_schedule_and_order_match_the_reference(S, po, name):
    c = _case(name)
    order, color = go.multicolor(c.A)
    B = _B(name, "multicolor")
    ns = _two_level(S, po, c, S.SymGaussSeidelSmoother(1, 1.0, "multicolor"))
    try:
        for forward in (True, False):
            want = dict(zip(("nsets", "max_set_rows", "nlaunches", "nwide"), gr.schedule(B, forward)))
            assert ns.gs_schedule(0, forward) == want
            if name in ("q1_3d-0", "q1_3d-1", LEVEL32):
                assert want["nsets"] == 8
            if name == "q1_2d":
                assert want["nsets"] == 4
            if name == LEVEL32:
                assert want["nlaunches"] == want["nwide"] == 8
        o = ns.gs_ordering(0)
        assert o["kind"] == "multicolor" and o["ncolors"] == color.max() + 1 and np.array_equal(o["order"], order)
        assert ns.sweep_signature(0).endswith(" gs=F+B")
    finally:
        ns.close()
    kind = "random"
    ns = _two_level(S, po, c, S.GaussSeidelSmoother(1, 1.0, "backward", _order(name, kind)[1]))
    try:
        assert ns.gs_schedule(0, False) == dict(zip(("nsets", "max_set_rows", "nlaunches", "nwide"), gr.schedule(_B(name, kind), False)))
        o = ns.gs_ordering(0)
        assert o["kind"] == "given" and o["ncolors"] == 0 and np.array_equal(o["order"], _order(name, kind)[0])
    finally:
        ns.close()


# ---------------------------------------------------------------- 5. whole passes, Krylov solvers and GMG
@pytest.mark.parametrize("name", ge.POISSON)
def test_whole_passes(S, po, pkg, name):
    c = _case(name)
    specs = {pkg.abi.PRE: (2, 1.0, "symmetric"), pkg.abi.POST: (3, 1.2, "backward")}
    ns = _two_level(S, po, c, *[S.GaussSeidelSmoother(*specs[w], ordering="multicolor") for w in (pkg.abi.PRE, pkg.abi.POST)])
    try:
        for which, spec in specs.items():
            x, r = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x, r, which)
            sm = go.OrderedGS(*spec, ordering="multicolor")
            xo, ro = c.x0.copy(), c.r0.copy()
            sm.smooth(sm.setup(c.A), xo, ro)
            ex, er = max_rel(x, xo), max_rel(r, ro)
            print(name, spec, "max_rel x %.2e r %.2e" % (ex, er))
            assert ex <= fr.TOL_KERNEL and er <= fr.TOL_KERNEL, (name, spec, ex, er)
    finally:
        ns.close()


def _device_smoother(S, spec):
    if spec[0] == "gs":
        return S.GaussSeidelSmoother(*spec[1:], ordering="multicolor")
    return S.RichardsonSmoother(S.JacobiLinearSolver(), *spec[1:])


def _agree(S, log, ref, rtol, x, tol=1e-10):
    xo, nit, hist = ref
    assert hist[-1] / hist[0] < rtol
    assert log.num_iters == nit and log.flag == S.SOLVER_CONVERGED_RTOL, (log.num_iters, nit, log.flag)
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= tol * hist[0])
    assert rel_err(x, xo) <= tol


@pytest.mark.parametrize("name", sorted(ge.KRYLOV))
def test_krylov_and_gmg_cases(S, po, hierarchy, name):
    c = ge.KRYLOV[name]
    H = hierarchy(c["nc"], c["nlev"])
    A, b = H["mats"][0], po.dirichlet_lift_rhs(c["nc"], 1)
    pre = _device_smoother(S, c["pre"])
    post = pre if c["post"] is c["pre"] else _device_smoother(S, c["post"])
    kw = dict(maxiter=100, atol=1e-14, rtol=c["rtol"])
    gkw = kw if c["solver"] == "gmg" else dict(maxiter=1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=[pre] * (c["nlev"] - 1),
                            post_smoothers=[post] * (c["nlev"] - 1), cycle_type=c["cycle"] + "_cycle",
                            mode="solver" if c["solver"] == "gmg" else "preconditioner", **gkw)
    if c["solver"] == "cg_smoother":
        solver = S.CGSolver((S.LinearSolverFromSmoother(gmg.pre_smoothers[0]), gmg), **kw)
    elif c["solver"] == "cg":
        solver = S.CGSolver(gmg, **kw)
    elif c["solver"] == "fgmres":
        solver = S.FGMRESSolver(5, gmg, **kw)
    else:
        solver = gmg
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    try:
        x = np.zeros(b.size)
        S.solve_(x, ns, b)
    finally:
        (ns if solver is gmg else ns.P_ns).close()
    ref = go.krylov_reference(name)
    assert ref[1] == go.KRYLOV_ITERS[name]
    _agree(S, solver.log, ref, c["rtol"], x)


# ---------------------------------------------------------------- 6. refresh
@pytest.mark.parametrize("kind", ["multicolor", "random"])
@pytest.mark.parametrize("options", [None, PLAIN_SELL], ids=["default-layout", "explicit-values"])
def test_value_refresh_is_bitwise_a_fresh_setup(S, po, options, kind):
    c = _case("q1_2d")
    arg = _order("q1_2d", kind)[1]
    pre, post = S.SymGaussSeidelSmoother(2, 1.2, arg), S.GaussSeidelSmoother(1, 1.0, "backward", arg)
    out = []
    for refreshed in (True, False):
        ns = _two_level(S, po, c, pre, post, scale=1.0 if refreshed else 1.7, options=options)
        try:
            before = (ns.gs_ordering(0), ns.gs_schedule(0, True), ns.gs_schedule(0, False))
            if refreshed:
                S.numerical_setup_(ns, _csr(po, c.A * 1.7), [_csr(po, c.A * 1.7), _csr(po, c.Ac * 1.7)])
                after = (ns.gs_ordering(0), ns.gs_schedule(0, True), ns.gs_schedule(0, False))
                assert before[1:] == after[1:] and before[0]["kind"] == after[0]["kind"] and before[0]["ncolors"] == after[0]["ncolors"]
                assert np.array_equal(before[0]["order"], after[0]["order"])
            dx = np.full(c.n, np.nan)
            ns.precond(0, c.r0, dx)
            x, r = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x, r, 1)
            out.append((dx, x, r, before[0]["order"], ns.gs_schedule(0, True), ns.gs_schedule(0, False)))
        finally:
            ns.close()
    for a, b in zip(out[0][:4], out[1][:4]):
        assert np.array_equal(a, b)
    assert out[0][4:] == out[1][4:]
    sm = go.OrderedGS(2, 1.2, "symmetric", _order("q1_2d", kind)[0])       # ... and those of the reference on the scaled matrix
    assert max_rel(out[0][0], sm.ldiv(sm.setup(c.A * 1.7), c.r0)) <= fr.TOL_KERNEL


# ---------------------------------------------------------------- 7. errors
def test_setter_and_getter_checks(S, po, pkg):
    abi = pkg.abi
    c = _case("q1_3d-1")
    ns = _two_level(S, po, c, S.SymGaussSeidelSmoother(1))
    try:
        lib, h, n = ns._lib, ns.h, c.n
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        good = np.arange(n, dtype=np.int32)[::-1].copy()
        twice, negative, beyond = good.copy(), good.copy(), good.copy()
        twice[40] = twice[7]
        negative[11] = -1
        beyond[5] = n
        for arr, length, where in ((good, n - 1, "position %d" % (n - 1)), (np.append(good, 0).astype(np.int32), n + 1, "position %d" % n),
                                   (twice, n, "position 40"), (negative, n, "position 11"), (beyond, n, "position 5")):
            assert lib.gmg_set_gs_ordering(h, 0, abi.GS_ORDER_GIVEN, ptr(arr), length) == abi.ERR_INVALID
            msg = lib.gmg_last_error(h).decode()
            assert "level 0" in msg and where in msg, msg
        assert lib.gmg_set_gs_ordering(h, 0, abi.GS_ORDER_GIVEN, None, n) == abi.ERR_INVALID
        for kind in (3, -1, 7):
            assert lib.gmg_set_gs_ordering(h, 0, kind, None, 0) == abi.ERR_INVALID
        for kind in (abi.GS_ORDER_NATURAL, abi.GS_ORDER_MULTICOLOR):
            assert lib.gmg_set_gs_ordering(h, 0, kind, ptr(good), n) == abi.ERR_INVALID
        assert lib.gmg_set_gs_ordering(h, 1, abi.GS_ORDER_MULTICOLOR, None, 0) == abi.ERR_INVALID      # the coarsest level
        dx = np.zeros(n)
        ns.precond(0, c.r0, dx)                               # the refused calls left the handle as it was
        assert max_rel(dx, gr.ldiv(gr.GS().setup(c.A.copy()), gr.GS(), c.r0)) <= fr.TOL_KERNEL
        assert ns.gs_ordering(0)["kind"] == "natural"
        kind, nc, room = C.c_int(-1), C.c_int64(-1), np.zeros(n, dtype=np.int32)
        assert lib.gmg_get_gs_ordering(h, 0, C.byref(kind), C.byref(nc), ptr(room), n - 1) == abi.ERR_INVALID
        assert lib.gmg_get_gs_ordering(h, 0, C.byref(kind), C.byref(nc), None, 0) == abi.OK and (kind.value, nc.value) == (0, 0)
        assert lib.gmg_get_gs_ordering(h, 1, C.byref(kind), C.byref(nc), None, 0) == abi.ERR_INVALID
        # a legal call takes effect at the next gmg_setup
        assert lib.gmg_set_gs_ordering(h, 0, abi.GS_ORDER_GIVEN, ptr(good), n) == abi.OK
        with pytest.raises(abi.GmgError) as e:
            ns.gs_ordering(0)
        assert e.value.code == abi.ERR_STATE
        ns.setup()
        o = ns.gs_ordering(0)
        assert o["kind"] == "given" and np.array_equal(o["order"], good)
    finally:
        ns.close()


def test_one_order_per_level(S, po):
    c = _case("q1_3d-1")
    rev = np.arange(c.n)[::-1]
    for pre, post in ((S.SymGaussSeidelSmoother(1, 1.0, "multicolor"), S.SymGaussSeidelSmoother(1)),
                      (S.SymGaussSeidelSmoother(1, 1.0, rev), S.SymGaussSeidelSmoother(1, 1.0, "multicolor")),
                      (S.SymGaussSeidelSmoother(1, 1.0, rev), S.GaussSeidelSmoother(1, 1.0, "forward", np.arange(c.n)))):
        with pytest.raises(ValueError):
            _two_level(S, po, c, pre, post)
    jac = S.RichardsonSmoother(S.JacobiLinearSolver(), 2, 2.0 / 3.0)
    ns = _two_level(S, po, c, jac, S.SymGaussSeidelSmoother(1, 1.0, rev))     # one of them Gauss-Seidel: its order is the level's
    try:
        assert ns.gs_ordering(0)["kind"] == "given"
    finally:
        ns.close()
    ns = _two_level(S, po, c, S.SymGaussSeidelSmoother(1, 1.0, rev), S.GaussSeidelSmoother(2, 0.9, "backward", rev.copy()))
    ns.close()


def test_an_order_on_a_jacobi_level_is_inert(S, po, pkg):
    abi = pkg.abi
    c = _case("q1_2d")
    jac = S.RichardsonSmoother(S.JacobiLinearSolver(), 2, 2.0 / 3.0)
    out = []
    for ordered in (False, True):
        ns = _two_level(S, po, c, jac)
        try:
            if ordered:
                abi.check(ns.h, ns._lib.gmg_set_gs_ordering(ns.h, 0, abi.GS_ORDER_MULTICOLOR, None, 0))
                ns.setup()
                with pytest.raises(abi.GmgError) as e:
                    ns.gs_ordering(0)
                assert e.value.code == abi.ERR_STATE
            x, r = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x, r)
            out.append((x, r, ns.sweep_signature(0), ns.device_bytes()))
        finally:
            ns.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2:] == out[1][2:] and " gs=" not in out[0][2]
