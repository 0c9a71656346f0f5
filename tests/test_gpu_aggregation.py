"""Smoothed-aggregation prolongations on the device (csrc/aggregation.inc.hpp, kernels.hpp agg_*) against the numpy twin
(tests/aggregation_reference.py).

1. bits: aggregates, rounds, rho, omega, P and the Galerkin matrix of the next level == the twin
2. matrices that are refused by name: zero diagonal, nonsymmetric pattern, a level that does not coarsen
3. solves on Q1 16^3, three algebraic levels, against the numpy composition; a mixed geometric / algebraic hierarchy
4. refresh: update(2 A0), update(A0') against the twin with the aggregates frozen, device bytes
5. refusals
6. a handle without Aggregation() computes what it computed before"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import aggregation_reference as ar
import chebyshev_reference as cr
import galerkin_reference as gal
import numpy_twin as nt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _jacobi(S, nlev):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0) for _ in range(nlev - 1)]


@functools.lru_cache(maxsize=None)
def _matrix(name):
    import __graft_entry__ as entry
    po = entry.import_package().poisson
    if name.startswith("chain"):
        return ar.chain(int(name[5:]))
    if name == "nonsym":
        return ar.nonsymmetric_values()
    if name in ("kappa_6x3", "kappa_16x3"):
        A = po.poisson_matrix_varcoef((6, 6, 6) if name == "kappa_6x3" else (16, 16, 16), po.smooth_kappa)
        return ar.M(A.shape, A.ptr, A.idx, A.val)
    nc, order, lengths = {"q1_8x2": ((8, 8), 1, None), "q1_9x8": ((9, 8), 1, None), "q1_6x3": ((6, 6, 6), 1, None),
                          "q2_4x3": ((4, 4, 4), 2, None), "aniso": ((8, 8), 1, (1.0, 0.1)), "q1_16x3": ((16, 16, 16), 1, None)}[name.split("+")[0]]
    A = po.poisson_matrix(nc, order, lengths=lengths)
    A = ar.M(A.shape, A.ptr, A.idx, A.val)
    if name.endswith("+isolated"):
        A = ar.with_isolated_rows(A, (A.shape[0] // 2, A.shape[0] - 1))
    if name.endswith("+zero"):
        A = ar.with_zero_row(A, A.shape[0] // 2)
    return A


@functools.lru_cache(maxsize=None)
def _twin(name, nlev, theta=0.25, smooth=True, omega=None, seed=0):
    """-> (mats, Ps, infos) of the twin; computed once, shared and left unchanged"""
    return ar.hierarchy(_matrix(name), nlev, theta=theta, smooth=smooth, omega=omega, seed=seed)


def _agg_ns(S, A0, nlev, sm=None, solver=None, **kw):
    """a handle with algebraic levels only; solver(gmg) wraps the GMG in a Krylov solver -> (outer solver, its setup, the GMG's setup)"""
    sm = _jacobi(S, nlev) if sm is None else sm
    cycle = kw.pop("cycle_type", "v_cycle")
    g = S.GMGLinearSolver([A0] + [S.Galerkin() for _ in range(nlev - 1)], [S.Aggregation(**kw) for _ in range(nlev - 1)],
                          pre_smoothers=sm, post_smoothers=sm, maxiter=1, cycle_type=cycle)
    top = g if solver is None else solver(g)
    ns = S.numerical_setup(S.symbolic_setup(top, A0), A0)
    return top, ns, (ns if solver is None else ns.P_ns)


def _same_level(gns, lev, info, want_next):
    agg, nagg = gns.aggregates(lev)
    assert agg.dtype == np.int32 and nagg == info["nagg"] and np.array_equal(agg, info["agg"]), f"aggregates of level {lev}"
    got = gns.aggregation_info(lev)
    assert got["rounds"] == info["rounds"], (got["rounds"], info["rounds"])
    assert got["rho"] == info["rho"] and got["omega"] == info["omega"], (got, info["rho"], info["omega"])
    assert got["strong_edges"] == info["strong_edges"]
    shape, ptr, idx, val = gns.prolongation(lev)
    P = info["P"]
    assert shape == P.shape and ptr.dtype == np.int64 and idx.dtype == np.int32
    assert np.array_equal(ptr, P.ptr) and np.array_equal(idx, P.idx), f"pattern of P of level {lev}"
    assert np.array_equal(val, P.val), f"values of P of level {lev}: max diff {np.max(np.abs(val - P.val)):.3e}"
    shape, ptr, idx, val = gns.level_matrix(lev + 1)
    assert shape == want_next.shape and np.array_equal(ptr, want_next.ptr) and np.array_equal(idx, want_next.idx)
    assert np.array_equal(val, want_next.val), f"Galerkin matrix of level {lev + 1}: max diff {np.max(np.abs(val - want_next.val)):.3e}"
    assert gns.level_size(lev + 1) == info["nagg"] == gns.sizes[lev + 1]


# ---------------------------------------------------------------- 1. bits
BIT_CASES = [("chain2", {}), ("chain3", {}), ("chain17", {}), ("chain64", {}), ("chain65", {}), ("chain129", {}),
             ("q1_8x2", {}), ("q1_9x8", {}), ("q1_6x3", {}), ("q2_4x3", {}), ("aniso", {}), ("aniso", dict(theta=0.75)),
             ("q1_8x2", dict(theta=0.0)), ("q1_8x2", dict(theta=1.0)), ("q1_8x2+isolated", {}), ("q1_8x2+zero", {}), ("nonsym", {}),
             ("q1_8x2", dict(smooth=False)), ("q1_6x3", dict(omega=0.5)), ("q1_8x2", dict(seed=1)), ("q1_6x3", dict(seed=1))]


@pytest.mark.parametrize("name,kw", BIT_CASES, ids=[n + "".join(f"-{k}{v}" for k, v in kw.items()) for n, kw in BIT_CASES])
def test_bits_two_levels(S, name, kw):
    """one aggregated level over every small matrix: rows across wave boundaries (65, 129), stored zeros, diagonal-only rows, a row
    whose off-diagonal entries are all 0.0, one-sided strength, rows of 125 entries (Q2 4^3)"""
    A0 = _matrix(name)
    mats, _Ps, infos = _twin(name, 2, **kw)
    if name == "q2_4x3":
        assert np.diff(A0.ptr).max() == 125
    if name == "q1_6x3":
        rows = np.repeat(np.arange(A0.shape[0]), np.diff(A0.ptr))
        assert np.any((A0.val == 0.0) & (rows != A0.idx))     # the stored zero face couplings
    _top, ns, gns = _agg_ns(S, A0, 2, **kw)
    try:
        _same_level(gns, 0, infos[0], mats[1])
        if kw.get("omega"):
            assert gns.aggregation_info(0)["omega"] == kw["omega"]
    finally:
        ns.close()


@pytest.mark.parametrize("name", ("q1_6x3", "q2_4x3", "chain129"))
def test_bits_three_levels(S, name):
    """the second aggregation reads the Galerkin product just formed"""
    A0 = _matrix(name)
    mats, _Ps, infos = _twin(name, 3)
    _top, ns, gns = _agg_ns(S, A0, 3)
    try:
        for l in (0, 1):
            _same_level(gns, l, infos[l], mats[l + 1])
        assert gns.sizes == [m.shape[0] for m in mats]
    finally:
        ns.close()


# ---------------------------------------------------------------- 2. matrices refused by name
def _raw_handle(S, pkg, A0, nlev=2, **kw):
    """a handle built through the C entry points alone (the Python constructor refuses much of this before a handle exists)"""
    abi, lib = pkg.abi, pkg.abi.load()
    h = C.c_void_p()
    abi.check(None, lib.gmg_create(C.byref(h), nlev, 0))
    S._set_op(lib.gmg_set_matrix, h, 0, A0)
    for l in range(nlev - 1):
        abi.check(h, lib.gmg_set_aggregation(h, l, kw.get("theta", 0.25), 1, 0.0, kw.get("seed", 0)))
        abi.check(h, lib.gmg_set_galerkin(h, l + 1))
        abi.check(h, lib.gmg_set_smoother_jacobi(h, l, abi.PRE_AND_POST, 10, 2.0 / 3.0))
    return lib, h


def test_single_row_does_not_coarsen(S, pkg):
    """n = 1: one round, one root, one aggregate -- and a level that does not coarsen is refused by name; the aggregates stay readable"""
    abi = pkg.abi
    A0 = ar.chain(1)
    info = ar.build(A0)
    lib, h = _raw_handle(S, pkg, A0)
    try:
        assert lib.gmg_setup(h) == abi.ERR_UNSUPPORTED
        msg = lib.gmg_last_error(h)
        assert b"level 0" in msg and b"does not coarsen" in msg
        nagg, agg, rounds = C.c_int64(), np.full(1, -1, dtype=np.int32), C.c_int()
        abi.check(h, lib.gmg_get_aggregates(h, 0, C.byref(nagg), _p(agg), 1))
        abi.check(h, lib.gmg_get_aggregation_info(h, 0, C.byref(rounds), None, None, None, None))
        assert nagg.value == info["nagg"] == 1 and np.array_equal(agg, info["agg"]) and rounds.value == info["rounds"] == 1
        assert lib.gmg_setup(h) == abi.ERR_UNSUPPORTED       # and again: the same answer, nothing half-built is used
    finally:
        lib.gmg_destroy(h)


def test_zero_diagonal_and_nonsymmetric_pattern(S, pkg):
    abi = pkg.abi
    A = ar.chain(70)
    rows = np.repeat(np.arange(70), np.diff(A.ptr))
    val = A.val.copy()
    val[(rows == 66) & (A.idx == 66)] = 0.0
    val[(rows == 3) & (A.idx == 3)] = 0.0
    lib, h = _raw_handle(S, pkg, ar.M(A.shape, A.ptr, A.idx, val))
    try:
        assert lib.gmg_setup(h) == abi.ERR_SINGULAR
        assert b"level 0" in lib.gmg_last_error(h) and b"row 3 " in lib.gmg_last_error(h)            # the first one
    finally:
        lib.gmg_destroy(h)
    Sp = A.to_scipy().tolil()
    Sp[68, 2] = 0.5
    Sp[1, 4] = 0.5
    lib, h = _raw_handle(S, pkg, ar.from_scipy(Sp.tocsr()))
    try:
        assert lib.gmg_setup(h) == abi.ERR_INVALID
        assert b"level 0" in lib.gmg_last_error(h) and b"(1, 4)" in lib.gmg_last_error(h)            # the first offending pair
    finally:
        lib.gmg_destroy(h)


# ---------------------------------------------------------------- 3. solves
def _twin_gmg(mats, Ps, smoother, cycle):
    sms = [cr.Cheb("jacobi", 3) if smoother == "chebyshev" else cr.Rich("jacobi", 10, 2.0 / 3.0) for _ in Ps]
    return cr.GMG(mats, Ps, [gal.transpose(P) for P in Ps], sms, cycle=cycle)


def _device_smoothers(S, smoother, nlev):
    if smoother == "chebyshev":
        return [S.ChebyshevSmoother(S.JacobiLinearSolver(), 3) for _ in range(nlev - 1)]
    return _jacobi(S, nlev)


def _check_solve(name, log, x, b, A0, want, rtol):
    xo, nit, hist = want
    res = np.asarray(log.residuals[: log.num_iters + 1])
    true_res = np.linalg.norm(b - A0.to_scipy() @ x) / np.linalg.norm(b)
    print(f"{name}: iterations {log.num_iters}, twin {nit}; max rel diff of the history "
          f"{np.max(np.abs(res[: nit + 1] - hist[: res.size]) / hist[: res.size]) if res.size == hist.size else float('nan'):.3e}; "
          f"|x - twin| / |twin| = {np.linalg.norm(x - xo) / np.linalg.norm(xo):.3e}; |b - A x| / |b| = {true_res:.3e}")
    assert log.num_iters == nit and log.flag == 1            # SOLVER_CONVERGED_RTOL
    assert np.all(np.abs(res - hist) <= 1e-8 * hist)
    assert np.linalg.norm(x - xo) <= 1e-10 * np.linalg.norm(xo)
    assert true_res <= rtol


@pytest.mark.parametrize("smoother,krylov", (("jacobi", "cg"), ("jacobi", "fgmres-w"), ("chebyshev", "cg")))
def test_solves_on_three_algebraic_levels(S, po, smoother, krylov):
    """Q1 16^3, [A0, Galerkin(), Galerkin()] and [Aggregation(), Aggregation()]: iteration count, residual history and x against the
    composition of the numpy GMG with the twin's P and the twin's Galerkin matrices.  The count is whatever that composition gives."""
    A0 = _matrix("q1_16x3")
    mats, Ps, infos = _twin("q1_16x3", 3)
    b = po.random_rhs(A0.shape[0])
    rtol = 1e-8
    kw = dict(maxiter=60, atol=1e-14, rtol=rtol)
    cycle = "w" if krylov == "fgmres-w" else "v"
    wrap = (lambda g: S.CGSolver(g, **kw)) if krylov == "cg" else (lambda g: S.FGMRESSolver(5, g, **kw))
    top, ns, gns = _agg_ns(S, A0, 3, sm=_device_smoothers(S, smoother, 3), solver=wrap, cycle_type=cycle + "_cycle")
    try:
        for l in (0, 1):
            _same_level(gns, l, infos[l], mats[l + 1])
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
    finally:
        ns.close()
    G = _twin_gmg(mats, Ps, smoother, cycle)
    As = A0.to_scipy().tocsr()
    want = nt.cg(As, b, Pl=G.solve, **kw) if krylov == "cg" else nt.fgmres(As, b, Pr=G.solve, m=5, **kw)
    _check_solve(f"{smoother} / {krylov}", top.log, x, b, A0, want, rtol)


def test_mixed_hierarchy(S, po, hierarchy):
    """Q1 16^3: a geometric P0 and the caller's A1, two aggregated levels below them"""
    H = hierarchy((16, 16, 16), 2, 1)
    A0, A1, P0 = H["mats"][0], H["mats"][1], H["prolongations"][0]
    A1m = ar.M(A1.shape, A1.ptr, A1.idx, A1.val)
    lower, lowerP, infos = ar.hierarchy(A1m, 3)
    mats, Ps = [A0] + lower, [P0] + lowerP
    b = po.random_rhs(A0.shape[0])
    kw = dict(maxiter=60, atol=1e-14, rtol=1e-8)
    sm = _jacobi(S, 4)
    g = S.GMGLinearSolver([A0, A1, S.Galerkin(), S.Galerkin()], [P0, S.Aggregation(), S.Aggregation()], pre_smoothers=sm, post_smoothers=sm,
                          maxiter=1)
    cg = S.CGSolver(g, **kw)
    ns = S.numerical_setup(S.symbolic_setup(cg, A0), A0)
    try:
        for l in (1, 2):
            _same_level(ns.P_ns, l, infos[l - 1], mats[l + 1])
        assert ns.P_ns.sizes == [m.shape[0] for m in mats]
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
    finally:
        ns.close()
    G = cr.GMG(mats, Ps, [gal.transpose(ar.M(P.shape, P.ptr, P.idx, P.val)) for P in Ps], [cr.Rich("jacobi", 10, 2.0 / 3.0) for _ in Ps])
    _check_solve("mixed", cg.log, x, b, A0, nt.cg(A0.to_scipy().tocsr(), b, Pl=G.solve, **kw), 1e-8)


# ---------------------------------------------------------------- 4. refresh
def test_update_keeps_the_aggregates(S, po):
    """update(2 A0): aggregates and P bitwise unchanged, the Galerkin matrices doubled; update(A0') with relative perturbations of 1e-6:
    the twin with the aggregates frozen; the device byte count does not move; the handle then solves like a fresh one given A0'.
    A0 is the variable-coefficient Q1 6^3 matrix: its layout stores every value, so new values do not change the layout of A0 itself
    (a constant-coefficient matrix is held as a few row patterns, and perturbing it changes that layout with or without aggregation)."""
    A0 = _matrix("kappa_6x3")
    mats, _Ps, infos = _twin("kappa_6x3", 3)
    rng = np.random.default_rng(7)
    Ap = ar.M(A0.shape, A0.ptr, A0.idx, A0.val * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, A0.val.size)))
    b = po.random_rhs(A0.shape[0])
    _top, ns, gns = _agg_ns(S, A0, 3)
    fresh = None
    try:
        nbytes = gns.device_bytes()
        before = [(gns.aggregates(l), gns.prolongation(l), gns.level_matrix(l + 1)) for l in (0, 1)]
        S.numerical_setup_(ns, ar.M(A0.shape, A0.ptr, A0.idx, 2.0 * A0.val))
        assert gns.device_bytes() == nbytes
        for l in (0, 1):
            (agg, nagg), (ps, pp, pi, pv), (ms, mp, mi, mv) = before[l]
            assert np.array_equal(gns.aggregates(l)[0], agg) and gns.aggregates(l)[1] == nagg
            s2, p2, i2, v2 = gns.prolongation(l)
            assert s2 == ps and np.array_equal(p2, pp) and np.array_equal(i2, pi) and np.array_equal(v2, pv)
            s2, p2, i2, v2 = gns.level_matrix(l + 1)
            assert s2 == ms and np.array_equal(p2, mp) and np.array_equal(i2, mi) and np.array_equal(v2, 2.0 * mv)
        S.numerical_setup_(ns, Ap)
        assert gns.device_bytes() == nbytes
        fmats, _fPs, finfos = ar.hierarchy(Ap, 3, frozen=infos)
        for l in (0, 1):
            _same_level(gns, l, finfos[l], fmats[l + 1])
            assert not np.array_equal(finfos[l]["P"].val, infos[l]["P"].val)
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
        # a fresh handle given A0' and the frozen prolongations as the caller's: the same cycle
        g = S.GMGLinearSolver([Ap, S.Galerkin(), S.Galerkin()], [f["P"] for f in finfos], pre_smoothers=_jacobi(S, 3),
                              post_smoothers=_jacobi(S, 3), maxiter=1)
        fresh = S.numerical_setup(S.symbolic_setup(g, Ap), Ap)
        xf = np.zeros_like(b)
        S.solve_(xf, fresh, b)
        assert np.all(np.isfinite(x)) and np.linalg.norm(x) > 0 and np.array_equal(x, xf)
    finally:
        ns.close()
        if fresh is not None:
            fresh.close()


def test_update_in_place_on_explicit_layouts(S, po):
    """variable-coefficient Q1 16^3, two levels: A0, P0 and R0 = P0^T are all stored with explicit values (3375 distinct rows), the
    case in which the new values of P and R are written into the kept layouts; the result is the twin with the aggregates frozen and
    the solve of a fresh handle given A0' and that P"""
    A0 = _matrix("kappa_16x3")
    _mats, _Ps, infos = _twin("kappa_16x3", 2)
    rng = np.random.default_rng(7)
    Ap = ar.M(A0.shape, A0.ptr, A0.idx, A0.val * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, A0.val.size)))
    b = po.random_rhs(A0.shape[0])
    _top, ns, gns = _agg_ns(S, A0, 2)
    fresh = None
    try:
        nbytes, fmt = gns.device_bytes(), [gns.level_format(l) for l in (0, 1)]
        assert not fmt[0]["row_patterns"] and not fmt[0]["value_dictionary"]
        S.numerical_setup_(ns, Ap)
        assert gns.device_bytes() == nbytes and [gns.level_format(l) for l in (0, 1)] == fmt
        fmats, _fPs, finfos = ar.hierarchy(Ap, 2, frozen=infos)
        _same_level(gns, 0, finfos[0], fmats[1])
        assert not np.array_equal(finfos[0]["P"].val, infos[0]["P"].val)
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
        g = S.GMGLinearSolver([Ap, S.Galerkin()], [finfos[0]["P"]], pre_smoothers=_jacobi(S, 2), post_smoothers=_jacobi(S, 2), maxiter=1)
        fresh = S.numerical_setup(S.symbolic_setup(g, Ap), Ap)
        xf = np.zeros_like(b)
        S.solve_(xf, fresh, b)
        assert np.all(np.isfinite(x)) and np.linalg.norm(x) > 0 and np.array_equal(x, xf)
    finally:
        ns.close()
        if fresh is not None:
            fresh.close()


def test_set_matrix_aggregates_afresh(S, pkg):
    """gmg_set_matrix with another structure on an aggregated handle: new aggregates, new sizes"""
    A0, B0 = _matrix("q1_8x2"), _matrix("q1_9x8")
    _top, ns, gns = _agg_ns(S, A0, 2)
    try:
        _same_level(gns, 0, _twin("q1_8x2", 2)[2][0], _twin("q1_8x2", 2)[0][1])
        S._set_op(ns._lib.gmg_set_matrix, ns.h, 0, B0)
        ns.setup()
        gns.sizes = [B0.shape[0], gns.level_size(1)]
        _same_level(gns, 0, _twin("q1_9x8", 2)[2][0], _twin("q1_9x8", 2)[0][1])
    finally:
        ns.close()


# ---------------------------------------------------------------- 5. refusals
def test_refused_at_setup(S, po, pkg):
    """every refusal of gmg_setup names the level; where the cause can be withdrawn the handle sets up again"""
    abi = pkg.abi
    A0 = _matrix("q1_8x2")
    mats, Ps, infos = _twin("q1_8x2", 3)
    P0 = Ps[0]

    def refused(h, lib, code, *words):
        assert lib.gmg_setup(h) == code, lib.gmg_last_error(h)
        msg = lib.gmg_last_error(h).decode()
        assert all(w in msg for w in words), msg

    lib, h = _raw_handle(S, pkg, A0, 3)
    try:
        abi.check(h, lib.gmg_setup(h))
        # level lev + 1 not marked with gmg_set_galerkin
        S._set_op(lib.gmg_set_matrix, h, 1, mats[1])
        refused(h, lib, abi.ERR_INVALID, "level 0", "level 1 is not marked with gmg_set_galerkin")
        abi.check(h, lib.gmg_set_galerkin(h, 1))
        abi.check(h, lib.gmg_setup(h))
        # an explicit restriction on the level
        S._set_op(lib.gmg_set_restriction, h, 0, gal.transpose(P0))
        refused(h, lib, abi.ERR_UNSUPPORTED, "level 0", "restriction")
    finally:
        lib.gmg_destroy(h)
    # a level matrix streamed with gmg_set_operator_rows
    lib, h = _raw_handle(S, pkg, A0, 2)
    try:
        ptr, idx = A0.ptr.astype(np.int64), A0.idx.astype(np.int64)
        abi.check(h, lib.gmg_set_operator_rows(h, 0, abi.OP_A, A0.shape[0], A0.shape[1], 0, A0.shape[0], _p(ptr), _p(idx), _p(A0.val), 0, 8))
        refused(h, lib, abi.ERR_UNSUPPORTED, "level 0", "streamed")
        S._set_op(lib.gmg_set_matrix, h, 0, A0)
        abi.check(h, lib.gmg_setup(h))
        # a patch-corrected prolongation on the level
        pp, pd = po.coarse_cell_interior_patches((4, 4), 1)
        pp, pd = np.ascontiguousarray(pp, dtype=np.int64), np.ascontiguousarray(pd, dtype=np.int64)
        abi.check(h, lib.gmg_set_prolongation_patch_correction(h, 0, 0, pp.size - 1, _p(pp), _p(pd), 0, 8))
        refused(h, lib, abi.ERR_UNSUPPORTED, "level 0", "patch-corrected")
    finally:
        lib.gmg_destroy(h)
    # a patch-based smoother on a level whose size comes from aggregation
    lib, h = _raw_handle(S, pkg, A0, 3)
    try:
        pp, pd = np.array([0, 2], dtype=np.int64), np.array([0, 1], dtype=np.int64)
        abi.check(h, lib.gmg_set_smoother_patch(h, 1, abi.PRE_AND_POST, 2, 0.5, 0, 1, _p(pp), _p(pd), 0, 8))
        refused(h, lib, abi.ERR_UNSUPPORTED, "level 1", "aggregation of level 0", "patch")
    finally:
        lib.gmg_destroy(h)
    # values_f32 refuses the Galerkin level below
    lib, h = _raw_handle(S, pkg, A0, 2)
    try:
        abi.check(h, lib.gmg_set_option(h, b"values_f32", 1.0))
        refused(h, lib, abi.ERR_INVALID, "level 1", "float32")
    finally:
        lib.gmg_destroy(h)
    # a communicator of two ranks (loopback)
    lib, h = _raw_handle(S, pkg, A0, 2)
    try:
        xfn = abi.HOST_EXCHANGE_FN(lambda *a: None)
        rfn = abi.HOST_ALLREDUCE_FN(lambda *a: None)
        abi.check(h, lib.gmg_comm_init_host(h, 0, 1, C.cast(xfn, C.c_void_p), C.cast(rfn, C.c_void_p), None))
        abi.check(h, lib.gmg_comm_set_loopback(h, 2))
        refused(h, lib, abi.ERR_UNSUPPORTED, "level 0", "communicator")
    finally:
        lib.gmg_destroy(h)


def test_entry_points_refuse_bad_arguments(S, pkg):
    abi = pkg.abi
    A0 = _matrix("q1_8x2")
    _top, ns, gns = _agg_ns(S, A0, 2)
    lib, h = ns._lib, ns.h
    try:
        assert lib.gmg_set_aggregation(h, 1, 0.25, 1, 0.0, 0) == abi.ERR_INVALID          # the coarsest level has no prolongation
        assert lib.gmg_set_aggregation(h, 0, 1.5, 1, 0.0, 0) == abi.ERR_INVALID
        assert lib.gmg_set_aggregation(h, 0, 0.25, 1, 0.0, -1) == abi.ERR_INVALID
        agg, nagg = np.zeros(A0.shape[0], dtype=np.int32), C.c_int64()
        assert lib.gmg_get_aggregates(h, 0, C.byref(nagg), _p(agg), agg.size - 1) == abi.ERR_INVALID
        nnz = C.c_int64()
        abi.check(h, lib.gmg_get_prolongation(h, 0, None, None, C.byref(nnz), None, None, None, 0, 0))
        val = np.zeros(nnz.value)
        assert lib.gmg_get_prolongation(h, 0, None, None, None, None, None, _p(val), 0, nnz.value - 1) == abi.ERR_INVALID
        abi.check(h, lib.gmg_get_prolongation(h, 0, None, None, None, None, None, _p(val), 0, nnz.value))
        assert np.array_equal(val, _twin("q1_8x2", 2)[1][0].val)
    finally:
        ns.close()
    # a handle without the marker has no aggregates to give
    H = S.GMGLinearSolver([A0, S.Galerkin()], [_twin("q1_8x2", 2)[1][0]], pre_smoothers=_jacobi(S, 2), post_smoothers=_jacobi(S, 2), maxiter=1)
    ns = S.numerical_setup(S.symbolic_setup(H, A0), A0)
    try:
        with pytest.raises(abi.GmgError) as e:
            ns.aggregates(0)
        assert e.value.code == abi.ERR_STATE and "level 0" in str(e.value)
        assert ns.level_size(1) == _twin("q1_8x2", 2)[0][1].shape[0]
    finally:
        ns.close()


# ---------------------------------------------------------------- 6. guard
@pytest.mark.parametrize("cyc", ("v", "w"))
def test_handle_without_the_marker_is_unchanged(S, hierarchy, cyc):
    """one cycle of a handle without Aggregation() on the Q1 16^3 problem of the committed q1_16cubed fixture: the bits the device gave
    on the commit before aggregation existed (tests/golden/q1_16cubed_device_cycles.npz, recorded there on an MI355X with the input
    below), and the fixture's own oracle result within the bound of test_gpu_parity.py"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "q1_16cubed.npz"))
    bits = np.load(os.path.join(ROOT, "tests", "golden", "q1_16cubed_device_cycles.npz"))
    H = hierarchy((16, 16, 16), 3)
    n = H["mats"][0].shape[0]
    r = np.random.Generator(np.random.MT19937(11)).uniform(-1.0, 1.0, n)
    g = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=_jacobi(S, 3), post_smoothers=_jacobi(S, 3), maxiter=1,
                          cycle_type=cyc + "_cycle")
    ns = S.numerical_setup(S.symbolic_setup(g, H["mats"][0]), H["mats"][0])
    try:
        z = np.zeros(n)
        S.solve_(z, ns, r)
    finally:
        ns.close()
    assert np.linalg.norm(z - gold["z_" + cyc]) <= 1e-11 * np.linalg.norm(gold["z_" + cyc])
    assert np.array_equal(z, bits["z_" + cyc])
