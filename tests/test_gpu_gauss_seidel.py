"""GaussSeidelSmoother / SymGaussSeidelSmoother on the device (csrc/gs.inc.hpp) against the numpy transcription of the reference
(tests/gs_reference.py) on the families of tests/gs_edge_problems.py.

1. triangular solves: precond (= ldiv!, niter 1, one direction) is BITWISE the reference's column-oriented loops on every family
2. gmg_get_gs_schedule reports the sets and launches of gs_reference.schedule
3. whole passes (smooth) on the Poisson families within the project's per-kernel gate (r -= A dx sums in another order than numpy)
4. the reference's own test, SmoothersTests.jl:46-56, and 5. GMG with these smoothers under CG / FGMRES / W-cycle / solver mode:
   iteration count and flag equal to the numpy reference, history within 1e-10 hist[0], solution within 1e-10 relative
6. value refresh is bitwise a fresh setup   7. errors"""
import itertools

import numpy as np
import pytest

import fullsize_reference as fr
import gs_edge_problems as ge
import gs_reference as gr
from conftest import max_rel, rel_err

pytestmark = pytest.mark.gpu

PLAIN_SELL = dict(pattern=0, vdict=0, idx16=0, opattern=0)   # a layout that stores explicit values: gmg_setup refreshes in place


def _csr(po, M):
    return po.CSR(M.shape, M.indptr, M.indices, M.data)      # raw: `shuffled` keeps its storage order


def _two_level(S, po, c, pre, post=None, scale=1.0, options=None):
    post = pre if post is None else post
    gmg = S.GMGLinearSolver([_csr(po, c.A * scale), _csr(po, c.Ac * scale)], [_csr(po, c.P)], [_csr(po, c.R)], pre_smoothers=[pre],
                            post_smoothers=[post], maxiter=1, mode="preconditioner", options=options)
    A = gmg.smatrices[0]
    if scale != 1.0 or c.name == "shuffled":                  # (scipy's scalar product keeps the storage order)
        assert np.array_equal(A.idx, c.A.indices)
    return S.numerical_setup(S.symbolic_setup(gmg, A), A)


def _one_direction(S, po, c, forward, omega, r, device=False):
    """precond of a one-direction, one-iteration smoother on a fresh handle -> (device result, reference ldiv!)"""
    kind = "forward" if forward else "backward"
    ns = _two_level(S, po, c, S.GaussSeidelSmoother(1, omega, kind))
    try:
        if device:
            import torch
            dx = torch.full((c.n,), float("nan"), dtype=torch.float64, device="cuda")
            ns.precond(0, torch.from_numpy(r).cuda(), dx)
            torch.cuda.synchronize()
            dx = dx.cpu().numpy()
        else:
            dx = np.full(c.n, np.nan)
            ns.precond(0, r, dx)
        sig = ns.sweep_signature(0)
    finally:
        ns.close()
    assert sig.endswith(" gs=F" if forward else " gs=B"), sig
    sm = gr.GS(1, omega, kind)
    return dx, gr.ldiv(sm.setup(gr.csr(c.A)), sm, r)


# ---------------------------------------------------------------- 1. triangular solves, bitwise
@pytest.mark.parametrize("name", ge.FAMILIES)
def test_triangular_solves_are_bitwise_the_reference(S, po, name):
    c = ge.case(name)
    for forward, omega in itertools.product((True, False), (1.0, 0.9)):
        dx, ref = _one_direction(S, po, c, forward, omega, c.r0)
        assert np.array_equal(dx, ref), (name, forward, omega, max_rel(dx, ref))


def test_triangular_solves_on_device_tensors_and_in_any_storage_order(S, po):
    b, s = ge.case("blocks"), ge.case("shuffled")
    for forward in (True, False):
        dx, ref = _one_direction(S, po, b, forward, 0.9, b.r0, device=True)
        assert np.array_equal(dx, ref)
        dxs, _ = _one_direction(S, po, s, forward, 0.9, b.r0)
        assert np.array_equal(dxs, dx)


# ---------------------------------------------------------------- 2. schedule
@pytest.mark.parametrize("name", ge.FAMILIES)
def test_schedule_matches_the_reference(S, po, pkg, name):
    c = ge.case(name)
    ns = _two_level(S, po, c, S.SymGaussSeidelSmoother(1))
    try:
        for forward in (True, False):
            want = dict(zip(("nsets", "max_set_rows", "nlaunches", "nwide"), gr.schedule(c.A, forward)))
            assert ns.gs_schedule(0, forward) == want
        assert ns.sweep_signature(0).endswith(" gs=F+B")
    finally:
        ns.close()
    ns = _two_level(S, po, c, S.GaussSeidelSmoother(2, 1.0, "forward"), S.GaussSeidelSmoother(1, 0.9, "forward"))
    try:
        assert ns.gs_schedule(0, True)["nsets"] == gr.schedule(c.A, True)[0]
        with pytest.raises(pkg.abi.GmgError) as e:
            ns.gs_schedule(0, False)
        assert e.value.code == pkg.abi.ERR_STATE
    finally:
        ns.close()


def test_tables_count_in_device_bytes_and_other_levels_keep_their_signature(S, po, pkg):
    c = ge.case("q1_2d")
    jac = S.RichardsonSmoother(S.JacobiLinearSolver(), 2, 2.0 / 3.0)
    ns = _two_level(S, po, c, jac)
    x, r = c.x0.copy(), c.r0.copy()
    ns.smooth(0, x, r)
    plain, sig = ns.device_bytes(), ns.sweep_signature(0)
    ns.close()
    ns = _two_level(S, po, c, jac, S.GaussSeidelSmoother(1, 1.0, "forward"))
    x, r = c.x0.copy(), c.r0.copy()
    ns.smooth(0, x, r)
    try:
        # perm + diagonal per row, (column, value) per strict lower entry at the least
        assert ns.device_bytes() - plain >= 12 * c.n + 12 * (c.A.nnz - c.n) // 2
        assert ns.sweep_signature(0) == sig + " gs=F" and " gs=" not in sig
    finally:
        ns.close()


# ---------------------------------------------------------------- 3. whole passes
COMBOS = list(itertools.product(gr.TYPES, (1, 2, 3)))


@pytest.mark.parametrize("name", ge.POISSON)
def test_whole_passes(S, po, pkg, name):
    c = ge.case(name)
    A = gr.csr(c.A)
    for k, (kind, niter) in enumerate(COMBOS):
        kind2, niter2 = COMBOS[(k + 4) % len(COMBOS)]
        specs = {pkg.abi.PRE: (niter, 1.0, kind), pkg.abi.POST: (niter2, 1.2, kind2)}
        ns = _two_level(S, po, c, S.GaussSeidelSmoother(*specs[pkg.abi.PRE]), S.GaussSeidelSmoother(*specs[pkg.abi.POST]))
        try:
            for which, spec in specs.items():
                x, r = c.x0.copy(), c.r0.copy()
                ns.smooth(0, x, r, which)
                sm = gr.GS(*spec)
                xo, ro = c.x0.copy(), c.r0.copy()
                gr.solve(xo, sm.setup(A), sm, ro)
                ex, er = max_rel(x, xo), max_rel(r, ro)
                print(name, spec, "max_rel x %.2e r %.2e" % (ex, er))
                assert ex <= fr.TOL_KERNEL and er <= fr.TOL_KERNEL, (name, spec, ex, er)
        finally:
            ns.close()


def test_whole_pass_on_a_level_larger_than_the_capped_grid_of_the_update(S, po):
    """x += w dx runs on a capped grid (2048 workgroups of 256 threads): every row past one pass of it must still be updated.
    One set of BIG_ROWS rows, no off-diagonal entry: the reference is dx = r / d written out."""
    c = ge.case("diagonal_big")
    assert c.n > 2048 * 256
    d = c.A.diagonal()
    ns = _two_level(S, po, c, S.GaussSeidelSmoother(1, 1.2, "forward"), S.GaussSeidelSmoother(2, 1.0, "backward"))
    try:
        assert ns.gs_schedule(0, True) == dict(nsets=1, max_set_rows=c.n, nlaunches=1, nwide=1)
        dx = np.full(c.n, np.nan)
        ns.precond(0, c.r0, dx)
        assert np.array_equal(dx, 1.2 * (c.r0 / d))
        x, r = c.x0.copy(), c.r0.copy()
        ns.smooth(0, x, r)
        step = 1.2 * (c.r0 / d)
        xo, ro = c.x0 + step, c.r0 - c.A @ step
        assert np.array_equal(x, xo) and max_rel(r, ro) <= fr.TOL_KERNEL
        x, r = c.x0.copy(), c.r0.copy()
        ns.smooth(0, x, r, 1)                                 # POST: two backward iterations at w = 1
        xo, ro = c.x0.copy(), c.r0.copy()
        for _ in range(2):
            step = ro / d
            xo, ro = xo + step, ro - c.A @ step
        assert max_rel(x, xo) <= fr.TOL_KERNEL                # (r is rounding residue after the first iteration: not compared)
    finally:
        ns.close()


# ---------------------------------------------------------------- 4. / 5. Krylov solvers and GMG with these smoothers
def _device_smoother(S, spec):
    if spec[0] == "gs":
        return S.GaussSeidelSmoother(*spec[1:])
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
    if c["solver"] == "cg_smoother":                          # SmoothersTests.jl:46-56
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
    ref = ge.krylov_reference(name)
    assert ref[1] == c["iters"]
    _agree(S, solver.log, ref, c["rtol"], x)


# ---------------------------------------------------------------- 6. refresh
@pytest.mark.parametrize("options", [None, PLAIN_SELL], ids=["default-layout", "explicit-values"])
def test_value_refresh_is_bitwise_a_fresh_setup(S, po, options):
    c = ge.case("q1_2d")
    pre, post = S.SymGaussSeidelSmoother(2, 1.2), S.GaussSeidelSmoother(1, 0.9, "backward")
    out = []
    for refreshed in (True, False):
        ns = _two_level(S, po, c, pre, post, scale=1.0 if refreshed else 1.7, options=options)
        try:
            if refreshed:
                S.numerical_setup_(ns, _csr(po, c.A * 1.7), [_csr(po, c.A * 1.7), _csr(po, c.Ac * 1.7)])
            dx = np.full(c.n, np.nan)
            ns.precond(0, c.r0, dx)
            x, r = c.x0.copy(), c.r0.copy()
            ns.smooth(0, x, r)
            out.append((dx, x, r, ns.gs_schedule(0, True), ns.gs_schedule(0, False)))
        finally:
            ns.close()
    for a, b in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(a, b)
    assert out[0][3:] == out[1][3:]
    sm = gr.GS(2, 1.2, "symmetric")                           # ... and those of the reference on the scaled matrix
    assert max_rel(out[0][0], gr.ldiv(sm.setup(gr.csr(c.A * 1.7)), sm, c.r0)) <= fr.TOL_KERNEL


# ---------------------------------------------------------------- 7. errors
@pytest.mark.parametrize("name", ge.SINGULAR)
def test_missing_or_zero_diagonal_is_singular_at_setup(S, po, pkg, name):
    with pytest.raises(pkg.abi.GmgError) as e:
        _two_level(S, po, ge.case(name), S.SymGaussSeidelSmoother(1))
    assert e.value.code == pkg.abi.ERR_SINGULAR and "level 0" in str(e.value)


def test_setter_checks(S, po, pkg):
    abi = pkg.abi
    ns = _two_level(S, po, ge.case("q1_3d-1"), S.SymGaussSeidelSmoother(1))
    try:
        for niter, omega, kind in ((0, 1.0, abi.GS_SYMMETRIC), (-2, 1.0, abi.GS_FORWARD), (1, 0.0, abi.GS_SYMMETRIC),
                                   (1, -0.5, abi.GS_BACKWARD), (1, 1.0, 7), (1, 1.0, -1)):
            assert ns._lib.gmg_set_smoother_gauss_seidel(ns.h, 0, abi.PRE, niter, omega, kind) == abi.ERR_INVALID
        assert ns._lib.gmg_set_smoother_gauss_seidel(ns.h, 1, abi.PRE, 1, 1.0, abi.GS_SYMMETRIC) == abi.ERR_INVALID   # the coarsest level
        dx = np.zeros(ns.n)
        ns.precond(0, ge.case("q1_3d-1").r0, dx)              # the refused calls left the handle as it was
        assert np.all(np.isfinite(dx)) and np.any(dx != 0.0)
    finally:
        ns.close()
