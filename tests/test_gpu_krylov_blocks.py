"""Krylov solvers around a GMG as block solvers on the device (GMG_BLOCK_KRYLOV_GMG, gmg_block_set_diag_krylov_gmg: FGMRESSolver(m, gmg) /
GMRESSolver(m; Pr | Pl = gmg) / CGSolver(gmg) as solvers[i] of a BlockDiagonalSolver, BlockTriangularSolver or SchurComplementSolver --
test/Applications/NavierStokesGMG.jl:159-169) against the composed CPU reference of tests/krylov_block_reference.py.

Tolerances are those tests/test_gpu_schur.py::_agree applies to the same comparison (inner iterative block solves amplify rounding):
x <= 1e-6 relative 2-norm, outer residual histories <= 1e-6 hist[0], ||K x - b|| < 1e-7, iteration counts and flags identical -- the
counts only because tests/test_krylov_block_host.py shows, on the CPU, that every stop-deciding residual of the reference is a factor 2
away from its threshold.  fgmres_fused = 1 and 0 must agree bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import block_refresh_problems as bp
import krylov_block_reference as kb
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL_X, TOL_HIST = kb.TOL_X, kb.TOL_HIST


def _setup(S, solver, A):
    return S.numerical_setup(S.symbolic_setup(solver, A), A)


def _block(ns):
    return ns.P_ns if hasattr(ns, "P_ns") else ns


def _apply(S, ns, b, x0=None):
    x = np.zeros(b.size) if x0 is None else x0.copy()
    S.solve_(x, _block(ns), np.array(b))
    return x


def _inner_log(S, ns, i=0):
    """(niters, flag, res0, res) of the last nested solve of block i"""
    abi = importlib.import_module(S.__name__.rsplit(".", 1)[0] + ".abi")
    res = abi.Result()
    abi.check_block(_block(ns).h, abi.load().gmg_block_diag_log(_block(ns).h, i, C.byref(res)))
    return int(res.niters), int(res.flag), float(res.res0), float(res.res)


def _check_inner(S, ns, solver, ref_call, what, i=0, res0=True):
    """the wrapper's log of its last nested solve against one call of the reference (res0: also its initial residual -- not for a
    solve that starts from a converged guess, whose initial residual is rounding of the previous one)"""
    nit, flag, hist = ref_call
    got = _inner_log(S, ns, i)
    print("%s: inner iters %d / %d, flag %d / %d, res0 %.3e / %.3e, res %.3e / %.3e" % (what, got[0], nit, got[1], flag, got[2], hist[0], got[3], hist[-1]))
    assert (solver.log.num_iters, solver.log.flag) == (nit, flag) == got[:2], what
    if res0:
        assert abs(got[2] - hist[0]) <= TOL_HIST * hist[0], what


# ---------------------------------------------------------------- 1: one application, 2: the second starts from the first's y
@pytest.mark.parametrize("variant", kb.VARIANTS)
def test_one_and_two_applications_upper_fgmres_around_gmg(S, variant):
    T, c = kb.stokes8(variant), kb.case("apply:" + variant)
    P, inner, cg = kb.device_stokes_solver(S, T, kb.SPECS["apply"])
    ns = _setup(S, P, T["A"])
    for k, key in enumerate(("x1", "x2")):
        x = _apply(S, ns, T["b"])
        print("apply %s, application %d: rel err x %.3e" % (variant, k + 1, rel_err(x, c[key])))
        _check_inner(S, ns, inner, c["inner"][k], "apply %s #%d" % (variant, k + 1), res0=(k == 0))
        assert cg.log.num_iters == c["cg"][k][0]
        assert rel_err(x, c[key]) <= TOL_X
        assert ns.diag_stats(0) == (k + 1, sum(n for n, _f, _h in c["inner"][: k + 1]))
        assert ns.diag_stats(1) == (k + 1, sum(n for n, _f, _h in c["cg"][: k + 1]))
    ns.close()


def test_second_application_starts_from_the_first(S):
    T, c = kb.stokes8("nonsym"), kb.case("guess:nonsym")
    assert rel_err(c["x2"], c["x1"]) >= 100 * TOL_X            # the references tell x0 = y1 from x0 = 0 ...
    P, inner, _cg = kb.device_stokes_solver(S, T, kb.SPECS["guess"])
    ns = _setup(S, P, T["A"])
    b = kb.guess_rhs(T)
    x1 = _apply(S, ns, b)
    _check_inner(S, ns, inner, c["inner"][0], "guess #1")
    x2 = _apply(S, ns, b)
    _check_inner(S, ns, inner, c["inner"][1], "guess #2", res0=False)
    print("guess: rel err #1 %.3e, #2 %.3e; |x2 - x1| / |x1| = %.3e (reference %.3e)" % (
        rel_err(x1, c["x1"]), rel_err(x2, c["x2"]), rel_err(x2, x1), rel_err(c["x2"], c["x1"])))
    assert rel_err(x1, c["x1"]) <= TOL_X and rel_err(x2, c["x2"]) <= TOL_X
    assert rel_err(x2, c["x1"]) >= 50 * TOL_X                  # ... and so does the device: the cache is live
    ns.close()


# ---------------------------------------------------------------- 3: growth and restart, 4: kinds and halves
ONE = [("grow", "upper"), ("restart", "upper")] + [(k, h) for k in kb.KINDS for h in kb.HALVES]


@pytest.mark.parametrize("sname,half", ONE)
def test_nested_kinds_growth_and_restart(S, sname, half):
    variant = "nonsym" if sname in ("grow", "restart") else "sym"   # growth and restart where five iterations still reduce the residual
    T, c = kb.stokes8(variant), kb.case("one:%s/%s/%s" % (sname, half, variant))
    P, inner, cg = kb.device_stokes_solver(S, T, kb.SPECS[sname], half)
    ns = _setup(S, P, T["A"])
    x = _apply(S, ns, T["b"])
    print("%s / %s: rel err x %.3e" % (sname, half, rel_err(x, c["x"])))
    _check_inner(S, ns, inner, c["inner"][0], "%s / %s" % (sname, half))
    assert cg.log.num_iters == c["cg"][0][0]
    assert rel_err(x, c["x"]) <= TOL_X
    ns.close()


# ---------------------------------------------------------------- 5: the nested solve on an 8-byte aligned sub-vector
def test_unaligned_subvector_fused_and_unfused(S):
    T, c = kb.unaligned_system(), kb.case("unaligned:")
    got = {}
    for fused in (0, 1):
        inner = kb.device_inner(S, kb.device_q1_gmg(S, T["H"], options={"fgmres_fused": fused}), kb.SPECS["unaligned"])
        P = S.BlockTriangularSolver([S.JacobiLinearSolver(), inner], coeffs=[[1.0, 0.0], [1.0, 1.0]], half="lower")
        ns = _setup(S, P, T["mat"])
        xs = []
        for k, key in enumerate(("x1", "x2")):
            x = _apply(S, ns, T["b"])
            print("unaligned, fgmres_fused = %d, application %d: rel err x %.3e" % (fused, k + 1, rel_err(x, c[key])))
            _check_inner(S, ns, inner, c["inner"][k], "unaligned #%d" % (k + 1), i=1, res0=(k == 0))
            assert rel_err(x, c[key]) <= TOL_X
            xs.append(x)
        got[fused] = (xs, _inner_log(S, ns, 1), ns.block_ns[1].device_bytes())
        ns.close()
    assert got[0][1] == got[1][1]
    assert got[1][2] > got[0][2]                              # the fused path ran: it alone holds the table of the Z pointers
    for a, b in zip(got[0][0], got[1][0]):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------- 6: outer solves
def _agree(log, c, x, K, b, what):
    nit, flag, hist = c["nit"], c["flag"], c["hist"]
    k = min(nit, log.num_iters)
    print("%s: iters %d / %d, flag %d / %d, max |hist - ref| / hist[0] = %.3e, rel err x = %.3e, ||K x - b|| = %.3e" % (
        what, log.num_iters, nit, log.flag, flag, np.max(np.abs(np.asarray(log.residuals[: k + 1]) - hist[: k + 1])) / hist[0],
        rel_err(x, c["x"]), np.linalg.norm(K @ x - b)))
    assert log.num_iters == nit and log.flag == flag
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= TOL_HIST * hist[0])
    assert rel_err(x, c["x"]) <= TOL_X
    assert np.linalg.norm(K @ x - b) < 1e-7


@pytest.mark.parametrize("variant", kb.VARIANTS)
@pytest.mark.parametrize("outer", ["fgmres", "gmres"])
def test_outer_solves_with_a_nested_fgmres(S, outer, variant):
    """NavierStokesGMG.jl:159-169: FGMRESSolver(20, BlockTriangularSolver(blocks, [FGMRESSolver(5, gmg; rtol = 1e-2), CG-Jacobi], coeffs, :upper))"""
    T, c = kb.stokes8(variant), kb.case("outer:%s/%s" % (outer, variant))
    spec = kb.outer_spec(outer)                              # under GMRES the nested solve is tight: Pr must be linear to the outer tolerance
    P, inner, cg = kb.device_stokes_solver(S, T, spec)
    solver = S.FGMRESSolver(20, P, **kb.OUTER) if outer == "fgmres" else S.GMRESSolver(20, Pr=P, **kb.OUTER)
    ns = _setup(S, solver, T["A"])
    x = np.zeros(T["n"])
    S.solve_(x, ns, np.array(T["b"]))
    _agree(solver.log, c, x, T["K"], T["b"], "%s(20, upper([FGMRES(5, gmg; rtol = %g), CG-Jacobi])) %s" % (outer, spec["rtol"], variant))
    napp, total = ns.P_ns.diag_stats(0)
    print("nested FGMRES: %d applications, %d iterations (reference %s)" % (napp, total, [n for n, _f, _h in c["inner"]]))
    assert (napp, total) == (len(c["inner"]), sum(n for n, _f, _h in c["inner"]))
    assert ns.P_ns.diag_stats(1) == (len(c["cg"]), sum(n for n, _f, _h in c["cg"]))
    assert (inner.log.num_iters, inner.log.flag) == c["inner"][-1][:2]           # the wrapper's log: its last solve
    ns.close()


# ---------------------------------------------------------------- 7: Schur
def test_schur_with_a_nested_fgmres_initial_guess_and_persistent_du(S):
    T, c = kb.stokes8("nonsym"), kb.case("schur:nonsym")
    assert rel_err(c["x2"], c["x1"]) >= 100 * TOL_X and rel_err(c["xz"], c["x1"]) >= 100 * TOL_X

    def device():
        inner = kb.device_inner(S, kb.device_velocity_gmg(S, T), kb.SPECS["schur"])
        cg = S.CGSolver(S.JacobiLinearSolver(), **kb.CG_P)
        return _setup(S, S.SchurComplementSolver((inner, None), T["B"], T["C"], (cg, T["Mp"])), T["A"]), inner

    ns, inner = device()
    x = kb.schur_x0(T)
    for k, key in enumerate(("x1", "x2")):                    # x prefilled, then left as returned; du persists
        S.solve_(x, ns, np.array(T["b"]))
        print("schur application %d: rel err %.3e" % (k + 1, rel_err(x, c[key])))
        assert rel_err(x, c[key]) <= TOL_X
        _check_inner(S, ns, inner, c["inner"][2 * k + 1], "schur #%d (du solve)" % (k + 1), res0=(k == 0))
        assert ns.diag_stats(0) == (2 * (k + 1), sum(n for n, _f, _h in c["inner"][: 2 * (k + 1)]))
    ns.close()
    ns, inner = device()
    xz = _apply(S, ns, T["b"])
    assert rel_err(xz, c["xz"]) <= TOL_X
    ns.close()


# ---------------------------------------------------------------- 8: numerical_setup!
def test_refresh_in_place_is_bitwise_a_fresh_setup(S, po, monkeypatch):
    monkeypatch.setenv("GMG_PATTERN", "0")                   # explicit values at (8, 8, 8): tests/test_gpu_block_refresh.py::explicit_layouts
    T1, T2 = bp.stokes_like(po, (8, 8, 8), 2, 2, explicit=True)
    b = np.random.default_rng(5).uniform(-1, 1, T1["n"])

    def make(T):
        inner = S.FGMRESSolver(3, kb.device_q1_gmg(S, T["H"]), maxiter=3, atol=1e-30, rtol=1e-30)
        cgj = S.CGSolver(S.JacobiLinearSolver(), maxiter=8, atol=1e-30, rtol=1e-30)
        blocks = [[S.NonlinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(T["Mp"])]]
        P = S.BlockTriangularSolver(blocks, [inner, cgj], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")
        solver = S.FGMRESSolver(20, P, atol=1e-10, rtol=1e-9, maxiter=60)
        return solver, _setup(S, solver, T["mat"])

    def solve(solver, ns):
        x = np.zeros(b.size)
        S.solve_(x, ns, b.copy())
        k = solver.log.num_iters
        return x, k, np.array(solver.log.residuals[: k + 1])

    sf, nf = make(T2)                                        # the fresh set-up on the new values
    z_f = _apply(S, nf, b)
    x_f, k_f, h_f = solve(sf, nf)
    s1, ns = make(T1)
    z0 = _apply(S, ns, np.zeros(b.size))                     # allocates the nested bases; every cache stays zero
    assert not z0.any() and _block(ns).diag_stats(0) == (1, 0)
    info0 = _block(ns).setup_info()
    gbytes0 = _block(ns).block_ns[0].device_bytes()
    assert info0["kind"] == 1
    S.numerical_setup_(ns, T2["mat"], smatrices=[T2["H"]["mats"], None], x=None)
    info = _block(ns).setup_info()
    assert info["kind"] == 2 and info["device_bytes"] == info0["device_bytes"]
    assert _block(ns).block_ns[0].device_bytes() == gbytes0   # the GMG handle kept its bases: nothing freed or allocated there either
    assert _block(ns).diag_stats(0) == (0, 0)                # counted since the setup
    z = _apply(S, ns, b)
    np.testing.assert_array_equal(z, z_f)
    x, k, h = solve(s1, ns)
    assert k == k_f and k > 0
    np.testing.assert_array_equal(h, h_f)
    np.testing.assert_array_equal(x, x_f)
    assert _block(ns).block_ns[0].device_bytes() >= gbytes0  # (the table of the Z pointers came with the first solution update, not with the refresh)
    _block(ns).close(); _block(nf).close()


# ---------------------------------------------------------------- 9: fgmres_fused 0 against 1, bit for bit
EDGE_NESTED = (1, 131074)                                    # 131074: the first length with 257 dot partials (krylov_edge_problems.py)
EDGE_DIRECT = EDGE_NESTED + (255, 256, 257)


def _edge_gmg(S, N, options):
    mats, Ps, Rs, b = kb.edge_hierarchy(N)
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 3, 2.0 / 3.0)]
    return S.GMGLinearSolver(mats, Ps, Rs, pre_smoothers=sm, post_smoothers=sm, maxiter=1, mode="preconditioner", options=options), mats, b


@pytest.mark.parametrize("N", EDGE_NESTED)
def test_fused_and_unfused_nested_solves_agree_bitwise(S, N):
    got, nbytes = {}, {}
    for fused in (0, 1):
        gmg, mats, b = _edge_gmg(S, N, {"fgmres_fused": fused})
        inner = S.FGMRESSolver(3, gmg, restart=(N > 1), maxiter=7, atol=1e-30, rtol=1e-12)
        ns = _setup(S, S.BlockDiagonalSolver([inner]), [[mats[0]]])
        out = []
        for _ in range(2):
            out.append((_apply(S, ns, b), _inner_log(S, ns)))
        got[fused] = out
        nbytes[fused] = ns.block_ns[0].device_bytes()
        ns.close()
    # which path ran: only the fused one builds the device table of the Z pointers on the GMG handle (its one solution update is a
    # pass over that table); everything else the two handles hold is the same
    assert nbytes[1] > nbytes[0] and nbytes[1] - nbytes[0] <= 64 + 8 * 64
    for (x0, l0), (x1, l1) in zip(got[0], got[1]):
        print("N = %d: inner log fused %s / unfused %s" % (N, l1, l0))
        assert l0 == l1
        np.testing.assert_array_equal(x0, x1)
        assert np.all(np.isfinite(x0))
    assert got[0][0][1][0] >= 1


@pytest.mark.parametrize("N", EDGE_DIRECT)
def test_fused_and_unfused_direct_solves_agree_bitwise(S, N):
    got, nbytes = {}, {}
    for fused in (None, 0, 1):
        gmg, mats, b = _edge_gmg(S, N, {} if fused is None else {"fgmres_fused": fused})
        solver = S.FGMRESSolver(3, gmg, restart=False, m_add=2, maxiter=12, atol=1e-30, rtol=1e-12)
        ns = _setup(S, solver, mats[0])
        if fused is None:
            assert ns.P_ns.get_option("fgmres_fused") == (None, "default")      # default: the entry point keeps its launches
        x = np.zeros(N)
        S.solve_(x, ns, b.copy())
        k = solver.log.num_iters
        got[fused] = (x, k, solver.log.flag, np.array(solver.log.residuals[: k + 1]))
        nbytes[fused] = ns.P_ns.device_bytes()
        ns.close()
    # which path ran: the default of a direct solve is the unfused one (no table of the Z pointers), fgmres_fused = 1 builds it
    assert nbytes[None] == nbytes[0] and nbytes[1] > nbytes[0]
    print("N = %d: %d iterations, flag %d" % (N, got[0][1], got[0][2]))
    for other in (None, 1):
        assert got[other][1:3] == got[0][1:3] and got[0][1] >= 1
        np.testing.assert_array_equal(got[other][3], got[0][3])
        np.testing.assert_array_equal(got[other][0], got[0][0])
    assert np.all(np.isfinite(got[0][0]))


# ---------------------------------------------------------------- 10: errors
def test_error_behaviour(S, po, pkg):
    abi = importlib.import_module(pkg.__name__ + ".abi")
    lib = abi.load()
    H = kb.q1((8, 8, 8), 2)
    A = H["mats"][0]; n = A.shape[0]
    g = S.GMGNumericalSetup(kb.device_q1_gmg(S, H), A)
    idx = A.idx.astype(np.int64); ptr = A.ptr.astype(np.int64)
    b = np.random.default_rng(4).uniform(-1, 1, n)
    v = np.zeros(n)

    def set_sys(h):
        return lib.gmg_block_set_system_block(h, 0, 0, n, n, A.nnz, ptr.ctypes.data, idx.ctypes.data, A.val.ctypes.data, 0, 0, 8)

    def kry(h, gh, krylov=abi.KRYLOV_FGMRES, m=3, side=0, m_add=1):
        return lib.gmg_block_set_diag_krylov_gmg(h, 0, gh, krylov, m, 0, m_add, 0, side, 2, 1e-30, 1e-30)

    h = C.c_void_p()
    sizes = np.array([n], dtype=np.int64)
    assert lib.gmg_block_create(C.byref(h), 1, sizes.ctypes.data, abi.BLOCK_DIAGONAL, 0) == abi.OK
    assert set_sys(h) == abi.OK
    # a bad krylov or side, m < 1, a null handle: GMG_ERR_INVALID, nothing set
    for bad in (dict(krylov=0), dict(krylov=4), dict(side=2), dict(side=-1), dict(side=1), dict(krylov=abi.KRYLOV_CG, side=0),
                dict(m=0), dict(krylov=abi.KRYLOV_GMRES, m=0), dict(m_add=0)):
        assert kry(h, g.h, **bad) == abi.ERR_INVALID, bad
        assert lib.gmg_block_setup(h) == abi.ERR_STATE                      # no solver set for block 0: the failed call changed nothing
    assert lib.gmg_block_set_diag_krylov_gmg(h, 0, None, abi.KRYLOV_FGMRES, 3, 0, 1, 0, 0, 2, 1e-30, 1e-30) == abi.ERR_INVALID
    assert lib.gmg_block_set_diag_krylov_gmg(h, 1, g.h, abi.KRYLOV_FGMRES, 3, 0, 1, 0, 0, 2, 1e-30, 1e-30) == abi.ERR_INVALID
    # a GMG handle that is not set up
    raw = C.c_void_p()
    assert lib.gmg_create(C.byref(raw), 2, 0) == abi.OK
    assert kry(h, raw) == abi.ERR_INVALID and b"not set up" in lib.gmg_block_last_error(h)
    assert lib.gmg_destroy(raw) == abi.OK
    # the handle is still usable: the valid call, a setup, an application, the statistics
    assert kry(h, g.h) == abi.OK
    assert lib.gmg_block_setup(h) == abi.OK
    assert lib.gmg_block_precond_apply(h, b.ctypes.data, v.ctypes.data, abi.MEM_HOST) == abi.OK
    na, ti = C.c_int64(-1), C.c_int64(-1)
    assert lib.gmg_block_diag_stats(h, 0, C.byref(na), C.byref(ti)) == abi.OK and (na.value, ti.value) == (1, 2)
    assert lib.gmg_block_diag_stats(h, 0, None, None) == abi.OK and lib.gmg_block_diag_stats(h, 3, None, None) == abi.ERR_INVALID
    first = v.copy()
    assert np.all(np.isfinite(first)) and np.linalg.norm(first) > 0
    assert lib.gmg_block_set_diag_solver(h, 0, abi.BLOCK_JACOBI, 0, 0.0, 0.0) == abi.OK     # a direct solver keeps no statistics
    assert lib.gmg_block_setup(h) == abi.OK
    assert lib.gmg_block_diag_stats(h, 0, C.byref(na), C.byref(ti)) == abi.ERR_STATE
    assert lib.gmg_block_destroy(h) == abi.OK
    # a size mismatch
    sizes2 = np.array([n + 1], dtype=np.int64)
    assert lib.gmg_block_create(C.byref(h), 1, sizes2.ctypes.data, abi.BLOCK_DIAGONAL, 0) == abi.OK
    assert kry(h, g.h) == abi.ERR_INVALID and b"size" in lib.gmg_block_last_error(h)
    assert lib.gmg_block_destroy(h) == abi.OK
    # a communicator of more than one rank: no partitioned nested solve exists, setup says so and names the block (the callbacks
    # are never called)
    xcb, rcb = abi.HOST_EXCHANGE_FN(lambda *a: None), abi.HOST_ALLREDUCE_FN(lambda *a: None)
    assert lib.gmg_block_create(C.byref(h), 1, sizes.ctypes.data, abi.BLOCK_DIAGONAL, 0) == abi.OK
    assert lib.gmg_block_comm_init_host(h, 0, 2, C.cast(xcb, C.c_void_p), C.cast(rcb, C.c_void_p), None) == abi.OK
    assert set_sys(h) == abi.OK
    assert kry(h, g.h) == abi.OK
    assert lib.gmg_block_setup(h) == abi.ERR_UNSUPPORTED
    msg = lib.gmg_block_last_error(h)
    assert b"single-GPU" in msg and b"block 0" in msg
    assert lib.gmg_block_precond_apply(h, b.ctypes.data, v.ctypes.data, abi.MEM_HOST) == abi.ERR_STATE
    assert lib.gmg_block_destroy(h) == abi.OK
    # ... and the GMG handle it named serves a fresh block handle: the same bits as the first application
    assert lib.gmg_block_create(C.byref(h), 1, sizes.ctypes.data, abi.BLOCK_DIAGONAL, 0) == abi.OK
    assert set_sys(h) == abi.OK and kry(h, g.h) == abi.OK and lib.gmg_block_setup(h) == abi.OK
    assert lib.gmg_block_precond_apply(h, b.ctypes.data, v.ctypes.data, abi.MEM_HOST) == abi.OK
    np.testing.assert_array_equal(v, first)
    assert lib.gmg_block_destroy(h) == abi.OK
    g.close()
    # the Python surface refuses what the device cannot nest before any handle exists
    with pytest.raises(NotImplementedError):
        _setup(S, S.BlockDiagonalSolver([S.FGMRESSolver(3, kb.device_q1_gmg(S, H), Pl=S.JacobiLinearSolver())]), [[A]])
