"""numerical_setup!(ns, A, x) of block solvers on the device (BlockTriangularSolvers.jl:156-186, BlockDiagonalSolvers.jl:153-163,
BlockSolverInterfaces.jl:104-118,232-236): gmg_block_update_values[_csc] + gmg_block_refresh_diag_solver + gmg_block_setup.

The in-place path (kind 2) and the full path (kind 1) must give the bits of a fresh numerical_setup on the new matrices, keep the
work caches (the CG block solvers' initial guesses, the Schur solver's du) and the null space, and follow the reference in which
solvers they set up again.  Inputs: tests/block_refresh_problems.py.

Work caches and "bitwise a fresh set-up": the block work cache y survives numerical_setup! by design (the reference keeps it), and
a CG-Jacobi block starts from it.  A handle that has APPLIED its preconditioner before the refresh therefore cannot give the bits of
a fresh handle, whose cache is zero, in anything that runs the CG block -- on either path, in the reference as well.  So the
comparisons against a fresh set-up that involve the preconditioner are made on handles whose CG blocks have not run before the
refresh (the operator has: ns.mul), and the handles that solve before the refresh are compared, state included, between the two
paths (test_fallback_*, test_state_*) and, where nothing is stateful (mul), against the fresh set-up as well."""
import ctypes as C

import numpy as np
import pytest

import block_refresh_problems as bp
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL_APPLY = 1e-11                                            # tests/test_gpu_block.py


def jac(S, nlev, niter=10, omega=2.0 / 3.0):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), niter, omega)] * (nlev - 1)


def setup(S, solver, A):
    return S.numerical_setup(S.symbolic_setup(solver, A), A)


def block_ns(ns):
    return ns.P_ns if hasattr(ns, "P_ns") else ns


def close(ns):
    block_ns(ns).close()


def apply(S, ns, b, x0=None):
    x = np.zeros(b.size) if x0 is None else x0.copy()
    S.solve_(x, block_ns(ns), b)
    return x


def mul(ns, v):
    y = np.zeros(v.size)
    block_ns(ns).mul(y, v)
    return y


# fixed iteration counts in the inner solvers: what is compared does not depend on a convergence test passing at another iteration
def stokes_solver(S, T, nlev, nonlinear=True, fgmres=True):
    H = T["H"]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=jac(S, nlev), post_smoothers=jac(S, nlev),
                            maxiter=2, rtol=1e-30, atol=1e-30, mode="preconditioner")
    cgj = S.CGSolver(S.JacobiLinearSolver(), maxiter=8, atol=1e-30, rtol=1e-30)
    d00 = S.NonlinearSystemBlock() if nonlinear else S.LinearSystemBlock()
    blocks = [[d00, S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(T["Mp"])]]
    P = S.BlockTriangularSolver(blocks, [gmg, cgj], coeffs=[[1.0, 1.0], [0.0, 1.0]], half="upper")
    return (S.FGMRESSolver(20, P, atol=1e-10, rtol=1e-9, maxiter=60) if fgmres else P), gmg, cgj


def stokes_oracle(orc, T):
    H = T["H"]
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=2, rtol=1e-30, atol=1e-30)
    Po = orc.BlockPreconditioner([T["n1"], T["n2"]], [go, (orc.BD_CG_JACOBI, T["Mp"], 8, 1e-30, 1e-30)],
                                 {(0, 1): (T["mat"][0][1], 1.0), (1, 0): (T["mat"][1][0], 0.0)}, orc.UPPER)
    return Po, go


def refresh_stokes(S, ns, T):
    """numerical_setup!(ns, A, x): every system block, all GMG levels of block 0 through smatrices"""
    return S.numerical_setup_(ns, T["mat"], smatrices=[T["H"]["mats"], None], x=None)


def solve_record(S, solver, ns, b):
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    k = solver.log.num_iters
    return x, k, solver.log.residuals[: k + 1].copy()


STOKES = [((8, 8, 8), 2), ((16, 16, 16), 3)]


def explicit_layouts(monkeypatch, nc):
    """At (8, 8, 8) the gradient block has 343 rows of at most 8 entries: with perturbed values no two rows are equal, and still the
    343 one-row "patterns" fit the row-pattern table (490 entries at that width) -- a layout chosen from the values, which sends
    numerical_setup! down the full path.  The in-place path is what these tests are about, so the row-pattern dictionary is off at
    that size (for the fresh set-ups of the comparison as well); at (16, 16, 16) the table overflows by itself."""
    if tuple(nc) == (8, 8, 8):
        monkeypatch.setenv("GMG_PATTERN", "0")


@pytest.mark.parametrize("nc,nlev", STOKES)
def test_in_place_refresh_is_bitwise_a_fresh_setup(S, po, orc, monkeypatch, nc, nlev):
    explicit_layouts(monkeypatch, nc)
    T1, T2 = bp.stokes_like(po, nc, nlev, 2, explicit=True)
    b = np.random.default_rng(5).uniform(-1, 1, T1["n"])
    # the fresh set-up on the second matrices
    solver_f, _, _ = stokes_solver(S, T2, nlev)
    nf = setup(S, solver_f, T2["mat"])
    y_f = mul(nf, b)
    z_f = apply(S, nf, b)
    x_f, k_f, h_f = solve_record(S, solver_f, nf, b)
    # (1) the sequence of a Newton step: solve on the first matrices, numerical_setup!, solve
    solver, _, _ = stokes_solver(S, T1, nlev)
    ns = setup(S, solver, T1["mat"])
    solve_record(S, solver, ns, b)
    bytes0 = block_ns(ns).setup_info()["device_bytes"]
    assert block_ns(ns).setup_info()["kind"] == 1
    refresh_stokes(S, ns, T2)
    info = block_ns(ns).setup_info()
    assert info["kind"] == 2 and info["blocks_refreshed"] == 4 and info["device_bytes"] == bytes0
    assert info["value_bytes"] == 8 * sum(m.val.size for row in T2["mat"] for m in row)
    np.testing.assert_array_equal(mul(ns, b), y_f)
    x, k, h = solve_record(S, solver, ns, b)                 # (its CG block starts from the first solve's cache: see the module text;
    assert k > 0 and np.all(np.isfinite(x))                  #  compared, state included, in test_fallback_paths_give_the_bits_...)
    close(ns)
    # (2) the same with a handle whose work cache is still zero at the refresh: every result has the bits of the fresh set-up
    solver, _, _ = stokes_solver(S, T1, nlev)
    ns = setup(S, solver, T1["mat"])
    mul(ns, b)
    bytes0 = block_ns(ns).setup_info()["device_bytes"]
    refresh_stokes(S, ns, T2)
    info = block_ns(ns).setup_info()
    assert info["kind"] == 2 and info["blocks_refreshed"] == 4 and info["device_bytes"] == bytes0
    np.testing.assert_array_equal(mul(ns, b), y_f)
    z = apply(S, ns, b)
    np.testing.assert_array_equal(z, z_f)
    x, k, h = solve_record(S, solver, ns, b)
    assert k == k_f and k > 0
    np.testing.assert_array_equal(h, h_f)
    np.testing.assert_array_equal(x, x_f)
    assert block_ns(ns).setup_info()["device_bytes"] >= bytes0       # (the Krylov basis was allocated by the solve, not by the refresh)
    Po, _go = stokes_oracle(orc, T2)
    assert rel_err(z, Po.apply(b)) <= TOL_APPLY
    close(ns); close(nf)


def _ref_solver(S, kind, half, nonlinear):
    mk = {"lu": S.LUSolver, "jacobi": S.JacobiLinearSolver,
          "cg": lambda: S.CGSolver(S.JacobiLinearSolver(), maxiter=6, atol=1e-30, rtol=1e-30)}[kind]
    blk = S.NonlinearSystemBlock if nonlinear else S.LinearSystemBlock
    if half == "diagonal":
        return S.BlockDiagonalSolver([blk(), blk()], [mk(), mk()])
    blocks = [[blk(), S.LinearSystemBlock()], [S.LinearSystemBlock(), blk()]]
    return S.BlockTriangularSolver(blocks, [mk(), mk()], half=half)


@pytest.mark.parametrize("kind", ["lu", "jacobi", "cg"])
@pytest.mark.parametrize("half", ["upper", "lower", "diagonal"])
def test_every_solver_kind_and_half_nonlinear_blocks(S, po, half, kind):
    """[[M, -M], [M, M]] -> [[M', -M'], [M', M']] with NonlinearSystemBlock diagonal blocks: bitwise a fresh set-up on M'."""
    M, M2 = bp.reference_pair(po)
    n = M.shape[0]
    b = np.random.default_rng(0).uniform(-1, 1, 2 * n)
    nf = setup(S, _ref_solver(S, kind, half, True), bp.block_system(po, M2, half == "diagonal"))
    ns = setup(S, _ref_solver(S, kind, half, True), bp.block_system(po, M, half == "diagonal"))
    mul(ns, b)
    S.numerical_setup_(ns, bp.block_system(po, M2, half == "diagonal"))
    assert ns.setup_info()["kind"] in (1, 2)                 # (M has constant coefficients: a value-dependent layout may force the full path)
    np.testing.assert_array_equal(mul(ns, b), mul(nf, b))
    for _ in range(2):                                       # twice: the CG blocks' caches evolve alike
        np.testing.assert_array_equal(apply(S, ns, b), apply(S, nf, b))
    close(ns); close(nf)


@pytest.mark.parametrize("kind", ["lu", "jacobi", "cg"])
def test_schur_kind_refresh(S, po, kind):
    """SchurComplementSolver: its blocks are its own matrices (MatrixBlock), numerical_setup! renews the system's: mul! follows the
    new matrices, the application keeps the solver's, both as a fresh set-up with those arguments."""
    M, M2 = bp.reference_pair(po)
    n = M.shape[0]
    mk = {"lu": S.LUSolver, "jacobi": S.JacobiLinearSolver,
          "cg": lambda: S.CGSolver(S.JacobiLinearSolver(), maxiter=6, atol=1e-30, rtol=1e-30)}[kind]
    negM = bp.scaled(po, M, -1.0)
    schur = lambda: S.SchurComplementSolver((mk(), M), negM, M, (mk(), M))
    b = np.random.default_rng(0).uniform(-1, 1, 2 * n)
    nf = setup(S, schur(), bp.block_system(po, M2))
    ns = setup(S, schur(), bp.block_system(po, M))
    mul(ns, b)
    S.numerical_setup_(ns, bp.block_system(po, M2))
    np.testing.assert_array_equal(mul(ns, b), mul(nf, b))
    for _ in range(2):
        np.testing.assert_array_equal(apply(S, ns, b), apply(S, nf, b))
    close(ns); close(nf)


@pytest.mark.parametrize("kind", ["lu", "jacobi"])
def test_linear_system_blocks_keep_their_first_setup(S, po, orc, kind):
    """BlockSolverInterfaces.jl:104-109: a LinearSystemBlock solver is NOT set up again -- the application is the one of the OLD
    diagonal matrices with the NEW off-diagonal blocks, and that is far from the all-new preconditioner."""
    M, M2 = bp.reference_pair(po)
    n = M.shape[0]
    okind = orc.BD_LU if kind == "lu" else orc.BD_JACOBI
    negM2 = bp.scaled(po, M2, -1.0)
    off = {(0, 1): (negM2, 1.0), (1, 0): (M2, 1.0)}
    P_old_diag = orc.BlockPreconditioner([n, n], [(okind, M), (okind, M)], off, orc.UPPER)
    P_all_new = orc.BlockPreconditioner([n, n], [(okind, M2), (okind, M2)], off, orc.UPPER)
    b = np.random.default_rng(0).uniform(-1, 1, 2 * n)
    zo, zn = P_old_diag.apply(b), P_all_new.apply(b)
    assert rel_err(zo, zn) > 1e-3
    ns = setup(S, _ref_solver(S, kind, "upper", False), bp.block_system(po, M))
    apply(S, ns, b)
    for env in (None, "0"):                                  # in place (where the layouts allow) and under GMG_REFRESH=0: the same rule
        with pytest.MonkeyPatch.context() as mp:
            if env is not None:
                mp.setenv("GMG_REFRESH", env)
            S.numerical_setup_(ns, bp.block_system(po, M2))
        z = apply(S, ns, b)
        assert rel_err(z, zo) <= TOL_APPLY
        assert rel_err(z, zn) > 1e-3
        K2 = np.block([[M2.to_scipy().toarray(), -M2.to_scipy().toarray()], [M2.to_scipy().toarray(), M2.to_scipy().toarray()]])
        assert rel_err(mul(ns, b), K2 @ b) <= 1e-13          # the system operator did follow
    close(ns)


def test_linear_system_block_in_place_keeps_its_inverse_diagonal(S, po):
    """the same rule on the in-place path: explicit values, one Jacobi block that is not marked"""
    A0, A1 = (bp.edge_system(po, "widths")[k][0][0] for k in (0, 1))
    b = np.random.default_rng(1).uniform(-1, 1, A0.shape[0])
    ns = setup(S, S.BlockDiagonalSolver([S.LinearSystemBlock()], [S.JacobiLinearSolver()]), [[A0]])
    z0 = apply(S, ns, b)
    S.numerical_setup_(ns, [[A1]])
    assert ns.setup_info()["kind"] == 2
    np.testing.assert_array_equal(apply(S, ns, b), z0)       # the old D^-1 ...
    nf = setup(S, S.BlockDiagonalSolver([S.JacobiLinearSolver()]), [[A1]])
    np.testing.assert_array_equal(mul(ns, b), mul(nf, b))    # ... and the new operator
    assert rel_err(z0, apply(S, nf, b)) > 1e-3
    ns.close(); nf.close()


def _edge_solver(S, nb):
    if nb == 1:
        return S.BlockDiagonalSolver([S.NonlinearSystemBlock()], [S.JacobiLinearSolver()])
    blocks = [[S.NonlinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.NonlinearSystemBlock()]]
    return S.BlockTriangularSolver(blocks, [S.JacobiLinearSolver(), S.JacobiLinearSolver()], half="upper")


@pytest.mark.parametrize("ptr64", [0, 1])
@pytest.mark.parametrize("name", bp.EDGE_NAMES)
def test_refill_edge_shapes(S, po, monkeypatch, name, ptr64):
    """ragged / rectangular / long-row blocks, both row-pointer widths: two refreshes, each bitwise a fresh set-up"""
    monkeypatch.setenv("GMG_FORCE_PTR64", str(ptr64))
    monkeypatch.setenv("GMG_PATTERN", "0")                   # (small blocks of distinct rows fit the row-pattern table: see explicit_layouts)
    seq = bp.edge_system(po, name)
    nb = len(seq[0])
    n = sum(seq[0][i][i].shape[0] for i in range(nb))
    b = np.random.default_rng(3).uniform(-1, 1, n)
    ns = setup(S, _edge_solver(S, nb), seq[0])
    apply(S, ns, b)
    bytes0 = ns.setup_info()["device_bytes"]
    for mats in seq[1:]:
        S.numerical_setup_(ns, mats)
        info = ns.setup_info()
        assert info["kind"] == 2 and info["blocks_refreshed"] == nb * nb and info["device_bytes"] == bytes0
        nf = setup(S, _edge_solver(S, nb), mats)
        np.testing.assert_array_equal(mul(ns, b), mul(nf, b))
        np.testing.assert_array_equal(apply(S, ns, b), apply(S, nf, b))
        nf.close()
    ns.close()


def test_csc_block_refreshed_twice_second_time_without_pattern(S, po, pkg, monkeypatch):
    """a block set in CSC layout: gmg_block_update_values_csc with the pattern, then with NULL colptr / rowidx"""
    monkeypatch.setenv("GMG_PATTERN", "0")
    abi = pkg.abi
    seq = bp.edge_system(po, "rect-257x63")
    tocsc = lambda mats: [[m.to_scipy().tocsc() for m in row] for row in mats]
    n = 257 + 63
    b = np.random.default_rng(3).uniform(-1, 1, n)
    ns = setup(S, _edge_solver(S, 2), tocsc(seq[0]))
    S.numerical_setup_(ns, tocsc(seq[1]))                    # records the transposition of every block
    assert ns.setup_info()["kind"] == 2
    nf = setup(S, _edge_solver(S, 2), seq[1])
    np.testing.assert_array_equal(mul(ns, b), mul(nf, b))
    np.testing.assert_array_equal(apply(S, ns, b), apply(S, nf, b))
    nf.close()
    lib = abi.load()
    for i in range(2):
        for j in range(2):
            v = np.ascontiguousarray(seq[2][i][j].to_scipy().tocsc().data)
            abi.check_block(ns.h, lib.gmg_block_update_values_csc(ns.h, abi.BLOCK_SLOT_SYSTEM, i, j, None, None, C.c_void_p(v.ctypes.data), 0, 4))
        abi.check_block(ns.h, lib.gmg_block_refresh_diag_solver(ns.h, i))
    abi.check_block(ns.h, lib.gmg_block_setup(ns.h))
    assert ns.setup_info()["kind"] == 2
    nf = setup(S, _edge_solver(S, 2), seq[2])
    np.testing.assert_array_equal(mul(ns, b), mul(nf, b))
    np.testing.assert_array_equal(apply(S, ns, b), apply(S, nf, b))
    # a CSR-set block has no CSC order
    assert lib.gmg_block_update_values_csc(nf.h, abi.BLOCK_SLOT_SYSTEM, 0, 0, None, None, C.c_void_p(v.ctypes.data), 0, 4) == abi.ERR_STATE
    nf.close(); ns.close()


def _newton_sequence(S, po, nc, nlev, explicit, env, monkeypatch, b):
    """set up on the first matrices, SOLVE, numerical_setup!, solve: everything the second solve gives, and what the setup did"""
    T1, T2 = bp.stokes_like(po, nc, nlev, 2, explicit=explicit)
    solver, _, _ = stokes_solver(S, T1, nlev)
    ns = setup(S, solver, T1["mat"])
    solve_record(S, solver, ns, b)
    with pytest.MonkeyPatch.context() as mp:
        if env is not None:
            mp.setenv("GMG_REFRESH", env)
        refresh_stokes(S, ns, T2)
    info = block_ns(ns).setup_info()
    out = (mul(ns, b), apply(S, ns, b)) + solve_record(S, solver, ns, b)
    close(ns)
    return info, out


def test_fallback_paths_give_the_bits_of_the_in_place_path(S, po, monkeypatch):
    nc, nlev = (8, 8, 8), 2
    explicit_layouts(monkeypatch, nc)
    n = bp.stokes_like(po, nc, nlev, 2)[0]["n"]
    b = np.random.default_rng(5).uniform(-1, 1, n)
    info_ip, out_ip = _newton_sequence(S, po, nc, nlev, True, None, monkeypatch, b)
    info_off, out_off = _newton_sequence(S, po, nc, nlev, True, "0", monkeypatch, b)
    assert info_ip["kind"] == 2 and info_off["kind"] == 1
    for a, c in zip(out_ip, out_off):
        np.testing.assert_array_equal(a, c)
    # B and Bt with constant-coefficient values: a value-dependent layout, the full path; with and without GMG_REFRESH the same bits,
    # and mul! those of a fresh set-up
    info_c, out_c = _newton_sequence(S, po, nc, nlev, False, None, monkeypatch, b)
    info_c0, out_c0 = _newton_sequence(S, po, nc, nlev, False, "0", monkeypatch, b)
    assert info_c["kind"] == 1 and info_c0["kind"] == 1
    for a, c in zip(out_c, out_c0):
        np.testing.assert_array_equal(a, c)
    T2 = bp.stokes_like(po, nc, nlev, 2, explicit=False)[1]
    solver_f, _, _ = stokes_solver(S, T2, nlev)
    nf = setup(S, solver_f, T2["mat"])
    np.testing.assert_array_equal(out_c[0], mul(nf, b))
    close(nf)


def test_fallback_without_prior_application_is_bitwise_fresh(S, po, monkeypatch):
    """the full path from a zero work cache: application and solve have the bits of a fresh set-up (and hence of the in-place path,
    test_in_place_refresh_is_bitwise_a_fresh_setup)"""
    nc, nlev = (8, 8, 8), 2
    explicit_layouts(monkeypatch, nc)
    for explicit, env in ((False, None), (True, "0")):
        T1, T2 = bp.stokes_like(po, nc, nlev, 2, explicit=explicit)
        b = np.random.default_rng(5).uniform(-1, 1, T1["n"])
        solver_f, _, _ = stokes_solver(S, T2, nlev)
        nf = setup(S, solver_f, T2["mat"])
        solver, _, _ = stokes_solver(S, T1, nlev)
        ns = setup(S, solver, T1["mat"])
        mul(ns, b)
        with pytest.MonkeyPatch.context() as mp:
            if env is not None:
                mp.setenv("GMG_REFRESH", env)
            refresh_stokes(S, ns, T2)
        assert block_ns(ns).setup_info()["kind"] == 1
        np.testing.assert_array_equal(mul(ns, b), mul(nf, b))
        np.testing.assert_array_equal(apply(S, ns, b), apply(S, nf, b))
        for a, c in zip(solve_record(S, solver, ns, b), solve_record(S, solver_f, nf, b)):
            np.testing.assert_array_equal(a, c)
        close(ns); close(nf)


def _state_sequence(S, po, kind, env):
    """set up, apply(b), numerical_setup!, apply(b) with a one-iteration CG-Jacobi block: the second application shows the cache"""
    A1, A2 = (bp.edge_system(po, "widths")[k][0][0] for k in (0, 1))
    n = A1.shape[0]
    b = np.random.default_rng(8).uniform(-1, 1, 2 * n if kind == "schur" else n)
    cg = lambda: S.CGSolver(S.JacobiLinearSolver(), maxiter=1, atol=1e-30, rtol=1e-30)
    if kind == "schur":
        I = bp.csr(po, bp.sp.diags(0.01 * (1.0 + 0.5 * np.random.default_rng(6).uniform(-1, 1, n)), format="csr"))   # explicit values
        mk = lambda A: (S.SchurComplementSolver((cg(), A1), I, I, (S.JacobiLinearSolver(), A1)), [[A, I], [I, A]])
    else:
        mk = lambda A: (S.BlockDiagonalSolver([S.NonlinearSystemBlock()], [cg()]), [[A]])
    solver, mat1 = mk(A1)
    ns = setup(S, solver, mat1)
    z1 = apply(S, ns, b)
    with pytest.MonkeyPatch.context() as mp:
        if env is not None:
            mp.setenv("GMG_REFRESH", env)
        S.numerical_setup_(ns, mk(A2)[1])
    info = ns.setup_info()
    z2 = apply(S, ns, b)
    ns.close()
    solver_f, mat2 = mk(A2)
    nf = setup(S, solver_f, mat2)
    zf = apply(S, nf, b)
    nf.close()
    return info, z1, z2, zf


@pytest.mark.parametrize("kind", ["diagonal", "schur"])
def test_state_survives_both_paths(S, po, kind):
    info_a, z1a, z2a, zfa = _state_sequence(S, po, kind, None)
    info_b, z1b, z2b, zfb = _state_sequence(S, po, kind, "0")
    assert info_a["kind"] == 2 and info_b["kind"] == 1
    np.testing.assert_array_equal(z1a, z1b)
    np.testing.assert_array_equal(z2a, z2b)                   # same bits on both paths ...
    np.testing.assert_array_equal(zfa, zfb)
    assert not np.array_equal(z2a, zfa)                       # ... which are not those of a fresh handle's first application
    assert rel_err(z2a, zfa) > 1e-6


def test_three_refreshes_in_a_row(S, po, monkeypatch):
    nc, nlev = (8, 8, 8), 2
    explicit_layouts(monkeypatch, nc)
    Ts = bp.stokes_like(po, nc, nlev, 4, explicit=True)
    b = np.random.default_rng(5).uniform(-1, 1, Ts[0]["n"])
    P, _, _ = stokes_solver(S, Ts[0], nlev, fgmres=False)
    ns = setup(S, P, Ts[0]["mat"])
    mul(ns, b)
    bytes0 = ns.setup_info()["device_bytes"]
    for T in Ts[1:]:
        refresh_stokes(S, ns, T)
        info = ns.setup_info()
        assert info["kind"] == 2 and info["blocks_refreshed"] == 4 and info["device_bytes"] == bytes0
    Pf, _, _ = stokes_solver(S, Ts[3], nlev, fgmres=False)
    nf = setup(S, Pf, Ts[3]["mat"])
    np.testing.assert_array_equal(mul(ns, b), mul(nf, b))
    np.testing.assert_array_equal(apply(S, ns, b), apply(S, nf, b))
    ns.close(); nf.close()


@pytest.mark.parametrize("env", [None, "0"])
def test_null_space_survives_a_refresh(S, po, pkg, monkeypatch, env):
    monkeypatch.setenv("GMG_PATTERN", "0")
    abi = pkg.abi
    lib = abi.load()
    seq = bp.edge_system(po, "rect-257x63")
    n = 257 + 63
    ns = setup(S, _edge_solver(S, 2), seq[0])
    V = np.ascontiguousarray(np.random.default_rng(2).uniform(-1, 1, (2, n)))
    abi.check_block(ns.h, lib.gmg_block_nullspace_set(ns.h, n, 2, C.c_void_p(V.ctypes.data), n, abi.MEM_HOST))
    abi.check_block(ns.h, lib.gmg_block_nullspace_orthonormalize(ns.h, 0))

    def size_and_projection():
        k, m = C.c_int(0), C.c_int64(0)
        abi.check_block(ns.h, lib.gmg_block_nullspace_size(ns.h, C.byref(k), C.byref(m)))
        v = np.random.default_rng(4).uniform(-1, 1, n)
        p, alpha = np.zeros(n), np.zeros(2)
        abi.check_block(ns.h, lib.gmg_block_nullspace_project(ns.h, C.c_void_p(v.ctypes.data), C.c_void_p(p.ctypes.data),
                                                              C.c_void_p(alpha.ctypes.data), abi.MEM_HOST, 0))
        return (k.value, m.value), p, alpha

    s0, p0, a0 = size_and_projection()
    assert s0 == (2, n) and np.linalg.norm(p0) > 0
    with pytest.MonkeyPatch.context() as mp:
        if env is not None:
            mp.setenv("GMG_REFRESH", env)
        S.numerical_setup_(ns, seq[1])
    assert ns.setup_info()["kind"] == (2 if env is None else 1)
    s1, p1, a1 = size_and_projection()
    assert s1 == s0
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(a1, a0)
    ns.close()


def test_status_codes(S, po, pkg):
    abi = pkg.abi
    lib = abi.load()
    A0, A1 = (bp.edge_system(po, "widths")[k][0][0] for k in (0, 1))
    n = A0.shape[0]
    vp = lambda a: C.c_void_p(a.ctypes.data)
    # update before the first set-up
    h = C.c_void_p()
    sizes = np.array([n], dtype=np.int64)
    assert lib.gmg_block_create(C.byref(h), 1, vp(sizes), abi.BLOCK_DIAGONAL, 0) == abi.OK
    ptr32 = A0.ptr.astype(np.int32)
    assert lib.gmg_block_set_system_block(h, 0, 0, n, n, A0.val.size, vp(ptr32), vp(A0.idx), vp(A0.val), abi.CSR, 0, 4) == abi.OK
    assert lib.gmg_block_set_diag_solver(h, 0, abi.BLOCK_JACOBI, 0, 0.0, 0.0) == abi.OK
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_SYSTEM, 0, 0, vp(A1.val)) == abi.ERR_STATE
    assert lib.gmg_block_refresh_diag_solver(h, 0) == abi.ERR_STATE
    k = C.c_int(-1)
    assert lib.gmg_block_get_setup_info(h, C.byref(k), None, None, None) == abi.OK and k.value == 0
    assert lib.gmg_block_setup(h) == abi.OK
    # absent block, wrong slot, block index out of range, no matrix of its own
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_PRECOND, 0, 0, vp(A1.val)) == abi.ERR_INVALID
    assert lib.gmg_block_update_values(h, 7, 0, 0, vp(A1.val)) == abi.ERR_INVALID
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_SYSTEM, 0, 1, vp(A1.val)) == abi.ERR_INVALID
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_DIAG_MATRIX, 0, 0, vp(A1.val)) == abi.ERR_INVALID
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_SYSTEM, 0, 0, None) == abi.ERR_INVALID
    assert lib.gmg_block_refresh_diag_solver(h, 3) == abi.ERR_INVALID
    b = np.random.default_rng(1).uniform(-1, 1, n)
    x0 = np.zeros(n)
    assert lib.gmg_block_precond_apply(h, vp(b), vp(x0), abi.MEM_HOST) == abi.OK     # nothing changed: still set up
    # a zero diagonal in a marked Jacobi block
    bad = A1.val.copy()
    bad[A1.ptr[5]:A1.ptr[6]][A1.idx[A1.ptr[5]:A1.ptr[6]] == 5] = 0.0
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_SYSTEM, 0, 0, vp(bad)) == abi.OK
    assert lib.gmg_block_refresh_diag_solver(h, 0) == abi.OK
    assert lib.gmg_block_setup(h) == abi.ERR_SINGULAR and b"block 0" in lib.gmg_block_last_error(h)
    # the good values again: a full set-up after the failed one, and it works
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_SYSTEM, 0, 0, vp(A1.val)) == abi.OK
    assert lib.gmg_block_refresh_diag_solver(h, 0) == abi.OK
    assert lib.gmg_block_setup(h) == abi.OK
    x1 = np.zeros(n)
    assert lib.gmg_block_precond_apply(h, vp(b), vp(x1), abi.MEM_HOST) == abi.OK
    np.testing.assert_allclose(x1, b / A1.to_scipy().diagonal(), rtol=5e-16, atol=0)     # D^-1 of the good values (b * (1/d): two roundings)
    # setting a block again: the next set-up is a full one
    assert lib.gmg_block_set_system_block(h, 0, 0, n, n, A0.val.size, vp(ptr32), vp(A0.idx), vp(A0.val), abi.CSR, 0, 4) == abi.OK
    assert lib.gmg_block_setup(h) == abi.OK
    assert lib.gmg_block_get_setup_info(h, C.byref(k), None, None, None) == abi.OK and k.value == 1
    assert lib.gmg_block_update_values(h, abi.BLOCK_SLOT_SYSTEM, 0, 0, vp(A1.val)) == abi.OK
    assert lib.gmg_block_setup(h) == abi.OK
    assert lib.gmg_block_get_setup_info(h, C.byref(k), None, None, None) == abi.OK and k.value == 2
    assert lib.gmg_block_destroy(h) == abi.OK
    # a CSC pattern of the wrong size: refused, and the handle still solves with the old values
    Ac0, Ac1 = A0.to_scipy().tocsc(), A1.to_scipy().tocsc()
    ns = setup(S, S.BlockDiagonalSolver([S.NonlinearSystemBlock()], [S.JacobiLinearSolver()]), [[Ac0]])
    z0 = apply(S, ns, b)
    wrong = bp.edge_system(po, "offsets")[0][0][0].to_scipy().tocsc()
    st = lib.gmg_block_update_values_csc(ns.h, abi.BLOCK_SLOT_SYSTEM, 0, 0, vp(wrong.indptr), vp(wrong.indices), vp(wrong.data), 0, 4)
    assert st == abi.ERR_INVALID
    np.testing.assert_array_equal(apply(S, ns, b), z0)
    S.numerical_setup_(ns, [[Ac1]])
    np.testing.assert_array_equal(apply(S, ns, b), x1)
    ns.close()
