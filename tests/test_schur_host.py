"""SchurComplementSolver (LinearSolvers/SchurComplementSolvers.jl) without a GPU: the numpy restatement the GPU tests compare against
(tests/schur_reference.py), checked against the definition of the block factorisation, and the public surface of the device solver
(header, ctypes constant, Julia binding, Python mirror and its constructor checks)."""
import os
import re

import numpy as np
import pytest

import schur_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_U, N_P = 40, 15


def _spd(rng, n, shift):
    G = rng.standard_normal((n, n))
    return G @ G.T / n + shift * np.eye(n)


@pytest.fixture(scope="module")
def dense_system():
    """[A B; C D]: A, D symmetric positive definite plus a diagonal shift, B and C unrelated and small enough that S = D - C A^-1 B
    stays well conditioned"""
    rng = np.random.default_rng(17)
    A, D = _spd(rng, N_U, 2.0), _spd(rng, N_P, 3.0)
    B = 0.3 * rng.standard_normal((N_U, N_P))
    C = 0.3 * rng.standard_normal((N_P, N_U))
    K = np.block([[A, B], [C, D]])
    S = D - C @ np.linalg.solve(A, B)
    y = rng.uniform(-1.0, 1.0, N_U + N_P)
    assert np.linalg.cond(K) < 1e3 and np.linalg.cond(S) < 1e3
    return dict(A=A, B=B, C=C, D=D, K=K, S=S, y=y)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_exact_blocks_give_the_inverse_of_the_block_matrix(dense_system):
    """exact A^-1 and the exact S = D - C A^-1 B: solve! is K^-1 (the factorisation of the reference's docstring, :2-9)"""
    T = dense_system
    x = np.random.default_rng(1).standard_normal(N_U + N_P)                # exact solvers overwrite the initial guess
    sr.schur_apply(x, T["y"], sr.exact_solver(T["A"]), sr.exact_solver(T["S"]), T["B"], T["C"], sr.SchurCache(N_U))
    err = _rel(x, np.linalg.solve(T["K"], T["y"]))
    print("schur_reference vs numpy.linalg.solve: %.3e" % err)
    assert err <= 1e-10


def test_inexact_s_gives_the_product_of_the_three_factors(dense_system):
    """S replaced by its diagonal: solve! = [I -A^-1 B; 0 I] [A^-1 0; 0 S~^-1] [I 0; -C A^-1 I], multiplied out explicitly"""
    T = dense_system
    St = np.diag(np.diag(T["S"]))
    Ai = np.linalg.inv(T["A"])
    I_u, I_p = np.eye(N_U), np.eye(N_P)
    upper = np.block([[I_u, -Ai @ T["B"]], [np.zeros((N_P, N_U)), I_p]])
    middle = np.block([[Ai, np.zeros((N_U, N_P))], [np.zeros((N_P, N_U)), np.linalg.inv(St)]])
    lower = np.block([[I_u, np.zeros((N_U, N_P))], [-T["C"] @ Ai, I_p]])
    want = upper @ (middle @ (lower @ T["y"]))
    x = np.zeros(N_U + N_P)
    sr.schur_apply(x, T["y"], sr.exact_solver(T["A"]), sr.jacobi_solver(T["S"]), T["B"], T["C"], sr.SchurCache(N_U))
    err = _rel(x, want)
    print("schur_reference vs the explicit product: %.3e" % err)
    assert err <= 1e-10
    assert _rel(x, np.linalg.solve(T["K"], T["y"])) > 1e-3                 # and that is not K^-1: the test can tell the two apart


def test_iterative_a_solver_starts_from_x_and_from_the_du_cache(dense_system):
    """CG-Jacobi with 2 iterations as A: x_u on entry and the du of the previous application are initial guesses (:65,:70)"""
    T = dense_system
    log = {}
    cg = sr.cg_jacobi_solver(T["A"], maxiter=2, atol=1e-30, rtol=1e-30, log=log)
    solveS = sr.jacobi_solver(T["S"])
    x0 = np.random.default_rng(2).uniform(-1.0, 1.0, N_U + N_P)
    cache = sr.SchurCache(N_U)
    x = sr.schur_apply(x0.copy(), T["y"], cg, solveS, T["B"], T["C"], cache)
    assert log["num_iters"] == 2
    # the same steps written out by hand
    xu = x0[:N_U].copy(); cg(xu, T["y"][:N_U])
    xp = np.diag(T["S"]) ** -1 * (T["y"][N_U:] - T["C"] @ xu)
    du = np.zeros(N_U); cg(du, T["B"] @ xp)
    assert np.array_equal(x, np.concatenate([xu - du, xp]))
    assert np.array_equal(cache.du, du)
    # a zero guess gives another x_u, and a warm du another correction
    cold = sr.schur_apply(np.zeros(N_U + N_P), T["y"], cg, solveS, T["B"], T["C"], sr.SchurCache(N_U))
    warm = sr.schur_apply(np.zeros(N_U + N_P), T["y"], cg, solveS, T["B"], T["C"], cache)
    assert _rel(x, cold) > 1e-6 and _rel(warm, cold) > 1e-6
    # maxiter = 0 returns the guess, many iterations the solution
    g = x0[:N_U].copy()
    sr.cg_jacobi_solver(T["A"], maxiter=0)(g, T["y"][:N_U])
    assert np.array_equal(g, x0[:N_U])
    sr.cg_jacobi_solver(T["A"], maxiter=200, atol=1e-14, rtol=1e-13)(g, T["y"][:N_U])
    assert _rel(g, np.linalg.solve(T["A"], T["y"][:N_U])) <= 1e-10


# ---------------------------------------------------------------- the public surface
def test_schur_kind_is_declared_in_header_ctypes_and_julia(pkg):
    import importlib
    abi = importlib.import_module(pkg.__name__ + ".abi")
    hdr = open(os.path.join(ROOT, "include", "gmg_amd.h")).read()
    jl = open(os.path.join(ROOT, "gridapsolvers.jl_amd", "julia", "GridapSolversAMD.jl")).read()
    assert re.search(r"GMG_BLOCK_SCHUR\s*=\s*3", hdr) and "SchurComplementSolvers.jl" in hdr
    assert abi.BLOCK_SCHUR == 3
    assert re.search(r"^export .*HipSchurComplementSolver", jl, re.M) and re.search(r"GMG_BLOCK_SCHUR\s*=\s*Cint\(3\)", jl)
    assert not [n for n in abi.SYMBOLS if "schur" in n.lower()]            # no new exported symbol: the block setters serve


def test_python_mirror_constructor_checks(S, po):
    M = po.poisson_matrix((8, 8), 1); n = M.shape[0]                       # 49 rows
    R = po.poisson_matrix((4, 4), 1); m = R.shape[0]                       # 9 rows
    import scipy.sparse as sp
    B = sp.random(n, m, density=0.2, random_state=1, format="csr")
    Cm = sp.random(m, n, density=0.2, random_state=2, format="csr")
    P = S.SchurComplementSolver((S.LUSolver(), M), B, Cm, (S.JacobiLinearSolver(), R))
    assert P.half == "schur" and "SchurComplementSolver" in S.__all__
    assert P.solvers[0] is P.A[0] and P.solvers[1] is P.S[0] and P.B is B and P.C is Cm
    assert "SchurComplementSolvers.jl:11-26" in S.SchurComplementSolver.__doc__
    cg = S.CGSolver(S.JacobiLinearSolver(), maxiter=5)
    assert S.SchurComplementSolver((cg, M), B, Cm, (S.LUSolver(), R)).solvers[0] is cg
    # TypeError: a solver type the block handle cannot run
    for bad in (S.CGSolver(None), S.FGMRESSolver(5, None), S.RichardsonSmoother(S.JacobiLinearSolver(), 3), "lu"):
        with pytest.raises(TypeError):
            S.SchurComplementSolver((bad, M), B, Cm, (S.LUSolver(), R))
        with pytest.raises(TypeError):
            S.SchurComplementSolver((S.LUSolver(), M), B, Cm, (bad, R))
    with pytest.raises(TypeError):
        S.SchurComplementSolver(S.LUSolver(), B, Cm, (S.LUSolver(), R))    # not a (solver, matrix) pair
    # ValueError: B is (n_A, n_S), C is (n_S, n_A)
    with pytest.raises(ValueError, match="B has shape"):
        S.SchurComplementSolver((S.LUSolver(), M), Cm, Cm, (S.LUSolver(), R))
    with pytest.raises(ValueError, match="C has shape"):
        S.SchurComplementSolver((S.LUSolver(), M), B, B, (S.LUSolver(), R))
    with pytest.raises(ValueError):
        S.SchurComplementSolver((S.LUSolver(), None), B, Cm, (S.LUSolver(), R))   # only a GMG brings its own matrix
    # a GMGLinearSolver without a matrix uses its smatrices[0]
    H = po.build_hierarchy((8, 8), 2, 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"])
    Pg = S.SchurComplementSolver((gmg, None), B, Cm, (S.LUSolver(), R))
    assert Pg.A[1] is H["mats"][0] and Pg.blocks[0][0].mat is H["mats"][0]
    # the setups accept it; GMRES takes it on one side only (the "not both" rule, raised before any device handle exists)
    assert isinstance(S.symbolic_setup(P), type(S.symbolic_setup(S.BlockDiagonalSolver([S.LUSolver()]))))
    assert isinstance(S.symbolic_setup(S.GMRESSolver(20, Pr=P)), type(S.symbolic_setup(S.CGSolver(None))))
    with pytest.raises(ValueError, match="not both"):
        S.numerical_setup(S.symbolic_setup(S.GMRESSolver(20, Pr=P, Pl=P)), [[M, B], [Cm, R]])
    side = S._KrylovNumericalSetup._side
    assert side(P) == (1, P) and side((None, P)) == (0, P)
