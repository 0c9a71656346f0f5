"""MINRESSolver (Krylov/MINRESSolvers.jl) without a GPU: the numpy transcription the GPU tests compare against, checked on its
own, and the public surface of the device solver (header, ctypes prototypes, Julia binding, Python mirror)."""
import importlib
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import minres_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poisson_2d(po, n):
    A = po.poisson_matrix((n, n), 1).to_scipy().tocsr()
    b = np.random.default_rng(7).standard_normal(A.shape[0])
    return A, b


@pytest.mark.parametrize("jacobi", [True, False])
def test_reference_solves_poisson(po, jacobi):
    """KrylovTests.jl:92 on a 2-D Q1 Poisson matrix: Pl = JacobiLinearSolver() and Pl = nothing"""
    A, b = _poisson_2d(po, 24)
    dinv = 1.0 / A.diagonal()
    Pl = (lambda r: dinv * r) if jacobi else None
    x, nit, flag, hist = mr.minres(lambda v: A @ v, b, Pl, maxiter=500, atol=1e-14, rtol=1e-10)
    assert flag == mr.CONVERGED_RTOL and 0 < nit < 500 and hist.size == nit + 1
    assert np.linalg.norm(b - A @ x) < 1e-7 * np.linalg.norm(b)
    x0 = np.random.default_rng(3).standard_normal(b.size)                  # a nonzero initial guess
    x1, nit1, flag1, hist1 = mr.minres(lambda v: A @ v, b, Pl, x0=x0, maxiter=500, atol=1e-14, rtol=1e-10)
    assert flag1 == mr.CONVERGED_RTOL and np.linalg.norm(b - A @ x1) < 1e-7 * np.linalg.norm(b)


def _stokes_pc(st, n, alpha, sign):
    sysd = st.stokes_system(n, alpha)
    nu, npp = sysd["sizes"]
    Auu = sysd["A"][0][0].to_scipy().tocsc()
    Mp = (sign * sysd["Mp_scaled"].to_scipy()).tocsc()           # sign = -1: +M_p / alpha (SPD) ; +1: the scaled block as shipped
    lu_u, lu_p = spla.splu(Auu), spla.splu(Mp)
    return sysd, (lambda r: np.concatenate([lu_u.solve(r[:nu]), lu_p.solve(r[nu:])]))


def test_reference_solves_stokes_with_spd_block_diagonal(pkg):
    """the symmetric indefinite Stokes system with blockdiag(A_uu, M_p / alpha)^-1: the textbook MINRES pairing"""
    st = importlib.import_module(pkg.__name__ + ".stokes")
    sysd, Pl = _stokes_pc(st, 8, 1.0e3, -1.0)
    K, b = sysd["K"], sysd["b"]
    assert abs(K - K.T).max() < 1e-12                                      # symmetric ...
    x, nit, flag, hist = mr.minres(lambda v: K @ v, b, Pl, maxiter=200, atol=1e-12, rtol=1e-10)
    assert flag == mr.CONVERGED_RTOL and nit < 100
    assert np.linalg.norm(K @ x - b) < 1e-7 * np.linalg.norm(b)
    assert np.all(np.diff(hist) <= 1e-12 * hist[0])                        # MINRES: the preconditioned residual never grows


def test_reference_rejects_an_indefinite_preconditioner(pkg):
    """blockdiag(A_uu, -M_p / alpha)^-1 is indefinite: @check beta_p > 0 (:97) or the DomainError of sqrt (:116)"""
    st = importlib.import_module(pkg.__name__ + ".stokes")
    sysd, Pl = _stokes_pc(st, 8, 1.0e3, 1.0)
    K, b = sysd["K"], sysd["b"]
    with pytest.raises(mr.NotPositiveDefinite):
        mr.minres(lambda v: K @ v, b, Pl, maxiter=200, atol=1e-12, rtol=1e-10)
    n = 50                                                                 # and at start-up: Pl = -I on an SPD matrix
    A = sp.diags([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)], [-1, 0, 1]).tocsr()
    with pytest.raises(mr.NotPositiveDefinite):
        mr.minres(lambda v: A @ v, np.ones(n), lambda r: -r)


def test_givens_returns_r_with_the_lapack_sign_rule(orc):
    for f, g in [(3.0, 4.0), (-3.0, 4.0), (-4.0, 3.0), (0.0, 2.0), (2.0, 0.0), (1e300, 3e300), (1e-300, -2e-300)]:
        c, s, r = orc.givens(f, g)
        assert abs(c * f + s * g - r) <= 1e-15 * abs(r) and abs(-s * f + c * g) <= 1e-15 * abs(r)
        if abs(f) > abs(g):
            assert c > 0


def test_minres_is_declared_prototyped_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gmg_amd.h")).read()
    abi_src = open(os.path.join(ROOT, "gridapsolvers.jl_amd", "abi.py")).read()
    jl = open(os.path.join(ROOT, "gridapsolvers.jl_amd", "julia", "GridapSolversAMD.jl")).read()
    for name in ("gmg_minres_solve", "gmg_block_minres_solve"):
        assert re.search(r"GMG_API int %s\(" % name, hdr), name
        assert f'"{name}":' in abi_src, name
        assert f"(:{name}, libgmgamd)" in jl, name
    assert re.search(r"^export .*HipMINRESSolver", jl, re.M)
    assert "MINRESSolvers.jl:75-148" in hdr


def test_python_mirror_has_minres_with_the_reference_defaults(S):
    s = S.MINRESSolver()
    assert s.Pl is None
    assert (s.log.maxiter, s.log.atol, s.log.rtol) == (1000, 1e-12, 1e-6)  # MINRESSolvers.jl:16
    assert "MINRESSolver" in S.__all__
    assert isinstance(S.symbolic_setup(S.MINRESSolver(Pl=None)), type(S.symbolic_setup(S.CGSolver(None))))
