"""GMRESSolver (Krylov/GMRESSolvers.jl) without a GPU: the numpy restatement the GPU tests compare against, checked on its own
against an independent definition of GMRES, and the public surface of the device solver (header, ctypes prototypes, Julia
binding, Python mirror)."""
import os
import re

import numpy as np
import pytest

import gmres_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poisson_2d(po, n):
    A = po.poisson_matrix((n, n), 1).to_scipy().tocsr()
    b = np.random.default_rng(11).standard_normal(A.shape[0])
    return A, b


def test_history_is_the_least_squares_minimum_over_the_krylov_space(po):
    """unrestarted, unpreconditioned: hist[k] = min ||b - A x|| over x0 + K_k(A, r0).  The Krylov basis is built explicitly and the
    minimum taken by numpy.linalg.lstsq; the explicit basis loses digits as k grows, hence k <= 8 and 1e-8 hist[0]."""
    A, b = _poisson_2d(po, 12)
    x0 = np.random.default_rng(2).standard_normal(b.size)
    r0 = b - A @ x0
    x, nit, flag, hist = gr.gmres(lambda v: A @ v, b, 3, x0=x0, maxiter=8, atol=0.0, rtol=0.0)   # m = 3: the basis grows (m_add)
    assert nit == 8 and flag == gr.DIVERGED_MAXITER and hist.size == 9
    assert abs(hist[0] - np.linalg.norm(r0)) <= 1e-14 * hist[0]
    K = np.empty((b.size, 8))
    v = r0 / np.linalg.norm(r0)
    for k in range(8):
        K[:, k] = v
        v = A @ v
        v = v / np.linalg.norm(v)
        y = np.linalg.lstsq(A @ K[:, : k + 1], r0, rcond=None)[0]
        best = np.linalg.norm(r0 - A @ (K[:, : k + 1] @ y))
        assert abs(hist[k + 1] - best) <= 1e-8 * hist[0], (k + 1, hist[k + 1], best)
    assert abs(np.linalg.norm(b - A @ x) - hist[8]) <= 1e-8 * hist[0]      # the returned x attains it


SHAPES = [dict(m=40, jr=True, jl=True, restart=False), dict(m=10, jr=False, jl=False, restart=False),
          dict(m=10, jr=False, jl=False, restart=True), dict(m=10, jr=True, jl=False, restart=True),
          dict(m=5, jr=False, jl=True, restart=True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "m%d%s%s%s" % (s["m"], "-Pr" * s["jr"], "-Pl" * s["jl"], "-restart" * s["restart"]))
def test_reference_solves_poisson_in_the_krylovtests_shapes(po, shape):
    """KrylovTests.jl:67-75: Pr = Pl = Jacobi, unpreconditioned, restarted, restarted with Pr, restarted with Pl"""
    A, b = _poisson_2d(po, 16)
    dinv = 1.0 / A.diagonal()
    jac = lambda r: dinv * r
    info = {}
    x, nit, flag, hist = gr.gmres(lambda v: A @ v, b, shape["m"], Pr=jac if shape["jr"] else None, Pl=jac if shape["jl"] else None,
                                  restart=shape["restart"], maxiter=400, atol=1e-14, rtol=1e-9, info=info)
    assert flag == gr.CONVERGED_RTOL and 0 < nit < 400 and hist.size == nit + 1
    assert np.linalg.norm(b - A @ x) < 1e-7 * np.linalg.norm(b)
    if shape["restart"]:
        assert info["basis"] == shape["m"] + 1 and info["cycles"] == -(-nit // shape["m"])
    else:
        assert info["cycles"] == 1 and info["basis"] == max(shape["m"], nit) + 1
    x0 = np.random.default_rng(3).standard_normal(b.size)                  # a nonzero initial guess
    x1, _, flag1, _ = gr.gmres(lambda v: A @ v, b, shape["m"], Pr=jac if shape["jr"] else None, Pl=jac if shape["jl"] else None,
                               x0=x0, restart=shape["restart"], maxiter=400, atol=1e-14, rtol=1e-9)
    assert flag1 == gr.CONVERGED_RTOL and np.linalg.norm(b - A @ x1) < 1e-7 * np.linalg.norm(b)


def test_gmres_is_declared_prototyped_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gmg_amd.h")).read()
    abi_src = open(os.path.join(ROOT, "gridapsolvers.jl_amd", "abi.py")).read()
    jl = open(os.path.join(ROOT, "gridapsolvers.jl_amd", "julia", "GridapSolversAMD.jl")).read()
    for name in ("gmg_gmres_solve", "gmg_block_gmres_solve"):
        assert re.search(r"GMG_API int %s\(" % name, hdr), name
        assert f'"{name}":' in abi_src, name
        assert f"(:{name}, libgmgamd)" in jl, name
    assert re.search(r"^export .*HipGMRESSolver", jl, re.M) and re.search(r"^export .*HipBlockGMRESSolver", jl, re.M)
    assert "GMRESSolvers.jl:132-210" in hdr and "gmres_fused" in hdr


def test_abi_prototypes_match_the_header_argument_counts(pkg):
    import importlib
    abi = importlib.import_module(pkg.__name__ + ".abi")
    hdr = open(os.path.join(ROOT, "include", "gmg_amd.h")).read()
    for name in ("gmg_gmres_solve", "gmg_block_gmres_solve"):
        args = re.search(r"GMG_API int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(args.split(",")) == 15 == len(abi.SYMBOLS[name]), name


def test_python_mirror_has_gmres_with_the_reference_defaults(S):
    s = S.GMRESSolver(10)
    assert s.Pr is None and s.Pl is None and s.restart is False and s.m_add == 1 and s.m == 10
    assert (s.log.maxiter, s.log.atol, s.log.rtol) == (100, 1e-12, 1e-6)   # GMRESSolvers.jl:25
    assert "GMRESSolver" in S.__all__
    assert isinstance(S.symbolic_setup(S.GMRESSolver(5)), type(S.symbolic_setup(S.CGSolver(None))))
    with pytest.raises(ValueError):                                        # no side names a device handle
        S.numerical_setup(S.symbolic_setup(S.GMRESSolver(5)), None)
