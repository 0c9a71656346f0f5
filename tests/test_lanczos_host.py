"""The Lanczos diagnostic of CGSolver and the Lanczos bounds of ChebyshevSmoother, on the host: the numpy definition
(tests/lanczos_reference.py) against literal restatements and known spectra, and the refusals of the Python layer.  No GPU."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import chebyshev_reference as cr
import lanczos_reference as lr
import numpy_twin as nt


# ---------------------------------------------------------------- the diagnostic
def _literal_replay(alphas, betas, max_iters):
    """CGSolvers.jl:83,87,114-115,128-138 and KrylovUtils.jl:69-81 line by line, 1-based like the reference"""
    k = [0]
    delta, gamma = [0.0] * max_iters, [0.0] * max_iters       # reset!
    alpha_last = 1.0                                          # :83
    for ak, bk in zip(alphas, betas):
        if k[0] == 0:                                         # iszero(k)
            d = 1.0 / ak
            g = 0.0
        else:
            d = (1.0 / ak) + (bk / alpha_last)
            g = math.sqrt(bk) / ak
        k[0] += 1                                             # update!
        delta[k[0] - 1] = d
        gamma[k[0] - 1] = g
        alpha_last = ak                                       # :115
    return k[0], np.array(delta), np.array(gamma)


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return sp.csr_matrix(Q @ np.diag(np.linspace(1.0, 50.0, n)) @ Q.T), rng.uniform(-1, 1, n)


@pytest.mark.parametrize("pl", ("none", "jacobi", "flexible"))
def test_replay_is_the_references_update(S, pl):
    A, b = _spd(40, 3)
    M = nt.Jacobi(A)
    kw = dict(Pl=None) if pl == "none" else dict(Pl=M.solve, flexible=pl == "flexible")
    x, it, hist, al, be = lr.cg(A, b, maxiter=30, atol=1e-14, rtol=1e-10, **kw)
    xo, ito, histo = nt.cg(A, b, maxiter=30, atol=1e-14, rtol=1e-10, **kw)
    assert it == ito and it > 5 and np.array_equal(x, xo) and np.array_equal(hist, histo)   # the twin's CG is numpy_twin's CG
    assert al.size == it == be.size and be[0] == (b @ (b if pl == "none" else M.solve(b))) / 1.0
    k, delta, gamma = _literal_replay(al.tolist(), be.tolist(), 31)
    d, g = lr.diagnostic(al, be, 31)
    assert k == it and np.array_equal(d, delta) and np.array_equal(g, gamma)
    diag = S.LanczosDiagnostic(31)
    diag.update_(7.0, 7.0)                                    # a used diagnostic: the replay starts with reset!
    diag.replay_(al, be)
    assert diag.k == it and np.array_equal(diag.delta, delta) and np.array_equal(diag.gamma, gamma)
    assert S.estimate_(diag) == lr.estimate(delta, gamma, k)
    # the off-diagonal is the reference's sqrt(beta_k)/alpha_k, not the textbook sqrt(beta_k)/alpha_{k-1}
    assert gamma[3] == math.sqrt(be[3]) / al[3] != math.sqrt(be[3]) / al[2]


def test_a_negative_beta_stores_nan(S):
    diag = S.LanczosDiagnostic(3).replay_([0.5, 0.25], [2.0, -1.0])
    assert diag.k == 2 and diag.delta[1] == 1.0 / 0.25 + -1.0 / 0.5 and np.isnan(diag.gamma[1]) and diag.gamma[2] == 0.0
    d, g = lr.diagnostic([0.5, 0.25], [2.0, -1.0], 3)
    assert np.array_equal(d, diag.delta) and np.isnan(g[1])


def test_estimate_against_eigvalsh(S):
    delta = np.array([2.0, 3.0, 1.5, 4.0, 9.0, 0.0])
    gamma = np.array([77.0, 0.5, -0.25, 1.0, 2.0, 0.0])       # gamma[0] is never read
    diag = S.LanczosDiagnostic(6)
    for d, g in zip(delta[:5], gamma[:5]):
        diag.update_(d, g)
    assert diag.k == 5
    T = np.diag(delta[:5]) + np.diag(gamma[1:5], 1) + np.diag(gamma[1:5], -1)
    lam = np.linalg.eigvalsh(T)
    want = abs(lam[-1] / lam[0])
    assert abs(S.estimate_(diag) - want) <= 1e-14 * want and abs(lr.estimate(delta, gamma, 5) - want) <= 1e-14 * want
    for k in (0, 1):
        diag.reset_()
        assert diag.k == 0 and not diag.delta.any() and not diag.gamma.any()
        for _ in range(k):
            diag.update_(3.0, 1.0)
        assert S.estimate_(diag) == 1.0 and lr.estimate(delta, gamma, k) == 1.0


# ---------------------------------------------------------------- the Lanczos bound of the Chebyshev smoother
class _Identity:
    def solve(self, r):
        return r.copy()


def test_five_distinct_eigenvalues_are_found_in_five_steps():
    eigs = np.array([0.5, 1.0, 2.0, 3.5, 8.0])
    A = sp.diags(np.repeat(eigs, (7, 3, 9, 4, 6))).tocsr()
    T, k = lr.lanczos_tridiagonal(A, _Identity(), 5)
    assert k == 5 and np.max(np.abs(np.linalg.eigvalsh(T) - eigs)) <= 1e-10
    T, k, gs = lr.lanczos_tridiagonal(A, _Identity(), 12, with_gammas=True)
    assert k == 5 and gs.size == 5                            # the 1e-24 stop fires at step 6
    assert abs(lr.lanczos_lambda_max(A, _Identity(), 12) - 8.0) <= 1e-10
    with pytest.raises(np.linalg.LinAlgError):
        lr.lanczos_lambda_max(-A, _Identity(), 5)


def _patch_operator(A, pp, pd):
    """M^-1 = sum_p R_p^T inv(A_pp) R_p as a sparse matrix"""
    A = A.tocsr()
    rows, cols, vals = [], [], []
    for p in range(pp.size - 1):
        d = np.asarray(pd[pp[p]:pp[p + 1]], dtype=np.int64)
        if d.size == 0:
            continue
        X = np.linalg.inv(A[d][:, d].toarray())
        rows.append(np.repeat(d, d.size)); cols.append(np.tile(d, d.size)); vals.append(X.ravel())
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=A.shape)


class _Sparse:
    def __init__(self, B):
        self.B = B

    def solve(self, r):
        return self.B @ r


@pytest.mark.parametrize("case", ("jacobi-q1-16^3", "jacobi-q1-64^2", "patch-q2-6^3"))
def test_ten_lanczos_steps_cover_lambda_max_where_ten_power_steps_do_not(po, hierarchy, case):
    if case.startswith("jacobi"):
        H = hierarchy((16, 16, 16) if case.endswith("16^3") else (64, 64), 2, 1)
        A = H["mats"][0].to_scipy().tocsr()
        M = nt.Jacobi(A)
        s = sp.diags(np.sqrt(M.dinv))
        true = float(spla.eigsh(s @ A @ s, k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0])
    else:
        H = hierarchy((6, 6, 6), 2, 2)
        A = H["mats"][0].to_scipy().tocsr()
        pp, pd = po.vertex_star_patches((6, 6, 6), 2)
        B = _patch_operator(A, pp, pd)
        M = _Sparse(B)
        true = float(np.max(spla.eigs(B @ A, k=1, which="LM", tol=1e-12, return_eigenvectors=False).real))
    lan, pw = lr.lanczos_lambda_max(A, M, 10), cr.power_iteration(A, M, 10)
    print(case, "true %.4f lanczos(10) %.4f power(10) %.4f" % (true, lan, pw))
    assert lan <= true * (1.0 + 1e-10)                         # a Ritz value never exceeds lambda_max
    assert 1.1 * lan >= true
    if case.startswith("jacobi"):
        assert pw < lan                                        # the same ten steps: the power estimate is the lower one
    if case == "jacobi-q1-16^3":
        # 1.1 * power(10) misses lambda_max (1.474 < 1.4763).  On 64^2 it does not: 1.1 * 1.390 = 1.529 > 1.4988, so the same
        # assertion cannot hold there (the figures are those of the table this feature was specified with); on 32^3, too slow for a
        # unit test, it misses again (1.1 * 1.336 = 1.470 < 1.494)
        assert 1.1 * pw < true


# ---------------------------------------------------------------- the refusals of the Python layer
def test_python_layer_refusals(S, po, hierarchy):
    with pytest.raises(ValueError):
        S.ChebyshevSmoother(S.JacobiLinearSolver(), 3, eig_method="arnoldi")
    assert S.ChebyshevSmoother(S.JacobiLinearSolver(), 3).eig_method == "power"
    assert S.ChebyshevSmoother(S.JacobiLinearSolver(), 3, eig_method="lanczos").eig_method == "lanczos"
    with pytest.raises(TypeError):
        S.CGSolver(None, diagnostic=np.zeros(3))
    assert S.CGSolver(None).diag is None
    with pytest.raises(ValueError):
        S.LanczosDiagnostic(-1)
    H = hierarchy((4, 4), 2, 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"])
    A = H["mats"][0]
    short = S.CGSolver((None, gmg), maxiter=10, diagnostic=S.LanczosDiagnostic(9))
    with pytest.raises(ValueError, match="9 iterations"):       # the reference: a BoundsError in iteration 10
        S.numerical_setup(S.symbolic_setup(short, A), A)
    block = S.CGSolver(S.BlockDiagonalSolver([gmg, gmg]), maxiter=10, diagnostic=S.LanczosDiagnostic(11))
    with pytest.raises(ValueError, match="block system"):
        S.numerical_setup(S.symbolic_setup(block, A), A)
