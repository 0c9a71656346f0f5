"""numpy restatement of the two Lanczos pieces of the device library; this file is the definition the device is held to.  Plain helper:
numpy / scipy only, no fixtures, no collection hooks.

  cg(A, b, Pl, ...)                 solve!(x, ::CGNumericalSetup, b) (Krylov/CGSolvers.jl:73-120) for Pl none / callable / flexible,
                                    returning the scalars as well: (x, iterations, history, alpha, beta)
  diagnostic(alpha, beta)           what the solve does to a LanczosDiagnostic (CGSolvers.jl:87,114-115,128-138) -> (delta, gamma).
                                    VERBATIM the reference: gamma_k = sqrt(beta_k) / alpha_k, where the textbook Lanczos matrix has
                                    sqrt(beta_k) / alpha_{k-1}
  estimate(delta, gamma)            estimate! (KrylovUtils.jl:83-90)
  lanczos_tridiagonal(A, M, steps)  the CG loop of ChebyshevSmoother(eig_method="lanczos") on chebyshev_reference.start_vector and its M
                                    objects -> (T in the TEXTBOOK form, steps done)
  lanczos_lambda_max(A, M, steps)   its largest eigenvalue, the lambda_est of the setup
  LanczosCheb                       chebyshev_reference.Cheb whose bounds come from lanczos_lambda_max
"""
import math

import numpy as np

import chebyshev_reference as cr


def cg(A, b, Pl=None, maxiter=1000, atol=1e-12, rtol=1e-6, flexible=False, x0=None):
    x = np.zeros_like(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A @ x                                             # :79
    p = np.zeros_like(b); z = np.zeros_like(b)                # :80-81
    gamma = 1.0                                               # :82
    res = np.linalg.norm(r); hist = [res]                     # :85
    it = 0
    done = it >= maxiter or 1.0 < rtol or res < atol          # :86
    alphas, betas = [], []
    while not done:
        if Pl is None:                                        # :90-92
            z = r.copy(); beta = gamma; gamma = r @ r; beta = gamma / beta
        elif not flexible:                                    # :93-95
            z = Pl(r); beta = gamma; gamma = z @ r; beta = gamma / beta
        else:                                                 # :96-99
            delta = z @ r; z = Pl(r); beta = gamma; gamma = z @ r; beta = (gamma - delta) / beta
        p = z + beta * p                                      # :101
        w = A @ p                                             # :104
        alpha = gamma / (p @ w)                               # :105
        x += alpha * p                                        # :108
        r -= alpha * w                                        # :109
        res = np.linalg.norm(r); hist.append(res); it += 1    # :111-112
        done = it >= maxiter or res / hist[0] < rtol or res < atol
        alphas.append(float(alpha)); betas.append(float(beta))    # :114
    return x, it, np.array(hist), np.array(alphas), np.array(betas)


def diagnostic(alpha, beta, max_iters=None):
    """-> (delta, gamma), zeros of length max_iters (default: the number of iterations) with the first len(alpha) entries filled"""
    k = len(alpha)
    m = k if max_iters is None else max_iters
    delta, gamma = np.zeros(m), np.zeros(m)
    alpha_last = 1.0
    for i in range(k):
        ak, bk = float(alpha[i]), float(beta[i])
        if i == 0:
            delta[i], gamma[i] = 1.0 / ak, 0.0
        else:
            delta[i] = (1.0 / ak) + (bk / alpha_last)
            gamma[i] = (math.sqrt(bk) if bk >= 0.0 else math.nan) / ak
        alpha_last = ak
    return delta, gamma


def estimate(delta, gamma, k=None):
    k = len(delta) if k is None else k
    if k < 2:
        return 1.0
    T = np.diag(np.asarray(delta[:k], dtype=np.float64)) + np.diag(gamma[1:k], 1) + np.diag(gamma[1:k], -1)
    lam = np.linalg.eigvalsh(T)
    return abs(lam.max() / lam.min())


def lanczos_tridiagonal(A, M, steps, with_gammas=False):
    r = cr.start_vector(A.shape[0])
    gamma_old, gamma0 = 1.0, None
    p = None
    al, be, gs = [], [], []
    k = 0
    while k < steps:
        z = M.solve(r)
        gamma = float(z @ r)
        if not (np.isfinite(gamma) and gamma > 0.0):
            break
        if k == 0:
            gamma0 = gamma
        elif gamma < 1e-24 * gamma0:
            break
        beta = gamma / gamma_old
        p = z.copy() if k == 0 else z + beta * p
        w = A @ p
        pw = float(p @ w)
        if not (np.isfinite(pw) and pw > 0.0):
            break
        alpha = gamma / pw
        r = r - alpha * w
        al.append(alpha); be.append(beta); gs.append(gamma)
        gamma_old = gamma
        k += 1
    T = np.zeros((k, k))
    for i in range(k):
        T[i, i] = 1.0 / al[i] + (be[i] / al[i - 1] if i > 0 else 0.0)
        if i + 1 < k:
            T[i, i + 1] = T[i + 1, i] = math.sqrt(be[i + 1]) / al[i]
    return (T, k, np.array(gs)) if with_gammas else (T, k)


def lanczos_lambda_max(A, M, steps):
    T, k = lanczos_tridiagonal(A, M, steps)
    if k == 0:
        raise np.linalg.LinAlgError("the Lanczos estimate recorded no step: M^-1 A is not positive definite")
    return float(np.linalg.eigvalsh(T).max())


class LanczosCheb(cr.Cheb):
    """chebyshev_reference.Cheb with eig_method = "lanczos" """

    def setup(self, A):
        M = cr.make_M(self.M, A)
        kw = self.kw
        if kw["lambda_max"] is None:
            est = lanczos_lambda_max(A, M, kw["eig_steps"])
            lmax = kw["eig_safety"] * est
        else:
            est, lmax = float("nan"), float(kw["lambda_max"])
        lmin = lmax / kw["eig_ratio"] if kw["lambda_min"] is None else float(kw["lambda_min"])
        return A, M, cr.coefficients(self.degree, lmin, lmax), (est, lmin, lmax)
