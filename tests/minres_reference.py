"""numpy transcription of solve!(x, ::MINRESNumericalSetup, b), Krylov/MINRESSolvers.jl:75-148, with the stopping rule of
SolverTolerances.jl:117-128 and the ConvergenceLog of ConvergenceLogs.jl (init! / update! / finalize!).

Test infrastructure only.  `A(v)` is the mat-vec, `Pl(r)` the preconditioner (None: copy!), `dot` / `norm` the reductions --
numpy's by default; the GPU tests pass the oracle's (orc.spmv, orc.dot, orc.norm) so that the reference runs on the same CPU
checker as the other parity tests.  The rotation is the oracle's LinearAlgebra.givensAlgorithm (orc.givens)."""
import numpy as np

import __graft_entry__ as entry

CONVERGED_ATOL, CONVERGED_RTOL, DIVERGED_MAXITER, DIVERGED_BREAKDOWN = 0, 1, 2, 3


class NotPositiveDefinite(ValueError):
    """@check beta_p > 0 (:97) / DomainError of sqrt(beta_p) (:116): the preconditioner is not positive definite."""


def _finished(niter, e_a, e_r, maxiter, atol, rtol):
    return niter >= maxiter or e_r < rtol or e_a < atol                     # SolverTolerances.jl:117-128


def _flag(niter, e_a, e_r, maxiter, atol, rtol):
    if e_r < rtol:
        return CONVERGED_RTOL
    if e_a < atol:
        return CONVERGED_ATOL
    if niter >= maxiter:
        return DIVERGED_MAXITER
    return DIVERGED_BREAKDOWN


def minres(A, b, Pl=None, x0=None, maxiter=1000, atol=1e-12, rtol=1e-6, dot=None, norm=None, givens=None):
    """-> (x, niters, flag, hist).  hist[k] = beta_r after k iterations (hist[0] = norm(Pl(b - A x0)))."""
    dot = dot or (lambda u, v: float(np.dot(u, v)))
    norm = norm or (lambda u: float(np.linalg.norm(u)))
    givens = givens or entry.import_oracle().givens
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    Vnew, V, Vold = np.zeros(n), np.zeros(n), np.zeros(n)                   # :80-82 (caches :39-44)
    Wnew, W, Wold = np.zeros(n), np.zeros(n), np.zeros(n)
    Znew, Z, Zold = np.zeros(n), np.zeros(n), np.zeros(n)

    Vnew = b - A(x)                                                         # :90-91
    Znew = Pl(Vnew) if Pl is not None else Vnew.copy()                      # :92-93

    beta_r = norm(Znew)                                                     # :95
    beta_p = dot(Znew, Vnew)                                                # :96
    if not beta_p > 0.0:                                                    # :97
        raise NotPositiveDefinite(f"beta_p = {beta_p}")

    gamma, gamma_old = np.sqrt(beta_p), 1.0                                 # :99
    c, c_old = 1.0, 1.0                                                     # :100
    s, s_old = 0.0, 0.0                                                     # :101

    V = Vnew / gamma                                                        # :103
    Z = Znew / gamma                                                        # :104

    eta = gamma                                                             # :106
    hist = [beta_r]                                                         # :107 init!(log, beta_r)
    niter = 0
    done = _finished(niter, beta_r, 1.0, maxiter, atol, rtol)
    while not done:
        Vnew = A(Z)                                                         # :110
        Znew = Pl(Vnew) if Pl is not None else Vnew.copy()                  # :111
        delta = dot(Vnew, Z)                                                # :112
        Vnew = Vnew - delta * V - gamma * Vold                              # :113
        Znew = Znew - delta * Z - gamma * Zold                              # :114
        beta_p = dot(Znew, Vnew)                                            # :115
        if beta_p < 0.0:                                                    # :116 sqrt -> DomainError
            raise NotPositiveDefinite(f"beta_p = {beta_p} in iteration {niter + 1}")
        gamma_new = np.sqrt(beta_p)                                         # :116

        Vnew = Vnew / gamma_new                                             # :118
        Znew = Znew / gamma_new                                             # :119

        alpha0 = c * delta - c_old * s * gamma                              # :122
        c_new, s_new, alpha1 = givens(alpha0, gamma_new)                    # :123
        alpha2 = s * delta + c_old * c * gamma                              # :124
        alpha3 = s_old * gamma                                              # :125

        Wnew = (Z - alpha2 * W - alpha3 * Wold) / alpha1                    # :128
        x = x + (c_new * eta) * Wnew                                        # :129
        eta = -s_new * eta                                                  # :130

        beta_r = abs(s_new) * beta_r                                        # :133

        Vold, V = V, Vnew                                                   # :136-142 swap3
        Wold, W = W, Wnew
        Zold, Z = Z, Znew
        gamma_old, gamma = gamma, gamma_new
        c_old, c = c, c_new
        s_old, s = s, s_new

        niter += 1                                                          # :144 update!(log, beta_r)
        hist.append(beta_r)
        done = _finished(niter, beta_r, beta_r / hist[0], maxiter, atol, rtol)
    flag = _flag(niter, beta_r, beta_r / hist[0], maxiter, atol, rtol)      # :147 finalize!
    return x, niter, flag, np.array(hist)
