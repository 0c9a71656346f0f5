"""numpy restatement of solve!(x, ::GMRESNumericalSetup, b), Krylov/GMRESSolvers.jl:132-210, with krylov_mul! / krylov_residual!
(KrylovUtils.jl:17-54), the restart rule (:31-37), the growth of the caches (:76-92), the stopping rule of
SolverTolerances.jl:117-128 and the ConvergenceLog of ConvergenceLogs.jl (init! / update! / finalize!).

Test infrastructure only.  `A(v)` is the mat-vec, `Pr(r)` / `Pl(r)` the right / left preconditioner (None: nothing), `dot` / `norm`
the reductions -- numpy's by default; the GPU tests pass the oracle's (orc.spmv, orc.dot, orc.norm, orc.givens) so that the
reference runs on the same CPU checker as the other parity tests."""
import numpy as np

import __graft_entry__ as entry

CONVERGED_ATOL, CONVERGED_RTOL, DIVERGED_MAXITER, DIVERGED_BREAKDOWN = 0, 1, 2, 3


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


def gmres(A, b, m, Pr=None, Pl=None, x0=None, restart=False, m_add=1, maxiter=100, atol=1e-12, rtol=1e-6, dot=None, norm=None,
          givens=None, info=None):
    """-> (x, niters, flag, hist).  hist[k] = beta after k iterations (hist[0] = norm(Pl(b - A x0))).
    info (a dict, optional) receives the final basis length and the number of Arnoldi cycles."""
    dot = dot or (lambda u, v: float(np.dot(u, v)))
    norm = norm or (lambda u: float(np.linalg.norm(u)))
    givens = givens or entry.import_oracle().givens
    b = np.asarray(b, dtype=np.float64)
    n = b.size
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)

    def residual(x):                                                        # krylov_residual!, KrylovUtils.jl:46-54
        w = b - A(x)
        return Pl(w) if Pl is not None else w

    def mul(v):                                                             # krylov_mul!, KrylovUtils.jl:17-32
        wr = Pr(v) if Pr is not None else v
        wl = A(wr)
        return Pl(wl) if Pl is not None else wl

    m0 = int(m)
    V = [np.zeros(n) for _ in range(m0 + 1)]                                # :60
    mc = m0                                                                 # krylov_cache_length, :71-74
    H, g, c, s = np.zeros((mc + 1, mc)), np.zeros(mc + 1), np.zeros(mc), np.zeros(mc)   # :64-67

    V[0] = residual(x)                                                      # :143
    beta = norm(V[0])                                                       # :144
    hist = [beta]                                                           # :145 init!(log, beta)
    niter, cycles = 0, 0
    done = _finished(niter, beta, 1.0, maxiter, atol, rtol)
    while not done:                                                         # :146
        cycles += 1
        j = 1                                                               # :148
        V[0] = V[0] / beta                                                  # :149
        H[:] = 0.0                                                          # :150
        g[:] = 0.0; g[0] = beta                                             # :151
        while not done and not (restart and j > m0):                        # :152, restart(solver, j) :31-37
            if j > mc:                                                      # :154-157, expand_krylov_caches! :76-92
                mn = mc + m_add
                V.extend(np.zeros(n) for _ in range(m_add))
                Hn = np.zeros((mn + 1, mn)); Hn[: mc + 1, :mc] = H
                gn = np.zeros(mn + 1); gn[: mc + 1] = g
                cn = np.zeros(mn); cn[:mc] = c
                sn = np.zeros(mn); sn[:mc] = s
                H, g, c, s, mc = Hn, gn, cn, sn, mn
            w = mul(V[j - 1])                                               # :160-161
            for i in range(1, j + 1):                                       # :162-165 modified Gram-Schmidt
                H[i - 1, j - 1] = dot(w, V[i - 1])
                w = w - H[i - 1, j - 1] * V[i - 1]
            H[j, j - 1] = norm(w)                                           # :166
            V[j] = w / H[j, j - 1]                                          # :167
            for i in range(1, j):                                           # :170-174
                gam = c[i - 1] * H[i - 1, j - 1] + s[i - 1] * H[i, j - 1]
                H[i, j - 1] = -s[i - 1] * H[i - 1, j - 1] + c[i - 1] * H[i, j - 1]
                H[i - 1, j - 1] = gam
            c[j - 1], s[j - 1], _ = givens(H[j - 1, j - 1], H[j, j - 1])    # :177
            H[j - 1, j - 1] = c[j - 1] * H[j - 1, j - 1] + s[j - 1] * H[j, j - 1]; H[j, j - 1] = 0.0   # :178
            g[j] = -s[j - 1] * g[j - 1]; g[j - 1] = c[j - 1] * g[j - 1]     # :179
            beta = abs(g[j])                                                # :181
            j += 1                                                          # :182
            niter += 1                                                      # :183 update!(log, beta)
            hist.append(beta)
            done = _finished(niter, beta, beta / hist[0], maxiter, atol, rtol)
        j -= 1                                                              # :185
        for i in range(j, 0, -1):                                           # :188-190 back substitution
            acc = 0.0
            for k in range(i + 1, j + 1):
                acc += H[i - 1, k - 1] * g[k - 1]
            g[i - 1] = (g[i - 1] - acc) / H[i - 1, i - 1]
        if Pr is None:                                                      # :193-196
            for i in range(1, j + 1):
                x = x + g[i - 1] * V[i - 1]
        else:                                                               # :198-203
            zl = np.zeros(n)
            for i in range(1, j + 1):
                zl = zl + g[i - 1] * V[i - 1]
            x = x + Pr(zl)
        V[0] = residual(x)                                                  # :205
    flag = _flag(niter, beta, beta / hist[0], maxiter, atol, rtol)          # :208 finalize!(log, beta)
    if info is not None:
        info["basis"], info["cycles"] = len(V), cycles
    return x, niter, flag, np.array(hist)
