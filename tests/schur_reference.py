"""numpy restatement of solve!(x, ::SchurComplementNumericalSetup, y), LinearSolvers/SchurComplementSolvers.jl:55-74:

    [A B]^-1   [I  -A^-1 B] [A^-1     ] [   I       ]
    [C D]    = [      I   ] [     S^-1] [-C A^-1  I ]          S ~ D - C A^-1 B

Test infrastructure only.  `solveA(x, b)` / `solveS(x, b)` stand for solve!(x, A, b) / solve!(x, S, b): they work in place on x, whose
content on entry is the initial guess (an exact solver overwrites it).  B and C are anything with `@` (numpy arrays, scipy sparse
matrices).  `cache` is the (du, bu, bp) tuple of the numerical setup (:42-47,58): only du matters between applications -- it is the
initial guess of the second A-solve -- so the cache object keeps that one vector."""
import numpy as np


class SchurCache:
    """ns.caches (get_shur_complement_caches, :42-47): du persists between applications, zero before the first."""

    def __init__(self, n_u):
        self.du = np.zeros(n_u)


def schur_apply(x, y, solveA, solveS, B, C, cache):
    """solve!(x, ns, y) in place on x (its content on entry: the block solvers' initial guesses); returns x."""
    n_u = cache.du.size
    y_u, y_p = y[:n_u], y[n_u:]                                             # :61
    x_u, x_p = x[:n_u], x[n_u:]                                             # :62 (views: the solves write into x)
    solveA(x_u, y_u)                                                        # :65 x_u = A^-1 y_u
    bp = y_p - C @ x_u                                                      # :66 bp = y_p - C (A^-1 y_u)
    solveS(x_p, bp)                                                         # :67 x_p = S^-1 bp
    bu = B @ x_p                                                            # :69 bu = B x_p
    solveA(cache.du, bu)                                                    # :70 du = A^-1 bu
    x_u -= cache.du                                                         # :71 x_u = x_u - du
    return x


# ---------------------------------------------------------------- block solvers as in-place callables
def exact_solver(M):
    """LUSolver(): a dense M through numpy.linalg.solve, a sparse one through scipy's splu"""
    if isinstance(M, np.ndarray):
        def solve(x, b):
            x[:] = np.linalg.solve(M, b)
        return solve
    import scipy.sparse.linalg as spla
    lu = spla.splu(M.tocsc())

    def solve(x, b):
        x[:] = lu.solve(np.ascontiguousarray(b))
    return solve


def jacobi_solver(M):
    """JacobiLinearSolver(), JacobiLinearSolvers.jl:43-47: x = inv_diag .* b"""
    dinv = 1.0 / (M.diagonal() if hasattr(M, "diagonal") else np.diag(M))

    def solve(x, b):
        x[:] = dinv * b
    return solve


def cg_jacobi_solver(M, maxiter=1000, atol=1e-12, rtol=1e-6, log=None):
    """CGSolver(JacobiLinearSolver(); maxiter, atol, rtol), solve! of Krylov/CGSolvers.jl:73-120 (flexible = false), the stopping
    rule of SolverTolerances.jl:117-128.  x on entry is the initial guess.  log (a dict, optional) receives num_iters."""
    dinv = 1.0 / (M.diagonal() if hasattr(M, "diagonal") else np.diag(M))

    def solve(x, b):
        r = b - M @ x                                                       # :79
        p = np.zeros_like(r); z = np.zeros_like(r)                          # :80-81
        gamma = 1.0                                                         # :82
        res = float(np.linalg.norm(r)); res0 = res                          # :85
        it = 0
        done = it >= maxiter or 1.0 < rtol or res < atol                    # :86 init!(log,res)
        while not done:                                                     # :88
            z = dinv * r                                                    # :94 solve!(z,Pl,r)
            beta = gamma; gamma = float(z @ r); beta = gamma / beta         # :95
            p = z + beta * p                                                # :101
            w = M @ p                                                       # :104
            alpha = gamma / float(p @ w)                                    # :105
            x += alpha * p                                                  # :108
            r -= alpha * w                                                  # :109
            res = float(np.linalg.norm(r)); it += 1                         # :111
            done = it >= maxiter or res / res0 < rtol or res < atol         # :112 update!(log,res)
        if log is not None:
            log["num_iters"] = it
    return solve
