"""numpy restatement of SolverInterfaces/NullSpaces.jl:33-139 (is_orthonormal, is_orthogonal, gram_schmidt!, modified_gram_schmidt!,
project!, make_orthogonal!, reconstruct!) and LinearSolvers/NullspaceSolvers.jl:59-120 (the :constrained and :projected solve!).

Test infrastructure only.  `dot` / `norm` are the reductions -- numpy's by default; the GPU tests pass the oracle's (orc.dot,
orc.norm) so that the reference runs on the same CPU checker as the other parity tests.  Vectors are numpy arrays, a null space is
a list of them; the functions with a trailing underscore mutate their argument as the reference's `!` functions do."""
import numpy as np


def _dot(dot):
    return dot or (lambda u, v: float(np.dot(u, v)))


def _norm(norm):
    return norm or (lambda u: float(np.linalg.norm(u)))


def nullspace_of_matrix(A):
    """NullSpace(A::Matrix), NullSpaces.jl:23-26: eachcol(nullspace(A)) -- LinearAlgebra.nullspace keeps the right singular vectors
    whose singular value is <= min(size(A)) * eps * sigma_max."""
    A = np.asarray(A, dtype=np.float64)
    _u, sv, vt = np.linalg.svd(A, full_matrices=True)
    tol = min(A.shape) * np.finfo(np.float64).eps * (sv[0] if sv.size else 0.0)
    r = int(np.sum(sv > tol))
    return [vt[i].copy() for i in range(r, A.shape[1])]


def is_orthogonal(V, other=None, tol=1e-12, dot=None, norm=None, A=None):
    """:40-47 (other = None), :49-55 (other = a vector), :57-65 (A = a mat-vec callable)"""
    dot, norm = _dot(dot), _norm(norm)
    if A is not None:
        for w in V:                                                              # :60-63
            if not (abs(norm(A(w))) < tol):
                return False
        return True
    if other is not None:
        assert len(other) == len(V[0])                                          # :50
        for w in V:                                                              # :51-53
            if not (abs(dot(w, other)) < tol):
                return False
        return True
    for k, w in enumerate(V):                                                    # :41-45
        for v in V[k + 1:]:
            if not (abs(dot(w, v)) < tol):
                return False
    return True


def is_orthonormal(V, tol=1e-12, dot=None, norm=None):
    """:33-38"""
    nrm = _norm(norm)
    for w in V:
        if not (abs(nrm(w) - 1.0) < tol):
            return False
    return is_orthogonal(V, tol=tol, dot=dot, norm=norm)


def gram_schmidt_(V, dot=None, norm=None):
    """:78-88"""
    dot, norm = _dot(dot), _norm(norm)
    n = len(V)
    for j in range(n):                                                           # :80
        for i in range(j):                                                       # :81
            a = dot(V[j], V[i])                                                  # :82
            V[j] -= a * V[i]                                                     # :83
        V[j] /= norm(V[j])                                                       # :85
    return V


def modified_gram_schmidt_(V, dot=None, norm=None):
    """:90-100"""
    dot, norm = _dot(dot), _norm(norm)
    n = len(V)
    for j in range(n):                                                           # :92
        V[j] /= norm(V[j])                                                       # :93
        for i in range(j + 1, n):                                                # :94
            a = dot(V[j], V[i])                                                  # :95
            V[i] -= a * V[j]                                                     # :96
    return V


def project_(p, V, v, dot=None):
    """:107-116 -> (p, alpha)"""
    dot = _dot(dot)
    assert len(v) == len(V[0])                                                   # :108
    alpha = np.zeros(len(V))                                                     # :109
    p[:] = 0.0                                                                   # :110
    for k, w in enumerate(V):                                                    # :111
        alpha[k] = dot(v, w)                                                     # :112
        p += alpha[k] * w                                                        # :113
    return p, alpha


def project(V, v, dot=None):
    """:102-105"""
    return project_(np.empty_like(v), V, v, dot=dot)


def make_orthogonal_(V, v, dot=None):
    """:118-126 -> (v, alpha)"""
    dot = _dot(dot)
    assert len(v) == len(V[0])                                                   # :119
    alpha = np.zeros(len(V))                                                     # :120
    for k, w in enumerate(V):                                                    # :121
        alpha[k] = dot(v, w)                                                     # :122
        v -= alpha[k] * w                                                        # :123
    return v, alpha


def reconstruct_(V, v, alpha):
    """:134-139"""
    for k, w in enumerate(V):
        v += alpha[k] * w                                                        # :136
    return v


def reconstruct(V, v, alpha):
    """:128-132"""
    return reconstruct_(V, v.copy(), alpha)


# ---- NullspaceSolvers.jl ---------------------------------------------------------------------------------------------------
def augmented_matrix(A, V):
    """:65-66  mat = [A K; K' zeros(nK,nK)] with K = stack(N.V) (dense)"""
    K = np.stack(V, axis=1)
    nK = K.shape[1]
    return np.block([[np.asarray(A, dtype=np.float64), K], [K.T, np.zeros((nK, nK))]])


def solve_constrained(A, V, b, x=None, direct=None):
    """solve!(x, ::NullspaceSolverNS{:constrained}, b), :92-107, with `direct(mat, rhs)` the inner direct solver"""
    direct = direct or np.linalg.solve
    nV, nK = len(b), len(V)
    mat = augmented_matrix(A, V)
    w2 = np.zeros(nV + nK)                                                       # :102-103
    w2[:nV] = b
    w1 = direct(mat, w2)                                                         # :104
    return w1[:nV].copy()                                                        # :105


def projected_guess(V, x, dot=None):
    """:115-116  w1, alpha = project!(w1, N, x) ; x .-= w1 -> the vector the inner solver starts from"""
    w1, _alpha = project(V, x, dot=dot)
    return x - w1


def solve_projected(V, x, b, inner, dot=None, norm=None):
    """solve!(x, ::NullspaceSolverNS{:projected}, b), :109-120, after the make_orthonormal!(N) of the numerical setup (:68), which
    mutates V.  `inner(x0, b)` runs the wrapped solver from the initial guess x0 and returns whatever it returns."""
    return inner(projected_guess(V, x, dot=dot), b)                              # :117
