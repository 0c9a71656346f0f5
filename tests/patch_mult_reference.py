"""numpy twin of the multiplicative patch smoother (csrc/pmult.inc.hpp, kernels.hpp patch_mult_*): plain helper, numpy and scipy only.

conflict rule      patches p, q conflict when they share a dof or a stored entry of A (either direction, explicit zeros count)
                   joins a dof of one to a dof of the other
greedy_coloring    first-fit in patch order on that rule -> (color, ncolors)
first_conflict     the first pair of equally coloured patches in conflict, or None
stored_row_sums    s_i = sum_k a(i, k) v[k] over the row in its STORED order, from 0.0, product and sum rounded separately -- what
                   the sweep kernels and the SELL-64 operator kernel compute
smooth             one pass: dx = 0; niter sweeps over the patches sorted stably by (colour, patch index), forward and / or
                   backward; x = x + dx; r = r - A dx
factor_inverse     the inverse the library builds from the caller's lu! factors
PMult              smoother object for gs_reference.GMG (setup / smooth), next to chebyshev_reference.Rich

The inverse blocks are patch_edge_problems.twin_inverses (the bits the device builds) or, lapack=True, numpy.linalg.inv."""
import numpy as np
import scipy.sparse as sp

import patch_edge_problems as pe

TYPES = ("symmetric", "forward", "backward")


def stored_csr(A):
    """scipy CSR of A with the storage order and the explicit zeros it came with"""
    A = A if sp.isspmatrix_csr(A) else sp.csr_matrix(A)
    return A


def _touched(A):
    """structural S = pattern(A) + pattern(A)^T + I as CSR of ones: row i lists the dofs that i is coupled to (and i)"""
    n = A.shape[0]
    P = sp.csr_matrix((np.ones(A.indices.size), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    S = (P + P.T + sp.identity(n, format="csr")).tocsr()
    S.sort_indices()
    return S


def _incidence(n, pp, pd):
    inc = [[] for _ in range(n)]
    for p in range(pp.size - 1):
        for i in pd[pp[p]:pp[p + 1]]:
            inc[int(i)].append(p)
    return inc


def neighbours(S, inc, pp, pd, p):
    """the patches in conflict with p (p itself excluded)"""
    dofs = pd[pp[p]:pp[p + 1]]
    if dofs.size == 0:
        return set()
    touched = np.unique(np.concatenate([S.indices[S.indptr[i]:S.indptr[i + 1]] for i in dofs]))
    out = set()
    for j in touched:
        out.update(inc[int(j)])
    out.discard(p)
    return out


def greedy_coloring(A, pp, pd):
    A = stored_csr(A)
    S, inc = _touched(A), _incidence(A.shape[0], pp, pd)
    npatch = pp.size - 1
    color = np.full(npatch, -1, dtype=np.int32)
    for p in range(npatch):
        held = {int(color[q]) for q in neighbours(S, inc, pp, pd, p) if q < p}
        c = 0
        while c in held:
            c += 1
        color[p] = c
    return color, (int(color.max()) + 1 if npatch else 0)


def first_conflict(A, pp, pd, color):
    """-> (q, p) with q < p, the first p that has one and its smallest q; None when the colouring is valid"""
    A = stored_csr(A)
    S, inc = _touched(A), _incidence(A.shape[0], pp, pd)
    for p in range(pp.size - 1):
        bad = sorted(q for q in neighbours(S, inc, pp, pd, p) if q < p and color[q] == color[p])
        if bad:
            return bad[0], p
    return None


def stored_row_sums(A, v, rows=None):
    rows = np.arange(A.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    start = A.indptr[rows].astype(np.int64)
    lens = A.indptr[rows + 1].astype(np.int64) - start
    s = np.zeros(rows.size)
    for j in range(int(lens.max()) if rows.size else 0):
        m = lens > j
        k = start[m] + j
        s[m] = s[m] + A.data[k] * v[A.indices[k]]
    return s


def patch_order(color, pp, forward=True):
    """non-empty patches sorted stably by (colour, patch index); backward: the colours descending"""
    p = np.array([q for q in range(pp.size - 1) if pp[q + 1] > pp[q]], dtype=np.int64)
    key = color[p] if forward else -color[p].astype(np.int64)
    return p[np.argsort(key, kind="stable")]


def sweep(A, X, pp, pd, order, omega, r0, dx):
    for p in order:
        rows = pd[pp[p]:pp[p + 1]]
        t = r0[rows] - stored_row_sums(A, dx, rows)
        d = np.zeros(rows.size)
        for k in range(rows.size):                           # row . vector, summed in column order (patch_apply_kernel)
            d = d + X[p][:, k] * t[k]
        dx[rows] = dx[rows] + omega * d


def correction(A, X, pp, pd, color, niter, omega, type_, r0):
    assert type_ in TYPES
    dx = np.zeros(A.shape[0])
    for _ in range(niter):
        if type_ != "backward":
            sweep(A, X, pp, pd, patch_order(color, pp, True), omega, r0, dx)
        if type_ != "forward":
            sweep(A, X, pp, pd, patch_order(color, pp, False), omega, r0, dx)
    return dx


def smooth(A, X, pp, pd, color, niter, omega, type_, x, r):
    """one pass, in place"""
    dx = correction(A, X, pp, pd, color, niter, omega, type_, r.copy())
    x[:] = x + dx
    r[:] = r - stored_row_sums(A, dx)
    return dx


def inverses(A, pp, pd, pivot=True, blocks=None, lapack=False):
    if not lapack:
        return pe.twin_inverses(A, pp, pd, None, pivot, blocks)
    out = []
    for p in range(pp.size - 1):
        B = blocks[p] if blocks is not None else pe.block(A, pd[pp[p]:pp[p + 1]], pd[pp[p]:pp[p + 1]])
        out.append(np.linalg.inv(B) if B.size else np.zeros((0, 0)))
    return out


def factor_inverse(F, ipiv):
    """the row-major inverse the library builds on the host from the caller's lu! factors (F: L and U in one matrix, ipiv: 1-based LAPACK
    pivots): ldiv!(F, I) column by column in getrs order -- the row swaps, L y = P e_c (unit diagonal), U x = y -- every update one
    rounded product and one rounded subtraction, exact zeros skipped"""
    n = F.shape[0]
    X = np.zeros((n, n))
    for c in range(n):
        col = np.zeros(n)
        col[c] = 1.0
        for r in range(n):
            q = int(ipiv[r]) - 1
            if q != r:
                col[r], col[q] = col[q], col[r]
        for k in range(n):
            if col[k] != 0.0:
                col[k + 1:] = col[k + 1:] - col[k] * F[k + 1:, k]
        for k in range(n - 1, -1, -1):
            if col[k] != 0.0:
                col[k] = col[k] / F[k, k]
                col[:k] = col[:k] - col[k] * F[:k, k]
        X[:, c] = col
    return X


class PMult:
    """MultiplicativePatchSmoother(PatchSolver(pp, pd), niter, omega, type, coloring) for gs_reference.GMG"""

    def __init__(self, pp, pd, niter=1, omega=1.0, type="symmetric", coloring=None, pivot=True, blocks=None, lapack=False):
        self.pp, self.pd, self.niter, self.omega, self.type = pp, pd, int(niter), float(omega), type
        self.coloring, self.pivot, self.blocks, self.lapack = coloring, pivot, blocks, lapack

    def setup(self, A):
        A = stored_csr(A)
        color = greedy_coloring(A, self.pp, self.pd)[0] if self.coloring is None else np.asarray(self.coloring)
        assert first_conflict(A, self.pp, self.pd, color) is None
        return A, inverses(A, self.pp, self.pd, self.pivot, self.blocks, self.lapack), color

    def smooth(self, ns, x, r):
        smooth(ns[0], ns[1], self.pp, self.pd, ns[2], self.niter, self.omega, self.type, x, r)


def product_form(A, X, pp, pd, order, omega):
    """I - prod_p (I - omega R_p^T inv(A_pp) R_p A), the factors applied in `order`: the operator E with dx = E r0 of one sweep"""
    n = A.shape[0]
    Ad = A.toarray()
    T = np.eye(n)                                             # error propagation of dx: e -> (I - B_p A) e
    for p in order:
        rows = pd[pp[p]:pp[p + 1]]
        B = np.zeros((n, n))
        B[np.ix_(rows, rows)] = omega * X[p]
        T = (np.eye(n) - B @ Ad) @ T
    return (np.eye(n) - T) @ np.linalg.inv(Ad)
