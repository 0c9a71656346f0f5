"""numpy / scipy restatement of the visiting orders of the Gauss-Seidel smoother (gmg_set_gs_ordering, csrc/gs.inc.hpp).  Plain helper:
numpy and scipy only, no fixtures, no collection hooks.

  stored_pattern / symmetrised_pattern   the pattern AS STORED, explicit zeros included, built from ones on indices / indptr --
                                         never from A + A.T on the values, which prunes the stored zeros (6 face couplings per row of the
                                         Q1 3-D operator) and then colours another graph
  greedy_colors / multicolor(A)          greedy first-fit in natural row order; the order is the rows sorted stably by colour
  permuted(A, order)                     B = A[order, order], rows sorted: the ordered sweeps of A are the natural sweeps of B
  forward / backward(A, order, r)        the ordered triangular solves: gs_reference.forward_rows / backward_rows on B and r[order],
                                         scattered back
  OrderedGS                              smoother object for gs_reference.GMG: triangular solves on B, r -= A @ dx in A's numbering
  krylov_reference(name, ordering)       gs_edge_problems.krylov_reference with every Gauss-Seidel smoother given that ordering
"""
import functools

import numpy as np
import scipy.sparse as sp

import gs_edge_problems as ge
import gs_reference as gr

# colours (= level sets per direction) of the structurally symmetric families under the multicolour order
COLORS = {"q1_3d-0": 8, "q1_3d-1": 8, "q1_2d": 4, "q2_3d": 27, "redblack": 2, "tridiagonal": 2, "diagonal": 1, "bidiagonal": 2, "one_row": 1}
SYMMETRIC_PATTERN = tuple(COLORS)
# the unsymmetric families: at most as many sets as colours
COLORS_UNSYMMETRIC = {"blocks": 10, "shuffled": 10}


def _csr_copy(A):
    A = sp.csr_matrix(A).copy()
    A.sort_indices()
    return A


def stored_pattern(A):
    A = sp.csr_matrix(A)
    return sp.csr_matrix((np.ones(A.indices.size), A.indices.copy(), A.indptr.copy()), shape=A.shape)


def symmetrised_pattern(A):
    P = stored_pattern(A)
    S = sp.csr_matrix(P + P.T)                                # sums of ones: nothing cancels, nothing is pruned
    S.sort_indices()
    return S


def greedy_colors(A):
    """every row, in natural order, takes the smallest colour no already-coloured neighbour holds (the diagonal is no neighbour)"""
    S = symmetrised_pattern(A)
    n = S.shape[0]
    color = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        nb = S.indices[S.indptr[i]:S.indptr[i + 1]]
        used = set(color[nb[nb < i]].tolist())
        c = 0
        while c in used:
            c += 1
        color[i] = c
    return color


def multicolor(A):
    """-> (order, color)"""
    color = greedy_colors(A)
    return np.argsort(color, kind="stable"), color


def inverse(order):
    pos = np.empty(len(order), dtype=np.int64)
    pos[np.asarray(order)] = np.arange(len(order))
    return pos


def permuted(A, order):
    """B = A[order, order] as sorted CSR, every stored entry kept (explicit zeros too)"""
    A = _csr_copy(A)
    order = np.asarray(order, dtype=np.int64)
    pos = inverse(order)
    lens = np.diff(A.indptr)[order]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    src = np.repeat(A.indptr[order] - indptr[:-1], lens) + np.arange(indptr[-1])
    B = sp.csr_matrix((A.data[src], pos[A.indices[src]], indptr), shape=A.shape)
    B.sort_indices()
    assert B.nnz == A.nnz
    return B


def forward(A, order, r, B=None):
    B = permuted(A, order) if B is None else B
    dx = np.empty_like(r)
    dx[order] = gr.forward_rows(B, r[order])
    return dx


def backward(A, order, r, B=None):
    B = permuted(A, order) if B is None else B
    dx = np.empty_like(r)
    dx[order] = gr.backward_rows(B, r[order])
    return dx


def resolve(A, ordering):
    """"natural" | "multicolor" | array -> order"""
    if isinstance(ordering, str):
        return np.arange(A.shape[0]) if ordering == "natural" else multicolor(A)[0]
    return np.asarray(ordering, dtype=np.int64)


class OrderedGS:
    """GaussSeidelSmoother(niter, omega, type, ordering) as the device runs it: the triangular solves on B = A[order, order] (the
    reference's column loops, bitwise the row-ordered ones: tests/test_gs_host.py), r -= A @ dx in the natural numbering"""

    def __init__(self, niter=1, omega=1.0, type="symmetric", ordering="multicolor"):
        assert type in gr.TYPES and niter > 0 and omega > 0.0
        self.niter, self.omega, self.type, self.ordering = int(niter), float(omega), type, ordering

    def setup(self, A):
        A = _csr_copy(A)
        order = resolve(A, self.ordering)
        return (A, order) + gr.GS().setup(permuted(A, order))

    def smooth(self, ns, x, r):
        A, order, B, diag, last = ns
        for _ in range(self.niter):
            for kind in ("forward", "backward"):
                if self.type not in (kind, "symmetric"):
                    continue
                t = r[order]
                t = gr.forward_sub(B, diag, last, t) if kind == "forward" else gr.backward_sub(B, diag, t)
                dx = np.empty_like(r)
                dx[order] = t
                dx = self.omega * dx
                x += dx
                r -= A @ dx

    def ldiv(self, ns, b):
        x, aux = np.zeros_like(b), b.copy()
        self.smooth(ns, x, aux)
        return x


def reference_smoother(spec, ordering):
    return OrderedGS(*spec[1:], ordering=ordering) if spec[0] == "gs" else gr.RJ(*spec[1:])


@functools.lru_cache(maxsize=None)
def krylov_reference(name, ordering="multicolor"):
    """gs_edge_problems.krylov_reference with every Gauss-Seidel smoother in the given ordering -> (x, iterations, residual history)"""
    c = ge.KRYLOV[name]
    po = ge._po()
    H = po.build_hierarchy(c["nc"], c["nlev"], 1)
    b = po.dirichlet_lift_rhs(c["nc"], 1)
    A = _csr_copy(H["mats"][0].to_scipy())
    pre, post = reference_smoother(c["pre"], ordering), reference_smoother(c["post"], ordering)
    G = gr.GMG(H["mats"], H["prolongations"], H["restrictions"], [pre] * (c["nlev"] - 1), [post] * (c["nlev"] - 1), cycle=c["cycle"])
    kw = dict(maxiter=100, atol=1e-14, rtol=c["rtol"])
    if c["solver"] == "cg_smoother":
        ns = pre.setup(A)
        return gr.cg(A, b, Pl=lambda r: pre.ldiv(ns, r), **kw)
    if c["solver"] == "cg":
        return gr.cg(A, b, Pl=G.solve, **kw)
    if c["solver"] == "fgmres":
        return gr.fgmres(A, b, Pr=G.solve, m=5, **kw)
    return G.solver(b, **kw)


# iteration counts of the Krylov cases with every Gauss-Seidel smoother in the multicolour order (tests/test_gs_ordering_host.py
# asserts them and that none sits on an edge; tests/test_gpu_gs_ordering.py repeats them on the device)
KRYLOV_ITERS = {"smoother-2d": 5, "smoother-3d": 4, "cg-2d-sym": 5, "cg-3d-mixed": 5, "fgmres-3d-fwd": 4, "cg-2d-wcycle": 3, "gmg-solver-2d": 6}
