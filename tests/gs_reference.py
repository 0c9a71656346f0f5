"""numpy / scipy restatement of the reference's Gauss-Seidel smoother (src/LinearSolvers/SymGaussSeidelSmoothers.jl) and of what
the device version adds to it (level sets, launch plan).  Plain helper: numpy and scipy only, no fixtures, no collection hooks.

  diagonal_indices / forward_sub / backward_sub / solve / ldiv    literal transcriptions, column-oriented on CSC as the reference
                                                                  (:21-43, :55-69, :77-91, :175-208, :210-214)
  forward_rows / backward_rows                                    the same solves seen from the rows, in the order the device uses:
                                                                  r_i minus a_ij x_j over ascending j < i (descending j > i), one
                                                                  rounded product and one rounded subtraction each, then / a_ii
  level_sets(A, forward)                                          set(i) = 1 + max set(j) over the stored j < i (j > i), 0 without
  launch_plan(set_sizes) / schedule(A, forward)                   the launch rule of csrc/gs.inc.hpp restated
  GS / RJ                                                         smoother objects of the V-cycle below
  GMG                                                             numpy_twin.GMG with smoother objects; cg / fgmres come from there
"""
import numpy as np
import scipy.sparse as sp

import numpy_twin as nt

CHAIN_ROWS = 1024                     # a set of at most this many rows is one pass of the chain workgroup
TYPES = ("symmetric", "forward", "backward")
cg, fgmres = nt.cg, nt.fgmres


class SingularException(Exception):
    pass


def csc(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A


def csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


# ------------------------------------------------------------------------------------------------ the reference, literally
def diagonal_indices(A):
    """DiagonalIndices(A, 1:n), :21-43, on a sorted CSC matrix -> (diag, last), 0-based positions"""
    n = min(A.shape)
    diag, last = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for col in range(n):
        r1, r2 = int(A.indptr[col]), int(A.indptr[col + 1]) - 1
        k = r1 + int(np.searchsorted(A.indices[r1:r2 + 1], col))
        if k > r2 or A.indices[k] != col or A.data[k] == 0.0:
            raise SingularException(col)
        diag[col] = k
        last[col] = r1 + int(np.searchsorted(A.indices[r1:r2 + 1], n)) - 1
    return diag, last


def forward_sub(A, diag, last, x):
    """forward_sub!, :55-69 (the rows of one column are distinct: the slice update is the loop :64-66)"""
    for col in range(diag.size):
        idx = diag[col]
        x[col] /= A.data[idx]
        rows = A.indices[idx + 1:last[col] + 1]
        x[rows] -= A.data[idx + 1:last[col] + 1] * x[col]
    return x


def backward_sub(A, diag, x):
    """backward_sub!, :77-91"""
    for col in range(diag.size - 1, -1, -1):
        idx = diag[col]
        x[col] = x[col] / A.data[idx]
        rows = A.indices[A.indptr[col]:idx]
        x[rows] -= A.data[A.indptr[col]:idx] * x[col]
    return x


class GS:
    """GaussSeidelSmoother(niter, omega, type), :105-118"""

    def __init__(self, niter=1, omega=1.0, type="symmetric"):
        assert type in TYPES and niter > 0 and omega > 0.0
        self.niter, self.omega, self.type = int(niter), float(omega), type

    def setup(self, A):
        """numerical_setup, :167-171 -> (A in CSC, diag, last)"""
        A = csc(A)
        return (A,) + diagonal_indices(A)

    def smooth(self, ns, x, r):
        solve(x, ns, self, r)


def solve(x, ns, sm, r):
    """solve!(x, ns, r), :175-208"""
    A, diag, last = ns
    for _ in range(sm.niter):
        if sm.type in ("forward", "symmetric"):
            dx = r.copy()
            forward_sub(A, diag, last, dx)
            dx = sm.omega * dx
            x += dx
            r -= A @ dx
        if sm.type in ("backward", "symmetric"):
            dx = r.copy()
            backward_sub(A, diag, dx)
            dx = sm.omega * dx
            x += dx
            r -= A @ dx
    return x


def ldiv(ns, sm, b):
    """ldiv!(x, ns, b), :210-214"""
    x = np.zeros_like(b)
    aux = b.copy()
    solve(x, ns, sm, aux)
    return x


# ------------------------------------------------------------------------------------------------ the device's order
def forward_rows(A, r):
    """L \\ r row by row on sorted CSR: ascending j < i"""
    A = csr(A)
    ptr, idx, val = A.indptr, A.indices, A.data
    x = np.array(r, dtype=np.float64)
    for i in range(A.shape[0]):
        acc = x[i]
        k = int(ptr[i])
        while idx[k] < i:
            acc = acc - val[k] * x[idx[k]]
            k += 1
        assert idx[k] == i
        x[i] = acc / val[k]
    return x


def backward_rows(A, r):
    """U \\ r row by row on sorted CSR: descending j > i"""
    A = csr(A)
    ptr, idx, val = A.indptr, A.indices, A.data
    x = np.array(r, dtype=np.float64)
    for i in range(A.shape[0] - 1, -1, -1):
        acc = x[i]
        k = int(ptr[i + 1]) - 1
        while idx[k] > i:
            acc = acc - val[k] * x[idx[k]]
            k -= 1
        assert idx[k] == i
        x[i] = acc / val[k]
    return x


def level_sets(A, forward=True):
    """-> set index of every row"""
    A = csr(A)
    n = A.shape[0]
    s = np.zeros(n, dtype=np.int64)
    order = range(n) if forward else range(n - 1, -1, -1)
    for i in order:
        c = A.indices[A.indptr[i]:A.indptr[i + 1]]
        dep = c[c < i] if forward else c[c > i]
        s[i] = 1 + s[dep].max() if dep.size else 0
    return s


def launch_plan(set_sizes):
    """-> [(s0, s1, wide)]: consecutive sets of at most CHAIN_ROWS rows share one chain launch, a larger set is one wide launch"""
    plan, s, n = [], 0, len(set_sizes)
    while s < n:
        if set_sizes[s] > CHAIN_ROWS:
            plan.append((s, s + 1, True))
            s += 1
            continue
        e = s
        while e < n and set_sizes[e] <= CHAIN_ROWS:
            e += 1
        plan.append((s, e, False))
        s = e
    return plan


def schedule(A, forward=True):
    """-> (nsets, max_set_rows, nlaunches, nwide): what gmg_get_gs_schedule reports"""
    sizes = np.bincount(level_sets(A, forward))
    plan = launch_plan(sizes)
    return int(sizes.size), int(sizes.max()), len(plan), sum(1 for q in plan if q[2])


# ------------------------------------------------------------------------------------------------ V-cycle with smoother objects
class RJ:
    """RichardsonSmoother(JacobiLinearSolver(), niter, omega)"""

    def __init__(self, niter=1, omega=1.0):
        self.niter, self.omega = int(niter), float(omega)

    def setup(self, A):
        return A, nt.Jacobi(A)

    def smooth(self, ns, x, r):
        nt.richardson(ns[0], ns[1], self.niter, self.omega, x, r)


class GMG(nt.GMG):
    """numpy_twin.GMG (operators, coarse LU, solve) with pre / post given as lists of smoother objects (GS / RJ)"""

    def __init__(self, mats, Ps, Rs, pre, post=None, cycle="v"):
        super().__init__(mats, Ps, Rs, list(pre), None if post is None else list(post), cycle)
        self.pre_ns = [sm.setup(A) for sm, A in zip(self.pre, self.A)]
        self.post_ns = [sm.setup(A) for sm, A in zip(self.post, self.A)]

    def cycle(self, l, x, r, ctype=None):
        ctype = self.cyc if ctype is None else ctype
        if l == len(self.A) - 1:
            x[:] = self.coarse.solve(r)                       # GMGLinearSolvers.jl:474
            return
        A = self.A[l]
        self.pre[l].smooth(self.pre_ns[l], x, r)              # :481
        for k in range(1 if ctype == "v" else 2):
            if k == 1:
                self.post[l].smooth(self.post_ns[l], x, r)    # W :531 / F :584
            rH = self.R[l] @ r                                # :484
            dxH = np.zeros(self.A[l + 1].shape[0])            # :487
            self.cycle(l + 1, dxH, rH, ctype if k == 0 else ("w" if ctype == "w" else "v"))   # :488
            dx = self.P[l] @ dxH                              # :491
            x += dx                                           # :494
            r -= A @ dx                                       # :495-496
        self.post[l].smooth(self.post_ns[l], x, r)            # :499

    def solver(self, b, maxiter=100, atol=1e-14, rtol=1e-8):
        """mode = :solver, GMGLinearSolvers.jl:612-645, x0 = 0 -> (x, iterations, residual history)"""
        x = np.zeros_like(b)
        r = b - self.A[0] @ x
        hist = [np.linalg.norm(r)]
        it = 0
        done = it >= maxiter or 1.0 < rtol or hist[0] < atol
        while not done:
            self.cycle(0, x, r)
            hist.append(np.linalg.norm(r)); it += 1
            done = it >= maxiter or hist[-1] / hist[0] < rtol or hist[-1] < atol
        return x, it, np.array(hist)
