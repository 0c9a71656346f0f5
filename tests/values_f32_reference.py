"""Reference side of cycle_values = "float32" (a helper, no tests): the float32 round trip of level matrices on CSR copies, and the
numpy twin (tests/numpy_twin.py) composed the way the feature is defined -- the multigrid cycle on the ROUNDED levels, the Krylov
method on the UNROUNDED finest matrix.

The feature's definition: the preconditioner is exactly the fp64 cycle on the matrices A~_l, where A~_l is A_l with every stored
value rounded to float32 (nearest even, numpy.astype(float32)) and read back as fp64; 1/diag of such a level is 1 / A~_ii; the
coarsest level and everything outside the cycle keep the fp64 values."""
import numpy as np

import numpy_twin as nt


def round_values(val):
    """fp64 -> float32 (round to nearest even) -> fp64"""
    with np.errstate(over="ignore"):
        return np.asarray(val, dtype=np.float64).astype(np.float32).astype(np.float64)


def round_levels(mats, which):
    """Copies of the CSR matrices `mats` (poisson.CSR-like: shape, ptr, idx, val); the levels listed in `which` carry the float32
    round trip of their values.  Pattern, explicit zeros and the order of the entries are untouched; nothing is shared with the
    input."""
    which = set(int(l) for l in which)
    out = []
    for l, M in enumerate(mats):
        val = round_values(M.val) if l in which else np.array(M.val, dtype=np.float64, copy=True)
        out.append(type(M)(M.shape, np.array(M.ptr, copy=True), np.array(M.idx, copy=True), val))
    return out


def f32_levels(mats):
    """The levels the option turns into float32 levels when every level but the coarsest lands on SELL-64 / SELL-O with explicit
    values (what variable-coefficient Q1 hierarchies get): all but the coarsest."""
    return list(range(len(mats) - 1))


def twin_gmg(H, sweeps, omega=2.0 / 3.0, which=None, cycle="v"):
    """The numpy twin's GMG(Jacobi, sweeps, omega) on the levels of hierarchy H rounded on `which` (default: all but the coarsest;
    [] gives the plain fp64 preconditioner).  Jacobi's 1/diag comes from the rounded matrix."""
    mats = H["mats"]
    which = f32_levels(mats) if which is None else which
    rm = round_levels(mats, which)
    pre = [(nt.Jacobi(m.to_scipy().tocsr()), sweeps, omega) for m in rm[:-1]]
    return nt.GMG(rm, H["prolongations"], H["restrictions"], pre, cycle=cycle)


def twin_cg(H, b, sweeps, rtol, which=None, maxiter=50, omega=2.0 / 3.0):
    """CG on the UNROUNDED finest matrix, preconditioned by the cycle on the rounded levels -> (x, iterations, residual history,
    host-computed ||b - A x|| / ||b|| with the unrounded A)"""
    A = H["mats"][0].to_scipy().tocsr()
    G = twin_gmg(H, sweeps, omega, which)
    x, it, hist = nt.cg(A, b, Pl=G.solve, maxiter=maxiter, atol=1e-300, rtol=rtol)
    return x, it, hist, np.linalg.norm(b - A @ x) / np.linalg.norm(b)


def twin_fgmres(H, b, sweeps, rtol, m=5, which=None, maxiter=50, omega=2.0 / 3.0):
    """FGMRES(m) on the unrounded finest matrix, right-preconditioned by the cycle on the rounded levels"""
    A = H["mats"][0].to_scipy().tocsr()
    G = twin_gmg(H, sweeps, omega, which)
    x, it, hist = nt.fgmres(A, b, Pr=G.solve, m=m, maxiter=maxiter, atol=1e-300, rtol=rtol)
    return x, it, hist, np.linalg.norm(b - A @ x) / np.linalg.norm(b)
