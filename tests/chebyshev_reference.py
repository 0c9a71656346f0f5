"""numpy / scipy restatement of the ChebyshevSmoother of the device library (csrc/cheb.inc.hpp).  The reference has no such smoother,
so this file IS the definition the device is held to.  Plain helper: numpy and scipy only, no fixtures, no collection hooks.

  coefficients(m, lmin, lmax)       the 2m - 1 coefficients, in double, in the order of Saad's Alg. 12.1
  chebyshev(A, M, co, x, r)         one pass of degree m on (x, r) in the residual form, z = M.solve(r) un-relaxed
  start_vector / power_iteration    the deterministic lambda_max(M^-1 A) estimate of the setup
  bounds(...)                       given or estimated bounds -> (lambda_est, lambda_min, lambda_max)
  Cheb / Rich                       smoother objects (setup(A) / smooth(ns, x, r)) over M = "jacobi" or a patch table
  GMG                               gs_reference.GMG (numpy_twin.GMG with smoother objects); cg / fgmres come from numpy_twin
"""
import numpy as np

import gs_reference as gr
import numpy_twin as nt

cg, fgmres, GMG = nt.cg, nt.fgmres, gr.GMG
DEFAULTS = dict(degree=3, eig_steps=10, eig_safety=1.1, eig_ratio=10.0)


def coefficients(m, lmin, lmax):
    """-> (a, b): sweep 0 is d = b[0] z, sweep k is d = a[k] d + b[k] z (a[0] is unused)"""
    theta = (lmax + lmin) / 2.0
    delta = (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    a, b = np.zeros(m), np.zeros(m)
    b[0] = 1.0 / theta
    for k in range(1, m):
        rho_k = 1.0 / (2.0 * sigma - rho)
        a[k] = rho_k * rho
        b[k] = (2.0 * rho_k) / delta
        rho = rho_k
    return a, b


def chebyshev(A, M, co, x, r, x_zero=False):
    """one pass on (x, r), both updated in place; x_zero: x is not read (the pass starts from x = 0)"""
    a, b = co
    d = None
    for k in range(b.size):
        z = M.solve(r)
        d = b[0] * z if k == 0 else a[k] * d + b[k] * z       # each product rounded, then the sum
        if x_zero and k == 0:
            x[:] = d
        else:
            x += d
        r -= A @ d
    return x, r


def start_vector(n):
    i = np.arange(n, dtype=np.uint64)
    v = 1.0 + ((i * np.uint64(2654435761)) % np.uint64(1024)).astype(np.float64) / 1024.0
    return v / np.linalg.norm(v)


def power_iteration(A, M, steps):
    """`steps` power steps on M^-1 A from start_vector -> lambda_est"""
    v = start_vector(A.shape[0])
    lam = None
    for _ in range(steps):
        w = M.solve(A @ v)
        lam = float(np.linalg.norm(w))
        v = w / lam
    return lam


def bounds(A, M, lambda_max=None, lambda_min=None, eig_ratio=10.0, eig_safety=1.1, eig_steps=10):
    """-> (lambda_est (NaN where lambda_max is given), lambda_min, lambda_max)"""
    if lambda_max is None:
        est = power_iteration(A, M, eig_steps)
        lmax = eig_safety * est
    else:
        est, lmax = float("nan"), float(lambda_max)
    lmin = lmax / eig_ratio if lambda_min is None else float(lambda_min)
    return est, lmin, lmax


class PatchInverses:
    """M of a patch table through the explicit inverses the kernels build (patch_edge_problems.twin_inverses): for patch sets
    whose blocks the device does not take through LAPACK-like factors (n_p > 64, caller blocks)"""

    def __init__(self, A, pp, rows, cols=None, pivot=True, blocks=None):
        import patch_edge_problems as pe
        self.pe, self.N, self.pp, self.rows = pe, A.shape[0], pp, rows
        self.cols = rows if cols is None else cols
        self.X = pe.twin_inverses(A, pp, rows, self.cols, pivot, blocks)

    def solve(self, r):
        return self.pe._twin_apply(self.X, self.pp, self.rows, self.cols, r, self.N)


def make_M(spec, A):
    """spec: "jacobi", ("patch", pp, rows[, pivot]) or a callable A -> object with solve(r)"""
    if spec == "jacobi":
        return nt.Jacobi(A)
    if callable(spec):
        return spec(A)
    kind, pp, rows = spec[:3]
    assert kind == "patch"
    return nt.Patch(A, pp, rows, pivot=spec[3] if len(spec) > 3 else True)


class Cheb:
    """ChebyshevSmoother(M, degree, lambda_max, lambda_min, eig_ratio, eig_safety, eig_steps)"""

    def __init__(self, M, degree=3, lambda_max=None, lambda_min=None, eig_ratio=10.0, eig_safety=1.1, eig_steps=10):
        assert degree >= 1 and eig_ratio > 1.0 and eig_safety >= 1.0 and eig_steps >= 1
        self.M, self.degree = M, int(degree)
        self.kw = dict(lambda_max=lambda_max, lambda_min=lambda_min, eig_ratio=eig_ratio, eig_safety=eig_safety, eig_steps=eig_steps)

    def setup(self, A):
        """-> (A, M, (a, b), (lambda_est, lambda_min, lambda_max))"""
        M = make_M(self.M, A)
        info = bounds(A, M, **self.kw)
        return A, M, coefficients(self.degree, info[1], info[2]), info

    def smooth(self, ns, x, r):
        chebyshev(ns[0], ns[1], ns[2], x, r)


class Rich:
    """RichardsonSmoother(M, niter, omega)"""

    def __init__(self, M, niter=1, omega=1.0):
        self.M, self.niter, self.omega = M, int(niter), float(omega)

    def setup(self, A):
        return A, make_M(self.M, A)

    def smooth(self, ns, x, r):
        nt.richardson(ns[0], ns[1], self.niter, self.omega, x, r)


def apply_smoother(sm, A, r):
    """LinearSolverFromSmoother(sm): x = 0 ; r = copy(b) ; solve!(x, sm, r) -> x"""
    ns = sm.setup(A)
    def Pl(b):
        x, rr = np.zeros_like(b), b.copy()
        sm.smooth(ns, x, rr)
        return x
    return Pl(r) if r is not None else Pl


# ------------------------------------------------------------------------------------------------ solver cases of the device tests
# m: ("patch" | "jacobi", degree); Q2 levels take the vertex-star patches of their mesh.  rhs = poisson.random_rhs, x0 = 0.
# solver: "cg" | "fgmres" (FGMRES(5)) | "gmg" (mode = :solver) | "fgmres_pl" (FGMRES(5, gmg, Pl = LinearSolverFromSmoother(pre[0])))
SOLVER_CASES = {
    "cg-q2-2lev-v": dict(nc=(8, 8, 8), order=2, nlev=2, m=("patch", 3), solver="cg", cycle="v", rtol=1e-8),
    "fgmres-q2-3lev-v": dict(nc=(8, 8, 8), order=2, nlev=3, m=("patch", 4), solver="fgmres", cycle="v", rtol=1e-6),
    "cg-q1-3lev-w": dict(nc=(16, 16, 16), order=1, nlev=3, m=("jacobi", 3), solver="cg", cycle="w", rtol=1e-9),
    "fgmres-q1-3lev-f": dict(nc=(16, 16, 16), order=1, nlev=3, m=("jacobi", 2), solver="fgmres", cycle="f", rtol=1e-8),
    "gmg-q1-2lev-v": dict(nc=(16, 16, 16), order=1, nlev=2, m=("jacobi", 3), solver="gmg", cycle="v", rtol=1e-8),
    "fgmres-pl-q2-2lev-v": dict(nc=(8, 8, 8), order=2, nlev=2, m=("patch", 2), solver="fgmres_pl", cycle="v", rtol=1e-3),
}


class _LeftPreconditioned:
    """v -> Pl(A v): with x0 = 0 FGMRES on (Pl A, Pl b) runs the iteration of FGMRES(m, Pr, Pl) on (A, b) (KrylovUtils.jl:14-18,46-50)"""

    def __init__(self, A, Pl):
        self.A, self.Pl = A, Pl

    def __matmul__(self, v):
        return self.Pl(self.A @ v)


def solver_reference(po, c):
    """the numpy reference of one solver case -> (x, iterations, residual history)"""
    H = po.build_hierarchy(c["nc"], c["nlev"], c["order"])
    A = H["mats"][0].to_scipy().tocsr()
    A.sort_indices()
    b = po.random_rhs(A.shape[0])
    kind, degree = c["m"]
    specs = ["jacobi" if kind == "jacobi" else ("patch",) + po.vertex_star_patches(cells, c["order"]) for cells in H["ncells"][:-1]]
    sms = [Cheb(s, degree) for s in specs]
    G = GMG(H["mats"], H["prolongations"], H["restrictions"], sms, cycle=c["cycle"])
    kw = dict(maxiter=100, atol=1e-14, rtol=c["rtol"])
    if c["solver"] == "cg":
        return cg(A, b, Pl=G.solve, **kw)
    if c["solver"] == "fgmres":
        return fgmres(A, b, Pr=G.solve, m=5, **kw)
    if c["solver"] == "fgmres_pl":
        ns = G.pre_ns[0]
        def Pl(v):
            x, r = np.zeros_like(v), v.copy()
            sms[0].smooth(ns, x, r)
            return x
        return fgmres(_LeftPreconditioned(A, Pl), Pl(b), Pr=G.solve, m=5, **kw)
    return G.solver(b, **kw)
