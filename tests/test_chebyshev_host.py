"""The ChebyshevSmoother on the host: the numpy restatement (tests/chebyshev_reference.py) against the closed form, the power iteration
against scipy's eigenvalues, the constructor checks of the Python mirror, and the claim the smoother is there for -- degree 4 over the
vertex-star patches needs no more FGMRES iterations than the stock Richardson(patch, 10, 0.2) with 2.5 times fewer patch sweeps."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import chebyshev_reference as cr
import numpy_twin as nt
from conftest import max_rel


class Identity:
    def solve(self, r):
        return r.copy()


def _cheb_T(m, t):
    """T_m(t) by the three-term recurrence (any real t)"""
    t = np.asarray(t, dtype=np.float64)
    a, b = np.ones_like(t), t.copy()
    if m == 0:
        return a
    for _ in range(m - 1):
        a, b = b, 2.0 * t * b - a
    return b


# ---------------------------------------------------------------- the recurrence
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_one_pass_is_the_scaled_chebyshev_polynomial(m):
    """diagonal A, M = I: the error component at eigenvalue lam is multiplied by T_m((theta - lam)/delta) / T_m(sigma)"""
    lmin, lmax = 0.5, 4.0
    lam = np.concatenate([np.linspace(lmin, lmax, 23), [0.1, 0.3, 4.5, 6.0]])     # inside and outside the interval
    A = sp.diags(lam).tocsr()
    xs = np.linspace(1.0, 2.0, lam.size)
    x, r = np.zeros(lam.size), A @ xs
    cr.chebyshev(A, Identity(), cr.coefficients(m, lmin, lmax), x, r)
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    want = _cheb_T(m, (theta - lam) / delta) / _cheb_T(m, np.array(theta / delta))
    got = (xs - x) / xs
    assert max_rel(got, want) <= 1e-13, (m, max_rel(got, want))
    assert max_rel(r, A @ (xs - x)) <= 1e-13                # r stays the residual of x
    inside = (lam >= lmin) & (lam <= lmax)
    assert np.all(np.abs(got[inside]) <= (1.0 + 1e-12) / _cheb_T(m, np.array(theta / delta)))


def test_coefficients_are_computed_in_the_stated_order():
    a, b = cr.coefficients(3, 0.88, 8.8)
    theta, delta = (8.8 + 0.88) / 2.0, (8.8 - 0.88) / 2.0
    sigma = theta / delta
    rho0 = 1.0 / sigma
    rho1 = 1.0 / (2.0 * sigma - rho0)
    rho2 = 1.0 / (2.0 * sigma - rho1)
    assert b[0] == 1.0 / theta and a[1] == rho1 * rho0 and b[1] == (2.0 * rho1) / delta
    assert a[2] == rho2 * rho1 and b[2] == (2.0 * rho2) / delta and a[0] == 0.0


def test_degree_one_is_one_richardson_sweep(po):
    A = po.build_hierarchy((8, 8), 2)["mats"][0].to_scipy().tocsr()
    rng = np.random.default_rng(3)
    x0, r0 = rng.uniform(-1, 1, A.shape[0]), rng.uniform(-1, 1, A.shape[0])
    lmin, lmax = 0.3, 1.7
    M = nt.Jacobi(A)
    x, r = x0.copy(), r0.copy()
    cr.chebyshev(A, M, cr.coefficients(1, lmin, lmax), x, r)
    xo, ro = x0.copy(), r0.copy()
    nt.richardson(A, M, 1, 1.0 / ((lmax + lmin) / 2.0), xo, ro)
    assert np.array_equal(x, xo) and np.array_equal(r, ro)


def test_sweep_zero_does_not_read_x_where_the_pass_starts_from_zero(po):
    A = po.build_hierarchy((8, 8), 2)["mats"][0].to_scipy().tocsr()
    r0 = np.random.default_rng(4).uniform(-1, 1, A.shape[0])
    co = cr.coefficients(3, 0.2, 2.0)
    x, r = np.full(A.shape[0], np.nan), r0.copy()
    cr.chebyshev(A, nt.Jacobi(A), co, x, r, x_zero=True)
    xo, ro = np.zeros(A.shape[0]), r0.copy()
    cr.chebyshev(A, nt.Jacobi(A), co, xo, ro)
    assert np.array_equal(x, xo) and np.array_equal(r, ro)


# ---------------------------------------------------------------- the estimate
def test_start_vector_is_the_stated_one():
    v = cr.start_vector(5000)
    i = 4321
    raw = 1.0 + ((i * 2654435761) % 1024) / 1024.0
    w = np.array([1.0 + ((k * 2654435761) % 1024) / 1024.0 for k in range(5000)])
    assert abs(np.linalg.norm(v) - 1.0) <= 1e-15 and v[i] == raw / np.linalg.norm(w)


def _lambda_max(A, M):
    op = spla.LinearOperator(A.shape, matvec=lambda v: M.solve(A @ v), dtype=np.float64)
    return float(np.real(spla.eigs(op, k=1, which="LM", tol=1e-10, return_eigenvectors=False)[0]))


def test_power_iteration_stays_below_the_largest_eigenvalue(po):
    """... and is a useful estimate of it: the patch case is sharp after ten steps, the Jacobi case is the documented under-estimate"""
    A = po.build_hierarchy((4, 4, 4), 2, order=2)["mats"][0].to_scipy().tocsr()
    pp, pd = po.vertex_star_patches((4, 4, 4), 2)
    assert A.shape[0] == 343 and np.diff(pp).min() == 1 and np.diff(pp).max() == 27
    M = nt.Patch(A, pp, pd)
    est, top = cr.power_iteration(A, M, 10), _lambda_max(A, M)
    print("patch Q2 4^3: estimate %.6f, eigs %.6f" % (est, top))
    assert 0.9 * top <= est <= top * (1.0 + 1e-10)
    A = po.build_hierarchy((16, 16, 16), 2)["mats"][0].to_scipy().tocsr()
    M = nt.Jacobi(A)
    est, top = cr.power_iteration(A, M, 10), _lambda_max(A, M)
    print("Jacobi Q1 16^3: estimate %.6f, eigs %.6f" % (est, top))
    assert 0.8 * top <= est <= top * (1.0 + 1e-10)
    assert cr.power_iteration(A, M, 40) >= est              # more steps only move it up
    e, lmin, lmax = cr.bounds(A, M)
    assert e == est and lmax == 1.1 * est and lmin == lmax / 10.0
    e, lmin, lmax = cr.bounds(A, M, lambda_max=2.0)
    assert np.isnan(e) and (lmin, lmax) == (0.2, 2.0)
    assert cr.bounds(A, M, lambda_max=2.0, lambda_min=0.5)[1:] == (0.5, 2.0)


# ---------------------------------------------------------------- the Python mirror
def test_constructor_checks(S, po):
    J = S.JacobiLinearSolver()
    c = S.ChebyshevSmoother(J)
    assert (c.degree, c.lambda_max, c.lambda_min, c.eig_ratio, c.eig_safety, c.eig_steps) == (3, None, None, 10.0, 1.1, 10)
    assert "ChebyshevSmoother" in S.__all__
    pp, pd = po.vertex_star_patches((4, 4), 2)
    for M in (S.PatchSolver(pp, pd), S.BlockJacobiSolver(pp, pd)):
        assert S.ChebyshevSmoother(M, 4, lambda_max=8.8, lambda_min=0.88).degree == 4
    for bad in (object(), None, S.GaussSeidelSmoother(1), S.RichardsonSmoother(J, 1, 1.0)):
        with pytest.raises(TypeError):
            S.ChebyshevSmoother(bad)
    for kw in (dict(degree=0), dict(degree=-1), dict(lambda_max=0.0), dict(lambda_max=-1.0), dict(lambda_max=1.0, lambda_min=0.0),
               dict(lambda_max=1.0, lambda_min=1.0), dict(lambda_max=1.0, lambda_min=2.0), dict(eig_ratio=1.0), dict(eig_ratio=0.5),
               dict(eig_safety=0.99), dict(eig_steps=0), dict(lambda_max=float("nan")), dict(eig_ratio=float("nan"))):
        with pytest.raises(ValueError):
            S.ChebyshevSmoother(J, **kw)
    S.ChebyshevSmoother(J, eig_safety=1.0, eig_steps=1, degree=1)


def test_accepted_where_a_richardson_smoother_is(S, po):
    H = po.build_hierarchy((8, 8), 2)
    c = S.ChebyshevSmoother(S.JacobiLinearSolver(), 2)
    g = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=[c], post_smoothers=[c])
    assert g.pre_smoothers[0] is c and g.post_smoothers[0] is c
    assert S.LinearSolverFromSmoother(c).smoother is c
    S.FGMRESSolver(5, g, Pl=S.LinearSolverFromSmoother(c))
    S.CGSolver((S.LinearSolverFromSmoother(c), g))
    with pytest.raises(ValueError):
        S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=[c, c])
    with pytest.raises(TypeError):
        S.LinearSolverFromSmoother(S.JacobiLinearSolver())


# ---------------------------------------------------------------- what it is for
def test_degree_four_matches_richardson_ten_with_fewer_patch_sweeps(po):
    """Q2 16^3, 3 levels, vertex-star patches, FGMRES(5) to 1e-6 on poisson.random_rhs: Richardson(patch, 10, 0.2) runs 20 patch sweeps
    per V-cycle and level, Chebyshev(patch, 4) with the default interval 8"""
    nc, nlev = (16, 16, 16), 3
    H = po.build_hierarchy(nc, nlev, order=2)
    A = H["mats"][0].to_scipy().tocsr()
    b = po.random_rhs(A.shape[0])
    specs = [("patch",) + po.vertex_star_patches(c, 2) for c in H["ncells"][:-1]]
    iters, est = {}, None
    for name, make in (("richardson", lambda s: cr.Rich(s, 10, 0.2)), ("chebyshev", lambda s: cr.Cheb(s, 4))):
        G = cr.GMG(H["mats"], H["prolongations"], H["restrictions"], [make(s) for s in specs])
        if name == "chebyshev":
            est = [ns[3][0] for ns in G.pre_ns]
        _x, iters[name], hist = cr.fgmres(A, b, Pr=G.solve, m=5, rtol=1e-6)
        assert hist[-1] / hist[0] < 1e-6
    print("FGMRES(5) iterations:", iters, "lambda_est per level:", est)
    assert iters["chebyshev"] <= iters["richardson"]
    assert all(7.9 <= e <= 8.0 for e in est)                # every dof sits in up to 2^3 patches
