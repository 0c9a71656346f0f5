"""The ChebyshevSmoother on partitioned levels, on the host: the folded twin of tests/cheb_dist_reference.py against the global
reference (chebyshev_reference.chebyshev on the folded global matrix), the start vector of the estimates, and the arguments
DistributedGMG refuses before it loads the library.

Tolerance of the passes: the twin and the reference differ in the order of the row sums only (own columns, then ghost columns, against
scipy's row order).  Degrees 1, 3, 4 with lambda_max = ||D^-1 A||_inf, lambda_min = lambda_max / 10 on every family gave
max|d| / max|ref| <= 4e-16 in x and r when the issue was written: fullsize_reference.TOL_KERNEL = 1e-13 has three digits of room."""
import importlib

import numpy as np
import pytest

import chebyshev_reference as cr
import cheb_dist_reference as cd
import fullsize_reference as fr
import gs_dist_reference as gd
import halo_edge_problems as he
import lanczos_reference as lr
import numpy_twin as nt
import operator_edge_problems as oe

TOL_KERNEL = fr.TOL_KERNEL
FAMILIES = ("bnd-1", "bnd-63", "bnd-64", "bnd-65", "one-way", "uncoupled", "fan-out", "dict-255", "gs-edge")
DEGREES = (1, 3, 4)


def _case(name):
    return gd.edge_case() if name == "gs-edge" else he.case(name)


def given_bounds(Af):
    """lambda_max = ||D^-1 A||_inf, lambda_min = lambda_max / 10"""
    lmax = float(np.max(np.abs(Af).sum(axis=1).A1 / np.abs(Af.diagonal())))
    return lmax / 10.0, lmax


@pytest.mark.parametrize("name", FAMILIES)
def test_twin_pass_is_the_global_reference(name):
    c = _case(name)
    L = c.levels[0]
    Af, blocks, perm = gd.folded(c.G["mats"][0], c.G["owners"][0])
    assert np.array_equal(perm, L.own_gid)
    assert np.array_equal(cd.dinv(L), 1.0 / Af.diagonal())
    lmin, lmax = given_bounds(Af)
    x0, r0 = he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0)
    M = nt.Jacobi(Af)
    for m in DEGREES:
        co = cr.coefficients(m, lmin, lmax)
        for x_zero in (False, True):
            tx, tr = cd.twin_pass(L, co, x0, r0, "jacobi", x_zero)
            rx, rr = cr.chebyshev(Af, M, co, x0.copy(), r0.copy(), x_zero)
            dev = (oe.max_rel(tx, rx), oe.max_rel(tr, rr))
            print(name, m, x_zero, "max_rel x, r of the twin against the global reference:", dev)
            assert max(dev) <= TOL_KERNEL, (name, m, x_zero, dev)


def test_patch_twin_pass_is_the_global_reference():
    """`patches`: z through he.patch_contributions / he.assemble against the additive Schwarz operator of the global patch table"""
    c = he.case("patches")
    L, p = c.levels[0], c.patch
    Af, _, perm = gd.folded(c.G["mats"][0], c.G["owners"][0])
    pos = np.empty(perm.size, dtype=np.int64)
    pos[perm] = np.arange(perm.size)
    M = nt.Patch(Af, p.pp, pos[p.pd])
    x0, r0 = he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0)
    z = cd.patch_M(c)(r0)
    assert oe.max_rel(z, M.solve(r0)) <= TOL_KERNEL
    co = cr.coefficients(3, 0.2, 2.0)
    tx, tr = cd.twin_pass(L, co, x0, r0, cd.patch_M(c))
    rx, rr = cr.chebyshev(Af, M, co, x0.copy(), r0.copy())
    dev = (oe.max_rel(tx, rx), oe.max_rel(tr, rr))
    print("patches: max_rel x, r of the twin against the global reference:", dev)
    assert max(dev) <= TOL_KERNEL, dev


def test_the_stacked_start_vector_gives_the_single_handle_estimates():
    c = he.case("fan-out")
    Af, blocks, _ = gd.folded(c.G["mats"][0], c.G["owners"][0])
    n = Af.shape[0]
    M = nt.Jacobi(Af)
    v = cd.start_vector([n])
    assert np.array_equal(v, cr.start_vector(n))
    for steps in (4, 10):
        assert cd.power_iteration(Af, M, steps, v) == cr.power_iteration(Af, M, steps)
    # the per-rank index is another vector: the estimate of true ranks depends on the partition
    counts = np.bincount(blocks)
    w = cd.start_vector(counts)
    assert abs(np.linalg.norm(w) - 1.0) <= 1e-15 and not np.array_equal(v, w)
    off = np.concatenate([[0], np.cumsum(counts)])
    for q in range(counts.size):
        seg = w[off[q]:off[q + 1]]
        assert np.allclose(seg / seg[0], cd.raw_start(counts[q]), rtol=1e-15, atol=0.0)   # (raw_start begins at 1.0: the index restarts per rank)
    assert cd.power_iteration(Af, M, 4, w) != cd.power_iteration(Af, M, 4, v)


def test_the_lanczos_estimate_from_the_stacked_vector(po):
    """SPD: Q1 on 8^3 cells.  cheb_dist_reference.lanczos_lambda_max from the stacked vector = lanczos_reference.lanczos_lambda_max"""
    A = po.build_hierarchy((8, 8, 8), 2, 1)["mats"][0].to_scipy().tocsr()
    M = nt.Jacobi(A)
    for steps in (4, 10):
        lam, k = cd.lanczos_lambda_max(A, M, steps, cd.start_vector([A.shape[0]]))
        assert k == steps and lam == lr.lanczos_lambda_max(A, M, steps)
        assert cd.estimate(A, M, "lanczos", steps, cd.start_vector([A.shape[0]])) == lam


def test_distributed_gmg_refuses_what_chebyshev_cannot_run_on(pkg):
    """ValueError before the library is loaded: a Gauss-Seidel smoother, the overlapping layout, a rank subset; the mapping itself is
    validated by ChebyshevSmoother's constructor"""
    mg = importlib.import_module(pkg.__name__ + ".multigpu")
    sv = importlib.import_module(pkg.__name__ + ".solvers")
    kw = dict(transport="host_loopback")
    with pytest.raises(ValueError, match="Gauss-Seidel"):
        mg.DistributedGMG((8, 8), 3, 0, 4, smoother=sv.GaussSeidelSmoother(), chebyshev={}, **kw)
    with pytest.raises(ValueError, match="own . ghost layout"):
        mg.DistributedGMG((8, 8), 3, 0, 4, depth=2, chebyshev={"degree": 3}, **kw)
    with pytest.raises(ValueError, match="own . ghost layout"):
        mg.DistributedGMG((8, 8), 3, 0, 4, finest_depth=2, chebyshev={"degree": 3}, **kw)
    with pytest.raises(ValueError, match="sub_from"):
        mg.DistributedGMG((8, 8), 4, 0, 4, sub_from=1, sub_ranks=2, chebyshev={}, **kw)
    with pytest.raises(ValueError, match="degree must be a positive integer"):
        mg.DistributedGMG((8, 8), 3, 0, 4, chebyshev={"degree": 0}, **kw)
    with pytest.raises(ValueError, match="eig_method"):
        mg.DistributedGMG((8, 8), 3, 0, 4, chebyshev={"eig_method": "qr"}, **kw)
    with pytest.raises(TypeError):
        mg.DistributedGMG((8, 8), 3, 0, 4, chebyshev={"niter": 3}, **kw)
