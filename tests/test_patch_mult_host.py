"""The multiplicative patch smoother on the host: the library's colouring (gmg_patch_multicolor, no GPU) against the numpy twin
(tests/patch_mult_reference.py), the twin against the closed forms of multiplicative Schwarz, the twin's iteration counts, and the
errors of the constructor and of the host function."""
import numpy as np
import pytest
import scipy.sparse as sp

import chebyshev_reference as cr
import gs_reference as gr
import numpy_twin as nt
import patch_edge_problems as pe
import patch_mult_reference as pm


def _q2(po, hierarchy, nc, nlev=2):
    H = hierarchy(nc, nlev, 2)
    A = H["mats"][0].to_scipy().tocsr()
    pp, pd = po.vertex_star_patches(nc, 2)
    return A, pp, pd


def _lib_coloring(S, A, pp, pd):
    color, nc = S.patch_multicolor(A, pp, pd)
    assert color.dtype == np.int32 and color.shape == (pp.size - 1,)
    return color, nc


# ---------------------------------------------------------------- colouring, entry by entry
@pytest.mark.parametrize("nc,ncolors", (((6, 6), 4), ((4, 4, 4), 8)))
def test_coloring_vertex_stars(S, po, hierarchy, nc, ncolors):
    A, pp, pd = _q2(po, hierarchy, nc)
    color, n = _lib_coloring(S, A, pp, pd)
    twin, nt_ = pm.greedy_coloring(A, pp, pd)
    assert np.array_equal(color, twin) and n == nt_
    assert n == ncolors                                       # the 2^d colours of a Cartesian mesh
    assert pm.first_conflict(A, pp, pd, color) is None


@pytest.mark.parametrize("name,kind", (("wave63", "lu"), ("wave64", "nopivot"), ("big", "nopivot"), ("dedup_ragged", "lu")))
def test_coloring_ragged_sets(S, name, kind):
    """ragged random patch sets: empty and 1-dof patches, dofs shared by 6 to 9 patches"""
    c = pe.case(name, kind)
    sizes = np.diff(c.pp)
    mult = int(pe.multiplicity(c.N, c.pp, c.pd).max())
    assert sizes.min() <= 1 and mult >= 6
    color, n = _lib_coloring(S, c.A, c.pp, c.pd)
    twin, nt_ = pm.greedy_coloring(c.A, c.pp, c.pd)
    assert np.array_equal(color, twin) and n == nt_
    assert pm.first_conflict(c.A, c.pp, c.pd, color) is None
    assert n >= mult                                          # the patches that share one dof all differ in colour
    assert np.all(color[sizes == 0] == 0)                    # a patch without dofs has no neighbour


def test_coloring_counts_explicit_zeros_and_transposed_entries(S):
    """a stored zero couples; an entry stored in one triangle only couples both ways"""
    pp, pd = np.array([0, 1, 2, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int32)
    A = sp.csr_matrix((np.array([1.0, 1.0, 0.0, 1.0]), np.array([0, 1, 0, 2]), np.array([0, 1, 2, 4])), shape=(3, 3))   # a(2, 0) = 0.0 stored
    assert A.nnz == 4
    color, n = _lib_coloring(S, A, pp, pd)
    assert np.array_equal(color, [0, 0, 1]) and n == 2
    assert np.array_equal(color, pm.greedy_coloring(A, pp, pd)[0])


def test_coloring_uncoupled_blocks(S):
    B = np.array([[4.0, 1.0, 0.0], [1.0, 4.0, 1.0], [0.0, 1.0, 4.0]])
    A = sp.block_diag([B] * 5, format="csr")
    pp, pd = np.arange(0, 16, 3, dtype=np.int64), np.arange(15, dtype=np.int32)
    color, n = _lib_coloring(S, A, pp, pd)
    assert n == 1 and np.all(color == 0)


# ---------------------------------------------------------------- the twin against formulas
@pytest.fixture(scope="module")
def small(po, hierarchy):
    A, pp, pd = _q2(po, hierarchy, (4, 4))
    assert A.shape[0] == 49
    X = pm.inverses(A, pp, pd, lapack=True)
    color = pm.greedy_coloring(A, pp, pd)[0]
    return A, pp, pd, X, color


@pytest.mark.parametrize("omega", (1.0, 0.7))
def test_twin_forward_is_the_product_form(small, omega):
    A, pp, pd, X, color = small
    E = pm.product_form(A, X, pp, pd, pm.patch_order(color, pp, True), omega)
    got = np.column_stack([pm.correction(A, X, pp, pd, color, 1, omega, "forward", e) for e in np.eye(49)])
    assert np.max(np.abs(got - E)) <= 1e-12 * np.max(np.abs(E))


def test_twin_symmetric_is_symmetric(small):
    A, pp, pd, X, color = small
    E = np.column_stack([pm.correction(A, X, pp, pd, color, 1, 1.0, "symmetric", e) for e in np.eye(49)])
    assert np.max(np.abs(E - E.T)) <= 1e-12 * np.max(np.abs(E))
    F = np.column_stack([pm.correction(A, X, pp, pd, color, 1, 1.0, "forward", e) for e in np.eye(49)])
    assert np.max(np.abs(F - F.T)) > 1e-3 * np.max(np.abs(F))        # (one direction alone is not)


def test_twin_backward_is_forward_reversed(small):
    A, pp, pd, X, color = small
    rng = np.random.default_rng(3)
    r = rng.uniform(-1, 1, 49)
    back = pm.correction(A, X, pp, pd, color, 1, 0.7, "backward", r)
    fwd = pm.correction(A, X, pp, pd, int(color.max()) - color, 1, 0.7, "forward", r)
    assert np.array_equal(back, fwd)
    E = pm.product_form(A, X, pp, pd, pm.patch_order(color, pp, False), 0.7)
    assert np.max(np.abs(back - E @ r)) <= 1e-12 * np.max(np.abs(back))


def test_twin_smooth_updates_x_and_r(small):
    A, pp, pd, X, color = small
    rng = np.random.default_rng(4)
    x0, r0 = rng.uniform(-1, 1, 49), rng.uniform(-1, 1, 49)
    x, r = x0.copy(), r0.copy()
    dx = pm.smooth(A, X, pp, pd, color, 2, 1.0, "symmetric", x, r)
    assert np.array_equal(x, x0 + dx) and np.max(np.abs(r - (r0 - A @ dx))) <= 1e-14 * np.max(np.abs(r0))
    assert np.array_equal(pm.stored_row_sums(A, dx, np.array([5, 7])), pm.stored_row_sums(A, dx)[[5, 7]])


# ---------------------------------------------------------------- iterations
def test_twin_iterations_against_damped_additive(po, hierarchy):
    """CG + GMG on Q2 16^2, 3 levels, rtol 1e-8: one forward sweep before and one backward sweep after the coarse correction need
    no more iterations than RichardsonSmoother(PatchSolver, 10, 0.2) before and after (measured: 4 and 4)"""
    nc = (16, 16)
    H = hierarchy(nc, 3, 2)
    A = H["mats"][0].to_scipy().tocsr()
    b = po.random_rhs(A.shape[0])
    tabs = [po.vertex_star_patches(cells, 2) for cells in H["ncells"][:-1]]
    rich = [cr.Rich(("patch",) + t, 10, 0.2) for t in tabs]
    pre = [pm.PMult(*t, type="forward", lapack=True) for t in tabs]
    post = [pm.PMult(*t, type="backward", lapack=True) for t in tabs]
    kw = dict(maxiter=50, atol=1e-14, rtol=1e-8)
    it_rich = nt.cg(A, b, Pl=gr.GMG(H["mats"], H["prolongations"], H["restrictions"], rich).solve, **kw)[1]
    G = gr.GMG(H["mats"], H["prolongations"], H["restrictions"], pre, post)
    assert [int(ns[2].max()) + 1 for ns in G.pre_ns] == [4, 4]
    it_mult = nt.cg(A, b, Pl=G.solve, **kw)[1]
    print("iterations: Richardson(patch, 10, 0.2) %d, multiplicative forward + backward %d" % (it_rich, it_mult))
    assert it_mult <= it_rich and it_mult < 50


# ---------------------------------------------------------------- constructor and argument errors
def test_constructor_errors(S):
    pp, pd = np.array([0, 2, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int32)
    M = S.PatchSolver(pp, pd)
    sm = S.MultiplicativePatchSmoother(M)
    assert (sm.niter, sm.omega, sm.type, sm.coloring) == (1, 1.0, "symmetric", "greedy")
    assert isinstance(S.MultiplicativePatchSmoother(S.BlockJacobiSolver(pp, pd), 2, 0.7, "forward", [0, 1]).coloring, np.ndarray)
    with pytest.raises(TypeError):
        S.MultiplicativePatchSmoother(S.JacobiLinearSolver())
    with pytest.raises(ValueError, match="type"):
        S.MultiplicativePatchSmoother(M, type="sym")
    with pytest.raises(ValueError, match="iterations"):
        S.MultiplicativePatchSmoother(M, niter=0)
    with pytest.raises(ValueError, match="relaxation"):
        S.MultiplicativePatchSmoother(M, omega=0.0)
    for bad in ("multicolor", None, [0.0, 1.0], [[0, 1]], [0, -1], [0, 1, 2]):
        with pytest.raises(ValueError, match="coloring"):
            S.MultiplicativePatchSmoother(M, coloring=bad)
    S.LinearSolverFromSmoother(sm)
    with pytest.raises(TypeError):
        S.ChebyshevSmoother(sm)


def test_host_function_errors(S, pkg):
    A = sp.identity(3, format="csr")
    good = (np.array([0, 2, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int32))
    assert S.patch_multicolor(A, *good)[1] == 1
    assert S.patch_multicolor(A, np.array([0], dtype=np.int64), np.zeros(0, dtype=np.int32)) [1] == 0
    for pp, pd in ((good[0], np.array([0, 1, 3], dtype=np.int32)), (good[0], np.array([0, -1, 2], dtype=np.int32)),
                   (np.array([0, 3, 2], dtype=np.int64), good[1]), (np.array([1, 2, 3], dtype=np.int64), good[1])):
        with pytest.raises(pkg.abi.GmgError):
            S.patch_multicolor(A, pp, pd)
    with pytest.raises(ValueError):
        S.patch_multicolor(sp.csr_matrix(np.ones((2, 3))), *good)
