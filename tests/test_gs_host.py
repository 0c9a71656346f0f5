"""Host side of the Gauss-Seidel smoother: the numpy reference (tests/gs_reference.py) against itself and scipy, the level sets and
the launch plan on every family of tests/gs_edge_problems.py, the constructor checks of the Python classes, and the iteration
counts of the Krylov cases the device tests (tests/test_gpu_gauss_seidel.py) repeat."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import gs_edge_problems as ge
import gs_reference as gr


@pytest.mark.parametrize("name", ge.FAMILIES)
def test_column_literal_and_row_ordered_solves_are_bitwise_equal(name):
    c = ge.case(name)
    A, diag, last = gr.GS().setup(c.A)
    assert np.array_equal(gr.forward_sub(A, diag, last, c.r0.copy()), gr.forward_rows(c.A, c.r0))
    assert np.array_equal(gr.backward_sub(A, diag, c.r0.copy()), gr.backward_rows(c.A, c.r0))


@pytest.mark.parametrize("name", ge.POISSON)
def test_solves_agree_with_scipy_triangular_solve(name):
    c = ge.case(name)
    A = gr.csr(c.A)
    for lower, mine in ((True, gr.forward_rows), (False, gr.backward_rows)):
        T = (gr.sp.tril(A) if lower else gr.sp.triu(A)).tocsr()
        ref = spla.spsolve_triangular(T, c.r0, lower=lower)
        x = mine(c.A, c.r0)
        assert np.linalg.norm(x - ref) <= 1e-12 * np.linalg.norm(ref)


@pytest.mark.parametrize("forward", [True, False])
@pytest.mark.parametrize("name", ge.FAMILIES)
def test_level_sets(name, forward):
    A = gr.csr(ge.matrix(name))
    s = gr.level_sets(A, forward)
    for i in range(A.shape[0]):
        cols = A.indices[A.indptr[i]:A.indptr[i + 1]]
        dep = cols[cols < i] if forward else cols[cols > i]
        assert np.all(s[dep] < s[i])                          # every stored dependency lies in an earlier set
        assert s[i] == 0 or np.any(s[dep] == s[i] - 1)        # every row of set s > 0 has a dependency in set s - 1
    sizes = np.bincount(s)
    want = ge.SETS_BIDIAGONAL[forward] if name == "bidiagonal" else ge.SETS[name]
    assert (sizes.size, int(sizes.max())) == want
    if name in ("blocks", "shuffled"):
        assert tuple(sizes) == (ge.BLOCK_SIZES if forward else ge.BLOCK_SIZES[::-1])
    if name == "redblack":
        assert tuple(sizes) == (2048, 2048)


def test_launch_plan():
    assert gr.launch_plan(ge.BLOCK_SIZES) == [(0, 6, False), (6, 7, True), (7, 8, True), (8, 10, False)]
    assert gr.launch_plan(ge.BLOCK_SIZES[::-1]) == [(0, 2, False), (2, 3, True), (3, 4, True), (4, 10, False)]
    assert gr.launch_plan([1024, 1025, 1024]) == [(0, 1, False), (1, 2, True), (2, 3, False)]
    for name, (nl, nw) in ge.PLANS.items():
        for forward in (True, False):
            nsets, biggest, launches, wide = gr.schedule(ge.matrix(name), forward)
            assert (launches, wide) == (nl, nw), (name, forward)
            assert (nsets, biggest) == ge.SETS[name]


@pytest.mark.parametrize("name", ge.SINGULAR)
def test_missing_or_zero_diagonal_is_singular(name):
    with pytest.raises(gr.SingularException) as e:
        gr.GS().setup(ge.matrix(name))
    assert e.value.args[0] == ge.BAD_ROW


def test_python_constructors(S):
    g = S.GaussSeidelSmoother()
    assert (g.niter, g.omega, g.type) == (1, 1.0, "symmetric")
    g = S.GaussSeidelSmoother(3, 1.2, "backward")
    assert (g.niter, g.omega, g.type) == (3, 1.2, "backward")
    s = S.SymGaussSeidelSmoother(5, 0.9)
    assert isinstance(s, S.GaussSeidelSmoother) and (s.niter, s.omega, s.type) == (5, 0.9, "symmetric")
    for bad in (dict(niter=0), dict(niter=-1), dict(omega=0.0), dict(omega=-1.0), dict(type="sideways")):
        with pytest.raises(ValueError):
            S.GaussSeidelSmoother(**bad)
    with pytest.raises(ValueError):
        S.SymGaussSeidelSmoother(0)
    assert S.LinearSolverFromSmoother(s).smoother is s
    with pytest.raises(TypeError):
        S.LinearSolverFromSmoother(S.JacobiLinearSolver())


@pytest.mark.parametrize("name", sorted(ge.KRYLOV))
def test_krylov_case_counts_do_not_sit_on_an_edge(name):
    c = ge.KRYLOV[name]
    _x, it, hist = ge.krylov_reference(name)
    rel = hist / hist[0]
    print(name, it, rel[-2] / c["rtol"], c["rtol"] / rel[-1])
    assert it == c["iters"]
    assert rel[-2] >= 1.5 * c["rtol"] and rel[-1] <= c["rtol"] / 1.5
