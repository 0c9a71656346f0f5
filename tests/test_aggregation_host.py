"""The numpy twin of the smoothed-aggregation prolongations (tests/aggregation_reference.py) by itself: properties that hold for any
correct implementation of the construction, on the matrices the GPU tests compare bits on.  No GPU."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import aggregation_reference as ar


@functools.lru_cache(maxsize=None)
def _matrix(name):
    import __graft_entry__ as entry
    po = entry.import_package().poisson
    if name.startswith("chain"):
        return ar.chain(int(name[5:]))
    if name == "nonsym":
        return ar.nonsymmetric_values()
    nc, order, lengths = {"q1_8x2": ((8, 8), 1, None), "q1_9x8": ((9, 8), 1, None), "q1_6x3": ((6, 6, 6), 1, None),
                          "q2_4x3": ((4, 4, 4), 2, None), "aniso": ((8, 8), 1, (1.0, 0.1))}[name.split("+")[0]]
    A = po.poisson_matrix(nc, order, lengths=lengths)
    A = ar.M(A.shape, A.ptr, A.idx, A.val)
    if name.endswith("+isolated"):
        A = ar.with_isolated_rows(A, (A.shape[0] // 2, A.shape[0] - 1))
    if name.endswith("+zero"):
        A = ar.with_zero_row(A, A.shape[0] // 2)
    return A


CASES = [("chain1", 0.25, 0), ("chain2", 0.25, 0), ("chain3", 0.25, 0), ("chain17", 0.25, 0), ("chain64", 0.25, 0), ("chain65", 0.25, 0),
         ("chain129", 0.25, 0), ("q1_8x2", 0.25, 0), ("q1_9x8", 0.25, 0), ("q1_6x3", 0.25, 0), ("q2_4x3", 0.25, 0), ("aniso", 0.25, 0),
         ("aniso", 0.75, 0), ("q1_8x2", 0.0, 0), ("q1_8x2", 1.0, 0), ("q1_8x2+isolated", 0.25, 0), ("q1_8x2+zero", 0.25, 0),
         ("nonsym", 0.25, 0), ("q1_8x2", 0.25, 1), ("q1_6x3", 0.25, 1)]


def _graph(g, n):
    G = sp.csr_matrix((np.ones(g["ei"].size), (g["ei"], g["ej"])), shape=(n, n))
    assert (G != G.T).nnz == 0                                # an edge is stored in both directions
    return G


@pytest.mark.parametrize("name,theta,seed", CASES)
def test_aggregation_is_valid(name, theta, seed):
    A = _matrix(name)
    n = A.shape[0]
    g = ar.build(A, theta=theta, seed=seed)
    agg, nagg, roots = g["agg"].astype(np.int64), g["nagg"], g["roots"]
    # every row is in exactly one aggregate, every aggregate has exactly one root, root ids ascend with the row index
    assert agg.shape == (n,) and agg.min() == 0 and agg.max() == nagg - 1
    assert np.array_equal(np.bincount(agg[roots], minlength=nagg), np.ones(nagg, dtype=np.int64))
    assert np.array_equal(agg[roots], np.arange(nagg))
    G = _graph(g, n)
    eye = sp.identity(n, format="csr")
    reach2 = ((eye + G + G @ G) != 0).tocsr()
    # roots are pairwise at graph distance >= 3
    rr = reach2[np.flatnonzero(roots)][:, np.flatnonzero(roots)]
    assert rr.nnz == nagg
    # every member is within distance 2 of the root of its aggregate
    root_row = np.flatnonzero(roots)[agg]
    assert np.all(np.asarray(reach2[np.arange(n), root_row]).ravel())
    # a pass-1 node that is not a root has exactly one root neighbour; the others have none
    nroot_nb = np.asarray(G[:, np.flatnonzero(roots)].sum(axis=1)).ravel()
    assert np.all(nroot_nb[g["pass1"] & ~roots] == 1) and np.all(nroot_nb[~g["pass1"]] == 0) and np.all(nroot_nb[roots] == 0)
    # a node without edges is a root and a singleton
    lonely = np.asarray(G.sum(axis=1)).ravel() == 0
    assert np.all(roots[lonely]) and np.all(np.bincount(agg, minlength=nagg)[agg[lonely]] == 1)
    assert g["strong_edges"] == G.nnz // 2


@pytest.mark.parametrize("name,theta,seed", CASES)
def test_prolongation_rows(name, theta, seed):
    A = _matrix(name)
    n = A.shape[0]
    g = ar.build(A, theta=theta, seed=seed)
    T, _om, _rho = ar.prolongation(A, g["agg"], g["nagg"], smooth=False)
    assert np.array_equal(T.to_scipy() @ np.ones(g["nagg"]), np.ones(n))        # the rows of T sum to 1
    P, om, rho = g["P"], g["omega"], g["rho"]
    S = A.to_scipy()
    assert om == (4.0 / 3.0) / rho
    assert abs(rho - np.max(np.asarray(abs(S).sum(axis=1)).ravel() / np.abs(S.diagonal()))) <= 1e-14 * rho
    want = 1.0 - om * (S @ np.ones(n)) / S.diagonal()
    assert np.max(np.abs(P.to_scipy() @ np.ones(g["nagg"]) - want)) <= 1e-14    # P 1 = 1 - omega D^-1 A 1
    assert np.all(np.diff(P.ptr) >= 1)
    for i in range(n):
        assert np.all(np.diff(P.idx[P.ptr[i]:P.ptr[i + 1]]) > 0)               # ascending, no column twice


@pytest.mark.parametrize("name", ("chain17", "q1_8x2", "q1_6x3", "q2_4x3", "nonsym"))
def test_power_of_two_scaling(name):
    """2 A and A / 4 give the same aggregates and the same P, bit for bit (every comparison and quotient is scale-free in binary)"""
    A = _matrix(name)
    g = ar.build(A)
    for c in (2.0, 0.25):
        h = ar.build(ar.M(A.shape, A.ptr, A.idx, A.val * c))
        assert np.array_equal(h["agg"], g["agg"]) and h["rounds"] == g["rounds"] and h["rho"] == g["rho"] and h["omega"] == g["omega"]
        assert np.array_equal(h["P"].ptr, g["P"].ptr) and np.array_equal(h["P"].idx, g["P"].idx) and np.array_equal(h["P"].val, g["P"].val)


def test_stored_zero_face_couplings_are_never_strong():
    """3-D Q1: the face couplings are stored 0.0; with theta = 0 every NONZERO entry is strong and they still are not edges"""
    A = _matrix("q1_6x3")
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.ptr))
    zero = (A.val == 0.0) & (rows != A.idx)
    assert zero.any()
    ei, ej, _w = ar.strength(A, 0.0)
    edges = set(zip(ei.tolist(), ej.tolist()))
    assert not any((int(i), int(j)) in edges for i, j in zip(rows[zero], A.idx[zero]))
    assert len(edges) == int(((A.val != 0.0) & (rows != A.idx)).sum())


def test_one_sided_strength_is_an_edge():
    A = _matrix("nonsym")
    ei, ej, w = ar.strength(A, 0.25)
    edges = dict(zip(zip(ei.tolist(), ej.tolist()), w.tolist()))
    assert (1, 0) in edges and (0, 1) in edges and edges[(1, 0)] == edges[(0, 1)] == 1.0   # (1, 0) holds 0.01 against a row maximum of 1
    assert (0, 2) not in edges and (2, 0) not in edges


def test_bad_matrices_are_named():
    A = ar.chain(5)
    val = A.val.copy()
    val[np.flatnonzero((np.repeat(np.arange(5), np.diff(A.ptr)) == 3) & (A.idx == 3))] = 0.0
    with pytest.raises(ValueError, match="row 3"):
        ar.build(ar.M(A.shape, A.ptr, A.idx, val))
    S = A.to_scipy().tolil()
    S[1, 4] = 0.5
    with pytest.raises(ValueError, match=r"\(1, 4\)"):
        ar.build(ar.from_scipy(S.tocsr()))


def test_python_marker_and_constructor_checks(S, po):
    """solvers.Aggregation and what GMGLinearSolver refuses before any handle exists"""
    A0 = po.poisson_matrix((4, 4), 1)
    ag = S.Aggregation()
    assert (ag.theta, ag.smooth, ag.omega, ag.seed) == (0.25, True, None, 0)
    for bad in (dict(theta=-0.1), dict(theta=1.5), dict(omega=0.0), dict(seed=-1)):
        with pytest.raises(ValueError):
            S.Aggregation(**bad)
    g = S.GMGLinearSolver([A0, S.Galerkin(), S.Galerkin()], [S.Aggregation(), S.Aggregation()])
    assert g.num_levels() == 3
    with pytest.raises(ValueError, match="smatrices\\[1\\] must be Galerkin"):
        S.GMGLinearSolver([A0, A0], [S.Aggregation()])
    with pytest.raises(ValueError, match="level 0 takes no explicit restriction"):
        S.GMGLinearSolver([A0, S.Galerkin()], [S.Aggregation()], [A0])
    pp, pd = po.vertex_star_patches((4, 4), 1)
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 2), S.RichardsonSmoother(S.PatchSolver(pp, pd), 2, 0.2)]
    with pytest.raises(ValueError, match="level 1 takes its size from the aggregation of level 0"):
        S.GMGLinearSolver([A0, S.Galerkin(), S.Galerkin()], [S.Aggregation(), S.Aggregation()], pre_smoothers=sm, post_smoothers=sm)
    with pytest.raises(ValueError, match="cycle_values='float32' does not take a Galerkin"):
        S.GMGLinearSolver([A0, S.Galerkin()], [S.Aggregation()], cycle_values="float32")
