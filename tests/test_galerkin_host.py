"""Galerkin coarse matrices on the host: the numpy twin (tests/galerkin_reference.py) against scipy's R @ (A @ P), the library's
symbolic phase (gmg_galerkin_pattern, no GPU) against the twin's patterns, the twin's iteration counts, and the argument checks of
the constructor, of update and of the host function."""
import ctypes as C

import numpy as np
import pytest

import galerkin_reference as gal
import numpy_twin as nt

TOL = 1e-13     # the project's per-kernel bound: max|a - b| / max|b|

CASES = (((8, 8), 1), ((8, 8, 8), 1), ((4, 4, 4), 2))


def _scipy_product(R, A, P):
    S = (R.to_scipy() @ (A.to_scipy() @ P.to_scipy())).tocsr()
    S.sort_indices()
    return S


def _same_pattern(got, want):
    ptr, col = got
    return ptr.dtype == np.int64 and col.dtype == np.int32 and np.array_equal(ptr, want.ptr) and np.array_equal(col, want.idx)


# ---------------------------------------------------------------- the twin against scipy
@pytest.mark.parametrize("nc,order", CASES)
def test_twin_against_scipy_on_hierarchies(hierarchy, nc, order):
    H = hierarchy(nc, 2, order)
    A, P, R = H["mats"][0], H["prolongations"][0], H["restrictions"][0]
    T, Ac = gal.galerkin(R, A, P)
    S = _scipy_product(R, A, P)                               # (scipy drops entries whose terms cancel to 0.0: compare values, not patterns)
    assert abs(Ac.to_scipy() - S).max() <= TOL * np.max(np.abs(S.data))
    # the structural pattern of R (A P) is the pattern of the re-discretised coarse matrix on these nested hierarchies
    red = H["mats"][1].to_scipy().tocsr()
    red.sort_indices()
    assert np.array_equal(Ac.ptr, red.indptr) and np.array_equal(Ac.idx, red.indices)
    assert np.max(np.abs(Ac.val - red.data)) <= 1e-12 * np.max(np.abs(red.data))
    # R = None is P^T
    Ac2 = gal.galerkin(None, A, P)[1]
    assert np.array_equal(Ac2.val, Ac.val)


def test_twin_against_scipy_on_the_ragged_case():
    c = gal.ragged_problem(gal.RAGGED_SEED)
    A, P, R = c["A"], c["P"], c["R"]
    assert np.diff(P.ptr).min() == 0 and np.diff(P.ptr).max() == 5 and np.unique(P.idx).size == P.shape[1]
    assert any(np.any(np.diff(A.idx[A.ptr[i]:A.ptr[i + 1]]) < 0) for i in range(A.shape[0])) and np.sum(A.val == 0.0) == 1
    Pt = gal.transpose(P)
    assert not np.array_equal(R.ptr, Pt.ptr)                                          # a perturbed P^T, values and pattern
    T, Ac = gal.galerkin(R, A, P)
    S = _scipy_product(R, A, P)
    D = Ac.to_scipy().toarray()
    assert np.linalg.cond(D) < 1e8
    assert np.max(np.abs(D - S.toarray())) <= TOL * np.max(np.abs(S.data))
    for X in (T, Ac):                                                                 # columns ascend in every row
        assert all(np.all(np.diff(X.idx[X.ptr[i]:X.ptr[i + 1]]) > 0) for i in range(X.shape[0]))


def test_twin_keeps_cancelled_entries():
    c = gal.cancelling_problem()
    T, Ac = gal.galerkin(c["R"], c["A"], c["P"])
    assert T.val[3] == 0.0 and (T.ptr[1], T.idx[3]) == (2, 1)                         # T(1, 1), stored
    assert np.array_equal(Ac.ptr, [0, 2, 4]) and np.array_equal(Ac.idx, [0, 1, 0, 1]) and Ac.val[2] == 0.0
    assert np.array_equal(Ac.val, [7.5, -1.0, 0.0, 1.0])


# ---------------------------------------------------------------- the library's symbolic phase against the twin
@pytest.mark.parametrize("nc,order", CASES)
def test_pattern_on_hierarchies(S, hierarchy, nc, order):
    H = hierarchy(nc, 2, order)
    A, P, R = H["mats"][0], H["prolongations"][0], H["restrictions"][0]
    T, Ac = gal.galerkin(R, A, P)
    tp, cp = S.galerkin_pattern(R, A, P)
    assert _same_pattern(tp, T) and _same_pattern(cp, Ac)


def test_pattern_on_the_ragged_case(S):
    c = gal.ragged_problem(gal.RAGGED_SEED)
    T, Ac = gal.galerkin(c["R"], c["A"], c["P"])
    tp, cp = S.galerkin_pattern(c["R"], c["A"], c["P"])                               # A's rows unsorted, one explicit zero
    assert _same_pattern(tp, T) and _same_pattern(cp, Ac)
    assert np.diff(tp[0]).min() == 0                                                  # a row of T without entries


def test_pattern_on_the_cancelling_case(S):
    c = gal.cancelling_problem()
    T, Ac = gal.galerkin(None, c["A"], c["P"])
    tp, cp = S.galerkin_pattern(gal.transpose(c["P"]), c["A"], c["P"])
    assert _same_pattern(tp, T) and _same_pattern(cp, Ac)


def test_pattern_many_rows_in_parallel_chunks(S, hierarchy):
    """enough rows for the symbolic phase to split them into chunks (one chunk below 4096 rows)"""
    H = hierarchy((96, 96), 2, 1)
    A, P, R = H["mats"][0], H["prolongations"][0], H["restrictions"][0]
    assert A.shape[0] > 2 * 4096
    tp, cp = S.galerkin_pattern(R, A, P)
    T, Ac = gal.galerkin(R, A, P)
    assert _same_pattern(tp, T) and _same_pattern(cp, Ac)
    assert np.sum(T.val == 0.0) > 0                           # entries of T that cancel to 0.0 (scipy's product drops them) stay stored


def test_pattern_argument_checks(pkg, S):
    c = gal.cancelling_problem()
    A, P = c["A"], c["P"]
    R = gal.transpose(P)
    with pytest.raises(ValueError):
        S.galerkin_pattern(P, A, P)                                                   # shapes do not chain
    lib, abi = pkg.abi.load(), pkg.abi
    p = lambda a: C.c_void_p(a.ctypes.data)
    tn, cn = C.c_int64(), C.c_int64()
    args = (2, 4, p(R.ptr), p(R.idx), p(A.ptr), p(A.idx), p(P.ptr), p(P.idx))
    assert lib.gmg_galerkin_pattern(*args, None, None, 0, C.byref(tn), None, None, 0, C.byref(cn)) == abi.OK
    assert (tn.value, cn.value) == (7, 4)
    tptr, tcol = np.empty(5, dtype=np.int64), np.empty(7, dtype=np.int32)
    assert lib.gmg_galerkin_pattern(*args, p(tptr), p(tcol), 6, C.byref(tn), None, None, 0, C.byref(cn)) == abi.ERR_INVALID   # tcap too small
    bad = P.idx.copy()
    bad[1] = 2                                                                        # a column of P outside [0, nc)
    assert lib.gmg_galerkin_pattern(2, 4, p(R.ptr), p(R.idx), p(A.ptr), p(A.idx), p(P.ptr), p(bad), None, None, 0, C.byref(tn),
                                    None, None, 0, C.byref(cn)) == abi.ERR_INVALID
    assert b"column index out of range" in lib.gmg_last_error(None)
    badptr = A.ptr.copy()
    badptr[2] = 1                                                                     # non-monotone row pointers of A
    assert lib.gmg_galerkin_pattern(2, 4, p(R.ptr), p(R.idx), p(badptr), p(A.idx), p(P.ptr), p(P.idx), None, None, 0, C.byref(tn),
                                    None, None, 0, C.byref(cn)) == abi.ERR_INVALID


# ---------------------------------------------------------------- iteration counts of the twin
def _twin_cg_iters(H, mats, seed=5):
    jac = [(nt.Jacobi(m.to_scipy().tocsr()), 10, 2.0 / 3.0) for m in mats[:-1]]
    g = nt.GMG(mats, H["prolongations"], H["restrictions"], jac)
    A0 = mats[0].to_scipy().tocsr()
    b = np.random.default_rng(seed).standard_normal(A0.shape[0])
    x, it, _hist = nt.cg(A0, b, Pl=g.solve, maxiter=50, atol=1e-14, rtol=1e-8)
    return it, x


@pytest.mark.parametrize("nc,order,nlev,iters", (((16, 16, 16), 1, 3, 3), ((32, 32), 1, 4, 4), ((16, 16), 2, 3, 4)))
def test_twin_iteration_counts(hierarchy, nc, order, nlev, iters):
    """CG + GMG(Jacobi 10, 2/3), rtol 1e-8: the same count with Galerkin and with re-discretised coarse matrices"""
    H = hierarchy(nc, nlev, order)
    mats = gal.chain(H["mats"][0], H["prolongations"], H["restrictions"])
    it_g, x_g = _twin_cg_iters(H, mats)
    it_r, x_r = _twin_cg_iters(H, H["mats"])
    assert it_g == it_r == iters
    assert np.linalg.norm(x_g - x_r) <= 1e-7 * np.linalg.norm(x_r)


# ---------------------------------------------------------------- constructor and update argument checks
def test_constructor_accepts_the_marker(S, po, hierarchy):
    H = hierarchy((8, 8), 3, 1)
    G = S.Galerkin
    g = S.GMGLinearSolver([H["mats"][0], G(), G()], H["prolongations"], H["restrictions"])
    assert g.num_levels() == 3 and isinstance(g.smatrices[1], G) and repr(g.smatrices[2]) == "Galerkin()"
    S.GMGLinearSolver([H["mats"][0], H["mats"][1], G()], H["prolongations"])          # mixed, R = P^T
    with pytest.raises(ValueError):
        S.GMGLinearSolver([G(), H["mats"][1], H["mats"][2]], H["prolongations"])      # the finest level cannot be one
    with pytest.raises(ValueError):
        S.GMGLinearSolver([H["mats"][0], G()], H["prolongations"])                    # the length check still holds


def test_coarse_nullspace_size_comes_from_the_prolongation(S, po):
    H = po.neumann_hierarchy((8, 8), 2, 1)
    nco = H["prolongations"][0].shape[1]
    ok = S.NullspaceSolver(S.LUSolver(), S.NullSpace(np.ones((nco, 1))))
    S.GMGLinearSolver([H["mats"][0], S.Galerkin()], H["prolongations"], coarsest_solver=ok)
    bad = S.NullspaceSolver(S.LUSolver(), S.NullSpace(np.ones((nco + 1, 1))))
    with pytest.raises(ValueError):
        S.GMGLinearSolver([H["mats"][0], S.Galerkin()], H["prolongations"], coarsest_solver=bad)


def test_update_refuses_a_matrix_for_a_galerkin_level(S, hierarchy):
    """the check runs before any native call: a setup object without a handle is enough"""
    H = hierarchy((8, 8), 3, 1)
    ns = S.GMGNumericalSetup.__new__(S.GMGNumericalSetup)
    ns.solver = S.GMGLinearSolver([H["mats"][0], S.Galerkin(), H["mats"][2]], H["prolongations"])
    ns.h = None
    with pytest.raises(ValueError, match="level 1 is a Galerkin level"):
        ns.update(H["mats"][0], smatrices=[None, H["mats"][1], H["mats"][2]])
