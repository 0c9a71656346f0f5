"""cycle_values = "float32", host side (no GPU): the reference helper (tests/values_f32_reference.py) does what the feature's
definition says, the numpy twin on rounded levels converges like the fp64 one, and the constructor refuses what it can see.

The three CG rows are the CPU experiment the feature was proposed on (variable-coefficient Q1, po.smooth_kappa, po.random_rhs,
CG + GMG(Jacobi, omega = 2/3), every level but the coarsest rounded): equal iteration counts with and without the rounding, and the
true residual ||b - A x|| / ||b|| (unrounded A) below rtol in both."""
import numpy as np
import pytest

import values_f32_reference as vr

ROWS = (((16, 16, 16), 3, 3, 1e-10), ((12, 8, 8), 3, 2, 1e-12), ((32, 32, 32), 4, 10, 1e-10))


def _varcoef(po, cells, nlev):
    return po.build_hierarchy(cells, nlev, kappa=po.smooth_kappa)


def test_round_levels_is_idempotent(po):
    mats = _varcoef(po, (12, 8, 8), 3)["mats"]
    once = vr.round_levels(mats, vr.f32_levels(mats))
    twice = vr.round_levels(once, vr.f32_levels(mats))
    changed = False
    for a, b, m in zip(once, twice, mats):
        assert np.array_equal(a.val, b.val)
        changed = changed or not np.array_equal(a.val, m.val)
    assert changed, "the variable-coefficient values are not all float32 numbers: the helper must have rounded something"
    assert np.array_equal(once[-1].val, mats[-1].val), "the coarsest level is not in f32_levels"
    for a, m in zip(once[:-1], mats[:-1]):
        assert np.array_equal(a.val.astype(np.float32).astype(np.float64), a.val)
        nz = m.val != 0.0
        assert (np.abs(a.val[nz] - m.val[nz]) / np.abs(m.val[nz])).max() <= 2.0 ** -24   # half an ulp of float32: round to nearest


def test_round_levels_keeps_pattern_zeros_and_symmetry(po):
    mats = list(_varcoef(po, (12, 8, 8), 3)["mats"])
    # plant stored zeros, symmetrically: every stored entry (i, j) with i + j divisible by 7 and i != j
    A0 = mats[0]
    rows = np.repeat(np.arange(A0.shape[0]), np.diff(A0.ptr))
    val = A0.val.copy()
    val[((rows + A0.idx) % 7 == 0) & (rows != A0.idx)] = 0.0
    mats[0] = po.CSR(A0.shape, A0.ptr, A0.idx, val)
    rounded = vr.round_levels(mats, range(len(mats)))
    assert (mats[0].val == 0.0).any()
    for A, B in zip(mats, rounded):
        assert B is not A and B.val is not A.val and not np.shares_memory(B.val, A.val)
        assert B.shape == A.shape and np.array_equal(B.ptr, A.ptr) and np.array_equal(B.idx, A.idx)
        zeros = A.val == 0.0
        assert np.array_equal(B.val == 0.0, zeros)           # explicit zeros stay, nothing else becomes one
        S0, S1 = A.to_scipy(), B.to_scipy()
        assert abs(S0 - S0.T).max() == 0.0
        assert abs(S1 - S1.T).max() == 0.0                   # rounding is entry-wise: a symmetric matrix stays symmetric
    untouched = vr.round_levels(mats, [])
    assert all(np.array_equal(A.val, B.val) for A, B in zip(mats, untouched))


@pytest.mark.parametrize("cells,nlev,sweeps,rtol", ROWS, ids=["16^3", "12x8x8", "32^3"])
def test_twin_converges_alike_on_rounded_levels(po, cells, nlev, sweeps, rtol):
    H = _varcoef(po, cells, nlev)
    b = po.random_rhs(H["mats"][0].shape[0])
    x64, it64, hist64, true64 = vr.twin_cg(H, b, sweeps, rtol, which=[])
    x32, it32, hist32, true32 = vr.twin_cg(H, b, sweeps, rtol)
    print("cells %s: iterations %d / %d, true residual %.4e / %.4e, |x32 - x64| / |x64| = %.1e"
          % (cells, it64, it32, true64, true32, np.linalg.norm(x32 - x64) / np.linalg.norm(x64)))
    assert it32 == it64
    assert true64 < rtol and true32 < rtol


def test_constructor_refuses_unknown_cycle_values(S, po):
    H = _varcoef(po, (4, 4, 4), 2)
    with pytest.raises(ValueError, match="cycle_values"):
        S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], cycle_values="float16")
    assert S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"]).cycle_values == "float64"
    assert S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], cycle_values="float32").cycle_values == "float32"


def test_constructor_refuses_float32_in_solver_mode(S, po):
    H = _varcoef(po, (4, 4, 4), 2)
    with pytest.raises(ValueError, match="preconditioner"):
        S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], cycle_values="float32", mode="solver")
    S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], cycle_values="float64", mode="solver")


def test_constructor_refuses_float32_with_a_galerkin_level(S, po):
    H = _varcoef(po, (4, 4, 4), 2)
    with pytest.raises(ValueError, match="Galerkin"):
        S.GMGLinearSolver([H["mats"][0], S.Galerkin()], H["prolongations"], H["restrictions"], cycle_values="float32")
