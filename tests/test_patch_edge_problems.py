"""Host checks of the inputs of tests/test_gpu_patch_edges.py (tests/patch_edge_problems.py): for every case the device file runs,
the level matrix, the patch set and the blocks are what they claim to be -- well conditioned, pivoting where pivoting is meant to be
exercised and nowhere else -- and the float64 restatement of the kernels stays within 1e-14 of the np.longdouble reference, which
is what lets the device gate be 1e-12: a device failure cannot be blamed on the inputs.  No GPU."""
import numpy as np
import pytest

import patch_edge_problems as pe

if not np.finfo(np.longdouble).eps < 2e-19:
    pytest.skip("np.longdouble is not an extended-precision type here (eps = %g): the references would be no better than the float64 "
                "arithmetic under test" % np.finfo(np.longdouble).eps, allow_module_level=True)

TWIN_GATE = 1e-14
KEYS = pe.CASE_KEYS
IDS = ["%s-%s" % k for k in KEYS]


def _cols(c):
    return c.pd if c.pc is None else c.pc


def _blocks(c):
    return c.blocks if c.blocks is not None else pe.blocks_of(c.A, c.pp, c.pd, c.pc)


def test_case_list_covers_the_device_file():
    assert set(pe.CASES) == {"wave63", "wave64", "dedup_ragged", "big", "big_cols", "wave_cols", "dense", "sell_refresh", "sell_refresh_big"}
    for name in ("wave63", "wave64", "dedup_ragged", "big", "sell_refresh", "sell_refresh_big"):
        assert pe.CASES[name]["kinds"] == ("lu", "nopivot")
    for name in ("big_cols", "wave_cols", "dense"):
        assert pe.CASES[name]["kinds"] == ("lu",)


@pytest.mark.parametrize("family", pe.FAMILIES)
def test_level_matrix_is_what_it_claims(family):
    A = pe.level_matrix(family)
    N = A.shape[0]
    assert N == (pe.N_PERIODIC if family.startswith("periodic") else pe.N_LEVEL) and N % 64 == 37
    assert A.has_sorted_indices and A.shape == (N, N)
    A2 = pe.level_matrix(family)
    assert np.array_equal(A.data, A2.data) and np.array_equal(A.indices, A2.indices) and np.array_equal(A.indptr, A2.indptr)
    assert np.any(pe.level_matrix(family, seed=1).data != A.data)
    co = A.tocoo()
    assert np.all(np.abs(co.col - co.row) <= pe.HALF) and A.nnz == sum(N - abs(k) for k in range(-pe.HALF, pe.HALF + 1))
    d = A.diagonal()
    assert np.all(d != 0.0)                                                  # D^-1 exists
    i = np.arange(N)
    q = np.array([pe.partner(k, N) for k in i])
    paired = q >= 0
    big = np.where(paired, np.asarray(A[i, np.where(paired, q, i)]).ravel(), d) if family.endswith("pairs") else d
    assert np.all((big >= 4.0) & (big < 5.0))
    if family.endswith("pairs"):
        assert np.all((d[paired] >= 0.025) & (d[paired] < 0.05))
    special = (co.row == co.col) | (co.col == q[co.row])
    assert np.all(np.abs(co.data[~special]) <= 0.2)
    if family.startswith("periodic"):
        # every value is a function of (i mod 14, j - i): rows 14 apart are bitwise equal away from the two ends
        for k in range(pe.HALF, N - pe.PERIOD - pe.HALF, 997):
            a, b = A[k], A[k + pe.PERIOD]
            assert np.array_equal(a.data, b.data) and np.array_equal(a.indices + pe.PERIOD, b.indices)
    H = pe.two_level(A, 8)
    P = H["prolongations"][0]
    assert P.shape == (N, (N + 7) // 8) and np.all(np.diff(P.indptr) == 1) and abs(H["restrictions"][0] - P.T).max() == 0.0
    assert np.array_equal(H["mats"][1].toarray(), 2.0 * np.eye(P.shape[1]))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_patch_set_is_what_it_claims(key):
    c = pe.case(*key)
    np_ = np.diff(c.pp)
    npatch = np_.size
    if c.name in ("wave63", "sell_refresh"):
        assert npatch == 43 and npatch % 4 == 3 and list(np_) == [pe.WAVE_SIZES[p % 10] for p in range(43)] and np_.max() == 63
    elif c.name in ("wave64", "wave_cols", "dense"):
        want = [pe.WAVE_SIZES[p % 10] for p in range(43)]
        diff = [p for p in range(43) if np_[p] != want[p]]
        assert len(diff) == 1 and np_[diff[0]] == 64 and np_.max() == 64 and np.sum(np_ == 64) == 1
    elif c.name == "dedup_ragged":
        assert npatch == 64 * 3 + 9 and list(np_) == [pe.DEDUP_SIZES[p % 6] for p in range(npatch)] and np_.max() == 32
    else:
        assert list(np_) == list(pe.BIG_SIZES) and np_.max() == 130 and np.sum(np_ > 64) == 5
    assert c.pd.dtype == np.int32 and c.pp.dtype == np.int64 and c.pd.size == c.pp[-1]
    assert c.pd.min() >= 0 and c.pd.max() < c.N
    in_patch = np.zeros(c.N, dtype=bool)
    unsorted = 0
    for p in range(npatch):
        d = c.pd[c.pp[p]:c.pp[p + 1]]
        assert np.unique(d).size == d.size
        in_patch[:] = False
        in_patch[d] = True
        for k in d:                                                          # no pair is split
            q = pe.partner(int(k), c.N)
            assert k % 7 == 6 or (q >= 0 and in_patch[q]), (p, int(k))
        unsorted += d.size >= 2 and not np.all(np.diff(d) > 0)
        if d.size >= 4:                                                      # not contiguous
            assert np.ptp(d) >= d.size
    assert unsorted >= 1
    if c.name != "dedup_ragged":                                             # shuffled: every patch of >= 2 dofs is out of order
        assert unsorted == np.sum(np_ >= 2)
    if c.pc is not None:
        for p in range(npatch):
            assert np.array_equal(c.pc[c.pp[p]:c.pp[p + 1]], c.pd[c.pp[p]:c.pp[p + 1]][::-1])
    m = pe.multiplicity(c.N, c.pp, _cols(c))
    have = set(m.tolist())
    # (the eight patches of the big set cannot hold a dof nine times)
    assert have >= ({0, 1, 3, 4, 5} if npatch < 9 else {0, 1, 3, 4, 5, 9}), sorted(have)
    assert {w % 4 for w in have} == {0, 1, 2, 3}                             # the tail of the gather's unrolled-by-4 loop
    # dofs of different patches interleave: between the smallest and the largest dof of a big patch lie dofs of other patches
    big = int(np.argmax(np_))
    d = c.pd[c.pp[big]:c.pp[big + 1]]
    others = np.setdiff1d(c.pd, d)
    assert np.any((others > d.min()) & (others < d.max()))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_blocks_are_well_conditioned_and_pivot_as_intended(key):
    c = pe.case(*key)
    ref = pe.reference(*key)
    np_ = np.diff(c.pp)
    worst = 0.0
    for p, B in enumerate(_blocks(c)):
        if np_[p] == 0:
            continue
        worst = max(worst, float(np.linalg.cond(B, 2)))
    print("%s %s: worst kappa_2 = %.3f, row swaps per patch %s" % (c.name, c.kind, worst, ref.swaps.tolist()[:12]))
    assert worst <= 10.0
    if c.pivot and (c.family.endswith("pairs") or c.pc is not None):
        for p in range(np_.size):
            if np_[p] >= 4:
                assert ref.swaps[p] >= np_[p] // 2 - 1, (p, int(np_[p]), int(ref.swaps[p]))
    if not c.pivot:
        assert np.all(ref.swaps == 0)
        assert np.all(ref.minpiv[np_ > 0] >= 1.0)


def test_dedup_case_has_bitwise_equal_blocks_per_size():
    """patches of one size of the periodic family have bitwise equal blocks (what block de-duplication needs), and there are few"""
    for kind in ("lu", "nopivot"):
        c = pe.case("dedup_ragged", kind)
        first = {}
        for p, B in enumerate(_blocks(c)):
            ref = first.setdefault(B.shape[0], B)
            assert np.array_equal(ref, B), p
        assert sorted(first) == sorted(pe.DEDUP_SIZES)
        assert 4 * len(first) <= c.pp.size - 1                               # build_patch keeps the compact store


def test_reference_counts_swaps_and_takes_the_first_maximum():
    F = pe._factor(np.array([[1.0, 2.0], [-1.0, 1.0]]), True)                # tie in column 0: the first maximum, no swap
    assert F[2] == 0 and np.array_equal(F[1], [0, 1])
    F = pe._factor(np.array([[0.0, 1.0], [1.0, 0.0]]), True)
    assert F[2] == 1 and np.array_equal(F[1], [1, 0])
    with pytest.raises(ZeroDivisionError):
        pe._factor(np.array([[0.0, 1.0], [1.0, 0.0]]), False)
    rng = np.random.default_rng(0)
    B = rng.uniform(-1, 1, (9, 9))
    b = rng.uniform(-1, 1, 9)
    x = pe._lu_solve(pe._factor(B, True), b)
    assert np.max(np.abs(B.astype(pe.LD) @ x - b)) <= 1e-16
    assert np.max(np.abs(pe.twin_inverse(B, True) @ B - np.eye(9))) <= 1e-12


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_float64_twin_stays_within_1e14_of_the_longdouble_reference(key):
    c = pe.case(*key)
    ref = pe.reference(*key)
    dx, x, r = pe.twin(*key)
    dev = [pe.max_rel(a.astype(pe.LD), b) for a, b in ((dx, ref.dx_ld), (x, ref.x_ld), (r, ref.r_ld))]
    print("%s %s: twin vs longdouble, max|a - b| / max|b|: precond %.3e, x %.3e, r %.3e" % (c.name, c.kind, *dev))
    assert all(np.all(np.isfinite(a)) for a in (dx, x, r))
    assert max(dev) <= TWIN_GATE
    cov = pe.multiplicity(c.N, c.pp, _cols(c)) > 0
    assert np.all(ref.dx_ld[~cov] == 0) and np.all(dx[~cov] == 0.0) and np.all(ref.dx[cov] != 0.0)
    # the smoother moves x and r by something the gate can see
    assert pe.max_rel(ref.x, c.x0) > 1e-3 and pe.max_rel(ref.r, c.r) > 1e-3


def test_tie_case_pins_the_first_maximum():
    """the device test's tie block: equal column maxima in columns 0 and 1, the first of them taken (no swap, then one swap with
    row 5); the float64 twin with the LAST maximum instead gives other bits in the inverse and in dx, so equal bits on the device
    mean the first-maximum rule"""
    c = pe.tie_case()
    ref = pe.adhoc_reference(c)
    B = c.blocks[0]
    assert B.shape == (33, 33) and np.linalg.cond(B, 2) <= 10.0
    for colj, rows, vals in pe.TIE_ROWS:
        assert [B[r, colj] for r in rows] == list(vals)
        others = np.delete(np.abs(B[:, colj]), rows)
        assert others.max() < min(abs(v) for v in vals)
    assert ref.swaps.tolist() == [1, 0, 0] and ref.perms[0][:6].tolist() == [0, 5, 2, 3, 4, 1]
    assert set(pe.multiplicity(c.N, c.pp, c.pd).tolist()) == {0, 1}
    first = pe.twin_inverse(B, True)
    last = pe.twin_inverse(B, True, tie_last=True)
    assert np.sum(first.view(np.int64) != last.view(np.int64)) > 0 and np.max(np.abs(first - last)) <= 1e-13
    X = pe.twin_inverses(c.A, c.pp, c.pd, None, True, c.blocks)
    dx = pe.twin_precond(c.A, c.pp, c.pd, None, c.r, True, inverses=X)
    dx_last = pe.twin_precond(c.A, c.pp, c.pd, None, c.r, True, inverses=[last] + X[1:])
    assert np.sum(dx.view(np.int64) != dx_last.view(np.int64)) > 0
    assert pe.max_rel(dx.astype(pe.LD), ref.dx_ld) <= TWIN_GATE and pe.max_rel(dx_last.astype(pe.LD), ref.dx_ld) <= TWIN_GATE


def test_antidiagonal_case():
    c = pe.antidiagonal_case(True)
    ref = pe.adhoc_reference(c)
    assert np.array_equal(c.blocks[2], [[0.0, 1.0], [1.0, 0.0]]) and ref.swaps.tolist() == [0, 0, 1, 0, 0]
    assert max(np.linalg.cond(B, 2) for B in c.blocks) <= 10.0
    with pytest.raises(ZeroDivisionError):
        pe.adhoc_reference(pe.antidiagonal_case(False))
