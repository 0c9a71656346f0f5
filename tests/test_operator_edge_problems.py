"""Host checks of tests/operator_edge_problems.py: the problems of the general sparse operator edge tests are what they claim to be
(so that a later edit cannot quietly soften them), the float64 twin of the kernels stays at the noise of the longdouble reference,
and every wrong kernel restated on the host shows on the family built for it.  No GPU."""
import numpy as np
import pytest

import operator_edge_problems as oe

TWIN_GATE = 1e-14                   # twin against the longdouble reference, max|a - ref| / max|ref|
GATE = 1e-13                        # the project's per-kernel gate (TOL_KERNEL)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _offdiag(A):
    rowof = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return A.data[A.indices != rowof], rowof


# ---------------------------------------------------------------- the matrices
@pytest.mark.parametrize("name", oe.CASES)
def test_square_matrices_are_dominant_sorted_and_scaled(name):
    c = oe.case(name)
    A = c.A
    assert A.shape == (c.n, c.n) and c.P.shape == (c.n, c.nH) and c.R.shape == (c.nH, c.n) and c.Ac.shape == (c.nH, c.nH)
    assert c.nH <= c.n <= 70001
    off, rowof = _offdiag(A)
    d = A.diagonal()
    need = 1.5 * np.bincount(rowof[A.indices != rowof], weights=np.abs(off), minlength=c.n) + 1.0
    assert np.all(d >= need) and np.all(d > 0)
    if c.values == "distinct":
        assert np.array_equal(d, need)
        assert np.unique(off).size == off.size              # every off-diagonal value differs
    if off.size:
        assert 1e-3 <= np.abs(off).min() and np.abs(off).max() <= 1e3
    if off.size > 1000:
        assert np.abs(off).min() < 1e-2 and np.abs(off).max() > 1e2
    for M in (A, c.P, c.R):
        for i in range(0, M.shape[0], max(1, M.shape[0] // 500)):
            cols = M.indices[M.indptr[i]:M.indptr[i + 1]]
            assert np.all(np.diff(cols) > 0)
    assert np.all(np.linalg.eigvalsh(c.Ac.toarray()) > 0)   # the given coarse matrix is SPD
    assert (c.R != c.P.T).nnz > 0 or c.family == "long"     # R is not P^T (the aggregation pair is, on purpose)


def test_ragged_row_lengths_and_diagonal_only_rows():
    for n in oe.SIZES:
        A = oe.case("ragged-%d" % n).A
        ln = np.diff(A.indptr) - 1
        assert ln.min() >= 0 and ln.max() <= min(40, n - 1)
        if n >= 63:
            assert np.count_nonzero(ln == 0) >= 1
        if n == 4283:
            assert 0.08 < np.mean(ln == 0) < 0.16 and ln.max() == 40
            assert (n + 63) // 64 == 67 and 67 % 8 == 3 and n - 64 * 66 == 59


def test_every_width_occurs_as_a_slice_maximum():
    for name in ("widths", "widths-few", "widths-few+1"):
        c = oe.case(name)
        assert oe.slice_widths(c.A).tolist() == list(oe.WIDTHS_SQUARE)
        assert oe.slice_widths(c.P).tolist() == list(oe.WIDTHS_TALL)
        for M, widths, least in ((c.A, oe.WIDTHS_SQUARE, 1), (c.P, oe.WIDTHS_TALL, 0)):
            ln = np.diff(M.indptr)
            for s, w in enumerate(widths):
                l = ln[64 * s:64 * s + 64]
                assert l.max() == w
                if w - 1 >= least:
                    assert np.any(l == w - 1), (name, w)     # a row shorter by exactly one entry
    assert set(oe.WIDTHS) == set(range(1, 11)) | {26, 27, 28, 31, 32, 33, 63, 64, 65, 66}
    assert {w % 4 for w in oe.WIDTHS} == {0, 1, 2, 3}
    for un in oe.SELL_UNROLLS:                                 # unrolled body only, remainder only, both
        assert any(w % un == 0 for w in oe.WIDTHS) and any(w < un for w in oe.WIDTHS) and any(w > un and w % un for w in oe.WIDTHS)


def test_long_rows_and_the_run_that_fills_a_tile():
    c = oe.case("long")
    ln = np.diff(c.A.indptr)
    for row, k in oe.LONG_ROWS.items():
        assert ln[row] == k and ln[row - 1] <= 13 and ln[row + 1] <= 16
    assert sorted(oe.LONG_ROWS.values()) == [2047, 2048, 2049, 3000]
    assert np.count_nonzero(ln > 16) == 4
    for lg in (-1, 0):
        blk, _ = oe.csr_blocks(c.A, lg)
        cnt = np.diff(c.A.indptr[blk])
        rows = np.diff(blk)
        assert np.any((cnt == oe.TILE) & (rows == oe.LONG_RUN[1]))          # 128 short rows: exactly one tile
        assert np.any((cnt == oe.TILE) & (rows == 1))                       # the 2048-entry row: still the tile branch
        assert sorted(cnt[cnt > oe.TILE].tolist()) == [2049, 3000] and np.all(rows[cnt > oe.TILE] == 1)
    ln_r = np.diff(c.R.indptr)
    assert ln_r.max() == 3000 and np.all(np.diff(c.P.indptr) == 1)          # R = P^T of the aggregation: one 3000-entry row
    assert (c.R != c.P.T).nnz == 0


def test_csr_partition_of_the_ragged_level():
    A = oe.case("ragged-4283").A
    blk, lg = oe.csr_blocks(A, 3)
    assert lg == 3 and blk.size - 1 == 134 and (blk.size - 1) % 8 != 0
    blk, lg = oe.csr_blocks(A)
    assert lg == 1 and blk[-1] == 4283
    for want in (0, 6):
        assert oe.csr_blocks(A, want)[1] == want


def test_value_counts_are_exactly_256_and_257():
    for name in oe.CASES:
        c = oe.case(name)
        k = np.unique(c.A.data.view(np.uint64)).size
        if c.values == "few":
            assert k == 256, (name, k)
        elif c.values == "few+1":
            assert k == 257, (name, k)
            few = oe.case(name[:-2]).A
            assert np.array_equal(few.indices, c.A.indices) and np.count_nonzero(few.data != c.A.data) == 1
        elif c.n >= 63:
            assert k > 257, (name, k)


def test_empty_rows_exist():
    for name in oe.CASES:
        c = oe.case(name)
        eP, eR = np.count_nonzero(np.diff(c.P.indptr) == 0), np.count_nonzero(np.diff(c.R.indptr) == 0)
        if c.family == "long":
            assert eP == 0 and eR == 0                          # aggregation: every row and every aggregate is used
        elif c.family == "offsets":
            assert eR > 0
        elif c.n >= 3:
            assert eP > 0 and eR > 0, (name, eP, eR)
    assert oe.slice_widths(oe.case("widths").P)[0] == 0       # a whole slice of empty rows


def test_wide_operator_has_both_span_kinds():
    c = oe.case("wide")
    spans = oe.column_spans(c.R)
    assert c.R.shape == (129, 70001) and c.P.shape == (70001, 129)
    assert np.any(spans > 65535) and np.any((spans >= 0) & (spans <= 65535)), spans
    lay = oe.expected_layout(c.R, oe.CONFIGS["sellc_dict_idx16"])
    assert lay["value_dictionary"] and lay["idx16"] and 0 < lay["slices16"] < lay["slices"]
    assert oe.expected_layout(c.P, oe.CONFIGS["sellc_dict_idx16"])["idx16"]


def test_base_column_operators_are_offset_patterns():
    c = oe.case("offsets")
    for M in (c.A, c.P, c.R):
        assert oe.expected_layout(M, oe.CONFIGS["sello"])["layout"] == "SELL-O"
    assert c.P.shape[1] < c.P.shape[0]                       # fewer columns than rows: offsets relative to a base column
    ln = np.diff(c.A.indptr)
    assert ln.max() == 7 and ln.min() < 7                    # rows shorter than the pattern width (clipped at the boundary)
    assert 0 < np.count_nonzero(ln[-(c.n % 64):] < 7)   # also in the ragged last slice


@pytest.mark.parametrize("pair", sorted(oe.INTENDED))
def test_padding_puts_each_pair_into_the_intended_branch(pair):
    name, cfg = pair
    got = oe.expected_layout(oe.case(name).A, oe.CONFIGS[cfg])
    want = oe.INTENDED[pair]
    assert {k: got[k] for k in want} == want, (pair, got)


def test_expected_layout_thresholds():
    A = oe.case("ragged-4283-few").A
    pad = oe.expected_layout(A, dict(pattern=0))["padding"]
    assert 1.25 < pad < 2.4                                   # beyond the bound, below 0.8 * 12 / 4: SELL only through the dictionary
    assert oe.expected_layout(A, dict(pattern=0, vdict=0))["layout"] == "CSR-stream"
    L = oe.case("long").A
    assert oe.expected_layout(L, dict(pattern=0, sell_maxpad=15.0))["layout"] == "CSR-stream"
    assert oe.expected_layout(L, dict(pattern=0, sell_maxpad=16.0))["layout"] == "SELL-64"
    with pytest.raises(ValueError):
        oe.expected_layout(A, None)


# ---------------------------------------------------------------- references
@pytest.mark.parametrize("name", oe.CASES)
def test_twin_stays_within_1e14_of_the_longdouble_reference(name):
    c, ref = oe.case(name), oe.reference(name)
    worst = 0.0
    for k in oe.SWEEPS:
        for start, want in ((c.x0, ref.sweeps[k]), (np.zeros(c.n), ref.zero[k])):
            x, r = oe.twin_sweeps(c.A, start, c.r0, k)
            worst = max(worst, oe.max_rel(x, want[0]), oe.max_rel(r, want[1]))
    dx = (1.0 / c.A.diagonal()) * c.r0
    worst = max(worst, oe.max_rel(dx, ref.dx))
    print("%s: twin against longdouble, worst max|a - ref| / max|ref| = %.3e" % (name, worst))
    assert worst <= TWIN_GATE, (name, worst)


@pytest.mark.parametrize("name", ("ragged-65", "ragged-4283", "widths", "long", "offsets"))
def test_row_reference_covers_all_rows(name):
    c, ref = oe.case(name), oe.reference(name)
    for key, M, v in (("A", c.A, c.x0), ("P", c.P, c.xc), ("R", c.R, c.x0)):
        seq, exact, bound = ref.rows[key]
        assert seq.size == M.shape[0]
        assert np.array_equal(_bits(seq), _bits(oe.seq_spmv(M, v)))          # the twin's row sum IS the CSR-order sum
        assert np.all(np.abs(seq - exact) <= bound)
        empty = np.diff(M.indptr) == 0
        assert np.all(_bits(seq[empty]) == 0) and np.all(bound[empty] == 0)  # empty rows: +0.0, nothing to round
        assert oe.max_rel(exact, oe.matvec_ld(M, v.astype(oe.LD))) <= 1e-15


# ---------------------------------------------------------------- sensitivity: every wrong kernel shows
@pytest.mark.parametrize("which", sorted(oe.CORRUPTIONS))
def test_corruptions_show(which):
    """each restated wrong kernel breaks the bit equality of y = A x with the CSR-order sum, or exceeds the 1e-13 gate of the
    sweeps, on the family built for it"""
    name, fn = oe.CORRUPTIONS[which]
    c, ref = oe.case(name), oe.reference(name)
    B = fn(c.A)
    seq = ref.rows["A"][0]
    nd = int(np.count_nonzero(_bits(oe.seq_spmv(B, c.x0)) != _bits(seq)))
    x, r = oe.twin_sweeps(c.A, c.x0, c.r0, 2, stream=B)
    dev = max(oe.max_rel(x, ref.sweeps[2][0]), oe.max_rel(r, ref.sweeps[2][1]))
    print("%s on %s: %d rows of A x differ in bits; two sweeps deviate by %.3e" % (which, name, nd, dev))
    assert nd > 0 or dev > GATE, (which, nd, dev)
    if which.startswith("drop_unroll_tail"):
        un = int(which.split("un")[-1])
        hit = {int(w) for w in oe.slice_widths(c.A) if w % un and un * (w // un) < w}
        assert hit and nd > 0
