"""Host checks of tests/coarse_inverse_problems.py (no GPU): the families are what tests/test_gpu_coarse_inverse.py takes them for, the
float64 twin of the device inversion and numpy's pivoted solve sit a factor ten inside the per-kernel gate on them -- the condition
that keeps that gate honest: a family that misses it is regenerated, never given a looser gate -- and every restated wrong kernel
misses the gate by three orders of magnitude on the nonsymmetric families, while the transposed inverse PASSES it on the symmetric
Poisson coarse matrix that used to be the only kind of input of the device inversion in a test."""
import numpy as np
import pytest

import coarse_inverse_problems as ci
import fullsize_reference as fr

GATE = fr.TOL_KERNEL                 # 1e-13: max |x - x_ref| / max |x_ref|
WIDTHS = {32: ci.SIZES_32, 64: ci.SIZES_64}


def _device_cases():
    """(family, panel width) as the device tests run them"""
    out = [("banded-%d" % n, w) for w in (32, 64) for n in WIDTHS[w]]
    out += [(name, 32) for name in ci.DENSE] + [("dense-129", 64), ("duplicates-129", 32)]
    return out


# ---------------------------------------------------------------- what the families are
def test_family_lists():
    assert ci.SIZES_32 == (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 511, 512, 513, 1025)
    assert ci.SIZES_64 == (1, 63, 64, 65, 127, 128, 129, 192, 193, 1023, 1024, 1025, 1089)
    assert ci.SIZES_GEMV == (511, 512, 513, 1023, 1024, 1025)
    assert ci.SIZES_DENSE == (33, 65, 129) and ci.SIZES_BANDLU == (1, 2, 33, 257, 1500) and ci.PIVOT_SIZES == (97, 1600)
    assert max(ci.PIVOT_SIZES) > ci.HOST_MAX_DEFAULT >= max(ci.SIZES_BANDLU)
    assert len(set(ci.FAMILIES)) == len(ci.FAMILIES)
    # past 1024 the 64-wide path has a ninth column tile of 128, a second super-tile row and a ragged last panel of 1 and of 1 + 64 columns
    assert [(n + 127) // 128 for n in (1025, 1089)] == [9, 9] and [(n + 1023) // 1024 for n in (1025, 1089)] == [2, 2]
    assert [n % 64 for n in (1025, 1089)] == [1, 1] and 1089 - 1024 == 1 + 64


@pytest.mark.parametrize("name", ci.BANDED + ci.DENSE)
def test_banded_and_dense_families(name):
    c = ci.case(name)
    n = c.n
    assert n == int(name.split("-")[1]) and c.D.shape == (n, n) and c.r.shape == (n,) and np.all(np.abs(c.r) < 1.0)
    off = c.D - np.diag(np.diag(c.D))
    assert np.all(np.abs(np.diag(c.D)) > np.abs(off).sum(axis=1))                 # row-dominant: no pivoting needed
    v = c.Ac.data[c.Ac.indices != np.repeat(np.arange(n), np.diff(c.Ac.indptr))]
    assert np.unique(v).size == v.size and (v.size == 0 or (np.abs(v).min() >= 1e-3 and np.abs(v).max() <= 1e3))
    if name.startswith("dense"):
        assert c.Ac.nnz == n * n and np.all(c.D != 0.0)
    else:
        kl, ku = ci.bandwidths(c.Ac)
        assert (kl, ku) == (min(ci.KL, n - 1), min(ci.KU, n - 1))
        band = sum(min(n, i + ci.KU + 1) - max(0, i - ci.KL) for i in range(n))
        assert n < 31 or 0.6 <= c.Ac.nnz / band <= 0.8
    if n >= 31:                                                                   # nonsymmetric in pattern and in value
        assert name.startswith("dense") or np.count_nonzero((c.D != 0.0) != (c.D.T != 0.0)) > n // 2
        assert np.max(np.abs(c.D - c.D.T)) > 0.5 * np.max(np.abs(off))
        Ainv = np.linalg.inv(c.D)
        assert ci.max_rel(Ainv.T, Ainv) > 0.1


def test_duplicates_family_is_banded_129_exactly():
    d, b = ci.case("duplicates-129"), ci.case("banded-129")
    assert d.Ac.nnz > b.Ac.nnz + b.Ac.nnz // 6
    same = (d.Ac.indices[1:] == d.Ac.indices[:-1]) & (np.diff(np.repeat(np.arange(d.n), np.diff(d.Ac.indptr))) == 0)
    assert np.count_nonzero(same) == d.Ac.nnz - b.Ac.nnz                          # stored as two entries of one column, side by side
    assert np.array_equal(d.D, b.D) and np.array_equal(d.r, b.r)                                           # += in storage order gives the value back exactly


@pytest.mark.parametrize("name", ci.ZERO_PIVOT)
def test_zero_pivots_sit_where_the_device_tests_expect_them(name):
    c = ci.case(name)
    n = c.n
    k = 0 if name.endswith("first") else ci.PIVOT_LAST[n]
    assert c.D[k, k] == 0.0 and not np.any(c.D[k, :k + 1]) and k % 32 == 0        # first row of a panel, nothing at or left of the diagonal
    base = ci.case("banded-%d" % n).D
    order = np.arange(n)
    order[[k, k + ci.PIVOT_SHIFT]] = k + ci.PIVOT_SHIFT, k
    assert np.array_equal(c.D, base[order])                                       # two rows exchanged, nothing else
    for width in (32, 64):
        with pytest.raises(ci.ZeroPivot) as e:
            ci.twin_inverse(c.D, width)
        assert e.value.args[0] == k, (name, width)
    if n == 97 and k:
        assert (k, n - k) == (64, 33)                                             # the ragged last panel of the 64-wide path
    assert np.linalg.cond(c.D, np.inf) < 1e5                                      # a well-conditioned matrix that only needs pivoting


def test_tiny_pivot_passes_the_zero_flag_and_fails_the_self_check():
    c = ci.case("pivot-97-tiny")
    assert c.D[0, 0] == ci.TINY and np.array_equal(c.D[1:], ci.case("pivot-97-first").D[1:])
    for width in (32, 64):
        Ainv = ci.twin_inverse(c.D, width)                                        # no ZeroPivot
        q = ci.self_check(c.D, Ainv)
        print("pivot-97-tiny width %d: self-check %.3e" % (width, q))
        assert q > 1e4 * ci.SELF_CHECK
    assert ci.self_check(c.D, np.linalg.inv(c.D)) < 1e-4 * ci.SELF_CHECK


@pytest.mark.parametrize("name", ci.BANDLU)
def test_bandlu_families_need_pivoting_inside_the_band(name):
    c = ci.case(name)
    n, (kl, ku) = c.n, (int(q) for q in name.split("-")[2].split("x"))
    got = ci.bandwidths(c.Ac)
    if n >= 33:
        assert got == (kl, ku)                                                    # kl != ku exactly: ju and the fill-in kv = kl + ku matter
    else:
        assert got[0] <= min(kl, n - 1) and got[1] <= min(ku, n - 1)
    if n >= 2:
        share = ci.offdiagonal_column_maxima(c.Ac)
        assert share >= 1.0 / 3.0 and (n < 33 or share <= 0.7)                    # some columns pivot, some do not
        off = np.abs(c.D - np.diag(np.diag(c.D)))
        assert np.count_nonzero(np.abs(np.diag(c.D)) < off.sum(axis=1)) >= n // 3   # not diagonally dominant
    if n >= 33:
        assert np.count_nonzero((c.D != 0.0) != (c.D.T != 0.0)) > n


def test_singular_family():
    c = ci.case("singular-65")
    assert np.array_equal(c.D[64], c.D[63]) and np.array_equal(c.D[:64], ci.case("banded-65").D[:64])
    assert np.linalg.matrix_rank(c.D) == 64
    assert ci.host_lu_smallest_pivot(c.D) <= 1e-2 < 1e2 <= ci.host_lu_smallest_pivot(ci.case("banded-65").D)   # the host LU's own test
    for name in ci.BANDLU + ci.PIVOT:
        assert ci.host_lu_smallest_pivot(ci.case(name).D) >= 1e2, name
    v = 1.0 + 0.5 * np.sin(0.37 * np.arange(65))                                  # the self-check vector is not in the range of A
    assert abs(v[64] - v[63]) / np.sqrt(2.0) / np.linalg.norm(v) > 1e3 * ci.SELF_CHECK


def test_condition_numbers():
    k = {name: np.linalg.cond(ci.case(name).D, np.inf) for name in ci.BANDED + ci.DENSE + ci.BANDLU if ci.case(name).n > 2}
    print("kappa_inf: %.1e .. %.1e" % (min(k.values()), max(k.values())))
    assert max(k.values()) < 1e5


# ---------------------------------------------------------------- the gate is honest
def test_twin_is_a_factor_ten_inside_the_gate_on_the_device_families():
    worst = {}
    for name, width in _device_cases():
        c = ci.case(name)
        e = ci.max_rel(ci.twin(c.D, c.r, width), ci.reference(name))
        worst[width] = max(worst.get(width, 0.0), e)
        assert e <= GATE / 10, (name, width, e)
    print("twin against the refined reference: " + ", ".join("%d-wide %.2e" % kv for kv in sorted(worst.items())))


def test_twins_of_both_widths_agree():
    for n in sorted(set(ci.SIZES_32) & set(ci.SIZES_64)) + [1089]:
        c = ci.case("banded-%d" % n)
        assert ci.max_rel(ci.twin(c.D, c.r, 64), ci.twin(c.D, c.r, 32)) <= GATE / 10, n


@pytest.mark.parametrize("names", [ci.PIVOT, ci.BANDLU, tuple("banded-%d" % n for n in ci.SIZES_GEMV)], ids=["pivot", "bandlu", "gemv"])
def test_pivoted_float64_solve_is_a_factor_ten_inside_the_gate(names):
    worst = 0.0
    for name in names:
        c = ci.case(name)
        e = ci.max_rel(np.linalg.solve(c.D, c.r), ci.reference(name))
        worst = max(worst, e)
        assert e <= GATE / 10, (name, e)
    print("numpy.linalg.solve against the refined reference: %.2e" % worst)


def test_reference_is_refined_and_scales():
    c = ci.case("banded-129")
    x = ci.reference("banded-129")
    res = c.r.astype(ci.LD) - c.D.astype(ci.LD) @ x.astype(ci.LD)
    assert float(np.max(np.abs(res))) <= 4 * fr.U * float(np.max(np.abs(c.D) @ np.abs(x)))   # the residual of a correctly rounded solution
    assert ci.max_rel(ci.reference("banded-129", 1.7) * 1.7, x) <= 4 * fr.U
    assert not x.flags.writeable
    Ainv = ci.inverse_reference("banded-65")
    assert ci.max_rel(ci.case("banded-65").D @ Ainv, np.eye(65)) <= 1e-13


# ---------------------------------------------------------------- every wrong kernel shows; the old input hides one
@pytest.mark.parametrize("which", sorted(ci.CORRUPTIONS))
def test_corruptions_miss_the_gate_by_three_orders(which):
    applies = ci.CORRUPTIONS[which]
    hit, least = 0, np.inf
    for name, width in _device_cases():
        c = ci.case(name)
        if not applies(c.n, width):
            continue
        e = ci.max_rel(ci.twin(c.D, c.r, width, wrong=which), ci.reference(name))
        hit, least = hit + 1, min(least, e)
        assert e >= 1e3 * GATE, (which, name, width, e)
    print("%s: %d cases, smallest deviation %.2e" % (which, hit, least))
    assert hit >= 8


def test_every_device_case_past_one_panel_meets_a_panel_corruption():
    for name, width in _device_cases():
        n = ci.case(name).n
        assert n <= width or any(ci.CORRUPTIONS[w](n, width) for w in ("swap_rc", "cp_left")), (name, width)


def test_the_transposed_inverse_passes_the_gate_on_the_poisson_coarse_matrix(po):
    """the gap these families close: on the symmetric coarse operator of hierarchy((16,16,16), 2) -- the kind of matrix that was the
    only input of the device inversion in a test -- a kernel that produced the transposed inverse would have passed"""
    A = po.build_hierarchy((16, 16, 16), 2)["mats"][1].to_scipy().toarray()
    assert np.array_equal(A, A.T)
    r = np.random.default_rng(5).uniform(-1.0, 1.0, A.shape[0])
    x = np.asarray(ci._refined(A, r), dtype=np.float64)
    for width in (32, 64):
        assert ci.max_rel(ci.twin(A, r, width), x) <= GATE
        assert ci.max_rel(ci.twin(A, r, width, wrong="transposed"), x) <= GATE
    c = ci.case("banded-129")
    assert ci.max_rel(ci.twin(c.D, c.r, 32, wrong="transposed"), ci.reference("banded-129")) >= 1e3 * GATE
