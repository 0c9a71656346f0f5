"""Host checks of the references the full-size GPU tests stand on (tests/fullsize_reference.py), of StreamedCSR.plane_rows, and of
the geometry of the ragged full-size problem (tests/test_gpu_fullsize.py).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import fullsize_reference as fr
from fullsize_reference import RAGGED_NC, RAGGED_NLEV


@pytest.mark.parametrize("make", ["matrix_q1", "matrix_q2", "prolongation_q2", "restriction_q1"])
def test_plane_rows_is_the_block_row_blocks_yields(po, make):
    """plane_rows(z) -- random access through the plane generator -- returns the very block row_blocks() yields for plane z (same
    row0, same ptr / idx / val bits), interior planes that the row plan only declares as "repeat" items included."""
    nc = (6, 5, 7)
    M = {"matrix_q1": lambda: po.poisson_matrix_stream(nc, 1, lengths=(1.0, 2.0, 0.5)),
         "matrix_q2": lambda: po.poisson_matrix_stream(nc, 2),
         "prolongation_q2": lambda: po.prolongation_stream(nc, 2),
         "restriction_q1": lambda: po.restriction_stream(nc, 1)}[make]()
    blocks = list(M.row_blocks())
    assert len(blocks) >= 5
    repeated = [it for it in M.row_plan() if it[0] == "repeat"]
    assert repeated, "no repeated plane: the case would not test the expansion"
    for z in list(range(len(blocks)))[::-1]:              # backwards: random access, not the generator's order
        row0, B = M.plane_rows(z)
        r0, Bz = blocks[z]
        assert row0 == r0 and B.shape == Bz.shape
        np.testing.assert_array_equal(B.ptr, Bz.ptr)
        np.testing.assert_array_equal(B.idx, Bz.idx)
        assert np.array_equal(B.val.view(np.int64), Bz.val.view(np.int64))
    with pytest.raises(IndexError):
        M.plane_rows(len(blocks))


def test_ragged_problem_lands_in_the_gate_bands(po):
    """Q1 (240, 232, 200) cells, 4 levels: level 0 >= pat_zwalk_rows (9e6; walk sweeps, above big_rows 4e6: XCD remap), level 1
    between 1e6 rows and pat_tile_rows (3.5e6: the pair sweep in its four-wave form), level 2 between pat_r2mv_min (1e5) and
    pat_coded_min_rows (5e5), the coarsest between GMG_GJ_WIDE_MIN (4096) and coarse_auto_cg_min (20 000): the device 64-wide
    Gauss-Jordan inverse with a ragged last panel (n % 64 = 32) and n not a multiple of 128; 199 node planes = 16 chains of 12 + 7;
    no axis a multiple of 64."""
    cells = [tuple(c >> l for c in RAGGED_NC) for l in range(RAGGED_NLEV)]
    n = [po.level_sizes(c, 1) for c in cells]
    nodes = [c - 1 for c in RAGGED_NC]
    assert n == [10986591, 1354815, 164787, 19488]
    assert n[0] >= 9e6 and 1e6 <= n[1] < 3.5e6 and 1e5 <= n[2] < 5e5 and 4096 <= n[3] < 20000
    assert n[3] % 64 == 32 and n[3] % 128 and n[3] // 64 == 304
    assert divmod(nodes[2], fr.ZWALK_T) == (16, 7) and all(v % 64 for v in nodes) and len(set(nodes)) == 3


def test_edge_rows_cover_the_chain_and_slice_ends():
    nx, ny, nz = 23, 17, 31
    P = nx * ny
    rows = fr.edge_rows(nx, ny, nz, nrand=100)
    assert rows.min() == 0 and rows.max() == P * nz - 1 and np.all(np.diff(rows) > 0)
    s = set(rows.tolist())
    for z in (0, 1, 11, 12, 13, 23, 24, 25, 29, 30):
        assert z * P in s and z * P + P - 1 in s, z
    for b in (63, 64, 65, 127, 128, 129):
        assert b in s and (nz - 1) * P + b in s


def test_row_reference_is_exact_and_the_sequential_sum_is_csr_order():
    rng = np.random.default_rng(5)
    n, k = 40, 9
    cols = rng.integers(0, n, (30, k))
    vals = rng.uniform(-1, 1, (30, k)) * 10.0 ** rng.integers(-8, 8, (30, k))
    ln = rng.integers(1, k + 1, 30)
    x = rng.uniform(-1, 1, n)
    seq, exact, bound = fr.row_reference(cols, vals, ln, x)
    for i in range(30):
        s = 0.0
        for j in range(ln[i]):
            s = s + vals[i, j] * x[cols[i, j]]
        assert s == seq[i]
        ex = sum(Fraction(vals[i, j]) * Fraction(x[cols[i, j]]) for j in range(ln[i]))
        assert exact[i] == float(ex)
        assert abs(Fraction(seq[i]) - ex) <= Fraction(bound[i])


def test_dot_reference_is_exact_under_cancellation():
    rng = np.random.default_rng(6)
    a = rng.uniform(-1, 1, 1001)
    b = -a + 1e-12 * rng.uniform(-1, 1, a.size)
    ex = sum(Fraction(u) * Fraction(v) for u, v in zip(a.tolist(), b.tolist()))
    assert fr.dot_exact(a, b, chunk=64) == float(ex)
    assert fr.dot_depth(1) == 1 + 1 + 17 and fr.dot_depth(288 ** 3) > np.log2(288 ** 3) + 60


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097, (1 << 20) + 3, 131074, 524289])
def test_dot_depth_of_the_unaligned_path_bounds_its_emulated_chain(n):
    """dot_partial_kernel's one-element path (an operand not 16-byte aligned) + reduce_final_kernel, emulated operation by
    operation (fr.dot_emulate_scalar_path) at the edge lengths of tests/test_gpu_fullsize.py, 131074 and 524289: no product
    passes through more roundings than dot_depth(n, vec=False), the emulated value is within that bound of the exact dot on
    random data and under heavy cancellation, and the 16-byte path's depth is a different number where the orders differ."""
    rng = np.random.default_rng(3000 + n)
    a = rng.uniform(-1, 1, n)
    for b in (rng.uniform(-1, 1, n), -a + 1e-12 * rng.uniform(-1, 1, n)):
        v, chain = fr.dot_emulate_scalar_path(a, b)
        assert 1 <= chain <= fr.dot_depth(n, vec=False)
        ex, bound = fr.dot_reference(a, b, vec=False)
        assert abs(v - ex) <= bound
        assert abs(v - ex) <= float(fr.gamma(chain) * np.sum(np.abs(a * b)))
    nb = max(1, min(fr.RED_BLOCKS, (n // 2 + fr.K_BLOCK - 1) // fr.K_BLOCK))
    assert fr.dot_depth(n, vec=False) == 1 + -(-n // (nb * fr.K_BLOCK)) + 8 + -(-nb // fr.K_BLOCK) + 8
    assert fr.dot_depth(n) == fr.dot_depth(n, vec=True)
    if n <= 2 * fr.K_BLOCK:                               # one workgroup: the whole vector is one term per lane (two at n > 256)
        assert fr.dot_depth(n, vec=False) == 1 + (1 if n <= fr.K_BLOCK else 2) + 17


def test_patch_precond_reference_is_the_oracles_patch_operator(po, orc):
    """patch_precond_reference (blocks from plane_rows, numpy LU) against the oracle's additive vertex-star patch operator on a
    small streamed Q2 level: the reference the sampled config-3 check stands on."""
    nc = (6, 4, 8)
    M = po.poisson_matrix_stream(nc, 2)
    A = M.materialize()
    pp, pd = po.vertex_star_patches(nc, 2)
    go = orc.GMG([A, po.poisson_matrix(tuple(c // 2 for c in nc), 2)], [po.prolongation(tuple(c // 2 for c in nc), 2)],
                 pre_smoothers=[orc.Smoother(orc.PATCH, 10, 0.2, pp, pd)], maxiter=1)
    r = np.random.default_rng(9).uniform(-1, 1, A.shape[0])
    sample = np.random.default_rng(10).integers(0, A.shape[0], 60)
    dofs, ref = fr.patch_precond_reference(M, pp, pd, sample, r)
    assert fr.max_rel(ref, go.precond(0, r)[dofs]) <= 1e-13
