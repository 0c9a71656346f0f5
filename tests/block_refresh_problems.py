"""Inputs of the block numerical_setup! tests (tests/test_block_refresh_host.py on the host, tests/test_gpu_block_refresh.py on the
device).  Plain helper, numpy and scipy only: no fixtures, no collection hooks, nothing read from outside the repository.

Every builder returns SEQUENCES of block matrices with identical ptr / idx and different values (same_pattern asserts it):

stokes_like(po, nc, nlev, nsteps, explicit)   [[A, Bt], [B, Mp]] in the shape of tests/test_gpu_block.py::_stokes_like: A from
                                              po.build_hierarchy(nc, nlev, 1, kappa=KAPPAS[k]) (variable coefficients: explicit
                                              values on the device), B = cb_k R with a seeded relative perturbation (explicit) or
                                              without one (constant-coefficient values: a dictionary / row-pattern layout), Mp fixed
reference_pair(po)                            the reference's block test problem [[M, -M], [M, M]] at (8, 8) and M -> M'
edge_systems()                                one- and two-block systems from tests/operator_edge_problems.py: row counts 1, 63, 64,
                                              65, 4283, SELL slices of every width, a last slice of 29 rows, a 3000-entry row, empty
                                              rows, rectangular blocks with fewer than 64 rows and with ncols < nrows
"""
import numpy as np
import scipy.sparse as sp

import operator_edge_problems as oe


def kappa2(X, Y, Z):
    return 2.0 + np.cos(3.0 * X) * np.sin(2.0 * Y + 0.2) + 0.5 * Z * Z


def kappa3(X, Y, Z):
    return 1.5 + 0.75 * np.sin(2.0 * X + 0.4) * np.cos(1.3 * Z) + 0.3 * Y


def kappa4(X, Y, Z):
    return 3.0 - np.cos(2.5 * Y + 0.1) * np.sin(1.1 * X + 0.9) + 0.2 * X * Z


def kappas(po):
    """four smooth, strictly positive coefficient fields: the first set-up and three refreshes"""
    return (po.smooth_kappa, kappa2, kappa3, kappa4)


def csr(po, M):
    """scipy -> po.CSR with the entries in the order given"""
    M = sp.csr_matrix(M)
    return po.CSR(M.shape, M.indptr.astype(np.int64), M.indices.astype(np.int32), np.array(M.data, dtype=np.float64))


def perturbed(po, M, seed, rel=0.3, scale=1.0):
    """same pattern, val * scale * (1 + rel * u), u uniform in (-1, 1), seeded: no two entries stay equal"""
    u = np.random.default_rng([seed, M.val.size]).uniform(-1.0, 1.0, M.val.size)
    return po.CSR(M.shape, M.ptr, M.idx, M.val * scale * (1.0 + rel * u))


def scaled(po, M, c):
    return po.CSR(M.shape, M.ptr, M.idx, M.val * c)


def same_pattern(a, b):
    """identical ptr / idx, different values"""
    if (a is None) != (b is None):
        return False
    if a is None:
        return True
    return a.shape == b.shape and np.array_equal(a.ptr, b.ptr) and np.array_equal(a.idx, b.idx) and not np.array_equal(a.val, b.val)


def assert_same_patterns(mats_a, mats_b, fixed=()):
    for i, (ra, rb) in enumerate(zip(mats_a, mats_b)):
        for j, (a, b) in enumerate(zip(ra, rb)):
            if (i, j) in fixed:
                assert a is b
            else:
                assert same_pattern(a, b), (i, j)


def stokes_like(po, nc, nlev, nsteps=2, explicit=True):
    """-> list of nsteps dicts(H, mat=[[A, Bt], [B, Mp]], Mp, n1, n2); Mp (the MatrixBlock of the preconditioner) is one object"""
    Hs = [po.build_hierarchy(nc, nlev, 1, kappa=k) for k in kappas(po)[:nsteps]]
    R = Hs[0]["restrictions"][0]
    Rt = csr(po, R.to_scipy().T.tocsr())
    n1, n2 = Hs[0]["mats"][0].shape[0], R.shape[0]
    alpha = 10.0
    # (a 1e-3 relative perturbation: no value twice, so that this block too is stored with explicit values at every size)
    Mp = perturbed(po, csr(po, (-1.0 / alpha) * (sp.identity(n2) + 0.1 * Hs[0]["mats"][1].to_scipy())), 31, rel=1e-3)
    out = []
    for k, H in enumerate(Hs):
        cb = 0.05 * (1.0 + 0.5 * k)
        B = perturbed(po, R, 11 + k, scale=cb) if explicit else scaled(po, R, cb)
        Bt = perturbed(po, Rt, 21 + k, scale=cb) if explicit else scaled(po, Rt, cb)
        out.append(dict(H=H, mat=[[H["mats"][0], Bt], [B, Mp]], Mp=Mp, n1=n1, n2=n2, n=n1 + n2))
    for a, b in zip(out[:-1], out[1:]):
        assert_same_patterns(a["mat"], b["mat"], fixed=((1, 1),))
        assert all(same_pattern(x, y) for x, y in zip(a["H"]["mats"], b["H"]["mats"]))
    return out


def reference_pair(po):
    """BlockTriangularSolversTests.jl:22-45: M = Q1 Laplacian at (8, 8); M' = the variable-coefficient operator on the same mesh
    (same pattern, diag(M') / diag(M) between 1.15 and 3.3: a preconditioner that keeps the old diagonal blocks is far from the new one)"""
    M = po.poisson_matrix((8, 8), 1)
    M2 = po.build_hierarchy((8, 8), 2, 1, kappa=kappa2)["mats"][0]
    assert same_pattern(M, M2)
    return M, M2


def block_system(po, M, diagonal=False):
    negM = scaled(po, M, -1.0)
    return [[M, None], [None, M]] if diagonal else [[M, negM], [M, M]]


def _square(rows, seed):
    """value set `seed` on the pattern `rows`; the factor also changes the diagonal-only rows (1.0 in every seed)"""
    return oe.square_matrix(rows, "distinct", seed) * (1.0 + 0.25 * seed)


def edge_systems(po):
    """name -> (mats_a, mats_b, mats_c): three value sets on one pattern.  One-block systems [[A]] and 2 x 2 systems
    [[A, P], [R, C]] with rectangular P (tall, empty rows, ncols < nrows) and R (wide)."""
    out = {}

    for n in (1, 63, 64, 65, 4283):                           # CSR-stream (ragged rows pad too much for SELL)
        rows = oe.ragged_structure(n)
        out["ragged-%d" % n] = [[[csr(po, _square(rows, s))]] for s in (0, 1, 2)]
    rows = oe.widths_structure()                              # SELL-64: one slice per width 1 .. 66
    out["widths"] = [[[csr(po, _square(rows, s))]] for s in (0, 1, 2)]
    rows = oe.offsets_structure()                             # 1501 rows: 23 full slices and one of 29 rows
    out["offsets"] = [[[csr(po, _square(rows, s))]] for s in (0, 1, 2)]
    rows = oe.long_structure()                                # rows of 2047, 2048, 2049 and 3000 entries
    out["long"] = [[[csr(po, _square(rows, s))]] for s in (0, 1, 2)]
    # rectangular off-diagonal blocks: R with fewer than 64 rows, P with ncols < nrows and empty rows
    n, nH = 257, 63
    ra, rc, rp, rr = oe.ragged_structure(n), oe.ragged_structure(nH), oe.tall_ragged(n, nH), oe.wide_ragged(nH, n)
    assert any(len(r) == 0 for r in rp) and any(len(r) == 0 for r in rr)
    out["rect-257x63"] = [[[csr(po, _square(ra, s)), csr(po, oe.rect_matrix(rp, nH, "distinct", s))],
                           [csr(po, oe.rect_matrix(rr, n, "distinct", s)), csr(po, _square(rc, s))]] for s in (0, 1, 2)]
    # R = P^T of an aggregation: one row of 3000 entries in a 97-row block
    n, nH = oe.LONG_N, oe.NH
    rp = oe.aggregation(n, nH)
    P0 = oe.rect_matrix(rp, nH, "distinct", 0)
    rr = [np.sort(P0.tocsc().indices[P0.tocsc().indptr[c]:P0.tocsc().indptr[c + 1]]) for c in range(nH)]
    assert max(len(r) for r in rr) == 3000
    ra, rc = oe.ragged_structure(n), oe.ragged_structure(nH)
    out["aggregation"] = [[[csr(po, _square(ra, s)), csr(po, oe.rect_matrix(rp, nH, "distinct", s))],
                           [csr(po, oe.rect_matrix(rr, n, "distinct", s)), csr(po, _square(rc, s))]] for s in (0, 1, 2)]
    for name, seq in out.items():
        for a, b in zip(seq[:-1], seq[1:]):
            assert_same_patterns(a, b)
    return out


EDGE_NAMES = ("ragged-1", "ragged-63", "ragged-64", "ragged-65", "ragged-4283", "widths", "offsets", "long", "rect-257x63", "aggregation")
_EDGE = {}


def edge_system(po, name):
    if not _EDGE:
        _EDGE.update(edge_systems(po))
    return _EDGE[name]
