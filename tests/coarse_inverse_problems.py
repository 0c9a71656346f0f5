"""Matrix families, reference, twin and corruptions of the dense coarse inverse tests (tests/test_coarse_inverse_problems.py on the
host, tests/test_gpu_coarse_inverse.py on the device).  Plain helper, numpy and scipy only: no fixtures, no collection hooks, nothing
read from outside the repository.

Under test: gmg_solver::build_dense_inverse (csrc/gmg_amd.hip) -- the host BandLU, the device Gauss-Jordan with 32-wide panels
(gj_diag_kernel, gj_panels_kernel, gj_update_mfma_kernel / gj_update_kernel) and with 64-wide panels on a padded leading dimension
(gj_diag64_kernel, gj_panel_rows_kernel, gj_panel_cols_kernel, gj_update64_kernel), densify_ld_kernel in front and dense_gemv_kernel
behind (csrc/kernels.hpp).  Every family is the COARSE matrix of a two-level hierarchy whose fine level is a diagonal matrix of the
same size with P = R = I (case()); the coarse solve is reached with coarse_solve().

family            n                                what it is there for
banded-n          SIZES_32 / SIZES_64 / SIZES_GEMV nonsymmetric band, kl = 5, ku = 11, ~70 % of it stored; values of
                                                   operator_edge_problems.square_matrix (distinct, 1e-3 .. 1e3, row-dominant diagonal)
dense-n           33, 65, 129                      fully dense, nonsymmetric, row-dominant: every entry of every tile is live
duplicates-129    129                              banded-129 with every fifth entry stored as two entries of its column whose sum is
                                                   the value EXACTLY: the dense matrix, and so every result, is that of banded-129
pivot-n-first     97, 1600                         banded-n with rows 0 and 6 exchanged: A[0, 0] is an exact zero (first panel)
pivot-n-last      97, 1600                         banded-n with rows k and k + 6 exchanged, k = PIVOT_LAST[n]: the new row k has no entry in
                                                   a column <= k, so A[k, k] is still an exact zero when its panel is inverted.  k = 64 at
                                                   n = 97: first row of the ragged last panel (33 wide) of the 64-wide path, of an inner
                                                   panel of the 32-wide path (whose own last panel is ONE column wide there: its pivot is
                                                   det A / det A[:96, :96], zero only for a singular matrix).  k = 1568 at n = 1600: first row
                                                   of the last 32-wide panel (1600 has no ragged panel at either width)
pivot-97-tiny     97                               pivot-97-first with A[0, 0] = 1e-20 stored: no zero pivot, a useless inverse
bandlu-n-KLxKU    1, 2, 33, 257, 1500              for the host LU: kl = 3, ku = 9 and kl = 9, ku = 3; a row-dominant band with rows 3q and
                                                   3q + 1 exchanged, so the largest entry of two columns in three sits below the diagonal
singular-65       65                               banded-65 with its last row replaced by a copy of the row before

reference(name)   numpy.linalg.solve refined three times in np.longdouble              inverse_reference(name): the same for A^-1
twin(A, r, width) float64 restatement of the unpivoted blocked Gauss-Jordan (kernels.hpp, "Device-side dense inversion"), then Ainv @ r
CORRUPTIONS       variants of the twin that a subtly wrong kernel would compute
"""
import functools
import types

import numpy as np
import operator_edge_problems as oe

LD = np.longdouble
KL, KU, KEEP = 5, 11, 0.7
SIZES_32 = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 511, 512, 513, 1025)
SIZES_64 = (1, 63, 64, 65, 127, 128, 129, 192, 193, 1023, 1024, 1025, 1089)
SIZES_GEMV = (511, 512, 513, 1023, 1024, 1025)
SIZES_DENSE = (33, 65, 129)
SIZES_BANDLU = (1, 2, 33, 257, 1500)
BANDS_BANDLU = ((3, 9), (9, 3))
PIVOT_SIZES = (97, 1600)
PIVOT_LAST = {97: 64, 1600: 1568}
PIVOT_SHIFT = 6                      # rows k and k + 6 are exchanged: row k + 6 of the band starts at column k + 1
TINY = 1.0e-20
HOST_MAX_DEFAULT = 1500              # coarse_host_max (include/gmg_amd.h)
SELF_CHECK = 1.0e-8                  # the device inversion's own gate on ||A (Ainv v) - v|| / ||v||

BANDED = tuple("banded-%d" % n for n in sorted(set(SIZES_32 + SIZES_64 + SIZES_GEMV)))
DENSE = tuple("dense-%d" % n for n in SIZES_DENSE)
ZERO_PIVOT = tuple("pivot-%d-%s" % (n, w) for n in PIVOT_SIZES for w in ("first", "last"))
PIVOT = ZERO_PIVOT + ("pivot-97-tiny",)
BANDLU = tuple("bandlu-%d-%dx%d" % (n, kl, ku) for n in SIZES_BANDLU for kl, ku in BANDS_BANDLU)
DEVICE_FAMILIES = BANDED + DENSE + ("duplicates-129",)
FAMILIES = DEVICE_FAMILIES + PIVOT + BANDLU + ("singular-65",)


class ZeroPivot(Exception):
    """the unpivoted elimination met an exact zero on the diagonal; args[0] = its row"""


def max_rel(a, b):
    """max |a - b| / max |b|; anything not finite counts as infinitely wrong"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        return np.inf
    m = float(np.max(np.abs(b))) if b.size else 0.0
    d = float(np.max(np.abs(a - b))) if b.size else 0.0
    return d / m if m > 0 else d


# ------------------------------------------------------------------------------------------------ structures and matrices
def band_structure(n, kl, ku, keep=KEEP, seed=0):
    """rows of a band: the diagonal always, every other entry of the band with probability `keep`"""
    rng = oe._rng(seed, n, kl, ku, 21)
    rows = []
    for i in range(n):
        c = np.arange(max(0, i - kl), min(n, i + ku + 1))
        rows.append(c[(rng.random(c.size) < keep) | (c == i)])
    return rows


def _take_rows(A, order):
    """raw CSR whose row i is row order[i] of A"""
    ptr = np.concatenate([[0], np.cumsum(np.diff(A.indptr)[order])])
    take = np.concatenate([np.arange(A.indptr[i], A.indptr[i + 1]) for i in order] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return oe._csr(A.data[take], A.indices[take], ptr, A.shape)


def _exchange_rows(A, pairs):
    order = np.arange(A.shape[0])
    for i, j in pairs:
        order[i], order[j] = order[j], order[i]
    return _take_rows(A, order)


def _bandlu_matrix(n, kl, ku):
    """band (kl - 1, ku - 1), off-diagonal +-U(0.25, 1), diagonal = +-(1.2 x the row's absolute sum + 1) -- the largest entry of its
    row AND of its column -- with rows 3q and 3q + 1 exchanged: band (kl, ku) exactly (n >= 3 + kl + ku), two columns in three have
    their largest entry one below the diagonal (n = 2: the one pair)"""
    rng = oe._rng(n, kl, ku, 22)
    rows = band_structure(n, kl - 1, ku - 1, keep=0.85, seed=3)
    indptr, indices = oe._from_rows(rows, n)
    rowof = np.repeat(np.arange(n), np.diff(indptr))
    data = rng.choice([-1.0, 1.0], indices.size) * rng.uniform(0.25, 1.0, indices.size)
    isdiag = indices == rowof
    data[isdiag] = rng.choice([-1.0, 1.0], n) * (1.2 * np.bincount(rowof[~isdiag], weights=np.abs(data[~isdiag]), minlength=n) + 1.0)
    return _exchange_rows(oe._csr(data, indices, indptr, (n, n)), [(i, i + 1) for i in range(0, n - 1, 3)])


def _split_entries(A, every=5):
    """every `every`-th stored entry v becomes two entries of the same column, 0.75 v (rounded) and the rest: the rest is exact
    (Sterbenz) and the two add up to v exactly, in either order"""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    split = np.arange(A.nnz) % every == 2
    first = np.where(split, 0.75 * A.data, A.data)
    second = A.data - first
    assert np.array_equal((first + second)[split], A.data[split]) and np.all(second[split] != 0.0)
    reps = np.where(split, 2, 1)
    idx, rws = np.repeat(A.indices, reps), np.repeat(rows, reps)
    val = np.repeat(first, reps)
    val[np.cumsum(reps)[split] - 1] = second[split]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rws, minlength=A.shape[0]))])
    return oe._csr(val, idx, ptr, A.shape)


def _with_entry(A, i, j, v):
    """raw CSR of A with one more stored entry (i, j) = v in front of row i (the entry must not be stored yet)"""
    assert j not in A.indices[A.indptr[i]:A.indptr[i + 1]]
    at = A.indptr[i]
    ptr = A.indptr.copy()
    ptr[i + 1:] += 1
    return oe._csr(np.insert(A.data, at, v), np.insert(A.indices, at, j), ptr, A.shape)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> scipy CSR, raw (the entries of a row stay as generated: duplicates are never summed)"""
    part = name.split("-")
    fam, n = part[0], int(part[1])
    if fam == "banded":
        return oe.square_matrix(band_structure(n, KL, KU))
    if fam == "dense":
        return oe.square_matrix([np.arange(n) for _ in range(n)], seed=1)
    if fam == "duplicates":
        return _split_entries(matrix("banded-%d" % n))
    if fam == "pivot":
        k = 0 if part[2] in ("first", "tiny") else PIVOT_LAST[n]
        A = _exchange_rows(matrix("banded-%d" % n), [(k, k + PIVOT_SHIFT)])
        return _with_entry(A, 0, 0, TINY) if part[2] == "tiny" else A
    if fam == "bandlu":
        kl, ku = (int(q) for q in part[2].split("x"))
        return _bandlu_matrix(n, kl, ku)
    if fam == "singular":
        return _take_rows(matrix("banded-%d" % n), np.append(np.arange(n - 1), n - 2))
    raise ValueError(name)


def dense(A):
    """the dense matrix as densify_ld_kernel and BandLU::factor build it: += in storage order"""
    D = np.zeros(A.shape)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    for k in range(A.nnz):                                    # (np.add.at sums in order too; the loop says so)
        D[rows[k], A.indices[k]] += A.data[k]
    return D


def bandwidths(A):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return int(np.max(rows - A.indices, initial=0)), int(np.max(A.indices - rows, initial=0))


def offdiagonal_column_maxima(A):
    """share of the columns whose largest entry (in modulus) is not on the diagonal"""
    D = np.abs(dense(A))
    return float(np.mean(np.argmax(D, axis=0) != np.arange(A.shape[0])))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, n, Ac, D, A, P, R, r): the family's matrix Ac (raw CSR; D = dense(Ac)) as the coarse level under a
    diagonal fine level A with P = R = I, and a seeded right-hand side r in (-1, 1)"""
    Ac = matrix(name)
    n = Ac.shape[0]
    fine = oe._csr(np.full(n, 2.0), np.arange(n), np.arange(n + 1), (n, n))
    eye = oe._csr(np.ones(n), np.arange(n), np.arange(n + 1), (n, n))
    key = name.replace("duplicates", "banded")               # (duplicates-n: banded-n's r)
    r = oe._rng(FAMILIES.index(key) if key in FAMILIES else len(FAMILIES), n, 23).uniform(-1.0, 1.0, n)
    c = types.SimpleNamespace(name=name, n=n, Ac=Ac, D=dense(Ac), A=fine, P=eye, R=eye.copy(), r=r)
    if name.startswith("bandlu") and n >= 2:
        assert offdiagonal_column_maxima(Ac) >= 1.0 / 3.0, name
    return c


# ------------------------------------------------------------------------------------------------ reference
def _refined(D, B):
    X = np.linalg.solve(D, B).astype(LD)
    Dl, Bl = D.astype(LD), np.asarray(B, dtype=LD)
    for _ in range(3):
        X = X + np.linalg.solve(D, (Bl - Dl @ X).astype(np.float64)).astype(LD)
    return X


@functools.lru_cache(maxsize=None)
def reference(name, scale=1.0):
    """x = (scale * A)^-1 r: numpy.linalg.solve refined three times in np.longdouble, rounded to float64 once; read-only"""
    c = case(name)
    x = _refined(c.D * scale, c.r).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def inverse_reference(name):
    X = _refined(case(name).D, np.eye(case(name).n)).astype(np.float64)
    X.setflags(write=False)
    return X


# ------------------------------------------------------------------------------------------------ twin
def _gj_block(M):
    """gj_diag_kernel / gj_diag64_kernel: Gauss-Jordan without pivoting on one diagonal block -> its inverse; ZeroPivot(local row)"""
    M = M.copy()
    X = np.eye(M.shape[0])
    for j in range(M.shape[0]):
        d = M[j, j]
        if d == 0.0:
            raise ZeroPivot(j)
        mj, xj, f = M[j] / d, X[j] / d, M[:, j].copy()
        M -= np.outer(f, mj)
        X -= np.outer(f, xj)
        M[j], X[j] = mj, xj
    return X


def _wrapped_block(W, k0, width):
    """the width x width block at (k0, k0) of the row-major n x n array as a kernel that ignores b = n - k0 reads it: columns past
    the row's end are the start of the next row, zeros past the end of the array"""
    n = W.shape[0]
    flat = np.concatenate([W.ravel(), np.zeros(width * (n + 1))])
    return np.array([[flat[(k0 + r) * n + k0 + c] for c in range(width)] for r in range(width)])


def twin_inverse(D, width, wrong=None):
    """float64 restatement of the unpivoted blocked Gauss-Jordan: for panel K = [k0, k0 + b)
         Pinv = A[K,K]^-1 ; R = Pinv A[K,:] ; C = A[:,K] ; A[i,j] -= C[i,:] R[:,j] (i, j not in K) ; A[K,notK] = R ;
         A[notK,K] = -C Pinv ; A[K,K] = Pinv
    wrong: None, or one of the panel-level slips of CORRUPTIONS.  ZeroPivot(global row) on an exact zero pivot."""
    W = np.array(D, dtype=np.float64)
    n = W.shape[0]
    for k0 in range(0, n, width):
        b = min(width, n - k0)
        K = slice(k0, k0 + b)
        try:
            if wrong == "ragged_as_full" and b < width:
                Pinv = _gj_block(_wrapped_block(W, k0, width))[:b, :b]
            else:
                Pinv = _gj_block(W[K, K])
        except ZeroPivot as e:
            raise ZeroPivot(k0 + e.args[0]) from None
        R = Pinv @ W[K, :]
        C = W[:, K].copy()
        Cp = -(C @ Pinv.T) if wrong == "cp_left" else -(C @ Pinv)
        U = (R.T @ C.T) if wrong == "swap_rc" else C @ R
        if wrong == "skip_last_row_tile":
            U[64 * ((n - 1) // 64):, :] = 0.0
        W -= U
        W[K, :] = R
        W[:, K] = Cp
        W[K, K] = Pinv
    return W


def twin(D, r, width, wrong=None):
    """the twin's coarse solve: the blocked inversion, then dense_gemv_kernel's x = Ainv r"""
    with np.errstate(all="ignore"):
        try:
            Ainv = twin_inverse(D, width, None if wrong in ("transposed", "gemv_no_tail") else wrong)
        except ZeroPivot:
            if wrong is None:
                raise
            return np.full(D.shape[0], np.nan)                # the wrong kernel's setup would be refused: as wrong as can be
        if wrong == "transposed":
            Ainv = Ainv.T
        if wrong == "gemv_no_tail":
            m = 512 * (D.shape[0] // 512)
            return Ainv[:, :m] @ r[:m]
        return Ainv @ r


def self_check(D, Ainv):
    """the device inversion's own check: ||A (Ainv v) - v|| / ||v|| for v_i = 1 + sin(0.37 i) / 2 (to be < SELF_CHECK)"""
    v = 1.0 + 0.5 * np.sin(0.37 * np.arange(D.shape[0]))
    with np.errstate(all="ignore"):
        e = D @ (Ainv @ v) - v
        q = float(np.sqrt(np.sum(e * e) / np.sum(v * v)))
    return q if np.isfinite(q) else np.inf


def host_lu_smallest_pivot(D):
    """BandLU::factor's singularity test restated on the dense matrix: Gaussian elimination with partial pivoting (first largest entry
    of the column) -> the smallest |pivot| / (n eps max|column of A|); the host refuses the matrix when that is <= 1"""
    U = np.array(D, dtype=np.float64)
    n = U.shape[0]
    cmax = np.max(np.abs(U), axis=0)
    least = np.inf
    for j in range(n):
        p = j + int(np.argmax(np.abs(U[j:, j])))
        if cmax[j] > 0.0:
            least = min(least, abs(U[p, j]) / (n * np.finfo(np.float64).eps * cmax[j]))
        if U[p, j] == 0.0:
            return 0.0
        U[[j, p]] = U[[p, j]]
        rows, cols = j + 1 + np.flatnonzero(U[j + 1:, j]), j + 1 + np.flatnonzero(U[j, j + 1:])   # (inside the band only)
        U[rows, j] /= U[j, j]
        U[np.ix_(rows, cols)] -= np.outer(U[rows, j], U[j, cols])
    return least


# name -> applies(n, width): the sizes and panel widths at which the slip changes what is computed
CORRUPTIONS = {
    "transposed": lambda n, w: n >= 31,                                  # an operand / accumulator layout that yields the transposed tile
    "swap_rc": lambda n, w: n > w,                                       # R and C exchanged in the trailing update
    "cp_left": lambda n, w: n > w,                                       # Cp = -Pinv C
    "ragged_as_full": lambda n, w: n > w and n % w != 0,                 # the ragged last panel inverted as a full one
    "skip_last_row_tile": lambda n, w: n > 64,                           # the last 64-row tile of the trailing update never runs
    "gemv_no_tail": lambda n, w: n % 512 != 0,                           # columns past the last multiple of 512 dropped by the GEMV
}
