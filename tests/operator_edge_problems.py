"""Inputs and references of the general sparse operator edge tests (tests/test_operator_edge_problems.py on the host,
tests/test_gpu_operator_edges.py on the device).  Plain helper, numpy and scipy only: no fixtures, no collection hooks, nothing
read from outside the repository.

The kernels under test carry every operator that is not a constant-coefficient stencil (csrc/kernels.hpp): csr_stream1_kernel,
sell_kernel, sellc_kernel, sello_kernel, fed by upload_csr / build_sell / sell_build_kernel (csrc/gmg_amd.hip).

ragged / widths / long_rows / offsets   square level matrices (full diagonal = 1.5 x the row's absolute sum + 1, off-diagonal
                                        magnitudes 1e-3 .. 1e3), with `distinct`, `few` (exactly 256 doubles) or `few+1` values
tall_ragged / wide_ragged / aggregation / widths_tall / base_offsets_* / mixed_span_*     rectangular P and R
case(name)                              everything one device case needs: A, P, R, A_c (a given SPD matrix), x0, r0, xc (cached)
row_reference_all                       fullsize_reference.row_reference over ALL rows (CSR-order sum, exact value, gamma_k bound)
ref_sweeps / twin_sweeps                k Richardson-Jacobi sweeps in np.longdouble / in float64 with the kernels' roundings
CORRUPTIONS                             wrong kernels, restated on the host: each must show on the family built for it
expected_layout(M, options)             the rules of build_sell restated; csr_blocks(M, lg): the workgroup partition of upload_csr
CONFIGS / INTENDED                      the option sets of the device tests and the layout each family is meant to reach with them
"""
import functools
import types

import numpy as np
import scipy.sparse as sp

import fullsize_reference as fr

LD = np.longdouble
OMEGA = 2.0 / 3.0
SWEEPS = (1, 2, 3, 4, 5)
NH = 97
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 257, 4283)
WIDTHS = tuple(range(1, 11)) + (26, 27, 28, 31, 32, 33, 63, 64, 65, 66)
WIDTHS_SQUARE = WIDTHS + (12,)                           # one more slice: the level has as many rows as the 21-slice P below
WIDTHS_TALL = (0,) + WIDTHS
SELL_UNROLLS = (2, 3, 4, 6, 9, 27)
TILE = 2048                                              # kTile of csrc/kernels.hpp
LONG_N = 4283
LONG_ROWS = {100: 2047, 700: 2048, 1500: 2049, 2900: 3000}   # row -> stored entries (diagonal included)
LONG_RUN = (1501, 128, 16)                               # first row, rows, entries per row: 128 * 16 = 2048 = one tile exactly
OFFSETS = (-37, -5, -1, 0, 1, 2, 40)
OFFSETS_N = 1501
WIDE_N, WIDE_NH = 70001, 129
NEW_VALUE = 0.7310585786300049                           # the 257th value of the `few+1` matrices


def coarse_size(n):
    """97 coarse dofs, fewer under small levels (the coarse level never has more dofs than the fine one)"""
    return min(NH, (n + 1) // 2)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _csr(data, indices, indptr, shape):
    """raw CSR: the entries stay in the order given (the kernels sum in storage order)"""
    return sp.csr_matrix((np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32), np.asarray(indptr, dtype=np.int64)),
                         shape=shape)


def _from_rows(rows, ncols):
    """rows: list of sorted column arrays -> (indptr, indices)"""
    ln = np.array([len(c) for c in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    indices = np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    assert indices.size == 0 or (indices.min() >= 0 and indices.max() < ncols)
    return indptr, indices


def _pick(rng, n, k, exclude=None):
    """k distinct sorted columns of range(n), never `exclude`"""
    if exclude is None:
        return np.sort(rng.choice(n, size=min(k, n), replace=False))
    k = min(k, n - 1)
    c = rng.choice(n - 1, size=k, replace=False) if k else np.zeros(0, dtype=np.int64)
    c = c + (c >= exclude)
    return np.sort(np.append(c, exclude))


# ------------------------------------------------------------------------------------------------ structures
def ragged_structure(n, seed=0):
    """off-diagonal row lengths uniform in 0..40 (as far as n allows), about one row in nine diagonal-only"""
    rng = _rng(seed, n, 1)
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 41))
        if rng.integers(0, 9) == 0 or (n >= 9 and i == n // 2):
            k = 0
        rows.append(_pick(rng, n, k, exclude=i))
    return rows


def widths_lengths(widths, seed=0, least=0):
    """row lengths of one slice of 64 rows per width w: lane a has w entries, lane b w - 1, the others `least`..w at random"""
    rng = _rng(seed, len(widths), 2)
    out = []
    for w in widths:
        ln = rng.integers(min(least, w), w + 1, 64)
        a, b = rng.choice(64, 2, replace=False)
        ln[a] = w
        ln[b] = max(w - 1, min(least, w))
        out.append(ln)
    return np.concatenate(out)


def widths_structure(seed=0):
    ln = widths_lengths(WIDTHS_SQUARE, seed, least=1)
    n = ln.size
    rng = _rng(seed, n, 3)
    return [_pick(rng, n, int(ln[i]) - 1, exclude=i) for i in range(n)]


def long_structure(seed=0):
    n = LONG_N
    rng = _rng(seed, n, 4)
    r0, nr, per = LONG_RUN
    rows = []
    for i in range(n):
        if i in LONG_ROWS:
            k = LONG_ROWS[i] - 1
        elif r0 <= i < r0 + nr:
            k = per - 1
        else:
            k = int(rng.integers(0, 13))
        rows.append(_pick(rng, n, k, exclude=i))
    return rows


def offsets_structure(n=OFFSETS_N):
    i = np.arange(n)
    return [np.array([i0 + d for d in OFFSETS if 0 <= i0 + d < n], dtype=np.int64) for i0 in i]


# ------------------------------------------------------------------------------------------------ values
def _magnitudes(rng, m):
    return rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-3.0, 3.0, m)


def square_matrix(rows, values="distinct", seed=0):
    """-> scipy CSR.  distinct: every off-diagonal value different, diag = 1.5 * sum|off-diagonal| + 1 (so the diagonal-only rows
    share the value 1.0 and nothing else repeats).  few: 200 off-diagonal values and 56 diagonal values, each used at least once --
    256 distinct doubles exactly; a diagonal is the smallest of the 56 levels that is >= 1.5 * sum|off-diagonal| + 1 (the levels are
    the largest requirement of each of 56 groups of requirements), so the matrix stays strictly diagonally dominant.
    few+1: the `few` matrix with one off-diagonal entry replaced by a 257th value of smaller modulus."""
    n = len(rows)
    rng = _rng(seed, n, 5)
    indptr, indices = _from_rows(rows, n)
    rowof = np.repeat(np.arange(n), np.diff(indptr))
    isdiag = indices == rowof
    assert np.count_nonzero(isdiag) == n
    noff = int(np.count_nonzero(~isdiag))
    data = np.zeros(indices.size)
    if values == "distinct":
        data[~isdiag] = _magnitudes(rng, noff)
    else:
        table = _magnitudes(rng, 200)
        assert noff >= 200 and n >= 56
        pick = rng.integers(0, 200, noff)
        pick[rng.permutation(noff)[:200]] = np.arange(200)
        data[~isdiag] = table[pick]
    need = 1.5 * np.bincount(rowof[~isdiag], weights=np.abs(data[~isdiag]), minlength=n) + 1.0
    if values == "distinct":
        data[isdiag] = need
    else:
        levels = np.array([g.max() for g in np.array_split(np.unique(need), 56)])
        data[isdiag] = levels[np.searchsorted(levels, need, side="left")]
        assert np.unique(data).size == 256
        if values == "few+1":
            for k in np.flatnonzero(~isdiag & (np.abs(data) >= 1.0))[::-1]:
                trial = data.copy()
                trial[k] = np.copysign(NEW_VALUE, data[k])
                if np.unique(trial).size == 257:
                    data = trial
                    break
            assert np.unique(data).size == 257
    return _csr(data, indices, indptr, (n, n))


def rect_matrix(rows, ncols, values="distinct", seed=0):
    """values +-U(0.25, 1): distinct, or drawn from a table of 16"""
    rng = _rng(seed, len(rows), ncols, 6)
    indptr, indices = _from_rows(rows, ncols)
    m = indices.size
    v = rng.choice([-1.0, 1.0], m) * rng.uniform(0.25, 1.0, m)
    if values == "few":
        v = v[:16][rng.integers(0, 16, m)] if m >= 16 else v
    return _csr(v, indices, indptr, (len(rows), ncols))


# ------------------------------------------------------------------------------------------------ rectangular structures
def tall_ragged(n, nH, seed=0):
    """P: 0..6 entries per row, about one row in seven truly empty"""
    rng = _rng(seed, n, nH, 7)
    rows = []
    for i in range(n):
        k = int(rng.integers(1, 7))
        if rng.integers(0, 7) == 0 or (n >= 3 and i == 1):
            k = 0
        rows.append(_pick(rng, nH, k))
    return rows


def wide_ragged(nH, n, seed=0):
    """R (not P^T): 0..60 entries per row, about one row in seven truly empty"""
    rng = _rng(seed, nH, n, 8)
    rows = []
    for i in range(nH):
        k = int(rng.integers(1, 61))
        if rng.integers(0, 7) == 0 or (nH >= 3 and i == nH - 2):
            k = 0
        rows.append(_pick(rng, n, k))
    return rows


def aggregation(n=LONG_N, nH=NH, big=3000, seed=0):
    """piecewise-constant P: aggregate 0 takes `big` fine dofs (scattered), the others share the rest -> R = P^T has a 3000-entry row"""
    rng = _rng(seed, n, nH, 9)
    agg = np.empty(n, dtype=np.int64)
    perm = rng.permutation(n)
    agg[perm[:big]] = 0
    agg[perm[big:]] = 1 + np.arange(n - big) % (nH - 1)
    return [np.array([a]) for a in agg]


def widths_tall(nH=NH, seed=0):
    ln = widths_lengths(WIDTHS_TALL, seed, least=0)
    rng = _rng(seed, ln.size, nH, 10)
    return [_pick(rng, nH, int(k)) for k in ln]


def base_offsets_tall(n=OFFSETS_N):
    """P[i, i // 3 + d], d in (0, 1, 2, 5) clipped: offsets relative to a base column"""
    nH = coarse_offsets_size(n)
    return [np.array([i // 3 + d for d in (0, 1, 2, 5) if i // 3 + d < nH], dtype=np.int64) for i in range(n)]


def coarse_offsets_size(n=OFFSETS_N):
    return (n - 1) // 3 + 3


def base_offsets_wide(n=OFFSETS_N):
    """R[I, 3 I + d], d in (-1 .. 3) clipped, every seventh row truly empty"""
    nH = coarse_offsets_size(n)
    return [np.array([3 * I + d for d in (-1, 0, 1, 2, 3) if 0 <= 3 * I + d < n and I % 7 != 3], dtype=np.int64) for I in range(nH)]


def mixed_span_wide(nH=WIDE_NH, n=WIDE_N, seed=0):
    """R, 129 x 70 001: rows of the first slice banded around 500 I (every slice column spans < 65 536), rows of the second slice
    alternately in the first and the last 2000 columns (spans above), the last row (a slice of its own) banded again; two rows truly empty"""
    rng = _rng(seed, nH, n, 11)
    rows = []
    for I in range(nH):
        k = int(rng.integers(3, 13))
        if I in (5, 70):
            k = 0
        if 64 <= I < 128:
            c = _pick(rng, 2000, k) + (0 if I % 2 == 0 else n - 2000)
        else:
            c = np.unique(np.clip(500 * I + rng.integers(-40, 41, k), 0, n - 1))
        rows.append(c)
    return rows


def mixed_span_tall(n=WIDE_N, nH=WIDE_NH):
    """P, 70 001 x 129: up to three neighbouring coarse columns per row (every span tiny), every 11th row truly empty"""
    rows = []
    for i in range(n):
        near = [(i * nH) // n + d for d in (-1, 0, 1)]
        keep = [c for c in near if 0 <= c < nH and (i + c) % 5 != 0]        # ragged: one entry in five is absent
        rows.append(np.array(keep if i % 11 != 7 else [], dtype=np.int64))
    return rows


def slice_widths(M):
    ln = np.diff(M.indptr)
    ns = (M.shape[0] + 63) // 64
    return np.array([ln[64 * s:64 * s + 64].max() for s in range(ns)], dtype=np.int64)


def column_spans(M):
    """per slice: the largest span (max - min column over the rows that have an entry j) of its slice columns; -1 for width 0"""
    ptr, idx = M.indptr, M.indices
    out = []
    for s in range((M.shape[0] + 63) // 64):
        rows = range(64 * s, min(M.shape[0], 64 * s + 64))
        w = max(ptr[i + 1] - ptr[i] for i in rows)
        span = -1
        for j in range(w):
            c = [idx[ptr[i] + j] for i in rows if ptr[i + 1] - ptr[i] > j]
            span = max(span, int(max(c)) - int(min(c)))
        out.append(span)
    return np.array(out, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ cases
def coarse_matrix(nH, scale):
    """the given SPD coarse matrix: scale * tridiag(-1, 2.5, -1) -- never the Galerkin product, so empty rows / columns of P and R
    cannot make it singular"""
    T = sp.diags([np.full(max(nH - 1, 0), -1.0), np.full(nH, 2.5), np.full(max(nH - 1, 0), -1.0)], [-1, 0, 1], format="csr") * scale
    T.sort_indices()
    return T


CASES = tuple("ragged-%d" % n for n in SIZES) + ("ragged-4283-few", "widths", "widths-few", "widths-few+1", "long", "offsets",
                                                  "offsets-few", "offsets-few+1", "wide")


def family(name):
    return name.split("-")[0]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, A, P, R, Ac, n, nH, x0, r0, xc): scipy CSR matrices and seeded vectors in (-1, 1)"""
    fam = family(name)
    values = "few+1" if name.endswith("few+1") else "few" if name.endswith("few") else "distinct"
    if fam == "ragged":
        n = int(name.split("-")[1])
        nH = coarse_size(n)
        A = square_matrix(ragged_structure(n), values)
        P = rect_matrix(tall_ragged(n, nH), nH)
        R = rect_matrix(wide_ragged(nH, n), n)
    elif fam == "widths":
        A = square_matrix(widths_structure(), values)
        n, nH = A.shape[0], NH
        P = rect_matrix(widths_tall(nH), nH, "few" if values != "distinct" else "distinct")
        R = rect_matrix(wide_ragged(nH, n), n)
    elif fam == "long":
        A = square_matrix(long_structure(), values)
        n, nH = LONG_N, NH
        P = rect_matrix(aggregation(n, nH), nH)
        T = P.T.tocsr()
        T.sort_indices()
        R = _csr(T.data, T.indices, T.indptr, (nH, n))
    elif fam == "offsets":
        A = square_matrix(offsets_structure(), values)
        n, nH = OFFSETS_N, coarse_offsets_size()
        P = rect_matrix(base_offsets_tall(), nH)
        R = rect_matrix(base_offsets_wide(), n)
    elif fam == "wide":
        n, nH, values = WIDE_N, WIDE_NH, "few"
        A = square_matrix(offsets_structure(n), "few")
        P = rect_matrix(mixed_span_tall(), nH, "few")
        R = rect_matrix(mixed_span_wide(), n, "few")
    else:
        raise ValueError(name)
    absum = lambda M: float(np.mean(np.abs(M).sum(axis=1))) or 1.0
    Ac = coarse_matrix(nH, float(np.mean(A.diagonal())) * absum(P) * absum(R))
    rng = _rng(CASES.index(name), n, 12)
    return types.SimpleNamespace(name=name, family=fam, values=values, A=A, P=P, R=R, Ac=Ac, n=n, nH=nH,
                                 x0=rng.uniform(-1, 1, n), r0=rng.uniform(-1, 1, n), xc=rng.uniform(-1, 1, nH))


# ------------------------------------------------------------------------------------------------ references
def max_rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    m = np.max(np.abs(b)) if b.size else LD(0)
    d = np.max(np.abs(a - b)) if b.size else LD(0)
    return float(d / m) if m > 0 else float(d)


def row_reference_all(M, x, budget=1 << 21):
    """fullsize_reference.row_reference over ALL rows of M -> (seq, exact, bound), each of length nrows.  Rows are handed over in
    groups of similar length (sorted by length, <= `budget` padded entries per group): a 3000-entry row is not padded 4283 times."""
    n = M.shape[0]
    ln = np.diff(M.indptr)
    order = np.argsort(ln, kind="stable")
    seq, exact, bound = np.zeros(n), np.zeros(n), np.zeros(n)
    at = 0
    while at < n:
        end = at + 1
        while end < n and (end + 1 - at) * max(int(ln[order[end]]), 1) <= budget:
            end += 1
        rows = order[at:end]
        c, v, l = fr.padded_rows(M.indptr, M.indices, M.data, rows)
        seq[rows], exact[rows], bound[rows] = fr.row_reference(c, v, l, x)
        at = end
    return seq, exact, bound


def seq_spmv(M, x):
    """every row summed left to right in storage order from 0.0, products and sums rounded separately (float64): the sum
    sell_kernel, sellc_kernel, sello_kernel and the reference's mul! take"""
    n = M.shape[0]
    ptr, idx, val = M.indptr, M.indices, M.data
    ln = np.diff(ptr)
    order = np.argsort(-ln, kind="stable")
    neg = -ln[order]
    y = np.zeros(n)
    x = np.asarray(x, dtype=np.float64)
    for j in range(int(ln.max()) if n else 0):
        act = order[:np.searchsorted(neg, -j, side="left")]
        k = ptr[act] + j
        y[act] = y[act] + val[k] * x[idx[k]]
    return y


def matvec_ld(M, v):
    y = np.zeros(M.shape[0], dtype=LD)
    np.add.at(y, np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), M.data.astype(LD) * v[M.indices])
    return y


def ref_sweeps(A, x, r, k, omega=OMEGA):
    """k sweeps of dx = omega D^-1 r; x += dx; r -= A dx (RichardsonSmoothers.jl:84-98 with JacobiLinearSolver) in longdouble"""
    x, r = np.array(x, dtype=LD), np.array(r, dtype=LD)
    dinv = LD(1) / A.diagonal().astype(LD)
    for _ in range(k):
        dx = LD(omega) * (dinv * r)
        x += dx
        r -= matvec_ld(A, dx)
    return x, r


def ref_precond(A, r):
    """dx of one Jacobi application from a zero guess: D^-1 r (JacobiLinearSolvers.jl:45)"""
    return np.asarray(r, dtype=LD) / A.diagonal().astype(LD)


def twin_sweeps(A, x, r, k, omega=OMEGA, stream=None):
    """the same in float64 with the kernels' roundings: dinv = 1 / diag, s = omega * (dinv * r), x + s, r - (CSR-order sum).
    stream: the matrix the row sums are taken over (a corruption of A; the diagonal is always A's)"""
    x, r = np.array(x, dtype=np.float64), np.array(r, dtype=np.float64)
    dinv = 1.0 / A.diagonal()
    S = A if stream is None else stream
    for _ in range(k):
        s = omega * (dinv * r)
        x = x + s
        r = r - seq_spmv(S, s)
    return x, r


@functools.lru_cache(maxsize=None)
def reference(name):
    """longdouble references of one case (computed once): dx of precond, (x, r) after k sweeps from (x0, r0) and from a zero guess,
    and the row references of y = A x0, P xc, R x0"""
    c = case(name)
    out = types.SimpleNamespace(dx=ref_precond(c.A, c.r0), sweeps={}, zero={}, rows={})
    for k in SWEEPS:
        out.sweeps[k] = ref_sweeps(c.A, c.x0, c.r0, k)
        out.zero[k] = ref_sweeps(c.A, np.zeros(c.n), c.r0, k)
    out.rows = dict(A=row_reference_all(c.A, c.x0), P=row_reference_all(c.P, c.xc), R=row_reference_all(c.R, c.x0))
    return out


# ------------------------------------------------------------------------------------------------ corruptions (host only)
def _edit(M, keep=None, cols=None, extra=None):
    """M with entries dropped (keep: bool per entry), columns replaced, or entries appended at row ends (extra: {row: [(col, val)]})"""
    ptr, idx, val = M.indptr, M.indices.copy(), M.data
    if cols is not None:
        idx = np.asarray(cols, dtype=np.int32)
    keep = np.ones(idx.size, dtype=bool) if keep is None else keep
    rows = []
    for i in range(M.shape[0]):
        s = slice(ptr[i], ptr[i + 1])
        c, v = idx[s][keep[s]], val[s][keep[s]]
        if extra and i in extra:
            c = np.concatenate([c, [e[0] for e in extra[i]]])
            v = np.concatenate([v, [e[1] for e in extra[i]]])
        rows.append((c, v))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])])
    return _csr(np.concatenate([v for _, v in rows] + [np.zeros(0)]), np.concatenate([c for c, _ in rows] + [np.zeros(0)]), indptr, M.shape)


def drop_unroll_tail(M, un):
    """sell_kernel with a remainder loop that starts one entry late: entry UN * (w // UN) of every row of a slice of width w is lost"""
    ptr = M.indptr
    keep = np.ones(M.indices.size, dtype=bool)
    w = slice_widths(M)
    for i in range(M.shape[0]):
        j0 = un * (int(w[i // 64]) // un)
        if j0 < ptr[i + 1] - ptr[i]:
            keep[ptr[i] + j0] = False
    return _edit(M, keep=keep)


def cut_at_tile(M):
    """csr_stream1_kernel taking a row of TILE + 1 entries through the tile branch: its last entry is lost"""
    ptr = M.indptr
    keep = np.ones(M.indices.size, dtype=bool)
    for i in np.flatnonzero(np.diff(ptr) == TILE + 1):
        keep[ptr[i + 1] - 1] = False
    return _edit(M, keep=keep)


def add_padding_products(M):
    """sellc_kernel without the row-length mask: a row shorter than its slice adds dict[0] * x[its first column] per padded entry
    (the padding of the packed code stream is code 0, the smallest bit pattern of the dictionary)"""
    keys = np.unique(M.data.view(np.uint64))
    d0 = keys[:1].view(np.float64)[0]
    w = slice_widths(M)
    ptr = M.indptr
    extra = {}
    for i in range(M.shape[0]):
        ln = int(ptr[i + 1] - ptr[i])
        if 0 < ln < w[i // 64]:
            extra[i] = [(int(M.indices[ptr[i]]), d0)] * (int(w[i // 64]) - ln)
    return _edit(M, extra=extra)


def skip_last_slice(M):
    keep = np.ones(M.indices.size, dtype=bool)
    keep[M.indptr[64 * ((M.shape[0] - 1) // 64)]:] = False
    return _edit(M, keep=keep)


def shortest_row_offsets(M):
    """sello_kernel reading one offset table per wave: every row of a slice gathers with the offsets of the slice's shortest row,
    offset 0 for the entries past that row's end (columns clipped to the matrix)"""
    ptr, idx = M.indptr, M.indices
    ln = np.diff(ptr)
    cols = idx.astype(np.int64).copy()
    for s in range((M.shape[0] + 63) // 64):
        rows = np.arange(64 * s, min(M.shape[0], 64 * s + 64))
        q = rows[np.argmin(ln[rows])]
        off = idx[ptr[q]:ptr[q + 1]].astype(np.int64) - q
        for i in rows:
            o = np.zeros(ln[i], dtype=np.int64)
            o[:min(off.size, ln[i])] = off[:ln[i]]
            cols[ptr[i]:ptr[i + 1]] = np.clip(i + o, 0, M.shape[1] - 1)
    return _edit(M, cols=cols)


CORRUPTIONS = dict([("drop_unroll_tail_un%d" % u, ("widths", functools.partial(drop_unroll_tail, un=u))) for u in SELL_UNROLLS] +
                   [("cut_at_tile", ("long", cut_at_tile)), ("add_padding_products", ("widths-few", add_padding_products)),
                    ("skip_last_slice", ("ragged-4283", skip_last_slice)), ("shortest_row_offsets", ("offsets", shortest_row_offsets))])


# ------------------------------------------------------------------------------------------------ host restatement of the setup
DEFAULTS = dict(sell=1, pattern=1, vdict=1, idx16=1, opattern=1, sell_maxpad=1.25, pat_un=9, lanes_log2=-1)


def csr_blocks(M, lanes_log2=-1):
    """upload_csr's greedy workgroup partition -> (row boundaries, lanes_log2): rows are added while the workgroup holds <= TILE
    entries and <= 256 >> lanes_log2 rows; a row longer than a tile is a workgroup of its own"""
    n, ptr = M.shape[0], M.indptr
    avg = ptr[-1] / n if n else 1.0
    lg = 0
    while lg < 6 and (1 << (lg + 1)) * 6.0 <= avg:
        lg += 1
    if lanes_log2 >= 0:
        lg = min(int(lanes_log2), 6)
    blk, r = [0], 0
    while r < n:
        e = r
        while e < n and ptr[e + 1] - ptr[r] <= TILE and e - r < (256 >> lg):
            e += 1
        if e == r:
            e = r + 1
        blk.append(e)
        r = e
    return np.array(blk, dtype=np.int64), lg


def _offset_patterns_fit(M, un):
    """detect_patterns(ignore_values = true) + the 32 KB bound of build_sell: rows are equal when their lengths and their column
    offsets (relative to the row index when ncols >= nrows, else -- or when that fails -- to their first column) are equal"""
    n, ncols = M.shape
    ptr, idx = M.indptr, M.indices
    wmax = int(np.diff(ptr).max())
    if wmax == 0 or wmax > 1024:
        return False
    max_np = min(65534, 48 * 1024 // (12 * wmax + 4) - 1)
    if max_np < 1:
        return False
    W = -(-wmax // un) * un
    for mode in ((0, 1) if ncols >= n else (1,)):
        pats = set()
        for i in range(n):
            c = idx[ptr[i]:ptr[i + 1]].astype(np.int64)
            pats.add((c - (i if mode == 0 else (c[0] if c.size else 0))).tobytes())
            if len(pats) > max_np:
                break
        if len(pats) <= max_np and (len(pats) + 1) * (12 * W + 4) <= 48 * 1024:
            return (len(pats) + 1) * W * 4 <= 32 * 1024
    return False


def expected_layout(M, options=None):
    """The layout build_sell gives a whole CSR operator under `options` (keys as gmg_set_option takes them, lower case):
    dict(layout, value_dictionary, idx16, padding).  Row-pattern detection (SELL-P) is not restated: pattern must be 0 unless sell is."""
    o = dict(DEFAULTS)
    o.update({str(k).lower().replace("gmg_", ""): v for k, v in (options or {}).items()})
    n, ncols = M.shape
    nnz = int(M.indptr[-1])
    csr = dict(layout="CSR-stream", value_dictionary=False, idx16=False, padding=1.0)
    if not o["sell"] or n == 0 or nnz == 0:
        return csr
    if o["pattern"] and n >= 64:
        raise ValueError("expected_layout does not restate the row-pattern detection: pass pattern=0")
    w = slice_widths(M)
    zp = 64 * int(w.sum())
    few = bool(o["vdict"]) and np.unique(M.data.view(np.uint64)).size <= 256
    if zp > o["sell_maxpad"] * nnz and (not few or 4.0 * zp > 0.8 * 12.0 * nnz):
        return csr
    n16 = 0
    if o["idx16"] and (few or o["idx16"] > 1):
        n16 = int(np.count_nonzero((w > 0) & (column_spans(M) <= 65535)))
    idx16 = n16 > 0 and (few or o["idx16"] > 1)
    pat_un = o["pat_un"]
    un = 27 if pat_un >= 27 else 14 if pat_un >= 14 else 9 if pat_un >= 9 else 6 if pat_un >= 6 else 3
    opat = not few and not idx16 and bool(o["opattern"]) and n >= 64 and ncols < (1 << 28) and _offset_patterns_fit(M, un)
    return dict(layout="SELL-O" if opat else "SELL-64", value_dictionary=few, idx16=idx16, padding=zp / nnz, slices16=n16, slices=w.size)


BIGPAD = 1.0e6
_SELL = dict(pattern=0, vdict=0, idx16=0, opattern=0, sell_maxpad=BIGPAD)
CONFIGS = {
    "csr": dict(sell=0),
    "sell": dict(_SELL),
    "sellc_dict_idx16": dict(pattern=0, vdict=1, idx16=1, sell_maxpad=BIGPAD),
    "sellc_idx16": dict(pattern=0, vdict=0, idx16=2, opattern=0, sell_maxpad=BIGPAD),
    "sellc_dict": dict(pattern=0, vdict=1, idx16=0, sell_maxpad=BIGPAD),
    "sello": dict(pattern=0, opattern=1, sell_maxpad=BIGPAD),
    "ragged_default_pad": dict(pattern=0),                  # the padding rule itself: default sell_maxpad = 1.25
}
_L = lambda layout, d=False, i=False: dict(layout=layout, value_dictionary=d, idx16=i)
# (case, configuration) -> the layout of A the pair is built to reach
INTENDED = {
    ("ragged-4283", "csr"): _L("CSR-stream"), ("long", "csr"): _L("CSR-stream"),
    ("ragged-4283", "sell"): _L("SELL-64"), ("widths", "sell"): _L("SELL-64"), ("long", "sell"): _L("SELL-64"), ("offsets", "sell"): _L("SELL-64"),
    ("ragged-1", "sell"): _L("SELL-64"), ("ragged-65", "sell"): _L("SELL-64"),
    ("widths-few", "sellc_dict_idx16"): _L("SELL-64", True, True), ("widths-few", "sellc_idx16"): _L("SELL-64", False, True),
    ("widths-few", "sellc_dict"): _L("SELL-64", True, False), ("widths-few+1", "sellc_dict_idx16"): _L("SELL-64", False, False),
    ("offsets-few", "sellc_dict_idx16"): _L("SELL-64", True, True), ("offsets-few+1", "sellc_dict_idx16"): _L("SELL-O", False, False),
    ("ragged-4283-few", "sellc_dict_idx16"): _L("SELL-64", True, True), ("wide", "sellc_dict_idx16"): _L("SELL-64", True, True),
    ("offsets", "sello"): _L("SELL-O"), ("ragged-4283", "sello"): _L("SELL-64"),
    # default padding bound: ragged rows pad far beyond 1.25 -> CSR-stream unless the stream compresses (<= 256 values and
    # 4 zp <= 9.6 nnz); the offsets matrices pad by a few per cent -> SELL
    ("ragged-4283", "ragged_default_pad"): _L("CSR-stream"), ("ragged-4283-few", "ragged_default_pad"): _L("SELL-64", True, True),
    ("long", "ragged_default_pad"): _L("CSR-stream"), ("offsets", "ragged_default_pad"): _L("SELL-O"),
    ("offsets-few", "ragged_default_pad"): _L("SELL-64", True, True),
}
