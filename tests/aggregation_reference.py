"""Numpy twin of the smoothed-aggregation prolongations (tests only): the construction of include/gmg_amd.h, gmg_set_aggregation,
restated with whole-array numpy operations -- no kernel is mirrored, the device result is compared with this bit for bit.

    strength    m_i = max over stored k != i of |a_ik|; (i, j), j != i, a_ij != 0, row-strong iff |a_ij| >= theta * m_i; {i, j} an edge
                iff (i, j) or (j, i) is row-strong; w_ij = max(|a_ij|, |a_ji|)
    priorities  key_i = mix(i + 0x9E3779B97F4A7C15 (seed + 1)) in wrapping 64-bit arithmetic, mix = the splitmix64 finaliser
                z = (z ^ z>>30) 0xBF58476D1CE4E5B9; z = (z ^ z>>27) 0x94D049BB133111EB; z ^= z>>31; nodes order by (key_i, i).  Here the
                pairs are replaced by their rank 1 .. n in that order, and "none" by 0: the same total order
    MIS-2       rounds until no node is undecided (see aggregate())
    aggregates  roots numbered in ascending row index, pass 1 (root neighbours), pass 2 (largest w_ij, ties to the smallest j)
    P           T, or (I - omega D^-1 A) T entry by entry with ordered sums (see prolongation())

Sums that the definition orders (row sums of |a_ik| for rho, the s_J of P) are accumulated position by position, so every partial sum
is rounded as a left-to-right loop rounds it (np.add.reduce would pair the terms).

Also the small test matrices the host and the GPU tests share.
"""
import numpy as np

from galerkin_reference import M, galerkin

GAMMA = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def keys(n, seed=0):
    z = np.arange(n, dtype=np.uint64) + np.uint64((GAMMA * (int(seed) + 1)) & MASK64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _entries(A):
    n = A.shape[0]
    if A.shape[0] != A.shape[1]:
        raise ValueError("square matrices only")
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.ptr))
    cols = A.idx.astype(np.int64)
    if np.any((np.diff(cols) <= 0) & (np.diff(rows) == 0)):
        raise ValueError("the columns of every row must ascend")
    return n, rows, cols, A.val


def diagonal(A):
    """a_ii of every row; ValueError naming the first row without a stored nonzero one"""
    n, rows, cols, a = _entries(A)
    d = np.zeros(n)
    on = rows == cols
    d[rows[on]] = a[on]
    if np.any(d == 0.0):
        raise ValueError(f"row {int(np.flatnonzero(d == 0.0)[0])} has no stored nonzero diagonal entry")
    return d


def _ordered_row_sums(ptr, x):
    """sum of x over every row, left to right from 0.0"""
    n, ln = ptr.size - 1, np.diff(ptr)
    s = np.zeros(n)
    for t in range(int(ln.max()) if n else 0):
        on = ln > t
        s[on] = s[on] + x[ptr[:-1][on] + t]
    return s


def strength(A, theta=0.25):
    """-> (ei, ej, w) over the stored entries that are edges of the strength graph, in stored order (both directions of every edge)"""
    n, rows, cols, a = _entries(A)
    diagonal(A)
    key = rows * n + cols
    tkey = cols * n + rows
    pos = np.minimum(np.searchsorted(key, tkey), key.size - 1)
    missing = key[pos] != tkey
    if np.any(missing):
        k = int(np.flatnonzero(missing)[0])
        raise ValueError(f"the stored pattern is not structurally symmetric: ({int(rows[k])}, {int(cols[k])})")
    absa = np.abs(a)
    off = rows != cols
    m = np.zeros(n)
    np.maximum.at(m, rows[off], absa[off])
    row_strong = off & (a != 0.0) & (absa >= theta * m[rows])
    edge = row_strong | row_strong[pos]
    w = np.maximum(absa, absa[pos])
    return rows[edge], cols[edge], w[edge]


def aggregate(A, theta=0.25, seed=0):
    """-> dict(agg, nagg, rounds, roots (bool), pass1 (bool: assigned by pass 1, roots included), ei, ej, w, strong_edges)"""
    n = A.shape[0]
    ei, ej, w = strength(A, theta)
    key = keys(n, seed)
    order = np.lexsort((np.arange(n), key))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(1, n + 1)

    def nmax(v):
        out = v.copy()
        np.maximum.at(out, ei, v[ej])
        return out

    state = np.zeros(n, dtype=np.int8)                        # 0 undecided, 1 root, 2 covered
    rounds = 0
    while np.any(state == 0):
        und = state == 0
        t2 = nmax(nmax(np.where(und, rank, 0)))
        new = und & (t2 == rank)
        f2 = nmax(nmax(new.astype(np.int64)))
        state[new] = 1
        state[und & ~new & (f2 > 0)] = 2
        rounds += 1
    roots = state == 1
    rootid = np.cumsum(roots) - 1
    agg1 = np.where(roots, rootid, -1)
    near = roots[ej] & ~roots[ei]
    agg1[ei[near][::-1]] = rootid[ej[near][::-1]]             # (the first root neighbour in stored order; there is at most one)
    agg = agg1.copy()
    cand = (agg1[ei] < 0) & (agg1[ej] >= 0)
    ci, cj, cw = ei[cand], ej[cand], w[cand]
    o = np.lexsort((cj, -cw, ci))                             # per row: largest w first, ties to the smallest j
    first = np.concatenate([[True], np.diff(ci[o]) != 0]) if o.size else np.zeros(0, dtype=bool)
    agg[ci[o][first]] = agg1[cj[o][first]]
    if np.any(agg < 0):
        raise AssertionError("a covered node found no assigned neighbour")
    return dict(agg=agg.astype(np.int32), nagg=int(roots.sum()), rounds=rounds, roots=roots, pass1=agg1 >= 0, ei=ei, ej=ej, w=w,
                strong_edges=int(ei.size // 2))


def rho_bound(A):
    """max_i (sum_k |a_ik| in stored order from 0.0) / |a_ii|"""
    return float(np.max(_ordered_row_sums(A.ptr, np.abs(A.val)) / np.abs(diagonal(A))))


def prolongation(A, agg, nagg, smooth=True, omega=None):
    """-> (P, omega, rho) for given aggregates (the value refresh keeps them and calls this with the new values)"""
    n, rows, cols, a = _entries(A)
    agg = np.asarray(agg, dtype=np.int64)
    rho = rho_bound(A)
    om = float(omega) if omega is not None and omega > 0 else (4.0 / 3.0) / rho
    if not smooth:
        return M((n, nagg), np.arange(n + 1), agg, np.ones(n)), om, rho
    J = agg[cols]
    o = np.lexsort((np.arange(cols.size), J, rows))           # by row, then aggregate, then stored order
    ro, Jo, ao = rows[o], J[o], a[o]
    start = np.flatnonzero(np.concatenate([[True], (np.diff(ro) != 0) | (np.diff(Jo) != 0)]))
    gptr = np.concatenate([start, [ro.size]])
    s = _ordered_row_sums(gptr, ao)
    prow, pcol = ro[start], Jo[start]
    wi = om * (1.0 / diagonal(A))
    q = wi[prow] * s
    val = np.where(pcol == agg[prow], 1.0, 0.0) - q
    ptr = np.concatenate([[0], np.cumsum(np.bincount(prow, minlength=n))])
    return M((n, nagg), ptr, pcol, val), om, rho


def build(A, theta=0.25, smooth=True, omega=None, seed=0):
    g = aggregate(A, theta, seed)
    P, om, rho = prolongation(A, g["agg"], g["nagg"], smooth, omega)
    g.update(P=P, omega=om, rho=rho)
    return g


def hierarchy(A0, nlev, theta=0.25, smooth=True, omega=None, seed=0, frozen=None):
    """algebraic levels only: -> (mats, Ps, infos); frozen = the infos of an earlier call whose aggregates are kept (value refresh)"""
    mats, Ps, infos = [A0], [], []
    for l in range(nlev - 1):
        if frozen is None:
            g = build(mats[-1], theta, smooth, omega, seed)
        else:
            g = dict(frozen[l])
            g["P"], g["omega"], g["rho"] = prolongation(mats[-1], g["agg"], g["nagg"], smooth, omega)
        infos.append(g)
        Ps.append(g["P"])
        mats.append(galerkin(None, mats[-1], g["P"])[1])
    return mats, Ps, infos


# ---- shared test matrices -----------------------------------------------------------------------------------------------------------
def from_scipy(S):
    S = S.tocsr().copy()
    S.sort_indices()
    return M(S.shape, S.indptr, S.indices, S.data)


def chain(n):
    """1-D Q1 stiffness matrix on n free dofs: tridiag(-1, 2, -1) (n + 1)"""
    ptr, idx, val = [0], [], []
    h = float(n + 1)
    for i in range(n):
        for j, v in ((i - 1, -h), (i, 2.0 * h), (i + 1, -h)):
            if 0 <= j < n:
                idx.append(j); val.append(v)
        ptr.append(len(idx))
    return M((n, n), ptr, idx, val)


def with_isolated_rows(A, isolated):
    """A with the off-diagonal entries of the rows and columns `isolated` removed from the pattern (diagonal-only rows)"""
    import scipy.sparse as sp
    S = A.to_scipy().tolil()
    for i in isolated:
        d = S[i, i]
        S[i, :] = 0.0
        S[:, i] = 0.0
        S[i, i] = d
    S = sp.csr_matrix(S)
    S.eliminate_zeros()
    return from_scipy(S)


def with_zero_row(A, i):
    """A with the off-diagonal entries of row and column i set to stored 0.0 (the pattern stays)"""
    val = A.val.copy()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.ptr))
    val[((rows == i) | (A.idx == i)) & (rows != A.idx)] = 0.0
    return M(A.shape, A.ptr, A.idx, val)


def nonsymmetric_values(n=12):
    """a chain whose values are not symmetric: a_(i,i+1) = -1, a_(i+1,i) = -0.01, and one weak symmetric coupling pair (0, 2) of -0.02:
    with theta = 0.25, (i, i+1) is row-strong in row i; in row i+1 the maximum is 1 (towards i+2), so (i+1, i) is not -- the edge
    exists through one direction only; (0, 2) is strong in neither row (row 0: 0.02 < 0.25; row 2: 0.02 < 0.25)"""
    import scipy.sparse as sp
    S = sp.lil_matrix((n, n))
    for i in range(n):
        S[i, i] = 3.0
        if i + 1 < n:
            S[i, i + 1] = -1.0
            S[i + 1, i] = -0.01
    S[0, 2] = S[2, 0] = -0.02
    return from_scipy(sp.csr_matrix(S))
