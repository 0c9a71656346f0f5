"""Inputs and references of the own | ghost split edge tests (tests/test_halo_edge_problems.py on the host,
tests/test_gpu_halo_edges.py on the device).  Plain helper, numpy and scipy only: no fixtures, no collection hooks, nothing read
from outside the repository.

The code under test finishes a partitioned level's mat-vec after the halo has arrived (csrc/comm.hpp: ghost_fix_kernel,
ghost_fix_sell_kernel in its plain-value and dictionary forms, halo_pack_kernel, halo_unpack_add_kernel) and the setup that feeds it
(gmg_setup: build_ghost_fix, the fused-pack tables pk_ptr / pk_slot, the split restriction).  Every family is a GLOBAL hierarchy of
general sparse matrices (operator_edge_problems style: full diagonal, diagonally dominant, magnitudes 1e-3 .. 1e3, nonsymmetric),
a dof -> owner map that is NOT a set of contiguous blocks, W virtual ranks partitioned by dpartition and folded onto one rank
(FoldedSpace / stack_rows), level 0 partitioned and the coarsest level replicated:

  bnd-N            exactly N boundary rows on the folded level 0 (N = 1, 63, 64, 65, 255, 256, 257) and R_BND[N] boundary rows of R
  widths           one slice of 64 boundary rows per ghost width w in WIDTHS: every w % 4 with lanes shorter and longer than the last quad
  dict-255 / dict-256 / dict-256-nopad   255 / 256 / 256 distinct ghost values; with padded slots the table holds one more (0.0)
  fan-out          symmetric pattern, owned rows sent to 1, 2 and >= 3 neighbours: the fused pack with pk_ptr ranges of 1, 2, >= 3
  one-way          nonsymmetric: sent rows without a ghost column (pack not fusable), one message direction of length zero
  uncoupled        block-diagonal across ranks: no ghosts, no sends, no boundary rows
  chain            three levels, levels 0 and 1 partitioned: P gathers from an exchanged coarse vector
  slabs, slabs-16  the Q1 3-D Poisson matrix in z-slabs of unequal thickness, one of them a single plane: the smallest grid whose
                   sweep gathers r (175 rows, 75 boundary rows), and one with several workgroups of boundary rows (3825 / 675)
  patches          fan-out with ragged patches (2 .. 12 dofs) reaching into ghost dofs of two neighbours: assemble!

Global dof 0 (= folded column 0: rank 0 owns it) is referenced by row 0 alone in every generated family, so a non-finite x[0] may
reach row 0 only -- unless a fix-up multiplies its padded (column 0, 0.0) slots.

case(name)          everything one device case needs (cached): the global matrices, the folded levels, the `local_hierarchy` dict
census(M, n_own)    build_ghost_fix restated: boundary rows, slice widths, slot table, distinct values, form
twin_apply          float64 restatement of the split arithmetic: own-column sum in storage order, ghost-column sum in storage order
                    from 0.0, own + ghost
ref_sweeps / twin_sweeps    k Richardson(Jacobi) sweeps in longdouble on the GLOBAL matrix / in float64 with the split row sums
patch_contributions / assemble    the patch smoother's local solves and assemble!: longdouble sum, and the twin's in message order
CORRUPTIONS         wrong kernels restated on the host: each must leave the gates of the device tests on the family built for it
"""
import functools
import importlib
import types

import numpy as np
import scipy.sparse as sp

import operator_edge_problems as oe

LD = np.longdouble
OMEGA = oe.OMEGA
SWEEPS = (1, 2, 3, 4, 5)
BND = (1, 63, 64, 65, 255, 256, 257)
R_BND = {1: 64, 63: 65, 64: 1, 65: 63, 255: 256, 256: 257, 257: 255}     # another such count for R's boundary rows
WIDTHS = tuple(range(1, 11)) + (12, 13, 16, 17)
# cells and the node planes the z-slabs begin at: 5 x 5 nodes per plane in slabs of 2, 1 and 4 planes; 15 x 15 in slabs of 6, 1 and 10
SLABS = {"slabs": ((6, 6, 8), (0, 2, 3, 7)), "slabs-16": ((16, 16, 18), (0, 6, 7, 17))}
CASES = tuple("bnd-%d" % n for n in BND) + ("widths", "dict-255", "dict-256", "dict-256-nopad", "fan-out", "one-way", "uncoupled",
                                             "chain", "slabs", "slabs-16", "patches")


def _mods():
    import __graft_entry__ as entry
    pkg = entry.import_package()
    return importlib.import_module(pkg.__name__ + ".dpartition"), pkg.poisson


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


# ------------------------------------------------------------------------------------------------ global structures
def scattered_owner(n, W, seed):
    """dof -> owner, not contiguous: seeded at random, every rank owns something, rank 0 owns dof 0"""
    rng = _rng(seed, n, W, 20)
    o = rng.integers(0, W, n)
    o[:W] = np.arange(W)
    return o.astype(np.int64)


def split_rows(rng, row_owner, col_owner, own_len, ghost_len, square, may=None, pools=None):
    """row i: own_len[i] columns among the dofs its owner owns (the diagonal first when `square`) and ghost_len[i] among the dofs of
    the ranks may[owner] (default: every other rank; pools[owner]: among these dofs instead); column 0 only in row 0 of a square
    matrix.  -> list of sorted column arrays"""
    W = int(max(row_owner.max(), col_owner.max())) + 1
    ids = np.arange(col_owner.size)
    own_pool = [ids[(col_owner == r) & (ids > 0)] for r in range(W)]
    oth_pool = pools or [ids[np.isin(col_owner, [q for q in (range(W) if may is None else may[r]) if q != r]) & (ids > 0)] for r in range(W)]
    rows = []
    for i in range(row_owner.size):
        r = int(row_owner[i])
        pool = own_pool[r][own_pool[r] != i] if square else own_pool[r]
        c = rng.choice(pool, size=min(int(own_len[i]), pool.size), replace=False)
        g = rng.choice(oth_pool[r], size=int(ghost_len[i]), replace=False)
        rows.append(np.sort(np.concatenate([[i] if square else [], c, g]).astype(np.int64)))
    return rows


def _values(rows, row_owner, col_owner, square, rng, table=0):
    """-> scipy CSR.  Square: off-diagonal magnitudes 1e-3 .. 1e3, diag = 1.5 * sum|off-diagonal| + 1; rectangular: +-U(0.25, 1).
    table > 0: the entries in ghost columns take exactly `table` distinct doubles (each at least once)."""
    ncols = col_owner.size
    indptr, indices = oe._from_rows(rows, ncols)
    n = len(rows)
    rowof = np.repeat(np.arange(n), np.diff(indptr))
    m = indices.size
    data = oe._magnitudes(rng, m) if square else rng.choice([-1.0, 1.0], m) * rng.uniform(0.25, 1.0, m)
    ghost = col_owner[indices] != row_owner[rowof]
    ng = int(np.count_nonzero(ghost))
    if table:
        assert ng >= table
        vals = data[ghost][:table].copy()
        assert np.unique(vals).size == table and not np.any(vals == 0.0)
        pick = rng.integers(0, table, ng)
        pick[rng.permutation(ng)[:table]] = np.arange(table)
        data[ghost] = vals[pick]
    if square:
        isdiag = indices == rowof
        assert np.count_nonzero(isdiag) == n
        data[isdiag] = 0.0
        data[isdiag] = 1.5 * np.bincount(rowof, weights=np.abs(data), minlength=n) + 1.0
    return oe._csr(data, indices, indptr, (n, ncols))


def ragged_lengths(rng, N, lo=1, hi=6):
    """ghost-row lengths of N boundary rows in folded order: ragged inside every slice of two rows or more"""
    ln = rng.integers(lo, hi + 1, N)
    for s in range(0, N, 64):
        if min(N, s + 64) - s >= 2:
            ln[s], ln[s + 1] = hi, lo
    return ln


def place_boundary(rng, owner, lengths, first=1):
    """ghost_len per global row: len(lengths) rows drawn at random from rows >= first become the boundary rows; lengths[q] goes to
    the q-th of them in FOLDED order (by rank, then id) -- the order the slices of the fix-up are cut in"""
    n = owner.size
    rows = first + rng.choice(n - first, size=len(lengths), replace=False)
    rows = rows[np.lexsort((rows, owner[rows]))]
    gl = np.zeros(n, dtype=np.int64)
    gl[rows] = lengths
    return gl


def general_family(name, n, nH, W, a_len, r_len, seed, table=0, may=None, own_hi=12):
    """two levels: A (n x n) and R (nH x n) with the given ghost-row lengths (in folded boundary order), P ragged over the
    replicated coarse level, a given SPD coarse matrix"""
    rng = _rng(seed, n, nH, 21)
    o0, o1 = scattered_owner(n, W, seed), scattered_owner(nH, W, seed + 1)
    A = _values(split_rows(rng, o0, o0, rng.integers(0, own_hi + 1, n), place_boundary(rng, o0, a_len), True, may), o0, o0, True, rng, table)
    R = _values(split_rows(rng, o1, o0, rng.integers(1, 9, nH), place_boundary(rng, o1, r_len, first=0), False, may), o1, o0, False, rng, table)
    P = oe.rect_matrix(oe.tall_ragged(n, nH, seed), nH)
    return dict(name=name, W=W, mats=[A, _coarse(A, P, R, nH)], P=[P], R=[R], owners=[o0, o1], part=1)


def _coarse(A, P, R, nH):
    absum = lambda M: float(np.mean(np.abs(M).sum(axis=1))) or 1.0
    return oe.coarse_matrix(nH, float(np.mean(A.diagonal())) * absum(P) * absum(R))


def _fan_out(name, seed=5):
    """symmetric pattern over W = 5 ranks: hubs are joined to leaves of m other ranks (m = 1, 2, 3, 4 in turn), a leaf to one hub only
    -- so a hub is sent to m neighbours and has ghosts of m ranks, a leaf is sent to one; values are not symmetric"""
    n, nH, W = 1200, 150, 5
    rng = _rng(seed, n, 22)
    o0, o1 = scattered_owner(n, W, seed), scattered_owner(nH, W, seed + 1)
    adj = [set([i]) for i in range(n)]
    for r in range(W):                                      # own x own: symmetric random edges, dof 0 left alone
        mine = np.flatnonzero((o0 == r) & (np.arange(n) > 0))
        for _ in range(3 * mine.size):
            a, b = rng.choice(mine, 2, replace=False)
            adj[a].add(int(b)); adj[b].add(int(a))
    free = [list(rng.permutation(np.flatnonzero((o0 == r) & (np.arange(n) > 0)))) for r in range(W)]
    for h in range(160):
        r = h % W
        hub = int(free[r].pop())
        others = [q for q in range(W) if q != r]
        for q in rng.choice(others, size=1 + h % 4, replace=False):
            for _ in range(int(rng.integers(1, 3))):
                leaf = int(free[int(q)].pop())
                adj[hub].add(leaf); adj[leaf].add(hub)
    rows = [np.array(sorted(a), dtype=np.int64) for a in adj]
    A = _values(rows, o0, o0, True, rng)
    # R's ghost columns among the dofs A already brings to the rank: every sent row stays a boundary row of A (the pack is fusable)
    pools = [np.unique(np.concatenate([rows[i][o0[rows[i]] != r] for i in np.flatnonzero(o0 == r)])) for r in range(W)]
    R = _values(split_rows(rng, o1, o0, rng.integers(1, 9, nH), place_boundary(rng, o1, ragged_lengths(rng, 40), first=0), False, pools=pools),
                o1, o0, False, rng)
    P = oe.rect_matrix(oe.tall_ragged(n, nH, seed), nH)
    return dict(name=name, W=W, mats=[A, _coarse(A, P, R, nH)], P=[P], R=[R], owners=[o0, o1], part=1)


def _chain(seed=9):
    """three levels, 0 and 1 partitioned: P_0 has ghost columns in the level-1 space, R_1 yields the replicated level's rows"""
    n, n1, n2, W = 1100, 300, 60, 3
    rng = _rng(seed, n, 23)
    o = [scattered_owner(n, W, seed), scattered_owner(n1, W, seed + 1), scattered_owner(n2, W, seed + 2)]
    A0 = _values(split_rows(rng, o[0], o[0], rng.integers(0, 13, n), place_boundary(rng, o[0], ragged_lengths(rng, 200)), True), o[0], o[0], True, rng)
    A1 = _values(split_rows(rng, o[1], o[1], rng.integers(0, 9, n1), place_boundary(rng, o[1], ragged_lengths(rng, 70)), True), o[1], o[1], True, rng)
    P0 = _values(split_rows(rng, o[0], o[1], rng.integers(0, 4, n), place_boundary(rng, o[0], ragged_lengths(rng, 300, 1, 3), first=0), False), o[0], o[1], False, rng)
    R0 = _values(split_rows(rng, o[1], o[0], rng.integers(1, 9, n1), place_boundary(rng, o[1], ragged_lengths(rng, 100), first=0), False), o[1], o[0], False, rng)
    P1 = oe.rect_matrix(oe.tall_ragged(n1, n2, seed), n2)
    R1 = _values(split_rows(rng, o[2], o[1], rng.integers(1, 9, n2), place_boundary(rng, o[2], ragged_lengths(rng, 30), first=0), False), o[2], o[1], False, rng)
    return dict(name="chain", W=W, mats=[A0, A1, _coarse(A1, P1, R1, n2)], P=[P0, P1], R=[R0, R1], owners=o, part=2)


def _slabs(name):
    """Q1 3-D Poisson (poisson.py) on the cells of SLABS[name], two levels, z-slabs beginning at the node planes SLABS[name] lists:
    2 | 1 | 4 planes (slabs), 6 | 1 | 10 (slabs-16); the coarse planes go to the ranks in turn"""
    _, po = _mods()
    cells, cuts = SLABS[name]
    H = po.build_hierarchy(cells, 2, 1)
    sc = lambda M: oe._csr(M.val, M.idx, M.ptr, M.shape)
    nodes = [tuple(c - 1 for c in cc) for cc in H["ncells"]]
    z = np.arange(np.prod(nodes[0])) // (nodes[0][0] * nodes[0][1])
    o0 = (np.searchsorted(np.asarray(cuts), z, side="right") - 1).astype(np.int64)
    zc = np.arange(np.prod(nodes[1])) // (nodes[1][0] * nodes[1][1])
    o1 = (zc % 3).astype(np.int64)
    return dict(name=name, W=3, mats=[sc(H["mats"][0]), sc(H["mats"][1])], P=[sc(H["prolongations"][0])], R=[sc(H["restrictions"][0])],
                owners=[o0, o1], part=1)


def _global(name):
    if name.startswith("bnd-"):
        N = int(name.split("-")[1])
        rng = _rng(N, 24)
        return general_family(name, 900, R_BND[N] + 60, 3, ragged_lengths(rng, N), ragged_lengths(rng, R_BND[N]), seed=N)
    if name == "widths":
        return general_family(name, 1800, 1000, 5, oe.widths_lengths(WIDTHS, 1, least=1), oe.widths_lengths(WIDTHS, 2, least=1), seed=31)
    if name in ("dict-255", "dict-256"):
        rng = _rng(len(name), 25)
        return general_family(name, 700, 220, 2, ragged_lengths(rng, 100, 2, 6), ragged_lengths(rng, 100, 2, 6), seed=41, table=int(name[5:]))
    if name == "dict-256-nopad":
        return general_family(name, 700, 220, 2, np.full(128, 4), np.full(128, 3), seed=43, table=256)
    if name in ("fan-out", "patches"):
        return _fan_out(name)
    if name == "one-way":
        rng = _rng(7, 26)
        return general_family(name, 900, 140, 3, ragged_lengths(rng, 150), ragged_lengths(rng, 40), seed=51, may={0: [1], 1: [2], 2: [1]})
    if name == "uncoupled":
        return general_family(name, 600, 90, 3, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), seed=61)
    if name == "chain":
        return _chain()
    if name in SLABS:
        return _slabs(name)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ partition + fold
class Level:
    overlap = False


def _po_csr(po, M):
    return po.CSR(M.shape, M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data)


def _to_scipy(M):
    return oe._csr(M.val, M.idx, M.ptr, M.shape)


def patch_tables(G, seed=3):
    """ragged patches on level 0 of the fan-out family: 2 .. 12 dofs each, owned by the owner of their first dof; patches seeded at a
    hub take the hub's leaves (ghost dofs of up to four neighbours) and fill up with owned dofs; every dof lies in some patch"""
    A, o0 = G["mats"][0], G["owners"][0]
    n = A.shape[0]
    rng = _rng(seed, n, 27)
    pp, pd = [0], []
    cover = np.zeros(n, dtype=bool)
    order = rng.permutation(n)
    for i in order:
        c = A.indices[A.indptr[i]:A.indptr[i + 1]]
        cross = c[o0[c] != o0[i]]
        if cover[i] and cross.size == 0:
            continue
        size = int(rng.integers(2, 13))
        mine = np.flatnonzero(o0 == o0[i])
        extra = rng.choice(mine[mine != i], size=size, replace=False)
        dofs = [int(i)] + [int(q) for q in cross[:size - 1]]
        dofs += [int(q) for q in extra if int(q) not in dofs][:size - len(dofs)]
        pd.append(np.array(dofs, dtype=np.int64)); pp.append(pp[-1] + len(dofs))
        cover[dofs] = True
    pd = np.concatenate(pd)
    pp = np.asarray(pp, dtype=np.int64)
    powner = o0[pd[pp[:-1]]]
    return pp, pd, powner


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace(name, G (the global hierarchy), W, levels (folded), local (the local_hierarchy dict of DistributedGMG), spaces,
    folded, X (three level-0 vectors), XC (three per coarser level), x0, r0 -- vectors global, seeded in (-1, 1))"""
    dp, po = _mods()
    G = _global(name)
    W, part, nlev = G["W"], G["part"], len(G["mats"])
    V = [dp.Space("v%d" % l, G["owners"][l], W) for l in range(nlev)]
    ops = []
    for l in range(part):
        ops += [(G["mats"][l], V[l], V[l]), (G["R"][l], V[l + 1], V[l])]
        if l + 1 < part:
            ops.append((G["P"][l], V[l], V[l + 1]))
    pats, ptab = [], None
    if name == "patches":
        ptab = patch_tables(G)
        pats = [(ptab[0], ptab[1], V[0], ptab[2])]
    dp.partition_spaces(V, ops, pats)
    F = [dp.FoldedSpace(V[l]) for l in range(part)]
    R_ = range(W)
    levels = []
    rep_gid = np.zeros(0, dtype=np.int64)
    for l in range(nlev):
        L = Level()
        if l < part:
            F[l].plan_into(L)
            nc = F[l].n_own + F[l].n_ghost
            L.replicated, L.own_gid = False, F[l].own_gid
            L.A = dp.stack_rows([dp.local_operator(G["mats"][l], V[l], V[l], r) for r in R_], F[l].cmap, nc)
            L.R = dp.stack_rows([dp.local_operator(G["R"][l], V[l + 1], V[l], r) for r in R_], F[l].cmap, nc)
            if l + 1 < part:
                L.P = dp.stack_rows([dp.local_operator(G["P"][l], V[l], V[l + 1], r) for r in R_], F[l + 1].cmap, F[l + 1].n_own + F[l + 1].n_ghost)
            else:                                            # to the replicated level: global coarse columns, the ranks' coarse rows stacked
                Pg = G["P"][l].tocsr()[F[l].own_gid]
                Pg.sort_indices()
                L.P = _po_csr(po, Pg)
                rep_gid = np.concatenate([V[l + 1].own[r] for r in R_])
        else:
            L.replicated = True
            L.A = _po_csr(po, G["mats"][l])
            L.n_own, L.n_ghost = L.A.shape[0], 0
            L.own_gid = np.arange(L.n_own)
            if l + 1 < nlev:
                L.P, L.R = _po_csr(po, G["P"][l]), _po_csr(po, G["R"][l])
        levels.append(L)
    local = dict(levels=levels, rep_from=part, rep_gid=np.ascontiguousarray(rep_gid, dtype=np.int64), cells=[(1, 1)] * nlev, grid=(2, 1),
                 rank=0, nranks=2)
    out = types.SimpleNamespace(name=name, G=G, W=W, part=part, nlev=nlev, levels=levels, local=local, spaces=V, folded=F, rep_gid=rep_gid)
    rng = _rng(CASES.index(name), 28)
    sizes = [M.shape[0] for M in G["mats"]]
    out.X = [rng.uniform(-1, 1, sizes[0]) for _ in range(3)]
    out.XC = [[rng.uniform(-1, 1, sizes[l]) for _ in range(3)] for l in range(nlev)]
    out.XC[0] = out.X
    out.x0, out.r0 = rng.uniform(-1, 1, sizes[0]), rng.uniform(-1, 1, sizes[0])
    if ptab is not None:
        loc = [dp.local_patches(ptab[0], ptab[1], V[0], ptab[2], r, G["mats"][0]) for r in R_]
        ptr = np.concatenate([np.zeros(1, dtype=np.int64)] + [loc[r][0][1:] + sum(int(loc[q][0][-1]) for q in range(r)) for r in R_])
        out.patch = types.SimpleNamespace(pp=ptab[0], pd=ptab[1], owner=ptab[2], ptr=ptr,
                                          dofs=np.concatenate([F[0].cmap[r][loc[r][1]] for r in R_]).astype(np.int64),
                                          gdofs=np.concatenate([loc[r][2] for r in R_]).astype(np.int64),
                                          blocks=np.ascontiguousarray(np.concatenate([loc[r][3] for r in R_])))
    return out


def fill(L, x_own):
    """the folded local vector of a level from its owned entries: consistent!(v) through the level's self-exchange plan"""
    return np.concatenate([x_own, x_own[L.snd_idx]])


def own_vec(c, l, xg):
    """a global vector of level l in the order the device holds it: folded owned order, or global on a replicated level"""
    return np.ascontiguousarray(xg[c.levels[l].own_gid])


def operators(c, l):
    """[(key, folded matrix, n_own of its column space (None: the operator is never split -- P sums its whole row in storage order
    after the coarse vector's exchange), global matrix, level of the input vector, global ids of the output rows)] of partitioned
    level l"""
    L = c.levels[l]
    nxt = c.levels[l + 1]
    rows_R = c.rep_gid if nxt.replicated else nxt.own_gid
    return [("A", L.A, L.n_own, c.G["mats"][l], l, L.own_gid),
            ("P", L.P, None, c.G["P"][l], l + 1, L.own_gid),
            ("R", L.R, L.n_own, c.G["R"][l], l, rows_R)]


# ------------------------------------------------------------------------------------------------ census: build_ghost_fix restated
def ghost_part(M, n_own):
    """(own, ghost): the entries of the folded CSR M in columns < n_own / >= n_own, storage order kept, as scipy CSR"""
    S = _to_scipy(M) if not sp.issparse(M) else M
    g = S.indices >= n_own
    rowof = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    def take(m):
        ptr = np.concatenate([[0], np.cumsum(np.bincount(rowof[m], minlength=S.shape[0]))])
        return oe._csr(S.data[m], S.indices[m], ptr, S.shape)
    return take(~g), take(g)


def census(M, n_own, sell=True, use_dict=True):
    """what gmg_setup makes of the ghost columns of the folded operator M: rows (the boundary rows, ascending), lens, widths (per
    slice of 64), slots (64 * sum of widths), padded, distinct (doubles among the ghost entries), table (distinct + the padding
    zero when there are padded slots and no entry is 0.0), order (the table in the order build_ghost_fix meets the values: slot by
    slot), form: none / csr / sliced / sliced+dict"""
    _, gh = ghost_part(M, n_own)
    ln = np.diff(gh.indptr)
    rows = np.flatnonzero(ln > 0)
    lens = ln[rows]
    nb = rows.size
    widths = np.array([lens[s:s + 64].max() for s in range(0, nb, 64)], dtype=np.int64)
    slots = int(64 * widths.sum())
    padded = slots > int(lens.sum())
    order = []
    if nb:
        seen = set()
        for s, w in enumerate(widths):                      # slot order: slice, entry, lane
            q = rows[64 * s:64 * s + 64]
            for e in range(int(w)):
                for lane in range(64):
                    v = 0.0
                    if lane < q.size and e < ln[q[lane]]:
                        v = float(gh.data[gh.indptr[q[lane]] + e])
                    key = np.float64(v).view(np.uint64)
                    if key not in seen:
                        seen.add(key); order.append(v)
    distinct = int(np.unique(gh.data.view(np.uint64)).size)
    table = len(order)
    form = "none" if nb == 0 else "csr" if not sell else "sliced+dict" if (use_dict and table <= 256) else "sliced"
    return types.SimpleNamespace(rows=rows, lens=lens, widths=widths, slots=slots, padded=padded, distinct=distinct, table=table,
                                 order=np.array(order), form=form, entries=int(lens.sum()), nb=int(nb))


def send_multiplicity(L):
    """send slots per owned row of a folded level"""
    return np.bincount(np.asarray(L.snd_idx, dtype=np.int64), minlength=L.n_own)


def fusable(L):
    """the rule of gmg_setup: the pack is fused into the fix-up when every sent row is a boundary row (and there is one)"""
    cz = census(L.A, L.n_own)
    return cz.nb > 0 and bool(np.all(np.isin(np.asarray(L.snd_idx), cz.rows)))


def expected_halo_info(c, l, options=None):
    """gmg_get_halo_info of partitioned level l under `options` (halo_* keys as gmg_set_option takes them)"""
    o = dict(halo_fix_sell=1, halo_fix_dict=1, halo_fuse_pack=1, halo_split_r=1)
    o.update({k: v for k, v in (options or {}).items() if k in o})
    L = c.levels[l]
    a = census(L.A, L.n_own, bool(o["halo_fix_sell"]), bool(o["halo_fix_dict"]))
    r = census(L.R, L.n_own, True, bool(o["halo_fix_dict"]))
    split = bool(o["halo_split_r"])
    return dict(boundary_rows=a.nb, send_slots=int(L.snd_ptr[-1]), ghost_entries=a.entries, fix_form=a.form,
                dict_values=a.table if a.form == "sliced+dict" else 0, pack_fused=bool(o["halo_fuse_pack"]) and fusable(L), r_split=split,
                r_boundary_rows=r.nb if split else 0, r_ghost_entries=r.entries if split else 0, r_form=r.form if split else "none",
                r_dict_values=r.table if split and r.form == "sliced+dict" else 0)


# ------------------------------------------------------------------------------------------------ references and twins
def twin_apply(M, n_own, v, split=True, ghost=None):
    """float64 twin of a split mat-vec on the folded vector v: own-column sum in storage order, ghost-column sum in storage order
    from 0.0, own + ghost on the rows that have ghost entries.  split = False: the whole row in storage order (an unsplit R).
    ghost: another ghost part (a corruption)."""
    S = _to_scipy(M)
    if n_own is None or not split:
        return oe.seq_spmv(S, v)
    own, gh = ghost_part(S, n_own)
    y = oe.seq_spmv(own, v)
    b = np.diff(gh.indptr) > 0
    g = oe.seq_spmv(gh if ghost is None else ghost, v)
    y[b] = y[b] + g[b]
    return y


def exact_rows(Mg, rows, xg):
    """fullsize_reference.row_reference of the rows `rows` of the GLOBAL matrix -> (seq, exact, bound)"""
    seq, exact, bound = oe.row_reference_all(Mg.tocsr(), xg)
    return seq[rows], exact[rows], bound[rows]


def ref_sweeps(c, k, l=0):
    """k Richardson(Jacobi) sweeps in longdouble on the global matrix -> (x, r) in the folded owned order"""
    x, r = oe.ref_sweeps(c.G["mats"][l], c.x0, c.r0, k)
    g = c.levels[l].own_gid
    return x[g], r[g]


def twin_sweeps(c, k, l=0, omega=OMEGA, first_slot_only=False):
    """the float64 twin of k sweeps on the folded level: s = omega * (dinv * r), x + s, r - (own sum), then - (ghost sum from 0.0) on
    the boundary rows.  first_slot_only: the corruption of the fused pack (see CORRUPTIONS)."""
    L = c.levels[l]
    S = _to_scipy(L.A)
    own, gh = ghost_part(S, L.n_own)
    b = np.diff(gh.indptr) > 0
    dinv = 1.0 / c.G["mats"][l].diagonal()[L.own_gid]
    x, r = own_vec(c, l, c.x0), own_vec(c, l, c.r0)
    snd = np.asarray(L.snd_idx, dtype=np.int64)
    first = np.zeros(snd.size, dtype=bool)
    first[np.unique(snd, return_index=True)[1]] = True
    ghost = np.zeros(snd.size)
    for it in range(k):
        s = omega * (dinv * r)
        fresh = s[snd]
        ghost = np.where(first | (it == 0), fresh, ghost) if first_slot_only else fresh
        v = np.concatenate([s, ghost])
        x = x + s
        r = r - oe.seq_spmv(own, v)
        r[b] = r[b] - oe.seq_spmv(gh, v)[b]
    return x, r


def patch_contributions(c, r_own, exact=False):
    """per patch (in the folded order of the ranks' owned patches) the local solve A_p^-1 r_p on a consistent r: the float64 twin
    of the device's explicit inverse (patch_edge_problems.twin_inverse, row . vector summed in column order), or with exact = True
    the pivoted LU in longdouble"""
    import patch_edge_problems as pe
    p, L = c.patch, c.levels[0]
    v = fill(L, np.asarray(r_own, dtype=np.float64))
    out = []
    at = 0
    for k in range(p.ptr.size - 1):
        d = p.dofs[p.ptr[k]:p.ptr[k + 1]]
        m = d.size
        B = p.blocks[at:at + m * m].reshape(m, m, order="F")
        at += m * m
        if exact:
            out.append(pe._lu_solve(pe._factor(B, True), v[d]))
        else:
            X = pe.twin_inverse(B, True)
            y = np.zeros(m)
            for j in range(m):
                y += X[:, j] * v[d][j]
            out.append(y)
    return out


def assemble(c, contrib, dtype=np.float64, only_first_neighbour=False):
    """assemble!(dx) of per-patch contributions: every owned dof takes the contributions of its rank's patches in patch order, then
    the ghost copies' sums message by message (the order of the halo_unpack_add_kernel launches); dtype longdouble: the reference
    sum.  only_first_neighbour: the corruption -- a dof keeps the first arriving message's contribution only."""
    p, L = c.patch, c.levels[0]
    loc = np.zeros(L.n_own + L.n_ghost, dtype=dtype)
    for k, y in enumerate(contrib):
        d = p.dofs[p.ptr[k]:p.ptr[k + 1]]
        for a in range(d.size):
            loc[d[a]] = loc[d[a]] + y[a]
    out = loc[:L.n_own].copy()
    snd = np.asarray(L.snd_idx, dtype=np.int64)
    got = np.zeros(L.n_own, dtype=bool)
    for m in range(len(L.snd_ptr) - 1):                    # message m: ghost segment m arrives at the rows of send segment m
        s0, s1 = int(L.snd_ptr[m]), int(L.snd_ptr[m + 1])
        for j in range(s0, s1):
            if only_first_neighbour and got[snd[j]]:
                continue
            out[snd[j]] = out[snd[j]] + loc[L.n_own + j]
            got[snd[j]] = True
    return out


def contributions_per_dof(c):
    """neighbour messages that carry a nonzero contribution, per owned dof of the patches family"""
    p, L = c.patch, c.levels[0]
    touched = np.zeros(L.n_own + L.n_ghost, dtype=bool)
    touched[p.dofs] = True
    snd = np.asarray(L.snd_idx, dtype=np.int64)
    return np.bincount(snd[touched[L.n_own:]], minlength=L.n_own)


# ------------------------------------------------------------------------------------------------ the gates (host and device alike)
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def bit_mismatches(y, twin):
    """rows whose bits differ from the twin's"""
    return np.flatnonzero(bits(y) != bits(twin))


def bound_violations(y, ref):
    """rows beyond gamma_k * sum|a x| of the exact value (a non-finite row counts); ref = (seq, exact, bound)"""
    return np.flatnonzero(~(np.abs(np.asarray(y, dtype=np.float64) - ref[1]) <= ref[2]))


def bound_fraction(y, ref):
    dev = np.abs(np.asarray(y, dtype=np.float64) - ref[1])
    return float(np.max(np.where(ref[2] > 0, dev / np.maximum(ref[2], 1e-300), 0.0))) if dev.size else 0.0


def inf_violations(y_inf, y_finite, skip_row0):
    """x[0] = inf: rows (but row 0 of A) that are not finite or changed their bits"""
    bad = ~np.isfinite(y_inf) | (bits(y_inf) != bits(y_finite))
    if skip_row0:
        bad[0] = False
    return np.flatnonzero(bad)


# ------------------------------------------------------------------------------------------------ corruptions (host only)
def _edit_ghost(gh, keep):
    rowof = np.repeat(np.arange(gh.shape[0]), np.diff(gh.indptr))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rowof[keep], minlength=gh.shape[0]))])
    return oe._csr(gh.data[keep], gh.indices[keep], ptr, gh.shape)


def _slice_of(cz, nrows):
    s = -np.ones(nrows, dtype=np.int64)
    s[cz.rows] = np.arange(cz.nb) // 64
    return s


def drop_quad_tail(c, key, M, n_own, v):
    """ghost_fix_sell_kernel without its remainder loop: entries 4 * (w // 4) .. w - 1 of every row of a slice of width w are lost"""
    _, gh = ghost_part(M, n_own)
    cz = census(M, n_own)
    sl = _slice_of(cz, gh.shape[0])
    rowof = np.repeat(np.arange(gh.shape[0]), np.diff(gh.indptr))
    e = np.arange(gh.indices.size) - gh.indptr[rowof]
    keep = e < 4 * (cz.widths[sl[rowof]] // 4)
    return twin_apply(M, n_own, v, ghost=_edit_ghost(gh, keep))


def add_padded_products(c, key, M, n_own, v):
    """the fix-up without the row-length mask: a row shorter than its slice adds 0.0 * v[0] per padded slot"""
    y = twin_apply(M, n_own, v)
    cz = census(M, n_own)
    short = cz.rows[cz.lens < cz.widths[np.arange(cz.nb) // 64]]
    with np.errstate(invalid="ignore"):
        y[short] = y[short] + 0.0 * v[0]
    return y


def skip_last_slice(c, key, M, n_own, v):
    """the fix-up launched over whole slices only: the rows of a ragged last slice keep their own-column sum"""
    cz = census(M, n_own)
    _, gh = ghost_part(M, n_own)
    rowof = np.repeat(np.arange(gh.shape[0]), np.diff(gh.indptr))
    last = cz.rows[64 * (cz.nb // 64):] if cz.nb % 64 else np.zeros(0, dtype=np.int64)
    return twin_apply(M, n_own, v, ghost=_edit_ghost(gh, ~np.isin(rowof, last)))


def wrap_codes(c, key, M, n_own, v):
    """build_ghost_fix keeping the dictionary with 257 table entries: the one-byte code of entry 256 wraps to entry 0"""
    cz = census(M, n_own)
    _, gh = ghost_part(M, n_own)
    data = gh.data.copy()
    for k in range(256, cz.table):
        data[gh.data == cz.order[k]] = cz.order[k % 256]
    return twin_apply(M, n_own, v, ghost=oe._csr(data, gh.indices, gh.indptr, gh.shape))


def stale_ghosts(c, key, M, n_own, v, previous):
    """the exchange omitted: the ghost segment still holds the previous vector's values (zeros before the first)"""
    w = v.copy()
    w[n_own:] = previous[n_own:] if previous is not None else 0.0
    return twin_apply(M, n_own, w)


# name -> (family, kind, function): kind "op" corrupts y = M v of A and R (gates: the twin's bits, the gamma_k bound), "inf" the same
# on a vector with x[0] = inf (gate: all rows but row 0 finite and unchanged), "stale" the second and third vector of a sequence,
# "sweeps" k >= 2 sweeps (gates: the twin's bits, TOL_KERNEL against ref_sweeps), "assemble" the patch smoother's dx
CORRUPTIONS = {
    "drop_quad_tail": ("widths", "op", drop_quad_tail),
    "add_padded_products": ("widths", "inf", add_padded_products),
    "skip_last_slice": ("bnd-65", "op", skip_last_slice),
    "wrap_codes": ("dict-256", "op", wrap_codes),
    "stale_ghosts": ("fan-out", "stale", stale_ghosts),
    "first_send_slot_only": ("fan-out", "sweeps", lambda c, k: twin_sweeps(c, k, first_slot_only=True)),
    "one_neighbour_only": ("patches", "assemble", lambda c, contrib: assemble(c, contrib, only_first_neighbour=True)),
}
