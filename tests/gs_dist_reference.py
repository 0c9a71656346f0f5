"""numpy / scipy restatement of the Gauss-Seidel smoother on a partitioned level (rank-block Gauss-Seidel, csrc/gs.inc.hpp; the
reference's distributed form: SymGaussSeidelSmoothers.jl:155-165 with :71-75 / :93-97 -- DiagonalIndices of the local matrix over
own_to_local(indices), forward_sub! / backward_sub! on own_values(x), mul!(Adx, A, dx) the distributed product).  Plain helper: numpy
and scipy only, no fixtures, no collection hooks.

Everything works on a GLOBAL matrix in OWN-FIRST NUMBERING PER RANK: the rows of rank 0, then those of rank 1, ... (what a partition
folded onto one rank holds as its owned rows); `blocks[i]` is the rank that owns row i.

  folded(A, owner)                 -> (Af, blocks, perm): A in that numbering (by rank, then by id), stored zeros kept
  block_part(Af, blocks)           Af with every cross-rank entry removed: the own x own blocks on the diagonal
  local_matrix(Af, blocks, rank)   the rank's n_own x (n_own + n_ghost) matrix, ghost columns in ascending global id
  solve_ranks                      (a) the literal per-rank form: gs_reference.diagonal_indices of the local CSC restricted to its
                                   n_own columns, forward_sub / backward_sub on the owned entries, the product the global A @ dx
  BlockGS / solve_blocks           (b) the global form: gs_reference's column loops with the triangles of block_part(Af), the product
                                   with Af itself; smoother object of gs_reference.GMG (blocks = None: a replicated level, global sweeps)
  first_dx                         the dx of the first direction of (b): what the triangular solve alone produces
  twin_pass                        the whole pass on a FOLDED level as the library sums it: triangular solves row by row in table
                                   order, r -= (own-column sum in storage order), then -= (ghost-column sum from 0.0) on the boundary
                                   rows -- the arithmetic of halo_edge_problems.twin_apply / twin_sweeps with the fix-up in mode 1
  own_block(L)                     the own x own block of a folded level's local matrix, as the library cuts it
  folded_hierarchy                 the global hierarchy renumbered level by level into the folded order of a folded partition
  edge_case                        a halo_edge_problems-style family of its own (W = 4): a rank whose own block is ONE row (with
                                   ghost columns, and sent to others), a rank WITHOUT boundary rows whose rows are sent all the same
                                   (the pack cannot fuse), two ragged ranks
"""
import functools
import types

import numpy as np
import scipy.sparse as sp

import gs_ordering_reference as go
import gs_reference as gr
import halo_edge_problems as he
import operator_edge_problems as oe


def _kept(A, keep):
    """the stored entries `keep` of the sorted CSR A (explicit zeros stay)"""
    rowof = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rowof[keep], minlength=A.shape[0]))])
    return sp.csr_matrix((A.data[keep], A.indices[keep], ptr), shape=A.shape)


def folded(A, owner):
    owner = np.asarray(owner, dtype=np.int64)
    perm = np.lexsort((np.arange(owner.size), owner))
    return go.permuted(A, perm), owner[perm], perm


def block_part(Af, blocks):
    A = go._csr_copy(Af)
    rowof = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return _kept(A, blocks[rowof] == blocks[A.indices])


def local_matrix(Af, blocks, rank):
    """-> (sorted CSR n_own x (n_own + n_ghost), own ids, ghost ids)"""
    A = go._csr_copy(Af)
    own = np.flatnonzero(blocks == rank)
    S = A[own]
    S.sort_indices()
    cols = np.unique(S.indices)
    ghost = cols[blocks[cols] != rank]
    cmap = -np.ones(A.shape[0], dtype=np.int64)
    cmap[own] = np.arange(own.size)
    cmap[ghost] = own.size + np.arange(ghost.size)
    M = sp.csr_matrix((S.data, cmap[S.indices], S.indptr), shape=(own.size, own.size + ghost.size))
    M.sort_indices()
    return M, own, ghost


def _permute_local(M, order):
    """the local matrix with its owned rows and owned columns in the order `order` (ghost columns stay)"""
    n = M.shape[0]
    pos = np.arange(M.shape[1])
    pos[np.asarray(order)] = np.arange(n)
    lens = np.diff(M.indptr)[order]
    ptr = np.concatenate([[0], np.cumsum(lens)])
    src = np.repeat(M.indptr[order] - ptr[:-1], lens) + np.arange(ptr[-1])
    B = sp.csr_matrix((M.data[src], pos[M.indices[src]], ptr), shape=M.shape)
    B.sort_indices()
    return B


def solve_ranks(x, Af, blocks, sm, r, orders=None):
    """(a) solve!(x, ns, r) rank by rank, literally; orders[rank]: the rank's visiting order of its owned rows (None: natural)"""
    A = go._csr_copy(Af)
    W = int(blocks.max()) + 1
    ns = []
    for q in range(W):
        M, own, _ = local_matrix(A, blocks, q)
        order = np.arange(own.size) if orders is None or orders[q] is None else np.asarray(orders[q], dtype=np.int64)
        C = gr.csc(_permute_local(M, order))
        diag, last = gr.diagonal_indices(C)                  # min(shape) = n_own columns; last[col] stops at the last owned row
        ns.append((own[order], C, diag, last))
    for _ in range(sm.niter):
        for kind in ("forward", "backward"):
            if sm.type not in (kind, "symmetric"):
                continue
            dx = np.zeros_like(r)
            for rows, C, diag, last in ns:
                t = r[rows]                                  # copy!(dx, r) on own_values
                dx[rows] = gr.forward_sub(C, diag, last, t) if kind == "forward" else gr.backward_sub(C, diag, t)
            dx = sm.omega * dx
            x += dx
            r -= A @ dx
    return x


class BlockGS(go.OrderedGS):
    """(b) GaussSeidelSmoother(niter, omega, type) whose triangles are those of A with every cross-rank entry removed; blocks = None:
    the triangles of A itself.  ordering: "natural" | "multicolor" | a permutation of all rows (of the block part)"""

    def __init__(self, niter=1, omega=1.0, type="symmetric", ordering="natural", blocks=None):
        super().__init__(niter, omega, type, ordering)
        self.blocks = None if blocks is None else np.asarray(blocks, dtype=np.int64)

    def triangles(self, A):
        return go._csr_copy(A) if self.blocks is None else block_part(A, self.blocks)

    def setup(self, A):
        A = go._csr_copy(A)
        T = self.triangles(A)
        order = go.resolve(T, self.ordering)
        return (A, order) + gr.GS().setup(go.permuted(T, order))


def solve_blocks(x, Af, blocks, sm, r, ordering="natural"):
    """(b) as a function: gs_reference.solve with the triangles of block_part(Af, blocks)"""
    s = BlockGS(sm.niter, sm.omega, sm.type, ordering, blocks)
    s.smooth(s.setup(Af), x, r)
    return x


def first_dx(Af, blocks, r, forward, ordering="natural"):
    """dx = T \\ r of one direction of (b), before omega"""
    s = BlockGS(1, 1.0, "forward" if forward else "backward", ordering, blocks)
    _, order, B, diag, last = s.setup(Af)
    t = np.array(r[order], dtype=np.float64)
    t = gr.forward_sub(B, diag, last, t) if forward else gr.backward_sub(B, diag, t)
    dx = np.empty_like(t)
    dx[order] = t
    return dx


def own_block(L):
    """the own x own block of the folded level L: rows as stored, the columns below n_own (stored zeros kept, storage order)"""
    own, _ = he.ghost_part(L.A, L.n_own)
    return sp.csr_matrix((own.data, own.indices, own.indptr), shape=(L.n_own, L.n_own))


def blocks_of(counts):
    """rank of every owned row of a folded level from the ranks' owned-row counts (FoldedSpace / fold_ranks stack the ranks' owned
    rows in rank order)"""
    counts = np.asarray(counts, dtype=np.int64)
    return np.repeat(np.arange(counts.size), counts)


def twin_pass(L, sm, x_own, r_own, order=None):
    """the float64 twin of a whole pass on the folded level L -> (x, r, first dx before omega)"""
    S = he._to_scipy(L.A)
    own, gh = he.ghost_part(S, L.n_own)
    b = np.diff(gh.indptr) > 0
    T = own_block(L)
    order = np.arange(L.n_own) if order is None else np.asarray(order, dtype=np.int64)
    B = go.permuted(T, order)
    x, r = np.array(x_own, dtype=np.float64), np.array(r_own, dtype=np.float64)
    first = None
    for _ in range(sm.niter):
        for kind in ("forward", "backward"):
            if sm.type not in (kind, "symmetric"):
                continue
            dx = np.empty_like(r)
            dx[order] = gr.forward_rows(B, r[order]) if kind == "forward" else gr.backward_rows(B, r[order])
            if first is None:
                first = dx.copy()
            dx = sm.omega * dx
            x = x + dx
            v = he.fill(L, dx)                               # consistent!(dx)
            r = r - oe.seq_spmv(own, v)                      # own columns, storage order
            r[b] = r[b] - oe.seq_spmv(gh, v)[b]              # the boundary fix-up, mode 1
    return x, r, first


def folded_hierarchy(H, levels):
    """the global hierarchy H (dict of poisson.build_hierarchy: mats, prolongations, restrictions as objects with to_scipy) in the
    numbering of the folded levels: level l by levels[l].own_gid (the identity on replicated levels) -> (mats, Ps, Rs) as scipy CSR"""
    g = [np.asarray(L.own_gid, dtype=np.int64) for L in levels]
    sc = lambda M: go._csr_copy(M.to_scipy() if hasattr(M, "to_scipy") else M)
    mats = [go.permuted(sc(M), g[l]) for l, M in enumerate(H["mats"])]
    Ps = [sc(P)[g[l]][:, g[l + 1]].tocsr() for l, P in enumerate(H["prolongations"])]
    Rs = [sc(R)[g[l + 1]][:, g[l]].tocsr() for l, R in enumerate(H["restrictions"])]
    for M in Ps + Rs:
        M.sort_indices()
    return mats, Ps, Rs


def build_case(G):
    """halo_edge_problems.case for a global hierarchy G of two levels that is not one of its named families (level 0 partitioned,
    the coarse level replicated): the same namespace"""
    dp, po = he._mods()
    W, nlev = G["W"], len(G["mats"])
    assert G["part"] == 1 and nlev == 2
    V = [dp.Space("v%d" % l, G["owners"][l], W) for l in range(nlev)]
    dp.partition_spaces(V, [(G["mats"][0], V[0], V[0]), (G["R"][0], V[1], V[0])], [])
    F = dp.FoldedSpace(V[0])
    R_ = range(W)
    L = he.Level()
    F.plan_into(L)
    nc = F.n_own + F.n_ghost
    L.replicated, L.own_gid = False, F.own_gid
    L.A = dp.stack_rows([dp.local_operator(G["mats"][0], V[0], V[0], r) for r in R_], F.cmap, nc)
    L.R = dp.stack_rows([dp.local_operator(G["R"][0], V[1], V[0], r) for r in R_], F.cmap, nc)
    Pg = G["P"][0].tocsr()[F.own_gid]
    Pg.sort_indices()
    L.P = he._po_csr(po, Pg)
    rep_gid = np.ascontiguousarray(np.concatenate([V[1].own[r] for r in R_]), dtype=np.int64)
    C = he.Level()
    C.replicated = True
    C.A = he._po_csr(po, G["mats"][1])
    C.n_own, C.n_ghost = C.A.shape[0], 0
    C.own_gid = np.arange(C.n_own)
    levels = [L, C]
    local = dict(levels=levels, rep_from=1, rep_gid=rep_gid, cells=[(1, 1)] * nlev, grid=(2, 1), rank=0, nranks=2)
    out = types.SimpleNamespace(name=G["name"], G=G, W=W, part=1, nlev=nlev, levels=levels, local=local, spaces=V, folded=[F], rep_gid=rep_gid)
    rng = he._rng(len(G["name"]), G["mats"][0].shape[0], 30)
    n = G["mats"][0].shape[0]
    out.x0, out.r0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return out


@functools.lru_cache(maxsize=None)
def edge_case():
    n, nH, W, seed = 520, 80, 4, 77
    rng = he._rng(seed, n, nH, 29)
    o0 = rng.integers(0, 3, n).astype(np.int64)
    o0[:3] = np.arange(3)
    o0[11] = 3                                               # rank 3 owns this dof alone
    o1 = he.scattered_owner(nH, W, seed + 1)
    gl = np.zeros(n, dtype=np.int64)
    cand = np.flatnonzero((o0 != 2) & (np.arange(n) > 0))    # rank 2: no ghost column in any row
    rows = rng.choice(cand, size=130, replace=False)
    gl[rows] = rng.integers(1, 6, rows.size)
    gl[11] = 3
    A = he._values(he.split_rows(rng, o0, o0, rng.integers(0, 9, n), gl, True), o0, o0, True, rng)
    R = he._values(he.split_rows(rng, o1, o0, rng.integers(1, 9, nH), he.place_boundary(rng, o1, he.ragged_lengths(rng, 30), first=0), False),
                   o1, o0, False, rng)
    P = oe.rect_matrix(oe.tall_ragged(n, nH, seed), nH)
    return build_case(dict(name="gs-edge", W=W, mats=[A, he._coarse(A, P, R, nH)], P=[P], R=[R], owners=[o0, o1], part=1))
