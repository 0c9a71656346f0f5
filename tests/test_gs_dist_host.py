"""Host side of the Gauss-Seidel smoother on partitioned levels (tests/gs_dist_reference.py): the literal per-rank form against the
global form with the cross-rank entries removed, one rank against gs_reference.solve, the level sets and the multicolour order of a
folded own block against the ranks' own, the twin of the library's sums against the reference, and the argument checks of
DistributedGMG that need no device."""
import importlib

import numpy as np
import pytest

import fullsize_reference as fr
import gs_dist_reference as gd
import gs_ordering_reference as go
import gs_reference as gr
import halo_edge_problems as he
import operator_edge_problems as oe

CASES = ("bnd-1", "bnd-65", "one-way", "uncoupled", "fan-out", "dict-255", "gs-edge")
PARAMS = [("symmetric", 1.0), ("forward", 1.2), ("backward", 1.0), ("symmetric", 1.2)]


def _global(name):
    c = gd.edge_case() if name == "gs-edge" else he.case(name)
    Af, blocks, perm = gd.folded(c.G["mats"][0], c.G["owners"][0])
    return c, Af, blocks, perm


def _rank_orders(blocks, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(int(np.count_nonzero(blocks == q))) for q in range(int(blocks.max()) + 1)]


def _stack(orders):
    off = np.concatenate([[0], np.cumsum([o.size for o in orders])])
    return np.concatenate([off[q] + o for q, o in enumerate(orders)])


@pytest.mark.parametrize("name", CASES)
def test_own_first_numbering_is_the_folded_partitions(name):
    """folded(A, owner) is the matrix whose owned rows the folded level holds: same row order, and the level's own x own block is the
    block part, entry for entry"""
    c, Af, blocks, perm = _global(name)
    L = c.levels[0]
    assert np.array_equal(perm, L.own_gid)
    counts = [len(c.spaces[0].own[q]) for q in range(c.W)]
    assert np.array_equal(blocks, gd.blocks_of(counts))
    T, B = gd.own_block(L), gd.block_part(Af, blocks)
    T.sort_indices()
    assert np.array_equal(T.indptr, B.indptr) and np.array_equal(T.indices, B.indices) and np.array_equal(T.data, B.data)


@pytest.mark.parametrize("type_,omega", PARAMS)
@pytest.mark.parametrize("name", CASES)
def test_per_rank_form_and_global_form_are_bitwise_equal(name, type_, omega):
    c, Af, blocks, _ = _global(name)
    sm = gr.GS(2, omega, type_)
    g = c.levels[0].own_gid
    for orders in (None, _rank_orders(blocks, 5)):
        xa, ra = c.x0[g].copy(), c.r0[g].copy()
        xb, rb = xa.copy(), ra.copy()
        gd.solve_ranks(xa, Af, blocks, sm, ra, orders)
        gd.solve_blocks(xb, Af, blocks, sm, rb, "natural" if orders is None else _stack(orders))
        assert np.array_equal(xa, xb) and np.array_equal(ra, rb)
        assert np.all(np.isfinite(xa)) and not np.array_equal(xa, c.x0[g])


def test_edge_family_has_a_one_row_rank_and_a_rank_without_boundary_rows():
    c, Af, blocks, _ = _global("gs-edge")
    L = c.levels[0]
    counts = np.bincount(blocks)
    bnd = np.bincount(blocks[he.census(L.A, L.n_own).rows], minlength=c.W)
    sent = np.bincount(blocks[np.unique(L.snd_idx)], minlength=c.W)
    assert c.W == 4 and counts[3] == 1 and bnd[3] == 1          # a rank whose own block is one row, coupled to other ranks
    assert bnd[2] == 0 and sent[2] > 0 and not he.fusable(L)    # a rank without boundary rows whose rows are sent: the pack cannot fuse


@pytest.mark.parametrize("type_,omega", PARAMS)
def test_one_rank_is_the_reference_solve(type_, omega):
    c, Af, blocks, _ = _global("bnd-65")
    one = np.zeros_like(blocks)
    sm = gr.GS(2, omega, type_)
    g = c.levels[0].own_gid
    want_x, want_r = c.x0[g].copy(), c.r0[g].copy()
    gr.solve(want_x, sm.setup(Af), sm, want_r)
    for fn in (gd.solve_ranks, gd.solve_blocks):
        x, r = c.x0[g].copy(), c.r0[g].copy()
        fn(x, Af, one, sm, r)
        assert np.array_equal(x, want_x) and np.array_equal(r, want_r)
    # ... and more than one rank is another method wherever a cross-rank entry exists
    x, r = c.x0[g].copy(), c.r0[g].copy()
    gd.solve_blocks(x, Af, blocks, sm, r)
    assert not np.array_equal(x, want_x)


@pytest.mark.parametrize("forward", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_level_sets_of_the_folded_block_are_the_union_of_the_ranks(name, forward):
    c, Af, blocks, _ = _global(name)
    s = gr.level_sets(gd.own_block(c.levels[0]), forward)
    for q in range(c.W):
        M, own, _ = gd.local_matrix(Af, blocks, q)
        mine = gr.level_sets(M[:, :own.size], forward)
        assert np.array_equal(s[own], mine)


@pytest.mark.parametrize("name", CASES)
def test_multicolour_order_of_the_folded_block_is_a_colouring_per_rank(name):
    c, Af, blocks, _ = _global(name)
    T = gd.own_block(c.levels[0])
    order, color = go.multicolor(T)
    assert np.array_equal(np.sort(order), np.arange(T.shape[0]))
    for q in range(c.W):
        M, own, _ = gd.local_matrix(Af, blocks, q)
        S = go.symmetrised_pattern(M[:, :own.size])
        rowof = np.repeat(np.arange(own.size), np.diff(S.indptr))
        off = rowof != S.indices
        assert np.all(color[own][rowof[off]] != color[own][S.indices[off]])      # neighbours inside the rank differ in colour
        assert np.array_equal(color[own], go.greedy_colors(M[:, :own.size]))        # ... and it is the rank's own greedy colouring
        mine = order[np.isin(order, own)]                                           # the rank's rows in visiting order
        assert np.array_equal(mine, own[go.multicolor(M[:, :own.size])[0]])


@pytest.mark.parametrize("type_,omega", PARAMS)
@pytest.mark.parametrize("name", ("bnd-65", "one-way", "fan-out"))
def test_twin_of_the_library_sums(name, type_, omega):
    """own-column sum, then the ghost part: the triangular solves are bitwise the reference's, the pass within rounding of it"""
    c, Af, blocks, _ = _global(name)
    L = c.levels[0]
    g = L.own_gid
    sm = gr.GS(3, omega, type_)
    for ordering in ("natural", "multicolor"):
        order = go.resolve(gd.own_block(L), ordering)
        tx, tr, first = gd.twin_pass(L, sm, c.x0[g], c.r0[g], order)
        assert np.array_equal(first, gd.first_dx(Af, blocks, c.r0[g], type_ != "backward", ordering))
        x, r = c.x0[g].copy(), c.r0[g].copy()
        gd.solve_blocks(x, Af, blocks, sm, r, ordering)
        assert oe.max_rel(tx, x) <= fr.TOL_KERNEL and oe.max_rel(tr, r) <= fr.TOL_KERNEL


def test_overlapping_layout_is_refused_before_any_handle(pkg):
    mg = importlib.import_module(pkg.__name__ + ".multigpu")
    sv = importlib.import_module(pkg.__name__ + ".solvers")
    for kw in (dict(depth=2), dict(depth=[0, 2, 0]), dict(finest_depth=1)):
        with pytest.raises(ValueError, match="own . ghost layout"):
            mg.DistributedGMG((8, 8), 3, 0, 4, transport="host_loopback", smoother=sv.GaussSeidelSmoother(), **kw)
    with pytest.raises(ValueError, match="gs_orders"):
        mg.DistributedGMG((8, 8), 3, 0, 4, transport="host_loopback", smoother=sv.GaussSeidelSmoother(ordering=np.arange(4)))
    with pytest.raises(ValueError, match="gs_orders"):
        mg.DistributedGMG((8, 8), 3, 0, 4, transport="host_loopback", smoother="jacobi", gs_orders=[np.arange(4)])
