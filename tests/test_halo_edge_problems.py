"""Host checks of tests/halo_edge_problems.py (no GPU): the census every family was built for, the folded operators against the
global ones, the float64 twin inside the exact reference's bound on every row, and every CORRUPTION leaving the gates that
tests/test_gpu_halo_edges.py applies to the device -- the twin's bits, the gamma_k bound of fullsize_reference.row_reference,
fr.TOL_KERNEL against the longdouble sweeps -- on the family built for it, while the uncorrupted twin passes them."""
import numpy as np
import pytest

import fullsize_reference as fr
import halo_edge_problems as he
import operator_edge_problems as oe


def _slices(cz):
    return [cz.lens[s:s + 64] for s in range(0, cz.nb, 64)]


# ---------------------------------------------------------------- census
@pytest.mark.parametrize("N", he.BND)
def test_bnd_families_have_exactly_n_boundary_rows(pkg, N):
    c = he.case("bnd-%d" % N)
    L = c.levels[0]
    for cz, want in ((he.census(L.A, L.n_own), N), (he.census(L.R, L.n_own), he.R_BND[N])):
        assert cz.nb == want and cz.widths.size == (want + 63) // 64
        for ln in _slices(cz):
            assert ln.size < 2 or ln.min() < ln.max(), "ghost-row lengths ragged inside every slice"
        assert (cz.nb % 64 != 0) == (want not in (64, 256)), "ragged last slice"
    assert not np.array_equal(np.sort(c.G["owners"][0]), c.G["owners"][0]), "owner map is not a set of contiguous blocks"
    info = he.expected_halo_info(c, 0)
    assert info["boundary_rows"] == N and info["r_boundary_rows"] == he.R_BND[N] and info["r_split"]


def test_widths_family_has_one_slice_per_width_with_short_and_long_lanes(pkg):
    c = he.case("widths")
    L = c.levels[0]
    for M in (L.A, L.R):
        cz = he.census(M, L.n_own)
        assert tuple(cz.widths) == he.WIDTHS and cz.nb == 64 * len(he.WIDTHS)
        for w, ln in zip(he.WIDTHS, _slices(cz)):
            assert ln.max() == w and ln.min() >= 1 and (w == 1 or np.any(ln == w - 1))
        assert {int(w) % 4 for w in cz.widths} == {0, 1, 2, 3}
        for w, ln in zip(he.WIDTHS, _slices(cz)):             # lanes that end before, and lanes that reach into, the last quad / the tail
            if w >= 5:
                assert np.any(ln <= 4 * ((w - 1) // 4)) and np.any(ln > 4 * ((w - 1) // 4))


@pytest.mark.parametrize("name,distinct,table,padded,form", [("dict-255", 255, 256, True, "sliced+dict"), ("dict-256", 256, 257, True, "sliced"),
                                                              ("dict-256-nopad", 256, 256, False, "sliced+dict")])
def test_dict_families_count_the_padding_zero(pkg, name, distinct, table, padded, form):
    c = he.case(name)
    L = c.levels[0]
    for M in (L.A, L.R):
        cz = he.census(M, L.n_own)
        assert (cz.distinct, cz.table, cz.padded, cz.form) == (distinct, table, padded, form)
        assert padded == bool(np.any(cz.order == 0.0))
        if not padded:
            assert cz.nb % 64 == 0 and all(ln.min() == ln.max() for ln in _slices(cz)) and cz.order.size == 256   # code 255 in use
        assert he.census(M, L.n_own, use_dict=False).form == "sliced" and he.census(M, L.n_own, sell=False).form == "csr"
    info = he.expected_halo_info(c, 0)
    assert info["fix_form"] == form and info["dict_values"] == (table if form == "sliced+dict" else 0)


def test_packing_families(pkg):
    c = he.case("fan-out")
    L = c.levels[0]
    mult = he.send_multiplicity(L)
    cz = he.census(L.A, L.n_own)
    assert he.fusable(L) and np.any(mult == 1) and np.any(mult == 2) and np.any(mult >= 3)
    assert np.array_equal(np.flatnonzero(mult > 0), cz.rows), "symmetric pattern: the sent rows are the boundary rows"
    A = c.G["mats"][0]
    assert (abs(A) > 0).astype(int).multiply((abs(A.T) > 0).astype(int)).nnz == A.nnz and abs(A - A.T).nnz > 0
    c = he.case("one-way")
    L = c.levels[0]
    mult = he.send_multiplicity(L)
    cz = he.census(L.A, L.n_own)
    assert not he.fusable(L) and np.setdiff1d(np.flatnonzero(mult > 0), cz.rows).size > 0, "a sent row without a ghost column"
    lens = np.diff(L.snd_ptr)
    assert np.any(lens == 0) and np.any(lens > 0), "a message direction of length zero"
    assert not he.expected_halo_info(c, 0)["pack_fused"]
    c = he.case("uncoupled")
    L = c.levels[0]
    assert he.census(L.A, L.n_own).nb == 0 and he.census(L.R, L.n_own).nb == 0 and L.n_ghost == 0 and len(L.snd_idx) == 0
    assert he.expected_halo_info(c, 0)["fix_form"] == "none"


def test_chain_prolongation_gathers_from_an_exchanged_coarse_vector(pkg):
    c = he.case("chain")
    assert c.part == 2 and not c.levels[1].replicated and c.levels[2].replicated
    assert he.census(c.levels[0].P, c.levels[1].n_own).nb > 0 and he.census(c.levels[1].A, c.levels[1].n_own).nb > 0


@pytest.mark.parametrize("name", sorted(he.SLABS))
def test_slabs_single_plane_is_all_boundary_rows_sent_to_two_neighbours(pkg, name):
    c = he.case(name)
    L = c.levels[0]
    o0 = c.G["owners"][0]
    sizes = np.bincount(o0)
    per_plane = (he.SLABS[name][0][0] - 1) * (he.SLABS[name][0][1] - 1)
    assert len(set(sizes.tolist())) == 3 and sizes[1] == per_plane, "unequal slabs, the middle one a single plane"
    assert c.G["mats"][0].shape[0] <= 40000
    plane = np.flatnonzero(o0[L.own_gid] == 1)
    cz = he.census(L.A, L.n_own)
    assert np.all(np.isin(plane, cz.rows)) and np.all(he.send_multiplicity(L)[plane] == 2)
    _, gh = he.ghost_part(L.A, L.n_own)
    nA = np.cumsum([0] + [c.spaces[0].n_ghost(r) for r in range(3)])
    for i in plane:                                          # ghosts on both sides: rank 1's ghost segment holds dofs of rank 0 and of rank 2
        g = c.spaces[0].ghost[1][gh.indices[gh.indptr[i]:gh.indptr[i + 1]] - L.n_own - nA[1]]
        assert set(o0[g].tolist()) == {0, 2}


def test_patches_reach_into_two_neighbours_and_dofs_receive_several_contributions(pkg):
    c = he.case("patches")
    p, L = c.patch, c.levels[0]
    sizes = np.diff(p.ptr)
    assert sizes.min() >= 2 and sizes.max() <= 12 and len(set(sizes.tolist())) > 4
    o0 = c.G["owners"][0]
    reach = [len(set(o0[p.gdofs[p.ptr[k]:p.ptr[k + 1]]].tolist())) - 1 for k in range(sizes.size)]
    assert max(reach) >= 2, "a patch with ghost dofs of two neighbours"
    assert he.contributions_per_dof(c).max() >= 2, "an owned dof receives contributions from two neighbours or more"


# ---------------------------------------------------------------- folded = global, twin within the bound
@pytest.mark.parametrize("name", he.CASES)
def test_folded_operators_are_the_global_ones_and_the_twin_is_within_the_bound(pkg, name):
    """owned rows of every folded operator applied to a consistent folded vector = the global operator on the global vector (the
    check of test_folded_partition_is_the_global_hierarchy), the twin within gamma_k * sum|a x| of the exact value on every row"""
    c = he.case(name)
    for l in range(c.part):
        L = c.levels[l]
        assert np.array_equal(np.sort(L.own_gid), np.arange(c.G["mats"][l].shape[0]))
        assert np.all(L.nbr_rank == 1) and L.snd_ptr[-1] == L.rcv_ptr[-1] == L.n_ghost
        for key, M, n_own, Mg, src, rows in he.operators(c, l):
            xg = c.XC[src][0]
            S = c.levels[src]
            v = xg if S.replicated else he.fill(S, he.own_vec(c, src, xg))
            y = M.matvec(v)
            want = (Mg @ xg)[rows]
            assert np.max(np.abs(y - want)) <= 1e-12 * max(np.max(np.abs(want)), 1.0), (name, l, key)
            ref = he.exact_rows(Mg, rows, xg)
            for split in (True, False):
                t = he.twin_apply(M, n_own, v, split=split)
                assert he.bound_violations(t, ref).size == 0, (name, l, key, split)


@pytest.mark.parametrize("name", ("widths", "fan-out", "one-way", "slabs", "slabs-16"))
def test_twin_sweeps_meet_the_kernel_tolerance(pkg, name):
    c = he.case(name)
    for k in he.SWEEPS:
        (x, r), (xr, rr) = he.twin_sweeps(c, k), he.ref_sweeps(c, k)
        assert oe.max_rel(x, xr) <= fr.TOL_KERNEL and oe.max_rel(r, rr) <= fr.TOL_KERNEL, (name, k)


# ---------------------------------------------------------------- corruptions
def _op_inputs(c):
    L = c.levels[0]
    out = []
    for key, M, n_own, Mg, src, rows in he.operators(c, 0):
        if key != "P":
            out.append((key, M, n_own, Mg, rows))
    return L, out


@pytest.mark.parametrize("name", sorted(k for k, v in he.CORRUPTIONS.items() if v[1] == "op"))
def test_operator_corruptions_leave_both_gates(pkg, name):
    fam, _, fn = he.CORRUPTIONS[name]
    c = he.case(fam)
    L, ops = _op_inputs(c)
    for key, M, n_own, Mg, rows in ops:
        xg = c.X[0]
        v = he.fill(L, he.own_vec(c, 0, xg))
        ref = he.exact_rows(Mg, rows, xg)
        twin = he.twin_apply(M, n_own, v)
        assert he.bound_violations(twin, ref).size == 0      # (the bit gate IS equality with this twin: only the bound can be checked of it)
        bad = fn(c, key, M, n_own, v)
        assert he.bit_mismatches(bad, twin).size > 0, (name, key, "bit gate")
        moved = np.flatnonzero(np.abs(bad - twin) > 2.0 * ref[2])
        assert moved.size > 0 and np.all(np.isin(moved, he.bound_violations(bad, ref))), (name, key, "bound gate")


def test_padded_products_leave_the_non_finite_gate(pkg):
    fam, _, fn = he.CORRUPTIONS["add_padded_products"]
    c = he.case(fam)
    L, ops = _op_inputs(c)
    for key, M, n_own, Mg, rows in ops:
        x = he.own_vec(c, 0, c.X[0])
        xi = x.copy()
        xi[0] = np.inf
        fin, inf = he.twin_apply(M, n_own, he.fill(L, x)), he.twin_apply(M, n_own, he.fill(L, xi))
        assert he.inf_violations(inf, fin, key == "A").size == 0, key
        assert he.inf_violations(fn(c, key, M, n_own, he.fill(L, xi)), fin, key == "A").size > 0, key


def test_stale_ghosts_leave_both_gates(pkg):
    fam, _, fn = he.CORRUPTIONS["stale_ghosts"]
    c = he.case(fam)
    L, ops = _op_inputs(c)
    for key, M, n_own, Mg, rows in ops:
        prev = None
        for xg in c.X:
            v = he.fill(L, he.own_vec(c, 0, xg))
            ref = he.exact_rows(Mg, rows, xg)
            twin = he.twin_apply(M, n_own, v)
            bad = fn(c, key, M, n_own, v, prev)
            assert he.bound_violations(twin, ref).size == 0
            assert he.bit_mismatches(bad, twin).size > 0 and he.bound_violations(bad, ref).size > 0, key
            prev = v


def test_first_send_slot_only_leaves_the_sweep_gates(pkg):
    fam, _, fn = he.CORRUPTIONS["first_send_slot_only"]
    c = he.case(fam)
    for k in he.SWEEPS:
        (x, r), (xr, rr), (xb, rb) = he.twin_sweeps(c, k), he.ref_sweeps(c, k), fn(c, k)
        if k == 1:                                           # (the first exchange of a pass is packed by halo_pack_kernel)
            assert he.bit_mismatches(rb, r).size == 0
            continue
        assert he.bit_mismatches(rb, r).size > 0 and oe.max_rel(rb, rr) > fr.TOL_KERNEL, k
        if k > 2:
            assert he.bit_mismatches(xb, x).size > 0 and oe.max_rel(xb, xr) > fr.TOL_KERNEL, k


def test_one_neighbour_only_leaves_the_assemble_gates(pkg):
    fam, _, fn = he.CORRUPTIONS["one_neighbour_only"]
    c = he.case(fam)
    r = he.own_vec(c, 0, c.r0)
    tw = he.patch_contributions(c, r)
    twin = he.assemble(c, tw)
    ref = he.assemble(c, he.patch_contributions(c, r, exact=True), dtype=he.LD)
    assert oe.max_rel(twin, ref) <= fr.TOL_KERNEL
    bad = fn(c, tw)
    assert he.bit_mismatches(bad, twin).size > 0 and oe.max_rel(bad, ref) > fr.TOL_KERNEL
    assert np.flatnonzero(he.contributions_per_dof(c) >= 2).size > 0
