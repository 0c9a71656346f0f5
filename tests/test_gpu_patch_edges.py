"""The patch smoother past 27 dofs: the three size regimes of gmg_solver::build_patch / patch_precond, blocks that need partial
pivoting in every column, ragged and shuffled patch sets, and the error paths -- against the np.longdouble references that
tests/test_patch_edge_problems.py pins on the host (tests/patch_edge_problems.py holds matrices, patch sets and references).

Per case: one application of the patch preconditioner (ns.precond) and Richardson(M, 3, 0.2) (ns.smooth) on level 0 of a two-level
handle.  Gates: max|a - ref| / max|ref| <= 1e-12 for dx, x and r (the per-kernel gate of the suite; the float64 restatement of the
kernels stays below 1e-14 on every case), uncovered dofs of dx exactly 0.0, r untouched by precond, every output finite.  Kind:
PatchSolver (LU) on the `pairs` matrices, BlockJacobiSolver (NoPivot) on the `dominant` ones, unless the case says otherwise."""
import numpy as np
import pytest

import patch_edge_problems as pe

pytestmark = pytest.mark.gpu

GATE = 1e-12
WORST = {}                                               # (case, kind, run) -> (dx, x, r) deviations, printed per case


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _csr(po, M):
    M = M.tocsr()
    M.sort_indices()
    return po.CSR(M.shape, M.indptr, M.indices, M.data)


def _solver(S, c, pp=None, pd=None, pc=None, **blocks):
    cls = S.PatchSolver if c.pivot else S.BlockJacobiSolver
    return cls(c.pp if pp is None else pp, c.pd if pd is None else pd, patch_cols=c.pc if pc is None else pc, **blocks)


def _setup(S, po, A, M, agg=8, options=None):
    H = pe.two_level(A, agg)
    sm = [S.RichardsonSmoother(M, pe.NITER, pe.OMEGA)]
    gmg = S.GMGLinearSolver([_csr(po, m) for m in H["mats"]], [_csr(po, m) for m in H["prolongations"]],
                            [_csr(po, m) for m in H["restrictions"]], pre_smoothers=sm, post_smoothers=sm, maxiter=1, options=options)
    return S.numerical_setup(S.symbolic_setup(gmg, gmg.smatrices[0]), gmg.smatrices[0])


def _apply(ns, c):
    """-> (dx, x, r) of one precond and one smooth on level 0"""
    r0 = c.r.copy()
    dx = np.full(c.N, np.nan)
    ns.precond(0, r0, dx)
    assert np.array_equal(_bits(r0), _bits(c.r)), "precond changed r"
    x, r = c.x0.copy(), c.r.copy()
    ns.smooth(0, x, r)
    return dx, x, r


def _run(S, po, c, M, options=None, check=None, info=None):
    ns = _setup(S, po, c.A, M, c.agg, options)
    try:
        if check is not None:
            check(ns)
        if info is not None:
            info["device_bytes"] = ns.device_bytes()
        return _apply(ns, c)
    finally:
        ns.close()


def _gate(c, ref, out, run=""):
    dx, x, r = out
    dev = tuple(pe.max_rel(a, b) for a, b in ((dx, ref.dx), (x, ref.x), (r, ref.r)))
    WORST[(c.name, c.kind, run)] = dev
    print("%s %s %s: max|a - ref| / max|ref|: precond %.3e, x %.3e, r %.3e" % (c.name, c.kind, run, *dev))
    for a in out:
        assert np.all(np.isfinite(a)), (c.name, c.kind, run, "non-finite output")
    cov = pe.multiplicity(c.N, c.pp, c.pd if c.pc is None else c.pc) > 0
    assert np.all(_bits(dx[~cov]) == 0), (c.name, c.kind, run, "uncovered dofs of dx are not +0.0")
    assert max(dev) <= GATE, (c.name, c.kind, run, dev)


def _same_bits(a, b, what):
    for u, v, name in zip(a, b, ("dx", "x", "r")):
        nd = np.flatnonzero(_bits(u) != _bits(v))
        assert nd.size == 0, (what, name, "differ at", nd[:8].tolist())


def _worst(name):
    rows = {k: v for k, v in WORST.items() if k[0] == name}
    print("%s: worst deviation over %d runs %.3e" % (name, len(rows), max(max(v) for v in rows.values())))


KINDS = ("lu", "nopivot")


# ---------------------------------------------------------------- 33 .. 64 dofs: wave inversion + patch_apply_kernel
@pytest.mark.parametrize("kind", KINDS)
def test_wave63_ragged_pivoting_patches(S, po, kind):
    """sizes (1, 2, 3, 17, 31, 32, 33, 47, 62, 63) cycled, 43 patches (a ragged last workgroup of patch_apply_kernel).  The two
    runs with patch_dedup = 1 and 0 are the issue's; de-duplication needs max_np <= 32 and >= 64 patches, so both take the same
    path and their equal bits are a second run of one configuration, not a check of the de-duplicated solve (dedup_ragged is)."""
    c, ref = pe.case("wave63", kind), pe.reference("wave63", kind)
    out = {}
    for dd in (1, 0):
        out[dd] = _run(S, po, c, _solver(S, c), dict(patch_dedup=dd))
        _gate(c, ref, out[dd], "patch_dedup=%d" % dd)
    _same_bits(out[1], out[0], "patch_dedup 1 / 0")
    _worst("wave63")


@pytest.mark.parametrize("kind", KINDS)
def test_wave64_largest_wave_patch(S, po, kind):
    """the same with one 64-dof patch: max_np == 64, the largest block of patch_invert_kernel (65 800 B of dynamic LDS).
    patch_dedup = 1 and 0: as in wave63, one path run twice."""
    c, ref = pe.case("wave64", kind), pe.reference("wave64", kind)
    out = {}
    for dd in (1, 0):
        out[dd] = _run(S, po, c, _solver(S, c), dict(patch_dedup=dd))
        _gate(c, ref, out[dd], "patch_dedup=%d" % dd)
    _same_bits(out[1], out[0], "patch_dedup 1 / 0")
    _worst("wave64")


def test_wave_cols_reversed_column_table(S, po):
    """`dominant` under LU with patch_cols = the rows reversed: the block is anti-diagonally dominant, every column swaps"""
    c, ref = pe.case("wave_cols", "lu"), pe.reference("wave_cols", "lu")
    assert np.all(ref.swaps[np.diff(c.pp) >= 4] >= np.diff(c.pp)[np.diff(c.pp) >= 4] // 2 - 1)
    _gate(c, ref, _run(S, po, c, _solver(S, c)))
    _worst("wave_cols")


# ---------------------------------------------------------------- <= 32 dofs, >= 64 patches: de-duplication
@pytest.mark.parametrize("kind", KINDS)
def test_dedup_ragged_mixed_sizes_and_short_last_chunk(S, po, kind):
    """sizes (1, 2, 5, 16, 31, 32) cycled over the periodic family, 64 * 3 + 9 patches: patch_apply_dedup_kernel with mixed sizes in
    every chunk of 64 (np != npB pairs) and a last chunk of 9 (hasB == false)"""
    c, ref = pe.case("dedup_ragged", kind), pe.reference("dedup_ragged", kind)
    M = lambda: _solver(S, c)
    not_pattern = lambda ns: _assert(not ns.level_format(0)["row_patterns"], ns.level_format(0))
    is_pattern = lambda ns: _assert(ns.level_format(0)["row_patterns"], ns.level_format(0))
    # The handle does not say which patch kernel ran, so the paths are told apart by what they must leave behind:
    # de-duplication keeps one inverse block per distinct block (6 here) instead of one per patch and drops the block offsets, so the
    # handle holds at least 8 (sum n_p^2 - sum over distinct n_p^2) - 8 (npatch + 7 + 1) - 4 npatch bytes less (the compact store's
    # offsets and block ids, 64 bytes of slack per array counted against it); a fall-back to patch_apply_kernel (hash mismatch,
    # the one-in-four rule) would hold the same bytes as patch_dedup = 0.
    n_p = np.diff(c.pp)
    saved = 8 * (int(np.sum(n_p ** 2)) - int(np.sum(np.array(pe.DEDUP_SIZES) ** 2))) - 8 * (n_p.size + 8) - 4 * n_p.size - 3 * 64
    assert saved > 500000
    # (1) blocks from the CSR, the patch-by-patch kernels: de-duplicated solve against patch_apply_kernel
    csr, nbytes = {}, {}
    for dd in (1, 0):
        info = {}
        csr[dd] = _run(S, po, c, M(), dict(pattern=0, patch_operator=0, patch_dedup=dd), not_pattern, info)
        nbytes[dd] = info["device_bytes"]
        _gate(c, ref, csr[dd], "csr patch_operator=0 patch_dedup=%d" % dd)
    print("device bytes: patch_dedup=1 %d, patch_dedup=0 %d, difference %d (>= %d expected)" % (nbytes[1], nbytes[0], nbytes[0] - nbytes[1], saved))
    assert nbytes[0] - nbytes[1] >= saved, "the blocks were not de-duplicated: patch_apply_dedup_kernel did not run"
    _same_bits(csr[1], csr[0], "patch_dedup 1 / 0")
    # (3) level in row-pattern layout: blocks of the representatives of equal source signatures, of every patch de-duplicated
    # afterwards, or not de-duplicated at all (whether the grouping by source ran cannot be seen from outside: same store, same bits)
    pat, pbytes = {}, {}
    for key, opt in (("src", dict(patch_source_dedup=1)), ("batch", dict(patch_source_dedup=0)), ("none", dict(patch_dedup=0))):
        info = {}
        pat[key] = _run(S, po, c, M(), dict(patch_operator=0, **opt), is_pattern, info)
        pbytes[key] = info["device_bytes"]
        _gate(c, ref, pat[key], "pattern patch_operator=0 %s" % opt)
    assert pbytes["none"] - pbytes["src"] >= saved and pbytes["none"] - pbytes["batch"] >= saved, pbytes
    _same_bits(pat["src"], pat["batch"], "patch_source_dedup 1 / 0")
    _same_bits(pat["src"], pat["none"], "pattern level: patch_dedup 1 / 0")
    # (dx only: x and r go through the level's mat-vec, which sums in another order in another layout)
    _same_bits(pat["src"][:1], csr[1][:1], "blocks from the row-pattern form / from the CSR")
    # (2) default options: level in row-pattern layout, additive-Schwarz operator in row-pattern form.  It sums the coefficients of
    # a column over the patches first (up to 10 patches per dof here), so its dx differs from the patch-by-patch dx in the last
    # bits of some dofs; bitwise equal dx would mean that the operator form was not taken.
    dflt = _run(S, po, c, M(), None, is_pattern)
    _gate(c, ref, dflt, "default")
    assert np.any(_bits(dflt[0]) != _bits(pat["src"][0])), "default options gave the bits of the patch-by-patch kernels: no operator form"
    _worst("dedup_ragged")


def _assert(ok, what):
    assert ok, what


# ---------------------------------------------------------------- > 64 dofs: patch_factor_kernel + patch_apply_big_kernel
@pytest.mark.parametrize("kind", KINDS)
def test_big_patches_up_to_130_dofs(S, po, kind):
    """sizes (65, 81, 125, 130, 3, 0, 64, 81): 3-D vector Q2 (81), 3-D Q3 (125) and beyond, with a small and an empty patch between"""
    c, ref = pe.case("big", kind), pe.reference("big", kind)
    _gate(c, ref, _run(S, po, c, _solver(S, c)))
    _worst("big")


def test_big_cols_reversed_column_table(S, po):
    """`dominant` under LU with patch_cols = the rows reversed and patches above 64 dofs: patch_factor_kernel must gather
    A[rows_p, cols_p] (matching the column table, as patch_invert_kernel does), not A[rows_p, rows_p].  With the kernel matching
    columns against the row table, as it did before it was given the column table, this test measures
    max|a - ref| / max|ref| = 1.39 (precond), 0.66 (x), 2.98 (r) on an MI355X instead of 2e-16."""
    c, ref = pe.case("big_cols", "lu"), pe.reference("big_cols", "lu")
    n_p = np.diff(c.pp)
    assert np.all(ref.swaps[n_p >= 4] >= n_p[n_p >= 4] // 2)            # every column of the anti-diagonally dominant blocks swaps
    _gate(c, ref, _run(S, po, c, _solver(S, c)))
    _worst("big_cols")


# ---------------------------------------------------------------- caller's patch matrices and lu! factors
def test_dense_caller_matrices_and_factors(S, po):
    """patch_mats = A[p, p] + 0.5 I of the `pairs` matrix on the wave64 patch set (PSRC_DENSE), and the same blocks handed over as
    lu! factors with LAPACK pivots (inverted on the host)"""
    import scipy.linalg as sla
    c, ref = pe.case("dense", "lu"), pe.reference("dense", "lu")
    _gate(c, ref, _run(S, po, c, _solver(S, c, patch_mats=pe.pack_colmajor(c.blocks))), "patch_mats")
    fac, piv = [], []
    for B in c.blocks:
        lu, ip = sla.lu_factor(B)
        fac.append(lu)
        piv.append(ip.astype(np.int32) + 1)                                 # LAPACK ipiv is 1-based
    ipiv = np.concatenate(piv)
    assert np.any(ipiv != np.concatenate([np.arange(1, p.size + 1) for p in piv]))   # the pivot vector is not trivial
    _gate(c, ref, _run(S, po, c, _solver(S, c, factors=pe.pack_colmajor(fac), pivots=ipiv)), "factors")
    _worst("dense")


# ---------------------------------------------------------------- value refresh: blocks from the SELL arrays
@pytest.mark.parametrize("kind", KINDS)
def test_sell_refresh_blocks_from_the_sell_arrays(S, po, kind):
    """pattern = 0, vdict = 0: explicit-value layout, the CSR copy is dropped after the first setup.  update_values with a second
    draw of the family re-gathers the blocks from the SELL arrays (PSRC_SELL): the reference of the new matrix, and the bits of a
    fresh setup on it.  Then the big patch set: patch_factor_kernel reads the CSR, which the refresh does not hold, so the refresh
    is GMG_ERR_UNSUPPORTED naming the 64-dof limit; a full setup (option refresh = 0) of the same handle, which keeps the new
    values, passes the same two checks."""
    from gridapsolvers_jl_amd import abi
    opts = dict(pattern=0, vdict=0)
    for name in ("sell_refresh", "sell_refresh_big"):
        c, ref = pe.case(name, kind), pe.reference(name, kind)
        A0 = pe.level_matrix(c.family, seed=0)
        assert c.seed == 1 and np.array_equal(A0.indices, c.A.indices) and np.all(A0.data != c.A.data)
        ns = _setup(S, po, A0, _solver(S, c), c.agg, opts)
        try:
            fmt = ns.level_format(0)
            assert fmt["layout"] in ("SELL-64", "SELL-O") and not fmt["row_patterns"] and not fmt["value_dictionary"], fmt
            old = _apply(ns, c)
            if name == "sell_refresh":
                ns.update(_csr(po, c.A))
            else:
                with pytest.raises(abi.GmgError) as e:
                    ns.update(_csr(po, c.A))
                assert e.value.code == abi.ERR_UNSUPPORTED and "64 dofs" in str(e.value), str(e.value)
                ns.set_option("refresh", 0)
                ns.setup()
            got = _apply(ns, c)
        finally:
            ns.close()
        assert pe.max_rel(old[0], ref.dx) > 1e-3                             # the first draw is another smoother
        _gate(c, ref, got, "after update_values")
        fresh = _run(S, po, c, _solver(S, c), opts)
        _gate(c, ref, fresh, "fresh setup")
        _same_bits(got, fresh, name + ": refreshed / fresh")
        _worst(name)


# ---------------------------------------------------------------- errors: a status and a message, never a fault
def _fails(S, po, A, M, code, needle, options=None):
    from gridapsolvers_jl_amd import abi
    with pytest.raises(abi.GmgError) as e:
        _setup(S, po, A, M, 8, options).close()
    assert e.value.code == code, str(e.value)
    assert needle in str(e.value), str(e.value)


def _good(S, po, c, ref, ns=None):
    """a correct smoother next to the failed one: a handle that was open all along (ns) or a new one"""
    if ns is not None:
        _gate(c, ref, _apply(ns, c), "open handle after a failed setup")
    else:
        _gate(c, ref, _run(S, po, c, _solver(S, c)), "new handle after a failed setup")


@pytest.mark.parametrize("kind", KINDS)
def test_singular_caller_block_in_the_wave_kernel(S, po, kind):
    """patch_mats with two bitwise equal rows in one 17-dof block: GMG_ERR_SINGULAR from patch_invert_kernel under LU and NoPivot"""
    from gridapsolvers_jl_amd import abi
    c, ref = pe.case("wave63", kind), pe.reference("wave63", kind)
    blocks = [B.copy() for B in pe.blocks_of(c.A, c.pp, c.pd, shift=0.5)]
    p = int(np.flatnonzero(np.diff(c.pp) == 17)[0])
    blocks[p][11] = blocks[p][4]
    ns = _setup(S, po, c.A, _solver(S, c))
    try:
        _fails(S, po, c.A, _solver(S, c, patch_mats=pe.pack_colmajor(blocks)), abi.ERR_SINGULAR, "singular patch block")
        _good(S, po, c, ref, ns)
    finally:
        ns.close()
    _good(S, po, c, ref)


def test_antidiagonal_two_by_two_block(S, po):
    """patch_mats with one block [[0, 1], [1, 0]]: GMG_ERR_SINGULAR under NoPivot (BlockJacobiSolvers.jl:163), a correct solve under LU"""
    from gridapsolvers_jl_amd import abi
    c = pe.antidiagonal_case(True)
    mats = pe.pack_colmajor(c.blocks)
    _fails(S, po, c.A, S.BlockJacobiSolver(c.pp, c.pd, patch_mats=mats), abi.ERR_SINGULAR, "singular patch block")
    ref = pe.adhoc_reference(c)
    assert ref.swaps[2] == 1
    _gate(c, ref, _run(S, po, c, S.PatchSolver(c.pp, c.pd, patch_mats=mats)))


def test_equal_column_maxima_take_the_first_row(S, po):
    """The tie rule of patch_invert_kernel's butterfly argmax (`v2 == v && i2 < idx`: dgetf2's idamax): a 33-dof caller block whose
    column 0 holds |5| in rows 0, 17, 32 and whose column 1 holds |6| in rows 5 and 20.  Every choice among equal maxima solves the
    system, so the gate alone cannot see the rule; the bits can: the library is built without contraction, the kernel and the
    float64 twin do the same operations in the same order, every dof lies in one patch, so dx must equal the twin's bit for bit --
    and the twin that takes the LAST maximum has other bits (tests/test_patch_edge_problems.py)."""
    c = pe.tie_case()
    ref = pe.adhoc_reference(c)
    assert ref.swaps.tolist() == [1, 0, 0]
    out = _run(S, po, c, S.PatchSolver(c.pp, c.pd, patch_mats=pe.pack_colmajor(c.blocks)))
    _gate(c, ref, out)
    X = pe.twin_inverses(c.A, c.pp, c.pd, None, True, c.blocks)
    first = pe.twin_precond(c.A, c.pp, c.pd, None, c.r, True, inverses=X)
    last = pe.twin_precond(c.A, c.pp, c.pd, None, c.r, True, inverses=[pe.twin_inverse(c.blocks[0], True, tie_last=True)] + X[1:])
    nd_first, nd_last = np.flatnonzero(_bits(out[0]) != _bits(first)), np.flatnonzero(_bits(out[0]) != _bits(last))
    print("tie: dx differs from the first-maximum twin at %d dofs, from the last-maximum twin at %d" % (nd_first.size, nd_last.size))
    assert nd_first.size == 0, ("dx is not the first-maximum elimination, bit for bit", nd_first[:8].tolist())
    assert nd_last.size > 0


@pytest.mark.parametrize("kind", KINDS)
def test_singular_level_block_in_the_big_kernel(S, po, kind):
    """a level matrix in which two dofs of the 65-dof patch have bitwise equal rows (non-zero diagonals, so D^-1 exists):
    GMG_ERR_SINGULAR from patch_factor_kernel under LU and NoPivot"""
    from gridapsolvers_jl_amd import abi
    c, ref = pe.case("big", kind), pe.reference("big", kind)
    d = c.pd[c.pp[0]:c.pp[1]]
    assert d.size == 65
    a = int(next(k for k in d if k % 7 in (0, 2, 4)))
    b = a + 1
    assert b in d
    A = c.A.copy()
    for i in (a, b):                                                        # rows a and b: 4.5 in columns a and b, 0.0 elsewhere
        s = slice(A.indptr[i], A.indptr[i + 1])
        A.data[s] = np.where((A.indices[s] == a) | (A.indices[s] == b), 4.5, 0.0)
    assert np.array_equal(A[a].toarray(), A[b].toarray()) and A[a, a] == 4.5 and A[b, b] == 4.5 and np.all(A.diagonal() != 0.0)
    ns = _setup(S, po, c.A, _solver(S, c))
    try:
        _fails(S, po, A, _solver(S, c), abi.ERR_SINGULAR, "singular patch block")
        _good(S, po, c, ref, ns)
    finally:
        ns.close()
    _good(S, po, c, ref)


def test_unsupported_and_invalid_patch_tables(S, po):
    """patch_mats with a patch above 64 dofs: GMG_ERR_UNSUPPORTED naming the limit; a patch dof equal to N: GMG_ERR_INVALID"""
    from gridapsolvers_jl_amd import abi
    c, ref = pe.case("big", "lu"), pe.reference("big", "lu")
    mats = pe.pack_colmajor(pe.blocks_of(c.A, c.pp, c.pd, shift=0.5))
    _fails(S, po, c.A, _solver(S, c, patch_mats=mats), abi.ERR_UNSUPPORTED, "64 dofs")
    bad = c.pd.copy()
    bad[c.pp[3] + 7] = c.N
    _fails(S, po, c.A, _solver(S, c, pd=bad), abi.ERR_INVALID, "out of range")
    w = pe.case("wave63", "lu")
    bad = w.pd.copy()
    bad[w.pp[-1] - 1] = w.N
    _fails(S, po, w.A, _solver(S, w, pd=bad), abi.ERR_INVALID, "out of range")
    _good(S, po, c, ref)
