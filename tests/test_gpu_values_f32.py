"""cycle_values = "float32" on the device: the cycle streams float32 copies of the SELL-64 / SELL-O value streams.

The feature's definition (include/gmg_amd.h, gmg_level_values): the preconditioner is EXACTLY the fp64 cycle on the matrices whose
stored values were rounded to float32, 1/diag included; nothing outside the cycle reads the rounded values.  So the comparison
handle D of every bit-for-bit test is the existing fp64 path with the option off, GIVEN the rounded matrices
(values_f32_reference.round_levels) and forced to the same layout: the parent's kernels on other data, not the code under test.
F is the handle under test: option on, the caller's fp64 matrices.

All hierarchies are variable-coefficient Q1 (po.build_hierarchy(cells, nlev, kappa=po.smooth_kappa)), whose values are distinct in
almost every entry: no lossless layout applies, they land on SELL-O / SELL-64 or, where the padding exceeds sell_maxpad, CSR tiles.
The small shapes of the sweep tests pad beyond the default sell_maxpad = 1.25, so those tests raise it (both handles alike)."""
import importlib

import numpy as np
import pytest

import operator_edge_problems as oe
import values_f32_reference as vr

pytestmark = pytest.mark.gpu

OMEGA = 2.0 / 3.0
# every level but the coarsest on SELL-O / SELL-64, whatever its padding and however few distinct values a tiny level has
FORCE = {"pattern": 0, "vdict": 0, "sell_maxpad": oe.BIGPAD}
LAYOUTS = {"SELL-O": {}, "SELL-64": {"opattern": 0}}
_H = {}


def _hier(po, cells, nlev, kappa=None):
    key = (cells, nlev, kappa)
    if key not in _H:
        _H[key] = po.build_hierarchy(cells, nlev, kappa=kappa or po.smooth_kappa)
    return _H[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _gmg(S, H, mats, sweeps, f32, options=None, smoothers=None, **kw):
    n = len(mats) - 1
    sm = smoothers or [S.RichardsonSmoother(S.JacobiLinearSolver(), sweeps, OMEGA)] * n
    kw.setdefault("maxiter", 1)
    return S.GMGLinearSolver(mats, H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, options=options,
                             cycle_values="float32" if f32 else "float64", **kw)


def _setup(S, solver, A):
    return S.numerical_setup(S.symbolic_setup(solver, A), A)


def _pair(S, H, sweeps, options, **kw):
    """-> (F, D): option on with the caller's matrices; option off with the matrices rounded on F's float32 levels"""
    mats = H["mats"]
    F = _setup(S, _gmg(S, H, mats, sweeps, True, options, **kw), mats[0])
    which = [l for l in range(len(mats)) if F.level_values(l)["dtype"] == "float32"]
    rm = vr.round_levels(mats, which)
    D = _setup(S, _gmg(S, H, rm, sweeps, False, options, **kw), rm[0])
    for l in range(len(mats)):
        assert D.level_format(l) == F.level_format(l), (l, D.level_format(l), F.level_format(l))
        assert D.level_values(l)["dtype"] == "float64"
    return F, D, which


def _vectors(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)


# ------------------------------------------------------------------------------------------------ 1. sweeps, bit for bit
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("cells,nlev", [((12, 8, 8), 3), ((20, 12), 2)], ids=["12x8x8", "20x12"])
def test_sweeps_are_the_fp64_sweeps_on_the_rounded_matrix(S, po, cells, nlev, layout):
    """ns.smooth(lev, x, r) of F against D, np.array_equal on x and r: 1, 2, 3 sweeps on every float32 level and 10 on level 0 (every
    x-update form of the deferred schedule), x zero and nonzero, unrolls sell_un 3 / 6 / 9, both gather forms of the sweep, and
    values_f32_nt 0 / 1 / 2 (cached, non-temporal stream, non-temporal row-wise operands too) with the same bits.
    (12,8,8): 539 rows = 8 full slices + one of 27 rows, row widths 8 / 12 / 18 / 27; (20,12): 209 rows, widths 4 / 6 / 9."""
    H = _hier(po, cells, nlev)
    sigs = set()
    for un in (3, 6, 9):
        for one_gather in ((1, 0) if un == 6 else (1,)):
            for niter in (1, 2, 3, 10):
                opts = dict(FORCE, sell_un=un, one_gather=one_gather, **LAYOUTS[layout])
                F, D, which = _pair(S, H, niter, opts)
                others = [_setup(S, _gmg(S, H, H["mats"], niter, True, dict(opts, values_f32_nt=nt)), H["mats"][0]) for nt in (0, 1, 2)]
                try:
                    assert which == list(range(nlev - 1)), which
                    want = layout if H["mats"][0].shape[0] >= 64 else "SELL-64"
                    assert F.level_format(0)["layout"] == want
                    for lev in (which if niter < 10 else [0]):
                        n = H["mats"][lev].shape[0]
                        x0, r0 = _vectors(n, 100 * lev + niter)
                        for xs in (np.zeros(n), x0):
                            xd, rd = xs.copy(), r0.copy()
                            D.smooth(lev, xd, rd)
                            assert np.all(np.isfinite(xd)) and np.all(np.isfinite(rd))
                            for tag, ns in [("auto", F)] + list(zip(("nt0", "nt1", "nt2"), others)):
                                xf, rf = xs.copy(), r0.copy()
                                ns.smooth(lev, xf, rf)
                                what = (cells, layout, "un", un, "one_gather", one_gather, "sweeps", niter, "level", lev, tag)
                                assert np.array_equal(_bits(xf), _bits(xd)), (what, "x", np.flatnonzero(xf != xd)[:8].tolist())
                                assert np.array_equal(_bits(rf), _bits(rd)), (what, "r", np.flatnonzero(rf != rd)[:8].tolist())
                    # the unrounded matrix gives other bits: the comparison can tell the two preconditioners apart
                    P = _setup(S, _gmg(S, H, H["mats"], niter, False, opts), H["mats"][0])
                    n = H["mats"][0].shape[0]
                    x0, r0 = _vectors(n, niter)
                    xp, rp, xd, rd = x0.copy(), r0.copy(), x0.copy(), r0.copy()
                    P.smooth(0, xp, rp); D.smooth(0, xd, rd); P.close()
                    assert not np.array_equal(rp, rd)
                    sigs.update(ns.sweep_signature(0) for ns in [F] + others)
                finally:
                    for ns in [F, D] + others:
                        ns.close()
    kernel = "sello_kernel<f32," if layout == "SELL-O" and H["mats"][0].shape[0] >= 64 else "sell_kernel<f32,"
    assert all(s.startswith(kernel) for s in sigs), sigs
    assert any("XM=*" in s for s in sigs) and any("2G" in s for s in sigs) and any("NT=2" in s for s in sigs), sigs


def test_sweeps_on_a_ragged_matrix(S, po):
    """the `widths` family of tests/operator_edge_problems.py (slice widths 1 .. 66, rows of every length up to them) on SELL-64:
    1 .. 3 sweeps, unrolls 3 / 6 / 9, against D"""
    c = oe.case("widths")
    csr = lambda M: po.CSR(M.shape, M.indptr, M.indices, M.data)
    H = dict(mats=[csr(c.A), csr(c.Ac)], prolongations=[csr(c.P)], restrictions=[csr(c.R)])
    for un in (3, 6, 9):
        for niter in (1, 2, 3):
            F, D, which = _pair(S, H, niter, dict(oe.CONFIGS["sell"], sell_un=un))
            try:
                assert which == [0] and F.level_format(0)["layout"] == "SELL-64" and F.sweep_signature(0) == ""
                for xs in (np.zeros(c.n), c.x0):
                    xf, rf, xd, rd = xs.copy(), c.r0.copy(), xs.copy(), c.r0.copy()
                    F.smooth(0, xf, rf); D.smooth(0, xd, rd)
                    assert np.all(np.isfinite(xd)) and np.all(np.isfinite(rd))
                    assert np.array_equal(_bits(xf), _bits(xd)) and np.array_equal(_bits(rf), _bits(rd)), (un, niter)
                assert F.sweep_signature(0).startswith("sell_kernel<f32,")
            finally:
                F.close(); D.close()


# ------------------------------------------------------------------------------------------------ 2. cycles, bit for bit
@pytest.mark.parametrize("forced", [False, True], ids=["default-layouts", "every-level-sell"])
@pytest.mark.parametrize("cycle", ["v_cycle", "w_cycle", "f_cycle"])
def test_cycles_are_the_fp64_cycles_on_the_rounded_matrices(S, po, cycle, forced):
    """solve_ of the bare GMG in preconditioner mode, maxiter 1 and 3, on (16,16,16) x 3 levels against D.  With the default
    sell_maxpad level 1 (343 rows, padding 1.51) stays on CSR tiles and fp64; forced onto SELL it is a float32 level that has
    released its fp64 values."""
    H = _hier(po, (16, 16, 16), 3)
    b = po.random_rhs(H["mats"][0].shape[0])
    for maxiter in (1, 3):
        F, D, which = _pair(S, H, 3, FORCE if forced else None, cycle_type=cycle, maxiter=maxiter, rtol=1e-300, atol=1e-300)
        try:
            assert which == ([0, 1] if forced else [0])
            xf, xd = np.zeros_like(b), np.zeros_like(b)
            S.solve_(xf, F, b); S.solve_(xd, D, b)
            assert np.all(np.isfinite(xd)) and np.linalg.norm(xd) > 0
            assert np.array_equal(_bits(xf), _bits(xd)), (cycle, maxiter, np.flatnonzero(xf != xd)[:8].tolist())
        finally:
            F.close(); D.close()


# ------------------------------------------------------------------------------------------------ 3. against the twin
@pytest.fixture(scope="module")
def problem3(po):
    """(16,16,16) x 3 levels, 3 / 3 sweeps, po.random_rhs; the float32 levels as the layout rule predicts them on the host"""
    H = _hier(po, (16, 16, 16), 3)
    b = po.random_rhs(H["mats"][0].shape[0])
    which = [l for l in range(2) if oe.expected_layout(H["mats"][l].to_scipy().tocsr(), {"pattern": 0})["layout"] in ("SELL-O", "SELL-64")]
    return H, b, which


def test_one_cycle_matches_the_twin(S, po, problem3):
    H, b, which = problem3
    F = _setup(S, _gmg(S, H, H["mats"], 3, True), H["mats"][0])
    try:
        assert [l for l in range(3) if F.level_values(l)["dtype"] == "float32"] == which == [0]
        x = np.zeros_like(b)
        S.solve_(x, F, b)
    finally:
        F.close()
    want = vr.twin_gmg(H, 3, OMEGA, which).solve(b)
    rel = np.linalg.norm(x - want) / np.linalg.norm(want)
    plain = vr.twin_gmg(H, 3, OMEGA, []).solve(b)
    print("one cycle: |x - twin(rounded)| / |twin| = %.2e; |twin(fp64) - twin(rounded)| / |twin| = %.2e"
          % (rel, np.linalg.norm(plain - want) / np.linalg.norm(want)))
    assert rel <= 1e-11


def test_cg_matches_the_twin_and_keeps_the_fp64_operator(S, po, problem3):
    """CG + GMG(float32), rtol 1e-10: the twin's iteration count (6 on the CPU), its history to 1e-8 relative, and the host-computed
    ||b - A x|| / ||b|| with the UNROUNDED A below 1e-10 -- which pins the fp64 Krylov side: solving the rounded system exactly
    leaves 2.9e-8 there on this problem."""
    H, b, which = problem3
    xt, it, hist, true_t = vr.twin_cg(H, b, 3, 1e-10, which)
    solver = S.CGSolver(_gmg(S, H, H["mats"], 3, True), maxiter=50, atol=1e-300, rtol=1e-10)
    ns = _setup(S, solver, H["mats"][0])
    try:
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
        assert ns.P_ns.level_values(0)["dtype"] == "float32"
    finally:
        ns.P_ns.close()
    A = H["mats"][0].to_scipy().tocsr()
    true = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    got = np.asarray(solver.log.residuals[: solver.log.num_iters + 1])
    print("CG: iterations %d (twin %d), true residual %.4e (twin %.4e)" % (solver.log.num_iters, it, true, true_t))
    assert it == 6 and solver.log.num_iters == it
    assert np.max(np.abs(got - hist) / hist) <= 1e-8
    assert true < 1e-10
    assert np.linalg.norm(x - xt) / np.linalg.norm(xt) <= 1e-10


def test_fgmres_matches_the_twin(S, po, problem3):
    H, b, which = problem3
    xt, it, hist, true_t = vr.twin_fgmres(H, b, 3, 1e-10, 5, which)
    solver = S.FGMRESSolver(5, _gmg(S, H, H["mats"], 3, True), maxiter=50, atol=1e-300, rtol=1e-10)
    ns = _setup(S, solver, H["mats"][0])
    try:
        x = np.zeros_like(b)
        S.solve_(x, ns, b)
    finally:
        ns.P_ns.close()
    A = H["mats"][0].to_scipy().tocsr()
    got = np.asarray(solver.log.residuals[: solver.log.num_iters + 1])
    assert solver.log.num_iters == it
    assert np.max(np.abs(got - hist) / hist) <= 1e-8
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) < 1e-10


# ------------------------------------------------------------------------------------------------ 4. what the handle reports
def test_level_values_and_signature(S, po, problem3):
    H, b, _ = problem3
    for options, bytes_per_nnz, kernel in ((None, 4.0, "sello_kernel<f32,"), ({"opattern": 0}, 8.0, "sell_kernel<f32,")):
        F = _setup(S, _gmg(S, H, H["mats"], 3, True, options), H["mats"][0])
        try:
            assert F.level_values(0) == dict(dtype="float32", cycle_stream_bytes_per_nnz=bytes_per_nnz)
            assert F.level_values(2)["dtype"] == "float64"
            for l in (1, 2):                                 # not float32 levels: the figure of level_format
                assert F.level_values(l)["cycle_stream_bytes_per_nnz"] == F.level_format(l)["stream_bytes_per_nnz"]
            x = np.zeros_like(b)
            S.solve_(x, F, b)
            assert F.sweep_signature(0).startswith(kernel), F.sweep_signature(0)
            assert F.get_option("values_f32") == (1.0, "handle")
            off = _setup(S, _gmg(S, H, H["mats"], 3, False, options), H["mats"][0])
            S.solve_(x, off, b)
            assert "f32" not in off.sweep_signature(0) and off.level_values(0)["dtype"] == "float64"
            assert off.level_format(0) == F.level_format(0)  # gmg_level_format itself is unchanged
            off.close()
        finally:
            F.close()


def test_operator_applications_outside_the_cycle_read_fp64(S, po, pkg, problem3):
    """op_apply(A) of level 0 gives the bits of the option off (the unrounded values) and not those of the rounded matrix; a level
    >= 1 that streams float32 has released its fp64 values: op_apply(A) there is a clean GMG_ERR_STATE"""
    abi = importlib.import_module(pkg.__name__ + ".abi")
    H, b, _ = problem3
    F, D, which = _pair(S, H, 3, FORCE)
    off = _setup(S, _gmg(S, H, H["mats"], 3, False, FORCE), H["mats"][0])
    try:
        assert which == [0, 1]
        y = {}
        for name, ns in (("on", F), ("off", off), ("rounded", D)):
            y[name] = np.full(b.size, np.nan)
            ns.op_apply(0, abi.OP_A, b, y[name])
        assert np.array_equal(_bits(y["on"]), _bits(y["off"])) and not np.array_equal(y["on"], y["rounded"])
        x1 = np.ones(H["mats"][1].shape[0])
        with pytest.raises(abi.GmgError) as e:
            F.op_apply(1, abi.OP_A, x1, np.zeros_like(x1))
        assert e.value.code == abi.ERR_STATE and "float32" in str(e.value), str(e.value)
        # the cycle still works after the refused call, and a coarse solve / transfers are untouched
        x = np.zeros_like(b)
        S.solve_(x, F, b)
        assert np.all(np.isfinite(x))
    finally:
        F.close(); D.close(); off.close()


def test_constant_coefficients_are_untouched(S, po):
    """kappa = None: every level is SELL-P / dense, none float32, and the results are those of the option off, bit for bit"""
    H = po.build_hierarchy((16, 16, 16), 3)
    b = po.random_rhs(H["mats"][0].shape[0])
    out = []
    for f32 in (True, False):
        ns = _setup(S, _gmg(S, H, H["mats"], 3, f32), H["mats"][0])
        try:
            assert all(ns.level_values(l)["dtype"] == "float64" for l in range(3))
            x = np.zeros_like(b)
            S.solve_(x, ns, b)
            out.append(x)
        finally:
            ns.close()
    assert np.array_equal(_bits(out[0]), _bits(out[1]))


# ------------------------------------------------------------------------------------------------ 5. refresh
def test_update_refills_both_streams(S, po):
    """update() with the values of kappa (1 + 0.3 X Y + 0.15 Z): the next cycle and the next CG solve are bit for bit those of a
    fresh setup on the new values; device_bytes() is unchanged by the update."""
    kappa2 = lambda X, Y, Z: po.smooth_kappa(X, Y, Z) * (1.0 + 0.3 * X * Y + 0.15 * Z)
    H, H2 = _hier(po, (16, 16, 16), 3), po.build_hierarchy((16, 16, 16), 3, kappa=kappa2)
    b = po.random_rhs(H["mats"][0].shape[0])
    for krylov in (False, True):
        wrap = (lambda g: S.CGSolver(g, maxiter=50, atol=1e-300, rtol=1e-10)) if krylov else (lambda g: g)
        s1, s2 = wrap(_gmg(S, H, H["mats"], 3, True, FORCE)), wrap(_gmg(S, H2, H2["mats"], 3, True, FORCE))
        n1, n2 = _setup(S, s1, H["mats"][0]), _setup(S, s2, H2["mats"][0])
        g1, g2 = (n1.P_ns, n2.P_ns) if krylov else (n1, n2)
        try:
            x1, x2, x3 = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
            S.solve_(x1, n1, b)
            before = g1.device_bytes()
            g1.update(H2["mats"][0], smatrices=H2["mats"])
            assert g1.device_bytes() == before == g2.device_bytes()
            assert [g1.level_values(l)["dtype"] for l in range(3)] == ["float32", "float32", "float64"]
            S.solve_(x2, n1, b); S.solve_(x3, n2, b)
            assert not np.array_equal(x1, x2)
            assert np.array_equal(_bits(x2), _bits(x3)), krylov
        finally:
            g1.close(); g2.close()


# ------------------------------------------------------------------------------------------------ 6. memory
def test_device_bytes(S, po):
    """Level 0 holds both streams: at most 4 B per padded entry more (nnz x padding of level_format(0)).  A level >= 1 swaps its
    8-byte stream for a 4-byte one: it must not grow -- it gives 4 B per padded entry back.  Allowance for the new small tables:
    one two-word flag buffer per handle and the 64 B of slack every allocation of the handle is counted with, per float stream --
    256 B is generous."""
    H = _hier(po, (16, 16, 16), 3)
    small = 256
    for nlev_f32, opts in ((1, None), (2, FORCE)):
        on, off = _setup(S, _gmg(S, H, H["mats"], 3, True, opts), H["mats"][0]), _setup(S, _gmg(S, H, H["mats"], 3, False, opts), H["mats"][0])
        try:
            assert sum(on.level_values(l)["dtype"] == "float32" for l in range(3)) == nlev_f32
            zpad = [int(round(H["mats"][l].nnz * on.level_format(l)["padding"])) for l in range(2)]
            grow = on.device_bytes() - off.device_bytes()
            print("float32 levels: %d, device bytes on - off = %d, padded entries %s" % (nlev_f32, grow, zpad))
            assert grow <= 4 * zpad[0] + small - (4 * zpad[1] if nlev_f32 == 2 else 0), (grow, zpad)
        finally:
            on.close(); off.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def _refused(S, abi, solver, A, *words):
    with pytest.raises(abi.GmgError) as e:
        _setup(S, solver, A)
    msg = str(e.value)
    assert e.value.code == abi.ERR_INVALID, msg
    assert "float32" in msg and all(w in msg for w in words), msg
    return msg


def test_refusals(S, po, pkg):
    abi = importlib.import_module(pkg.__name__ + ".abi")
    H = _hier(po, (16, 16, 16), 3)
    A0 = H["mats"][0]
    jac = S.RichardsonSmoother(S.JacobiLinearSolver(), 3, OMEGA)
    pp, pd = po.vertex_star_patches((16, 16, 16), 1)
    bad = {"Chebyshev": S.ChebyshevSmoother(S.JacobiLinearSolver(), 3),
           "Gauss-Seidel": S.GaussSeidelSmoother(1, 1.0),
           "patch": S.RichardsonSmoother(S.PatchSolver(pp, pd), 1, 0.5)}
    for name, sm in bad.items():
        _refused(S, abi, _gmg(S, H, H["mats"], 3, True, smoothers=[sm, jac]), A0, "level 0", "smoother")
    # the same smoothers on a level that is NOT float32 (level 1 on CSR tiles with the default sell_maxpad) are accepted
    _setup(S, _gmg(S, H, H["mats"], 3, True, smoothers=[jac, S.GaussSeidelSmoother(1, 1.0)]), A0).close()
    # a Galerkin level / solver mode through the options of a float64 solver: the constructor cannot see those, gmg_setup refuses
    g = _gmg(S, H, [A0, S.Galerkin(), S.Galerkin()], 3, False, {"values_f32": 1})
    _refused(S, abi, g, A0, "Galerkin")
    _refused(S, abi, _gmg(S, H, H["mats"], 3, False, {"values_f32": 1}, mode="solver"), A0, "solver")
    # values outside float32's normal range: level and row are named
    for scale in (1e-42, 1e40):                              # float32 subnormal / overflow
        As = po.CSR(A0.shape, A0.ptr, A0.idx, A0.val * scale)
        _refused(S, abi, _gmg(S, H, [As] + H["mats"][1:], 3, True), As, "level 0", "row 0", "normal range")
    one = A0.val.copy()
    k = int(A0.ptr[1234]) + 3
    one[k] = 1e39
    As = po.CSR(A0.shape, A0.ptr, A0.idx, one)
    _refused(S, abi, _gmg(S, H, [As] + H["mats"][1:], 3, True), As, "level 0", "row 1234")
    # ... and the same matrices are fine with the option off
    _setup(S, _gmg(S, H, [As] + H["mats"][1:], 3, False), As).close()


def test_partitioned_handle_is_refused(pkg, po):
    abi = importlib.import_module(pkg.__name__ + ".abi")
    pa, mg = importlib.import_module(pkg.__name__ + ".partition"), importlib.import_module(pkg.__name__ + ".multigpu")
    cells, nlev, W = (16, 16, 16), 3, 2
    grid = pa.rank_grid(W, len(cells))
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, None, None, "jacobi") for r in range(W)])
    with pytest.raises(abi.GmgError) as e:
        mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport="host_loopback", local_hierarchy=F, cells_global=cells,
                          options={"values_f32": 1})
    assert e.value.code == abi.ERR_INVALID and "float32" in str(e.value) and "partitioned" in str(e.value), str(e.value)
