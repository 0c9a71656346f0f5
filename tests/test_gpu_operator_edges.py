"""The general sparse operator kernels -- csr_stream1_kernel, sell_kernel, sellc_kernel, sello_kernel and the setup that feeds them
(upload_csr, build_sell, sell_build_kernel) -- on ragged, long-row, rectangular and empty-row operators, against the references
that tests/test_operator_edge_problems.py pins on the host (tests/operator_edge_problems.py holds matrices and references).

Per case and configuration, on two-level handles:
  op_apply of A, P and R (device vectors pre-filled with NaN): every SELL-family layout equals the CSR-order float64 sum bit for
    bit on EVERY row, every layout stays within gamma_k * sum|a x| of the exact value, empty rows give +0.0;
  precond (dx of one Jacobi application from a zero guess) and smooth with 1 .. 5 sweeps, omega = 2/3, nonzero x, on level 0:
    max|a - ref| / max|ref| <= 1e-13 against the longdouble reference for dx, x and r; r untouched by precond; everything finite;
    every SELL-family layout gives the bits of the float64 twin of the kernels (so they all agree with each other bit for bit);
  level_format(0) equals expected_layout on every configuration but the default; sweep_signature(0) names the kernel and its
    UN / XM variant where the dispatcher notes one (CSR-stream and SELL-C sweeps note nothing).
One V-cycle and three solver-mode iterations from a nonzero x run against the sequential oracle (1e-11 on the result, 1e-8 on the
residual history): there the EPI_SUB, EPI_RESID and EPI_ADDTO epilogues and the x_zero form of the sweeps meet the ragged and
rectangular rows.  A smoother's sweep count is fixed at setup, so one configuration takes three handles: (pre, post) sweeps
(1, 2), (3, 4) and (5, 5)."""
import itertools

import numpy as np
import pytest

import fullsize_reference as fr
import operator_edge_problems as oe

pytestmark = pytest.mark.gpu

TOL_KERNEL, TOL_VCYCLE, TOL_HIST = fr.TOL_KERNEL, 1e-11, 1e-8
REACHED = {}                                              # family -> {(configuration family, layout, sweep signature)}
SELL_FAMILY = ("SELL-64", "SELL-O")
DISTINCT = tuple("ragged-%d" % n for n in oe.SIZES) + ("widths", "long", "offsets")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _csr(po, M):
    return po.CSR(M.shape, M.indptr, M.indices, M.data)


def _hier(po, c):
    return dict(mats=[_csr(po, c.A), _csr(po, c.Ac)], prolongations=[_csr(po, c.P)], restrictions=[_csr(po, c.R)])


def _setup(S, po, c, options, pre, post, **kw):
    H = _hier(po, c)
    sm = lambda k: [S.RichardsonSmoother(S.JacobiLinearSolver(), k, oe.OMEGA)]
    kw.setdefault("maxiter", 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm(pre),
                            post_smoothers=sm(post), options=options, **kw)
    return S.numerical_setup(S.symbolic_setup(gmg, gmg.smatrices[0]), gmg.smatrices[0]), gmg


def _device_op(ns, op, x, nout, offset=0):
    """y = op x on device tensors, y pre-filled with NaN; offset = 1: both are views 8 bytes off a 16-byte boundary"""
    import torch
    xb = torch.zeros(x.size + offset + 1, dtype=torch.float64, device="cuda")
    xb[offset:offset + x.size].copy_(torch.from_numpy(np.ascontiguousarray(x)))
    yb = torch.full((nout + offset + 1,), np.nan, dtype=torch.float64, device="cuda")
    xd, yd = xb[offset:offset + x.size], yb[offset:offset + nout]
    assert xd.data_ptr() % 16 == 8 * offset and yd.data_ptr() % 16 == 8 * offset
    torch.cuda.synchronize()                              # the library runs on its own stream: torch's fills must be done first
    ns.op_apply(0, op, xd, yd)
    torch.cuda.synchronize()
    out = yb.cpu().numpy()
    assert np.all(np.isnan(out[:offset])) and np.all(np.isnan(out[offset + nout:])), "op_apply wrote outside its vector"
    return out[offset:offset + nout]


def _check_ops(ns, c, ref, options, tag, offset=0):
    """op_apply of A, P, R on every row -> worst |y - exact| as a fraction of the bound"""
    from gridapsolvers_jl_amd import abi
    worst = 0.0
    for key, op, M, v in (("A", abi.OP_A, c.A, c.x0), ("P", abi.OP_P, c.P, c.xc), ("R", abi.OP_R, c.R, c.x0)):
        y = _device_op(ns, op, v, M.shape[0], offset)
        what = "%s %s op_apply %s%s" % (c.name, tag, key, " (8 bytes off)" if offset else "")
        assert np.all(np.isfinite(y)), (what, "rows left unwritten or non-finite", np.flatnonzero(~np.isfinite(y))[:8].tolist())
        lay = None if options is None else oe.expected_layout(M, options)["layout"]
        frac, _ = fr.check_rows(y, None, None, None, v, "", what, bound_only=lay not in SELL_FAMILY, reference=ref.rows[key])
        empty = np.diff(M.indptr) == 0
        assert np.all(_bits(y[empty]) == 0), (what, "empty rows are not +0.0")
        worst = max(worst, frac)
    return worst


def _check_level(S, po, c, options, tag, cfg_family, want_sig=None, ops=True):
    """the per-case checks of one configuration -> dict(dx, sweeps {k: (x, r)}, sigs, fmt, worst)"""
    ref = oe.reference(c.name)
    out = dict(sweeps={}, sigs=[], worst=0.0, frac=0.0)
    for pre, post in ((1, 2), (3, 4), (5, 5)):
        ns, _ = _setup(S, po, c, options, pre, post)
        try:
            from gridapsolvers_jl_amd import abi
            fmt = ns.level_format(0)
            out["fmt"] = fmt
            if options is not None:
                want = oe.expected_layout(c.A, options)
                assert (fmt["layout"], fmt["value_dictionary"], fmt["idx16"]) == (want["layout"], want["value_dictionary"], want["idx16"]), \
                    (c.name, tag, fmt, want)
                if fmt["layout"] != "CSR-stream":
                    assert abs(fmt["padding"] - want["padding"]) <= 1e-12 * want["padding"], (c.name, tag, fmt, want)
            if pre == 1:
                if ops:
                    out["frac"] = _check_ops(ns, c, ref, options, tag)
                r0 = c.r0.copy()
                dx = np.full(c.n, np.nan)
                ns.precond(0, r0, dx)
                assert np.array_equal(_bits(r0), _bits(c.r0)), (c.name, tag, "precond changed r")
                assert np.all(np.isfinite(dx)), (c.name, tag, "precond: non-finite dx")
                out["dx"] = dx
                out["worst"] = max(out["worst"], oe.max_rel(dx, ref.dx))
                assert oe.max_rel(dx, ref.dx) <= TOL_KERNEL, (c.name, tag, "precond", oe.max_rel(dx, ref.dx))
            for k, which in ((pre, abi.PRE), (post, abi.POST)):
                if k in out["sweeps"]:
                    continue
                x, r = c.x0.copy(), c.r0.copy()
                ns.smooth(0, x, r, which=which)
                assert np.all(np.isfinite(x)) and np.all(np.isfinite(r)), (c.name, tag, k, "smooth: non-finite output")
                dev = (oe.max_rel(x, ref.sweeps[k][0]), oe.max_rel(r, ref.sweeps[k][1]))
                out["worst"] = max(out["worst"], *dev)
                assert max(dev) <= TOL_KERNEL, (c.name, tag, "%d sweeps" % k, dev)
                out["sweeps"][k] = (x, r)
                if which == abi.PRE:
                    out["sigs"].append(ns.sweep_signature(0))
        finally:
            ns.close()
    if out["fmt"]["layout"] in SELL_FAMILY:                   # the bits of the twin: row sums in CSR order, the same roundings elsewhere
        for k in oe.SWEEPS:
            tx, tr = _twin(c.name, k)
            for got, want, what in ((out["sweeps"][k][0], tx, "x"), (out["sweeps"][k][1], tr, "r")):
                nd = np.flatnonzero(_bits(got) != _bits(want))
                assert nd.size == 0, (c.name, tag, "%d sweeps: %s differs from the float64 twin at" % (k, what), nd[:8].tolist())
    if want_sig is not None:
        for i, sig in enumerate(out["sigs"]):
            for part in want_sig(i):
                assert part in sig, (c.name, tag, "handle %d" % i, sig, part)
    REACHED.setdefault(c.family, set()).add((cfg_family, out["fmt"]["layout"] + ("+dict" if out["fmt"]["value_dictionary"] else "")
                                             + ("+idx16" if out["fmt"]["idx16"] else ""), out["sigs"][1]))
    return out


_TWIN = {}


def _twin(name, k):
    if (name, k) not in _TWIN:
        c = oe.case(name)
        _TWIN[(name, k)] = oe.twin_sweeps(c.A, c.x0, c.r0, k)
    return _TWIN[(name, k)]


def _report(name, cfg_family, runs):
    w = max(o["worst"] for o in runs.values())
    f = max(o["frac"] for o in runs.values())
    print("%s [%s]: %d configurations, worst max|a - ref| / max|ref| %.3e, worst |y - exact| %.3g of the bound" % (name, cfg_family, len(runs), w, f))
    for lay, sig in sorted({(o["fmt"]["layout"], s) for o in runs.values() for s in o["sigs"]}):
        print("    %s  %s" % (lay, sig or "(no sweep signature noted)"))


# ---------------------------------------------------------------- CSR-stream
@pytest.mark.parametrize("name", DISTINCT)
def test_csr_stream_lanes_and_pointer_types(S, po, name):
    """sell = 0: csr_stream1_kernel with the default lanes per row and lanes_log2 0, 3, 6, with 32- and 64-bit row pointers, one- and
    two-gather sweeps.  `long`
    takes the long-row branch (2049 and 3000 entries) next to the tile branch (2047, 2048, a run of exactly 2048); ragged-4283 with
    lanes_log2 = 3 has 134 workgroups (>= 64 and no multiple of 8: the XCD remap with a remainder)."""
    c = oe.case(name)
    runs = {}
    for lanes, p64, oneg in itertools.product((None, 0, 3, 6), (0, 1), (1, 0)):
        opt = dict(oe.CONFIGS["csr"], force_ptr64=p64, one_gather=oneg)
        if lanes is not None:
            opt["lanes_log2"] = lanes
        runs[(lanes, p64, oneg)] = _check_level(S, po, c, opt, "csr lanes_log2=%s ptr64=%d oneg=%d" % (lanes, p64, oneg), "csr", ops=(oneg == 1))
        assert runs[(lanes, p64, oneg)]["fmt"]["layout"] == "CSR-stream"
    for key, o in runs.items():                              # neither the pointer type nor the gather form changes a bit
        for k in oe.SWEEPS:
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(o["sweeps"][k], runs[(key[0], 0, 1)]["sweeps"][k])), (name, key, k)
    _report(name, "csr", runs)


# ---------------------------------------------------------------- SELL-64
@pytest.mark.parametrize("un", oe.SELL_UNROLLS)
@pytest.mark.parametrize("name", DISTINCT)
def test_sell_unrolls_blocks_gathers_deferral_remap(S, po, name, un):
    """sell_kernel<UN> with workgroups of 1 (auto), 2 and 4 waves, one-gather and two-gather sweeps, the deferred x update on and
    off (XM = 1 / 2 run with UN = 6 and one gather only) and the XCD remap on and off"""
    c = oe.case(name)
    runs = {}
    for block, oneg, defer, remap in itertools.product((0, 128, 256), (1, 0), (1, 0), (1, 0)):
        opt = dict(oe.CONFIGS["sell"], sell_un=un, sell_block=block, one_gather=oneg, sell_defer=defer, xcd_remap=remap)
        deferred = bool(oneg and defer and un == 6)
        sig = lambda i, d=deferred, g=oneg: ("sell_kernel<EPI_SWEEP,%s,UN=%d," % ("ONEG" if g else "2G", un),
                                             "XM=*" if d and i > 0 else "XM=0", "wpb=%d" % max(1, block // 64))
        # (op_apply depends on neither the gather form nor the deferral: it runs where both are at their defaults)
        runs[(block, oneg, defer, remap)] = _check_level(S, po, c, opt, "sell un=%d block=%d oneg=%d defer=%d remap=%d" % (un, block, oneg, defer, remap),
                                                         "sell", sig, ops=(oneg == 1 and defer == 1))
    _report(name, "sell UN=%d" % un, runs)


def test_sell_operands_eight_bytes_off_a_16_byte_boundary(S, po):
    """op_apply of A, P and R on device vectors viewed 8 bytes off a 16-byte boundary, in the SELL-64 and the CSR-stream layout"""
    c, ref = oe.case("ragged-129"), oe.reference("ragged-129")
    for cfg in ("sell", "csr", "sellc_idx16"):
        ns, _ = _setup(S, po, c, oe.CONFIGS[cfg], 1, 1)
        try:
            frac = _check_ops(ns, c, ref, oe.CONFIGS[cfg], cfg, offset=1)
        finally:
            ns.close()
        print("ragged-129 [%s] 8 bytes off: worst |y - exact| %.3g of the bound" % (cfg, frac))


# ---------------------------------------------------------------- SELL-C
@pytest.mark.parametrize("name", ("widths-few", "offsets-few", "ragged-4283-few", "wide"))
def test_sellc_dictionary_and_16_bit_offsets(S, po, name):
    """sellc_kernel<ONEG, VDICT, NT=0> (one- and two-gather sweeps, with and without the dictionary: the four instantiations a level
    of this size can reach) in its three forms -- dictionary + 16-bit offsets, 16-bit offsets alone, dictionary alone -- on
    matrices of exactly 256 distinct values: widths with w % 4 = 0 .. 3, w = 31, 32, 33 (one request round of 32 entries against
    two) and w = 65, 66 in 16-bit mode (base columns past lane 63); `wide` has R with 16- and 32-bit slices in one matrix"""
    c = oe.case(name)
    runs = {}
    for cfg, oneg in itertools.product(("sellc_dict_idx16", "sellc_idx16", "sellc_dict"), (1, 0)):
        runs[(cfg, oneg)] = _check_level(S, po, c, dict(oe.CONFIGS[cfg], one_gather=oneg), "%s oneg=%d" % (cfg, oneg), "sellc", ops=(oneg == 1))
        f = runs[(cfg, oneg)]["fmt"]
        assert (f["layout"], f["value_dictionary"], f["idx16"]) == ("SELL-64", cfg != "sellc_idx16", cfg != "sellc_dict"), (name, cfg, f)
    _report(name, "sellc", runs)


@pytest.mark.parametrize("name", ("widths-few+1", "offsets-few+1"))
def test_257_values_take_no_dictionary(S, po, name):
    c = oe.case(name)
    out = _check_level(S, po, c, oe.CONFIGS["sellc_dict_idx16"], "sellc_dict_idx16", "sellc")
    assert not out["fmt"]["value_dictionary"] and not out["fmt"]["idx16"], out["fmt"]
    _report(name, "sellc (257 values)", {0: out})


# ---------------------------------------------------------------- SELL-O
def test_sello_offset_patterns_and_base_columns(S, po):
    """sello_kernel on the distinct-valued `offsets` level (offsets relative to the row, rows clipped at the boundary shorter than
    the pattern width, dead lanes in the last slice of 29 rows), its P (a third as many columns as rows: offsets relative to a base column) and
    its R (base columns, truly empty rows); unrolls 3, 9, 27, deferred x update on and off"""
    c = oe.case("offsets")
    runs = {}
    for un, defer in itertools.product((3, 9, 27), (1, 0)):
        opt = dict(oe.CONFIGS["sello"], sell_un=un, sell_defer=defer)
        deferred = bool(defer and un < 27)
        sig = lambda i, d=deferred: ("sello_kernel<EPI_SWEEP,ONEG,UN=%d," % (9 if d and i > 0 else un), "XM=*" if d and i > 0 else "XM=0")
        runs[(un, defer)] = _check_level(S, po, c, opt, "sello un=%d defer=%d" % (un, defer), "sello", sig)
        assert runs[(un, defer)]["fmt"]["layout"] == "SELL-O"
    _report("offsets", "sello", runs)


# ---------------------------------------------------------------- default options
@pytest.mark.parametrize("name", oe.CASES)
def test_default_options(S, po, name):
    """no options: whatever layout the setup picks (recorded, not asserted) meets the same gates"""
    c = oe.case(name)
    out = _check_level(S, po, c, None, "default", "default")
    _report(name, "default", {0: out})


# ---------------------------------------------------------------- cycles: EPI_SUB, EPI_RESID, EPI_ADDTO and x_zero
CYCLE_CONFIGS = {
    "ragged-4283": ("csr", "sell", "sellc_idx16", "sello", None),
    "long": ("csr", "sell", "sellc_idx16", None),
    "widths": ("csr", "sell", "sellc_idx16", None),
    "widths-few": ("sellc_dict_idx16", "sellc_dict", None),
    "offsets": ("csr", "sell", "sello", None),
    "ragged-65": ("csr", "sell", None),
    "wide": ("sellc_dict_idx16", None),
}


@pytest.mark.parametrize("name", sorted(CYCLE_CONFIGS))
def test_vcycle_and_solver_mode_against_the_oracle(S, po, orc, name):
    """one V-cycle (preconditioner mode: x starts from zero, the sweeps' x_zero form) and three solver-mode iterations from a
    nonzero x with Richardson(Jacobi, 3, 2/3) before and after, on the hierarchies with ragged, empty-row and long-row P and R"""
    c = oe.case(name)
    H = _hier(po, c)
    sm = [orc.Smoother(orc.JACOBI, 3, oe.OMEGA)]
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1)
    zo, _, _, ho = go.solve(c.r0)
    gs = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, mode=orc.SOLVER, maxiter=3,
                 atol=1e-300, rtol=1e-300)
    xo, nit, flag, hs = gs.solve(c.r0, x=c.x0.copy())
    assert nit == 3 and np.all(np.isfinite(zo)) and np.all(np.isfinite(xo))
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    for cfg in CYCLE_CONFIGS[name]:
        opt = None if cfg is None else oe.CONFIGS[cfg]
        ns, gmg = _setup(S, po, c, opt, 3, 3)
        try:
            z = np.full(c.n, 123.0)
            S.solve_(z, ns, c.r0)
            fmt, sig = ns.level_format(0), ns.sweep_signature(0)
        finally:
            ns.close()
        hist = np.array(gmg.log.residuals[:2])
        ns, gmg2 = _setup(S, po, c, opt, 3, 3, mode="solver", maxiter=3, atol=1e-300, rtol=1e-300)
        try:
            x = c.x0.copy()
            S.solve_(x, ns, c.r0)
        finally:
            ns.close()
        hist2 = np.array(gmg2.log.residuals[:gmg2.log.num_iters + 1])
        dev = (rel(z, zo), float(np.max(np.abs(hist - ho) / ho)), rel(x, xo), float(np.max(np.abs(hist2 - hs) / hs)) if hist2.size == hs.size else np.inf)
        print("%s [%s] %s %s: V-cycle %.3e (history %.3e), 3 solver iterations %.3e (history %.3e)" % ((name, cfg or "default", fmt["layout"], sig) + dev))
        assert np.all(np.isfinite(z)) and np.all(np.isfinite(x)), (name, cfg)
        assert gmg2.log.num_iters == 3, (name, cfg, gmg2.log.num_iters)
        assert dev[0] <= TOL_VCYCLE and dev[2] <= TOL_VCYCLE, (name, cfg, dev)
        assert dev[1] <= TOL_HIST and dev[3] <= TOL_HIST, (name, cfg, dev)
        REACHED.setdefault(c.family, set()).add(("cycle " + (cfg or "default"), fmt["layout"], sig))


def test_zz_report_layouts_and_signatures_reached():
    """the run's record: per family, the layouts and sweep signatures the tests above reached"""
    for fam in sorted(REACHED):
        print(fam + ":")
        for row in sorted(REACHED[fam], key=str):
            print("    %-22s %-22s %s" % (row[0], row[1], row[2] or "(no sweep signature noted)"))
