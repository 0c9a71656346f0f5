"""The own | ghost split of a partitioned level -- ghost_fix_kernel, ghost_fix_sell_kernel<MODE, DICT>, halo_pack_kernel,
halo_unpack_add_kernel (csrc/comm.hpp) and the setup that feeds them (build_ghost_fix, the fused-pack tables, the split
restriction) -- on general, ragged partitions, against the references that tests/test_halo_edge_problems.py pins on the host
(tests/halo_edge_problems.py holds families, references, twins and gates).  One process, one GPU: W virtual ranks folded onto one
rank, every message a self message through the host-staged loopback (the RCCL loopback in the one child-process test).

Per family, under each of the six OPTION_SETS (the own x own streams are pinned to SELL-64, whose rows sum in storage order; the
slabs run a second time with no layout option changed, `plain`, where the gates are the bound and the tolerances):
  op_apply of A, R and P with three vectors in sequence on one handle (a stale ghost segment would show), output pre-filled with
    NaN between guard entries: the bits of the float64 twin, every row within gamma_k * sum|a x| of the exact value of the GLOBAL
    row, all option sets bit-identical (an unsplit R sums its whole row in storage order: its own twin);
  x[0] = inf on A and R: every row but row 0 finite and unchanged in bits;
  gmg_smooth PRE with 1 .. 5 Richardson(Jacobi) sweeps: the twin's bits where the signature shows no FMA taps, fr.TOL_KERNEL
    against the longdouble sweeps on the global matrix;
  two solver-mode iterations from a nonzero x (r = b - A x, r -= A dx: fix-up mode 1) against the sequential oracle on the global
    hierarchy: iteration count and flag, TOL_VCYCLE on x, TOL_HIST on the history;
  gmg_get_halo_info equals halo_edge_problems.expected_halo_info: the case reached the form its family was built for.
CG + GMG (widths, one-way, slabs) and the patch smoother's assemble! (patches) run under each option set as well; the RCCL
loopback repeats op_apply and a pass of three sweeps (see that test for why three)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import fullsize_reference as fr
import halo_edge_problems as he
import operator_edge_problems as oe
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_KERNEL, TOL_VCYCLE, TOL_HIST = fr.TOL_KERNEL, 1e-11, 1e-8
BASE = dict(oe.CONFIGS["sell"])
OPTION_SETS = {
    "default": {},
    "csr_fix": {"halo_fix_sell": 0},
    "no_dict": {"halo_fix_dict": 0},
    "no_fuse": {"halo_fuse_pack": 0},
    "unsplit_r": {"halo_split_r": 0},
    "async": {"host_async": 1, "overlap": 1},
}
REACHED = set()
WORST = {}                                                  # form -> largest |y - exact| as a fraction of the bound / largest max_rel of a sweep
FORMS = {("fix", f, m) for f in ("csr", "sliced", "sliced+dict") for m in (0, 1, 2, 3)} | \
        {("r", "sliced"), ("r", "sliced+dict"), ("r", "unsplit"), ("pack", "fused"), ("pack", "kernel"), ("fix", "none", 0), ("fix", "none", 2)}


def _mg(pkg):
    return importlib.import_module(pkg.__name__ + ".multigpu")


def _handle(pkg, c, options, niter=1, transport="host_loopback", plain=False, **kw):
    opts = {} if plain else dict(BASE)
    opts.update(options)
    return _mg(pkg).DistributedGMG((1, 1), c.nlev, 0, 2, device_id=0, transport=transport, local_hierarchy=c.local, cells_global=(1, 1),
                                   options=opts, niter=niter, omega=he.OMEGA, **kw)


def _device_op(g, lev, op, x_own, nout):
    """y = op x on device tensors; y lies between two guard entries of a NaN-filled buffer"""
    import torch
    from gridapsolvers_jl_amd import abi
    xd = torch.from_numpy(np.ascontiguousarray(x_own)).cuda()
    yb = torch.full((nout + 4,), np.nan, dtype=torch.float64, device="cuda")
    yd = yb[2:2 + nout]
    torch.cuda.synchronize()                              # the library runs on its own stream: torch's fills must be done first
    abi.check(g.h, g._lib.gmg_op_apply(g.h, lev, op, C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), abi.MEM_DEVICE))
    torch.cuda.synchronize()
    out = yb.cpu().numpy()
    assert np.all(np.isnan(out[:2])) and np.all(np.isnan(out[2 + nout:])), "op_apply wrote outside its vector"
    return out[2:2 + nout]


def _smooth(g, x, r):
    from gridapsolvers_jl_amd import abi
    x, r = np.ascontiguousarray(x).copy(), np.ascontiguousarray(r).copy()
    abi.check(g.h, g._lib.gmg_smooth(g.h, 0, abi.PRE, C.c_void_p(x.ctypes.data), C.c_void_p(r.ctypes.data), abi.MEM_HOST))
    return x, r


_REF = {}


def _op_reference(c, l, key, j, split):
    """(twin, (seq, exact, bound)) of vector j through operator `key` of level l, computed once"""
    k = (c.name, l, key, j, split)
    if k not in _REF:
        for kk, M, n_own, Mg, src, rows in he.operators(c, l):
            if kk == key:
                xg = c.XC[src][j]
                S = c.levels[src]
                v = xg if S.replicated else he.fill(S, he.own_vec(c, src, xg))
                ek = (c.name, l, key, j, "exact")
                if ek not in _REF:
                    _REF[ek] = he.exact_rows(Mg, rows, xg)
                _REF[k] = (he.twin_apply(M, n_own, v, split=split), _REF[ek])
    return _REF[k]


def _sweep_reference(c, k):
    key = (c.name, "sweeps", k)
    if key not in _REF:
        _REF[key] = (he.twin_sweeps(c, k), he.ref_sweeps(c, k))
    return _REF[key]


def _note(form, value):
    WORST[form] = max(WORST.get(form, 0.0), float(value))


def _check_info(g, c, options, tag):
    infos = []
    for l in range(c.part):
        info, want = g.halo_info(l), he.expected_halo_info(c, l, options)
        assert info == want, (c.name, tag, l, info, want)
        infos.append(info)
    return infos


def _check_ops(g, c, options, tag, bits_gate=True):
    """op_apply of A, R, P of every partitioned level on three vectors in sequence -> {(level, key, j): y}"""
    from gridapsolvers_jl_amd import abi
    infos = _check_info(g, c, options, tag)
    out = {}
    for l in range(c.part):
        split_r = infos[l]["r_split"]
        for key, M, n_own, Mg, src, rows in he.operators(c, l):
            op = dict(A=abi.OP_A, P=abi.OP_P, R=abi.OP_R)[key]
            form = ("fix", infos[l]["fix_form"], 0) if key == "A" else ("r", infos[l]["r_form"] if split_r else "unsplit") if key == "R" else ("p",)
            for j in range(3):
                y = _device_op(g, l, op, he.own_vec(c, src, c.XC[src][j]), M.shape[0])
                twin, ref = _op_reference(c, l, key, j, split_r or key != "R")
                what = (c.name, tag, "level %d op_apply %s vector %d" % (l, key, j))
                assert np.all(np.isfinite(y)), (what, "rows left unwritten or non-finite", np.flatnonzero(~np.isfinite(y))[:8].tolist())
                bad = he.bound_violations(y, ref)
                assert bad.size == 0, (what, "rows beyond gamma_k * sum|a x| of the exact value", bad[:8].tolist())
                if bits_gate:
                    nd = he.bit_mismatches(y, twin)
                    assert nd.size == 0, (what, "rows differ from the float64 twin", nd[:8].tolist())
                _note(form, he.bound_fraction(y, ref))
                out[(l, key, j)] = y
            REACHED.add(form)
    return out


def _check_inf(g, c, tag):
    from gridapsolvers_jl_amd import abi
    L = c.levels[0]
    x = he.own_vec(c, 0, c.X[0])
    xi = x.copy()
    xi[0] = np.inf
    for key, op, M in (("A", abi.OP_A, L.A), ("R", abi.OP_R, L.R)):
        fin, inf = _device_op(g, 0, op, x, M.shape[0]), _device_op(g, 0, op, xi, M.shape[0])
        bad = he.inf_violations(inf, fin, key == "A")
        assert bad.size == 0, (c.name, tag, key, "x[0] = inf reached rows other than row 0", bad[:8].tolist())
        if key == "A":
            assert not np.isfinite(inf[0])


def _check_sweeps(pkg, c, options, tag, plain=False):
    """1 .. 5 sweeps, one handle each -> {k: (x, r)}"""
    out = {}
    for k in he.SWEEPS:
        g = _handle(pkg, c, options, niter=k, plain=plain)
        try:
            info = g.halo_info(0)
            x, r = _smooth(g, he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0))
            sig = g.sweep_signature(0)
        finally:
            g.close()
        (tx, tr), (rx, rr) = _sweep_reference(c, k)
        assert np.all(np.isfinite(x)) and np.all(np.isfinite(r)), (c.name, tag, k, "smooth: non-finite output")
        dev = (oe.max_rel(x, rx), oe.max_rel(r, rr))
        mode = 3 if "rsweep" in sig or "r2sweep" in sig else 2
        form = ("fix", info["fix_form"], mode)
        _note(form, max(dev))
        assert max(dev) <= TOL_KERNEL, (c.name, tag, "%d sweeps" % k, sig, dev)
        if not plain and not fr.fma_taps(sig):
            for got, want, what in ((x, tx, "x"), (r, tr, "r")):
                nd = he.bit_mismatches(got, want)
                assert nd.size == 0, (c.name, tag, "%d sweeps: %s differs from the float64 twin at" % (k, what), sig, nd[:8].tolist())
        REACHED.add(form)
        if k >= 2 and info["boundary_rows"] > 0:
            REACHED.add(("pack", "fused" if info["pack_fused"] else "kernel"))
        out[k] = (x, r)
        out.setdefault("modes", set()).add(mode)
    return out


def _oracle_gmg(orc, po, c, k, **kw):
    H = [he._po_csr(po, M) for M in c.G["mats"]]
    P = [he._po_csr(po, M) for M in c.G["P"]]
    R = [he._po_csr(po, M) for M in c.G["R"]]
    sm = [orc.Smoother(orc.JACOBI, k, he.OMEGA)] * (c.nlev - 1)
    return H, orc.GMG(H, P, R, pre_smoothers=sm, post_smoothers=sm, **kw)


def _check_mode1(pkg, po, orc, c, options, tag, plain=False):
    """gmg_apply in solver mode, maxiter = 2, from a nonzero x: r = b - A x and r -= A dx finish their boundary rows with fix-up
    mode 1 (y -= ghost part) -> x"""
    key = (c.name, "solver mode")
    if key not in _REF:
        _, go = _oracle_gmg(orc, po, c, 3, mode=orc.SOLVER, maxiter=2, atol=1e-300, rtol=1e-300)
        _REF[key] = go.solve(c.r0, x=c.x0.copy())
    xo, nit, flag, ho = _REF[key]
    g = _handle(pkg, c, options, niter=3, plain=plain, mode="solver", gmg_maxiter=2, gmg_atol=1e-300, gmg_rtol=1e-300)
    try:
        info = g.halo_info(0)
        x = he.own_vec(c, 0, c.x0)
        log = g.apply(he.own_vec(c, 0, c.r0), x, maxiter=2)
    finally:
        g.close()
    hist = np.array(log.residuals[:log.num_iters + 1])
    assert log.num_iters == nit == 2 and log.flag == flag and np.all(np.isfinite(x)), (c.name, tag, log.num_iters, nit, log.flag, flag)
    dev = (rel_err(x, xo[c.levels[0].own_gid]), float(np.max(np.abs(hist - ho) / ho)))
    assert dev[0] <= TOL_VCYCLE and dev[1] <= TOL_HIST, (c.name, tag, "two solver iterations", dev)
    _note(("fix", info["fix_form"], 1), dev[0])
    REACHED.add(("fix", info["fix_form"], 1))
    return x


ALL = tuple(OPTION_SETS)


def _family(pkg, po, orc, name, inf=False):
    """every per-family check under each of the six option sets; every set must give the bits of the first (R under unsplit_r
    apart: an unsplit R is another sum)"""
    c = he.case(name)
    first, first_sw, first_x = None, None, None
    for tag in ALL:
        options = OPTION_SETS[tag]
        g = _handle(pkg, c, options)
        try:
            ys = _check_ops(g, c, options, tag)
            if inf:
                _check_inf(g, c, tag)
        finally:
            g.close()
        first = first or ys
        for k, y in ys.items():
            if not (tag == "unsplit_r" and k[1] == "R"):
                assert np.array_equal(he.bits(y), he.bits(first[k])), (name, tag, k, "differs from option set " + ALL[0])
        sw = _check_sweeps(pkg, c, options, tag)
        first_sw = first_sw or sw
        for k in he.SWEEPS:
            assert all(np.array_equal(he.bits(a), he.bits(b)) for a, b in zip(sw[k], first_sw[k])), (name, tag, k)
        x = _check_mode1(pkg, po, orc, c, options, tag)
        if tag != "unsplit_r":                               # (the cycle restricts: an unsplit R is another sum)
            first_x = x if first_x is None else first_x
            assert np.array_equal(he.bits(x), he.bits(first_x)), (name, tag, "solver mode differs from option set " + ALL[0])
    print("%s: %d option sets bit-identical" % (name, len(ALL)))


@pytest.mark.parametrize("N", he.BND)
def test_boundary_row_counts_at_slice_and_workgroup_edges(pkg, po, orc, N):
    """N = 1, 63, 64, 65, 255, 256, 257 boundary rows (and R_BND[N] of R): the 64-row slice and the 256-thread workgroup, the ragged
    last slice, the lanes that return at i >= nb"""
    _family(pkg, po, orc, "bnd-%d" % N, inf=True)


def test_slice_widths_every_remainder_of_the_quad_loop(pkg, po, orc):
    _family(pkg, po, orc, "widths", inf=True)


@pytest.mark.parametrize("name", ("dict-255", "dict-256", "dict-256-nopad"))
def test_dictionary_boundary_255_256_257_table_entries(pkg, po, orc, name):
    _family(pkg, po, orc, name, inf=True)


def test_fan_out_fused_pack_with_one_two_and_more_send_slots(pkg, po, orc):
    _family(pkg, po, orc, "fan-out", inf=True)


def test_one_way_pack_kernel_every_sweep_and_a_zero_length_message(pkg, po, orc):
    _family(pkg, po, orc, "one-way", inf=True)


def test_uncoupled_ranks_no_boundary_rows(pkg, po, orc):
    _family(pkg, po, orc, "uncoupled", inf=True)


def test_chain_two_partitioned_levels(pkg, po, orc):
    _family(pkg, po, orc, "chain", inf=True)


@pytest.mark.parametrize("name", sorted(he.SLABS))
def test_slabs_single_plane_slab_and_the_r_gathering_sweep(pkg, po, orc, name):
    """the Poisson slabs, first with no layout option changed -- the row-pattern own x own stream, and with it the sweep that
    gathers r (mode 3); the pattern kernels need not sum in storage order, so the gates there are the bound, TOL_KERNEL and
    TOL_VCYCLE -- then like every other family"""
    c = he.case(name)
    for tag in ALL:
        options = OPTION_SETS[tag]
        g = _handle(pkg, c, options, plain=True)
        try:
            _check_ops(g, c, options, tag + " (plain)", bits_gate=False)
        finally:
            g.close()
        sw = _check_sweeps(pkg, c, options, tag + " (plain)", plain=True)
        assert 3 in sw["modes"], "no pass of the slabs family took the sweep that gathers r: the mode-3 fix-up did not run"
        _check_mode1(pkg, po, orc, c, options, tag + " (plain)", plain=True)
    _family(pkg, po, orc, name)


# ---------------------------------------------------------------- CG
@pytest.mark.parametrize("name", ("widths", "one-way", "slabs", "slabs-16"))
def test_cg_gmg_against_the_oracle_on_the_global_hierarchy(pkg, po, orc, name):
    """CG + GMG under every option set (the slabs with no layout option changed): the oracle's iteration count and flag, its
    history within TOL_HIST, its solution within the 1e-10 of the loopback tests"""
    import torch
    c = he.case(name)
    H, go = _oracle_gmg(orc, po, c, 3, maxiter=1)
    b = c.r0
    xo, nit, flag, hist = orc.cg_solve(H[0], b, Pl=go, maxiter=20, atol=1e-14, rtol=1e-6)
    for tag in ALL:
        g = _handle(pkg, c, OPTION_SETS[tag], niter=3, plain=(name in he.SLABS))
        try:
            bd = torch.from_numpy(he.own_vec(c, 0, b)).cuda()
            xd = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            log = g.cg_solve(bd, xd, maxiter=20, atol=1e-14, rtol=1e-6)
            torch.cuda.synchronize()
            x = xd.cpu().numpy()
        finally:
            g.close()
        assert log.num_iters == nit and log.flag == flag, (name, tag, log.num_iters, nit, log.flag, flag)
        h = np.array(log.residuals[:log.num_iters + 1])
        dev = (float(np.max(np.abs(h - hist) / hist)), rel_err(x, xo[c.levels[0].own_gid]))
        print("%s [%s] CG + GMG: %d iterations, flag %d, history %.3e, solution %.3e" % (name, tag, nit, flag, dev[0], dev[1]))
        _note(("cg",), dev[0])
        assert dev[0] <= TOL_HIST and dev[1] < 1e-10, (name, tag, dev)


# ---------------------------------------------------------------- assemble!
def test_patch_smoother_assemble_in_neighbour_order(pkg):
    """gmg_precond_apply with the patch smoother on `patches`: consistent!(r), local solves, assemble!(dx) -- halo_unpack_add_kernel once
    per message in message order; an owned dof takes contributions of several neighbours, so the order decides the bits"""
    from gridapsolvers_jl_amd import abi
    c = he.case("patches")
    p = c.patch
    r = he.own_vec(c, 0, c.r0)
    twin = he.assemble(c, he.patch_contributions(c, r))
    ref = he.assemble(c, he.patch_contributions(c, r, exact=True), dtype=he.LD)
    tabs = [(p.ptr, p.dofs, p.blocks)] + [None] * (c.nlev - 1)
    for tag in ALL:
        g = _handle(pkg, c, OPTION_SETS[tag], smoother="patch", patch_tables=tabs)
        try:
            dx = np.full(r.size, np.nan)
            abi.check(g.h, g._lib.gmg_precond_apply(g.h, 0, abi.PRE, C.c_void_p(r.ctypes.data), C.c_void_p(dx.ctypes.data), abi.MEM_HOST))
        finally:
            g.close()
        assert np.all(np.isfinite(dx))
        dev = oe.max_rel(dx, ref)
        print("patches [%s]: assemble! max|dx - ref| / max|ref| %.3e" % (tag, dev))
        _note(("assemble",), dev)
        assert dev <= TOL_KERNEL, (tag, dev)
        nd = he.bit_mismatches(dx, twin)
        assert nd.size == 0, (tag, "dx differs from the twin's neighbour-order sum at", nd[:8].tolist())
    REACHED.add(("assemble",))


# ---------------------------------------------------------------- RCCL loopback
@pytest.mark.child_process
def test_rccl_loopback_gives_the_bits_of_the_host_loopback(pkg):
    """op_apply and a pass of three sweeps (pack kernel, then prepacked exchanges where the pack is fused) of widths, one-way and
    dict-256 with every message through RCCL (one real rank, self messages).  A smoother's sweep count is fixed at setup and every
    RCCL communicator takes about a second to create, so the pass lengths 1, 2, 4 and 5 are left to the host loopback: the
    transport sees a pass only as a sequence of exchanges, and three sweeps hold both kinds (packed by kernel, prepacked)."""
    for name in ("widths", "one-way", "dict-256"):
        c = he.case(name)
        res = {}
        for tr in ("host_loopback", "rccl_loopback"):
            g = _handle(pkg, c, {}, niter=3, transport=tr)    # (one communicator per family: creating one takes a second)
            try:
                assert g.comm_info()["transport"] == ("host" if tr == "host_loopback" else "rccl")
                ys = _check_ops(g, c, {}, tr)
                sw = {3: _smooth(g, he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0))}
            finally:
                g.close()
            (tx, tr_), _ = _sweep_reference(c, 3)
            assert he.bit_mismatches(sw[3][0], tx).size == 0 and he.bit_mismatches(sw[3][1], tr_).size == 0, (name, tr)
            res[tr] = (ys, sw)
        h, r = res["host_loopback"], res["rccl_loopback"]
        assert all(np.array_equal(he.bits(h[0][k]), he.bits(r[0][k])) for k in h[0]), name
        assert all(np.array_equal(he.bits(a), he.bits(b)) for k in h[1] for a, b in zip(h[1][k], r[1][k])), name


def test_halo_info_error_paths_and_null_outputs(pkg, S, po):
    """gmg_get_halo_info: any output may be NULL; GMG_ERR_STATE before a setup, on a replicated level and on a single-rank handle;
    GMG_ERR_INVALID for a level out of range"""
    from gridapsolvers_jl_amd import abi
    lib = abi.load()
    null = [None] * 11
    c = he.case("bnd-1")
    g = _handle(pkg, c, {})
    try:
        assert lib.gmg_get_halo_info(g.h, 0, *null) == abi.OK
        nb = C.c_int64(-1)
        assert lib.gmg_get_halo_info(g.h, 0, C.byref(nb), *null[1:]) == abi.OK and nb.value == 1
        assert lib.gmg_get_halo_info(g.h, 1, *null) == abi.ERR_STATE            # the replicated coarsest level
        assert lib.gmg_get_halo_info(g.h, 2, *null) == abi.ERR_INVALID and lib.gmg_get_halo_info(g.h, -1, *null) == abi.ERR_INVALID
        with pytest.raises(abi.GmgError):
            g.halo_info(1)
    finally:
        g.close()
    h = C.c_void_p()
    abi.check(None, lib.gmg_create(C.byref(h), 2, 0))
    try:
        assert lib.gmg_get_halo_info(h, 0, *null) == abi.ERR_STATE              # before gmg_setup
    finally:
        lib.gmg_destroy(h)
    e = oe.case("ragged-65")
    csr = lambda M: po.CSR(M.shape, M.indptr, M.indices, M.data)
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 1, he.OMEGA)]
    gmg = S.GMGLinearSolver([csr(e.A), csr(e.Ac)], [csr(e.P)], [csr(e.R)], pre_smoothers=sm, post_smoothers=sm, maxiter=1)
    ns = S.numerical_setup(S.symbolic_setup(gmg, gmg.smatrices[0]), gmg.smatrices[0])
    try:
        assert lib.gmg_get_halo_info(ns.h, 0, *null) == abi.ERR_STATE           # one rank: no partitioned level
    finally:
        ns.close()


def test_zz_every_form_was_reached():
    """the run's record: the forms the cases above reached, with the largest deviation measured per form; every form the own |
    ghost split has must be among them.  The FORM (none / CSR / sliced / sliced + dictionary, R split or not, pack fused or not)
    is what gmg_get_halo_info reported and each case asserted against the family's census.  The kernel MODE is not reported by
    the library: 0 = op_apply of A ran, 1 = a solver-mode cycle ran (r = b - A x, r -= A dx), 2 / 3 = a sweep ran whose
    sweep_signature names the s-carrying / the r-gathering kernel -- the entry points that launch that mode and no other."""
    for form in sorted(REACHED, key=str):
        print("    %-34s %.3e" % (" ".join(str(f) for f in form), WORST.get(form, 0.0)))
    missing = FORMS - REACHED
    assert not missing, sorted(missing, key=str)
