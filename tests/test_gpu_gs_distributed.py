"""The Gauss-Seidel smoother on partitioned levels (rank-block sweeps, csrc/gs.inc.hpp) on the device: W virtual ranks folded onto one
rank, every message a self message through the host-staged loopback (the RCCL loopback in the child-process test).

  triangular solves   the general families of tests/halo_edge_problems.py (boundary counts 1, 63, 64, 65, one-way, uncoupled, fan-out,
                      W = 2, 3, 5) and gs_dist_reference.edge_case (W = 4: a rank of one row, a rank without boundary rows), types
                      forward / backward / symmetric, omega 1.0 / 1.2, orders natural / multicolour / given: the first dx of gmg_smooth
                      and gmg_precond_apply bit for bit the global form with the cross-rank entries removed (reference (b))
  whole passes        niter 1 and 3: x and r within fullsize_reference.TOL_KERNEL of reference (b) and bit for bit the twin that sums
                      the product as the library does; gs_pack_fused 0 and 1 the same bits; inert where the pack cannot fuse
  launch shapes       2-D Q1 96^2 cells, W = 4, multicolour: all wide launches, the x update folded at omega = 1;
                      3-D Q1 16^3 cells, W = 8, natural: chain launches; gmg_get_gs_schedule = gs_reference.schedule of the own block
  solves              CG + GMG with SymGaussSeidelSmoother(1) against the numpy twin with reference (b) per level; RCCL loopback
  errors              overlapping layout, zero owned diagonal, bad given orders, value refresh
The own x own streams are pinned to SELL-64 (rows sum in storage order) wherever the twin's bits are asserted."""
import ctypes as C
import importlib

import numpy as np
import pytest

import fullsize_reference as fr
import gs_dist_reference as gd
import gs_ordering_reference as go
import gs_reference as gr
import halo_edge_problems as he
import operator_edge_problems as oe
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_KERNEL = fr.TOL_KERNEL
BASE = dict(oe.CONFIGS["sell"])
FAMILIES = ("bnd-1", "bnd-63", "bnd-64", "bnd-65", "one-way", "uncoupled", "fan-out", "dict-255", "gs-edge")
ORDERS = ("natural", "multicolor", "given")
TYPES = ("forward", "backward", "symmetric")
OMEGAS = (1.0, 1.2)


def _mods(pkg):
    m = lambda n: importlib.import_module(pkg.__name__ + "." + n)
    return m("partition"), m("multigpu"), m("solvers"), m("abi")


def _case(name):
    return gd.edge_case() if name == "gs-edge" else he.case(name)


def _counts(c):
    return [len(c.spaces[0].own[q]) for q in range(c.W)]


_REF = {}


def _global(c):
    if c.name not in _REF:
        Af, blocks, perm = gd.folded(c.G["mats"][0], c.G["owners"][0])
        assert np.array_equal(perm, c.levels[0].own_gid) and np.array_equal(blocks, gd.blocks_of(_counts(c)))
        _REF[c.name] = (Af, blocks)
    return _REF[c.name]


def _order(c, kind):
    """-> (ordering of the reference: "natural" | "multicolor" | array, the permutation itself)"""
    T = gd.own_block(c.levels[0])
    if kind == "given":                                      # a seeded permutation per rank, stacked
        rng = np.random.default_rng(17)
        off = np.concatenate([[0], np.cumsum(_counts(c))])
        perm = np.concatenate([off[q] + rng.permutation(n) for q, n in enumerate(_counts(c))])
        return perm, perm
    return kind, go.resolve(T, kind)


def _handle(pkg, c, kind, sm_args=(1, 1.0, "symmetric"), transport="host_loopback", options=None, **kw):
    _, mg, sv, _ = _mods(pkg)
    ordering, perm = _order(c, kind)
    sm = sv.GaussSeidelSmoother(*sm_args, ordering=kind if kind != "given" else "natural")
    opts = dict(BASE)
    opts.update(options or {})
    return mg.DistributedGMG((1, 1), c.nlev, 0, 2, device_id=0, transport=transport, local_hierarchy=c.local, cells_global=(1, 1),
                             options=opts, smoother=sm, gs_orders=[perm] if kind == "given" else None, **kw)


def _reset(pkg, g, niter, omega, type_, lev=0):
    """another Gauss-Seidel smoother on the same handle: gmg_set_smoother_gauss_seidel + gmg_setup"""
    _, _, sv, abi = _mods(pkg)
    abi.check(g.h, g._lib.gmg_set_smoother_gauss_seidel(g.h, lev, abi.PRE_AND_POST, niter, omega, sv.GaussSeidelSmoother._TYPES[type_]))
    abi.check(g.h, g._lib.gmg_setup(g.h))


def _smooth(abi, g, x, r, lev=0):
    x, r = np.ascontiguousarray(x, dtype=np.float64).copy(), np.ascontiguousarray(r, dtype=np.float64).copy()
    abi.check(g.h, g._lib.gmg_smooth(g.h, lev, abi.PRE, C.c_void_p(x.ctypes.data), C.c_void_p(r.ctypes.data), abi.MEM_HOST))
    return x, r


def _precond(abi, g, r, lev=0):
    r = np.ascontiguousarray(r, dtype=np.float64).copy()
    z = np.full(r.size, np.nan)
    abi.check(g.h, g._lib.gmg_precond_apply(g.h, lev, abi.PRE, C.c_void_p(r.ctypes.data), C.c_void_p(z.ctypes.data), abi.MEM_HOST))
    return z


def _set_fused(abi, g, on):
    abi.check(g.h, g._lib.gmg_set_option(g.h, b"gs_pack_fused", float(on)))


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("name", FAMILIES)
def test_triangular_solves_are_bitwise_the_block_reference(pkg, name, kind):
    """niter = 1 from x = 0: x = omega dx of the first direction.  forward / backward: bit for bit omega * (T \\ r) of reference (b);
    symmetric: bit for bit the twin, whose first dx is reference (b)'s.  gmg_precond_apply (ldiv!) gives the same x."""
    abi = _mods(pkg)[3]
    c = _case(name)
    Af, blocks = _global(c)
    L = c.levels[0]
    r0 = he.own_vec(c, 0, c.r0)
    ordering, perm = _order(c, kind)
    g = _handle(pkg, c, kind)
    try:
        got = g.gs_ordering(0)
        assert got["kind"] == kind and np.array_equal(got["order"], perm)
        for type_ in TYPES:
            for omega in OMEGAS:
                _reset(pkg, g, 1, omega, type_)
                x, r = _smooth(abi, g, np.zeros(L.n_own), r0)
                tx, tr, first = gd.twin_pass(L, gr.GS(1, omega, type_), np.zeros(L.n_own), r0, perm)
                want = gd.first_dx(Af, blocks, r0, type_ != "backward", ordering)
                what = (name, kind, type_, omega)
                assert np.array_equal(first, want), what
                if type_ != "symmetric":
                    assert np.array_equal(x, omega * want), (what, np.flatnonzero(x != omega * want)[:8].tolist())
                assert np.array_equal(x, tx), (what, np.flatnonzero(x != tx)[:8].tolist())
                z = _precond(abi, g, r0)
                assert np.array_equal(z, tx), (what, "ldiv!", np.flatnonzero(z != tx)[:8].tolist())
    finally:
        g.close()


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("name", FAMILIES)
def test_whole_passes(pkg, name, kind):
    abi = _mods(pkg)[3]
    c = _case(name)
    Af, blocks = _global(c)
    L = c.levels[0]
    x0, r0 = he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0)
    ordering, perm = _order(c, kind)
    g = _handle(pkg, c, kind)
    try:
        info = g.halo_info(0)
        assert info["pack_fused"] == he.fusable(L)
        if name == "one-way":
            assert not info["pack_fused"]                    # the option has nothing to switch here: the same bits below
        for type_ in TYPES:
            for omega in OMEGAS:
                for niter in (1, 3):
                    _reset(pkg, g, niter, omega, type_)
                    sm = gr.GS(niter, omega, type_)
                    _set_fused(abi, g, 1)
                    x, r = _smooth(abi, g, x0, r0)
                    _set_fused(abi, g, 0)
                    x2, r2 = _smooth(abi, g, x0, r0)
                    _set_fused(abi, g, 1)
                    what = (name, kind, type_, omega, niter)
                    assert np.array_equal(he.bits(x), he.bits(x2)) and np.array_equal(he.bits(r), he.bits(r2)), (what, "gs_pack_fused 0 / 1 differ")
                    rx, rr = x0.copy(), r0.copy()
                    gd.solve_blocks(rx, Af, blocks, sm, rr, ordering)
                    dev = (oe.max_rel(x, rx), oe.max_rel(r, rr))
                    print(what, "max_rel x, r against reference (b):", dev)
                    assert max(dev) <= TOL_KERNEL, (what, dev)
                    tx, tr, _ = gd.twin_pass(L, sm, x0, r0, perm)
                    for got, want, v in ((x, tx, "x"), (r, tr, "r")):
                        nd = he.bit_mismatches(got, want)
                        assert nd.size == 0, (what, "%s differs from the float64 twin at" % v, nd[:8].tolist())
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ structured partitions
_POISSON = {}


def _poisson(pkg, po, cells, nlev, W, rep=None):
    """-> (folded local hierarchy, per level the rank of every owned row (None: replicated), the global hierarchy)"""
    key = (cells, nlev, W, rep)
    if key not in _POISSON:
        pa = _mods(pkg)[0]
        grid = pa.rank_grid(W, len(cells))
        locs = [pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, rep, None, "jacobi") for r in range(W)]
        blocks = [None if locs[0]["levels"][l].replicated else gd.blocks_of([h["levels"][l].n_own for h in locs]) for l in range(nlev)]
        _POISSON[key] = (pa.fold_ranks(locs), blocks, po.build_hierarchy(cells, nlev, 1))
    return _POISSON[key]


def _poisson_handle(pkg, F, cells, nlev, sm, transport="host_loopback", options=None, cycle_type="v_cycle"):
    mg = _mods(pkg)[1]
    return mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport=transport, local_hierarchy=F, cells_global=cells, options=options,
                             smoother=sm, cycle_type=cycle_type)


@pytest.mark.parametrize("cells,W,kind,shape", [((96, 96), 4, "multicolor", "wide"), ((16, 16, 16), 8, "natural", "chain")])
def test_launch_shapes(pkg, po, cells, W, kind, shape):
    _, _, sv, abi = _mods(pkg)
    F, blocks, H = _poisson(pkg, po, cells, 2, W)
    L = F["levels"][0]
    T = gd.own_block(L)
    B = go.permuted(T, go.resolve(T, kind))
    rng = np.random.default_rng(3)
    x0, r0 = rng.uniform(-1, 1, L.n_own), rng.uniform(-1, 1, L.n_own)
    Af = go.permuted(H["mats"][0].to_scipy(), L.own_gid)
    g = _poisson_handle(pkg, F, cells, 2, sv.GaussSeidelSmoother(1, 1.0, "symmetric", ordering=kind))
    try:
        sched = {}
        for fwd in (True, False):
            sched[fwd] = g.gs_schedule(0, fwd)
            assert tuple(sched[fwd][k] for k in ("nsets", "max_set_rows", "nlaunches", "nwide")) == gr.schedule(B, fwd), (fwd, sched[fwd])
            if shape == "wide":
                sizes = np.bincount(gr.level_sets(B, fwd))
                assert sizes.min() > gr.CHAIN_ROWS and sched[fwd]["nwide"] == sched[fwd]["nlaunches"] == sizes.size
            else:
                assert sched[fwd]["nwide"] == 0 and sched[fwd]["nlaunches"] == 1
        solve_launches = sched[True]["nlaunches"] + sched[False]["nlaunches"]
        for omega in OMEGAS:
            _reset(pkg, g, 1, omega, "symmetric")
            g.profile(0, True)
            x, r = _smooth(abi, g, x0, r0)
            launches = g.kernel_stats()["launches"]
            g.profile(0, False)
            folds = shape == "wide" and omega == 1.0            # the x update rides in the wide launches: no update launch
            assert launches == solve_launches + (0 if folds else 2), (shape, omega, launches, solve_launches)
            rx, rr = x0.copy(), r0.copy()
            gd.solve_blocks(rx, Af, blocks[0], gr.GS(1, omega, "symmetric"), rr, kind)
            dev = (oe.max_rel(x, rx), oe.max_rel(r, rr))
            print(shape, omega, "max_rel x, r against reference (b):", dev)
            assert max(dev) <= TOL_KERNEL, (shape, omega, dev)
    finally:
        g.close()


def _twin_solve(po, F, blocks, H, cells, kind, cycle):
    """CG + GMG with reference (b) per level on the global hierarchy in the folded numbering -> (x, iterations, history), b"""
    key = ("twin", cells, len(blocks), tuple(b is None for b in blocks), kind, cycle)
    if key not in _POISSON:
        lv = F["levels"]
        mats, Ps, Rs = gd.folded_hierarchy(H, lv)
        w = lambda Ms: [he._po_csr(po, M) for M in Ms]
        sms = [gd.BlockGS(1, 1.0, "symmetric", kind, blocks[l]) for l in range(len(lv) - 1)]
        G = gr.GMG(w(mats), w(Ps), w(Rs), sms, sms, cycle={"v_cycle": "v", "w_cycle": "w", "f_cycle": "f"}[cycle])
        b = po.dirichlet_lift_rhs(cells, 1)[lv[0].own_gid]
        _POISSON[key] = (gr.cg(mats[0], b, Pl=G.solve, maxiter=100, atol=1e-14, rtol=1e-8), b)
    return _POISSON[key]


def _device_solve(pkg, F, cells, nlev, kind, cycle, b, transport="host_loopback"):
    import torch
    sv = _mods(pkg)[2]
    g = _poisson_handle(pkg, F, cells, nlev, sv.SymGaussSeidelSmoother(1, 1.0, ordering=kind), transport=transport, cycle_type=cycle)
    try:
        bd = torch.from_numpy(np.ascontiguousarray(b)).cuda()
        x = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
        log = g.cg_solve(bd, x, maxiter=100, atol=1e-14, rtol=1e-8)
        torch.cuda.synchronize()
        return x.cpu().numpy(), log
    finally:
        g.close()


def _agree(sv, log, ref, x, tol=1e-10):
    xo, nit, hist = ref
    assert hist[-1] / hist[0] < 1e-8
    assert log.num_iters == nit and log.flag == sv.SOLVER_CONVERGED_RTOL, (log.num_iters, nit, log.flag)
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= 1e-8 * hist[0])
    assert rel_err(x, xo) <= tol


SOLVES = [((16, 16, 16), 3, 8, None), ((32, 32), 4, 4, 3), ((32, 32), 4, 4, 2)]   # the last: level 2 replicated AND smoothed, global sweeps there


@pytest.mark.parametrize("kind", ["natural", "multicolor"])
@pytest.mark.parametrize("cells,nlev,W,rep", SOLVES)
def test_cg_gmg_solves(pkg, po, cells, nlev, W, rep, kind):
    sv = _mods(pkg)[2]
    F, blocks, H = _poisson(pkg, po, cells, nlev, W, rep)
    assert [b is None for b in blocks] == [l >= (nlev - 1 if rep is None else rep) for l in range(nlev)]
    for cycle in (("v_cycle", "w_cycle", "f_cycle") if rep is None else ("v_cycle",)):
        ref, b = _twin_solve(po, F, blocks, H, cells, kind, cycle)
        x, log = _device_solve(pkg, F, cells, nlev, kind, cycle, b)
        print(cells, kind, cycle, "iterations", log.num_iters, "reference", ref[1])
        _agree(sv, log, ref, x)


@pytest.mark.child_process
@pytest.mark.parametrize("kind", ["natural", "multicolor"])
def test_rccl_loopback_is_bitwise_the_host_loopback(pkg, po, kind):
    cells, nlev, W, rep = SOLVES[0]
    F, blocks, H = _poisson(pkg, po, cells, nlev, W, rep)
    b = po.dirichlet_lift_rhs(cells, 1)[F["levels"][0].own_gid]
    xh, lh = _device_solve(pkg, F, cells, nlev, kind, "v_cycle", b)
    xr, lr = _device_solve(pkg, F, cells, nlev, kind, "v_cycle", b, transport="rccl_loopback")
    assert lr.num_iters == lh.num_iters and np.array_equal(xr, xh)
    assert np.array_equal(np.asarray(lr.residuals[: lr.num_iters + 1]), np.asarray(lh.residuals[: lh.num_iters + 1]))


def test_levels_handed_over_in_row_blocks_give_the_same_bits(pkg, po):
    """stream_rows > 0: the matrices of the own | ghost levels arrive in blocks of rows (gmg_set_operator_rows splits every block into
    the own x own stream and the ghost columns).  A Gauss-Seidel level gets its rows back for the tables and the column split: the bits
    of the handle that was given whole matrices."""
    import torch
    mg, sv = _mods(pkg)[1:3]
    cells, nlev, W, rep = SOLVES[0]
    F, blocks, H = _poisson(pkg, po, cells, nlev, W, rep)
    b = torch.from_numpy(np.ascontiguousarray(po.dirichlet_lift_rhs(cells, 1)[F["levels"][0].own_gid])).cuda()
    out = []
    for stream_rows in (0, 64):
        g = mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport="host_loopback", local_hierarchy=F, cells_global=cells,
                              smoother=sv.SymGaussSeidelSmoother(1, 1.0, ordering="multicolor"), stream_rows=stream_rows)
        try:
            assert (0 in g.streamed_levels) == (stream_rows > 0)
            x = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
            log = g.cg_solve(b, x, maxiter=100, atol=1e-14, rtol=1e-8)
            torch.cuda.synchronize()
            out.append((x.cpu().numpy(), np.asarray(log.residuals[: log.num_iters + 1]), g.gs_schedule(0, True)))
        finally:
            g.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


# ------------------------------------------------------------------------------------------------ refresh and errors
def test_value_refresh_is_bitwise_a_fresh_setup(pkg):
    """gmg_update_values with scaled values + gmg_setup on a partitioned level against a fresh setup with those values.  (A handle with
    a communicator of several ranks never refreshes in place: the setup that follows is a full one.)"""
    import copy
    abi = _mods(pkg)[3]
    c = _case("fan-out")
    L = c.levels[0]
    x0, r0 = he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0)
    scaled = np.ascontiguousarray(L.A.val * (1.0 + 0.25 * np.cos(np.arange(L.A.val.size))))
    out = {}
    g = _handle(pkg, c, "multicolor", (2, 1.2, "symmetric"))
    try:
        before = _smooth(abi, g, x0, r0)
        abi.check(g.h, g._lib.gmg_update_values(g.h, 0, C.c_void_p(scaled.ctypes.data)))
        abi.check(g.h, g._lib.gmg_setup(g.h))
        out["refreshed"] = _smooth(abi, g, x0, r0)
    finally:
        g.close()
    c2 = copy.copy(c)
    L2 = copy.copy(L)
    L2.A = type(L.A)(L.A.shape, L.A.ptr, L.A.idx, scaled)
    c2.levels = [L2] + list(c.levels[1:])
    c2.local = dict(c.local, levels=c2.levels)
    g = _handle(pkg, c2, "multicolor", (2, 1.2, "symmetric"))
    try:
        out["fresh"] = _smooth(abi, g, x0, r0)
    finally:
        g.close()
    for a, b in zip(out["refreshed"], out["fresh"]):
        assert np.array_equal(he.bits(a), he.bits(b))
    assert not np.array_equal(before[0], out["fresh"][0])


def _local_with(c, **changes):
    import copy
    L2 = copy.copy(c.levels[0])
    for k, v in changes.items():
        setattr(L2, k, v)
    levels = [L2] + list(c.levels[1:])
    c2 = copy.copy(c)
    c2.levels, c2.local = levels, dict(c.local, levels=levels)
    return c2


def test_errors(pkg, po):
    pa, mg, sv, abi = _mods(pkg)
    c = _case("bnd-65")
    L = c.levels[0]
    # a zero OWNED diagonal entry: GMG_ERR_SINGULAR naming the row
    S = he._to_scipy(L.A)
    row = 37
    k = S.indptr[row] + int(np.flatnonzero(S.indices[S.indptr[row]:S.indptr[row + 1]] == row)[0])
    val = L.A.val.copy()
    val[k] = 0.0
    with pytest.raises(abi.GmgError, match=r"zero diagonal entry in row 37 on level 0") as e:
        _handle(pkg, _local_with(c, A=type(L.A)(L.A.shape, L.A.ptr, L.A.idx, val)), "natural")
    assert e.value.code == abi.ERR_SINGULAR
    # a given order of the wrong length / with a repeat: the messages of one rank, with n_own
    n = L.n_own
    with pytest.raises(abi.GmgError, match=r"level 0: the order has %d entries, the level has %d rows \(position %d\)" % (n - 1, n, n - 1)):
        mg.DistributedGMG((1, 1), c.nlev, 0, 2, transport="host_loopback", local_hierarchy=c.local, cells_global=(1, 1), options=BASE,
                          smoother=sv.GaussSeidelSmoother(), gs_orders=[np.arange(n - 1)])
    rep = np.arange(n)
    rep[5] = 4
    with pytest.raises(abi.GmgError, match=r"level 0: not a permutation: position 5 holds row 4"):
        mg.DistributedGMG((1, 1), c.nlev, 0, 2, transport="host_loopback", local_hierarchy=c.local, cells_global=(1, 1), options=BASE,
                          smoother=sv.GaussSeidelSmoother(), gs_orders=[rep])
    # n_own + n_ghost entries are not an order of the level either
    with pytest.raises(abi.GmgError, match=r"the order has %d entries, the level has %d rows" % (n + L.n_ghost, n)):
        mg.DistributedGMG((1, 1), c.nlev, 0, 2, transport="host_loopback", local_hierarchy=c.local, cells_global=(1, 1), options=BASE,
                          smoother=sv.GaussSeidelSmoother(), gs_orders=[np.arange(n + L.n_ghost)])
    # the overlapping layout: refused by the driver before any handle exists, and by the library at gmg_setup naming level and layout
    with pytest.raises(ValueError, match="own . ghost layout"):
        mg.DistributedGMG((8, 8), 3, 0, 4, transport="host_loopback", smoother=sv.GaussSeidelSmoother(), depth=2)
    cells, nlev, W = (32, 32), 4, 4
    grid = pa.rank_grid(W, 2)
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, 3, [0, 2, 0, 0], "jacobi") for r in range(W)])
    g = mg.DistributedGMG(cells, nlev, 0, 2, transport="host_loopback", local_hierarchy=F, cells_global=cells)
    try:
        abi.check(g.h, g._lib.gmg_set_smoother_gauss_seidel(g.h, 1, abi.PRE_AND_POST, 1, 1.0, abi.GS_SYMMETRIC))
        rc = g._lib.gmg_setup(g.h)
        assert rc == abi.ERR_UNSUPPORTED
        with pytest.raises(abi.GmgError, match=r"level 1: the overlapping layout"):
            abi.check(g.h, rc)
    finally:
        g.close()
