"""The ChebyshevSmoother on partitioned levels (csrc/cheb.inc.hpp, SEVERAL RANKS) on the device: W virtual ranks folded onto one rank,
every message a self message through the host-staged loopback (the RCCL loopback in the child-process test), and two TRUE ranks as
threads of a child process.

  passes, Jacobi M    the general families of tests/halo_edge_problems.py (boundary counts 1, 63, 64, 65, one-way, uncoupled, fan-out,
                      dict-255, W = 2, 3, 5) and gs_dist_reference.edge_case (W = 4: a rank of one row, a pack that cannot fuse), degrees
                      1, 3, 4, given bounds, from x = 0 and x != 0: bit for bit the folded twin (cheb_dist_reference.twin_pass), within
                      fullsize_reference.TOL_KERNEL of the global reference; cheb_pack_fused 0 / 1 the same bits and one launch per sweep
                      apart where the pack fuses; degree 1 = the device Richardson sweep with omega = 1/theta
  passes, patch M     `patches`: consistent!(r), local solves, assemble!(z), update -- bit for bit the twin; gmg_precond_apply = assembled z
  estimates           Q1 16^3 cells W = 8 and Q1 96^2 cells W = 4: power / Lanczos, 4 / 10 steps against the twin from the stacked start
                      vector; replicated levels bitwise the single-GPU handle; a value refresh bitwise a fresh setup
  solves              CG + GMG(Chebyshev(Jacobi, 3)) and FGMRES(5) + GMG(Chebyshev(patch, 4)) against the numpy twin; RCCL loopback
  two true ranks      lambda_est per level against the twin with the per-rank start vector, CG iterations, one pass bitwise the folded run
  errors              overlapping layout, rank subset, a communicator without a layout
The own x own streams are pinned to SELL-64 (rows sum in storage order) wherever the twin's bits are asserted."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import chebyshev_reference as cr
import cheb_dist_reference as cd
import cheb_dist_worker as cw
import fullsize_reference as fr
import gs_dist_reference as gd
import halo_edge_problems as he
import numpy_twin as nt
import operator_edge_problems as oe
from conftest import rel_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TOL_KERNEL = fr.TOL_KERNEL
TOL_EST = 1e-8                                               # lambda_est against the twin: the bound of tests/test_gpu_chebyshev.py
BASE = dict(oe.CONFIGS["sell"])
FAMILIES = ("bnd-1", "bnd-63", "bnd-64", "bnd-65", "one-way", "uncoupled", "fan-out", "dict-255", "gs-edge")
DEGREES = (1, 3, 4)


def _mods(pkg):
    m = lambda n: importlib.import_module(pkg.__name__ + "." + n)
    return m("partition"), m("multigpu"), m("solvers"), m("abi")


def _case(name):
    return gd.edge_case() if name == "gs-edge" else he.case(name)


def given_bounds(Af):
    """lambda_max = ||D^-1 A||_inf, lambda_min = lambda_max / 10"""
    lmax = float(np.max(np.abs(Af).sum(axis=1).A1 / np.abs(Af.diagonal())))
    return lmax / 10.0, lmax


def _handle(pkg, c, cheb, transport="host_loopback", options=None, **kw):
    mg = _mods(pkg)[1]
    opts = dict(BASE)
    opts.update(options or {})
    return mg.DistributedGMG((1, 1), c.nlev, 0, 2, device_id=0, transport=transport, local_hierarchy=c.local, cells_global=(1, 1),
                             options=opts, chebyshev=cheb, **kw)


def _reset(abi, g, degree, lmin=0.0, lmax=0.0, method="power", steps=10, lev=0):
    """other Chebyshev parameters on the slot's M: gmg_set_smoother_chebyshev [+ gmg_set_chebyshev_eig_method] + gmg_setup"""
    abi.check(g.h, g._lib.gmg_set_smoother_chebyshev(g.h, lev, abi.PRE_AND_POST, degree, lmin, lmax, steps, 10.0, 1.1))
    if method != "power":
        abi.check(g.h, g._lib.gmg_set_chebyshev_eig_method(g.h, lev, abi.PRE_AND_POST, abi.CHEB_EIG_LANCZOS))
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
    abi.check(g.h, g._lib.gmg_set_option(g.h, b"cheb_pack_fused", float(on)))


def _profiled_pass(abi, g, x, r):
    g.profile(0, True)
    out = _smooth(abi, g, x, r)
    launches = g.kernel_stats()["launches"]
    g.profile(0, False)
    return out, launches


def _same_bits(got, want, what):
    for a, b, v in zip(got, want, ("x", "r")):
        nd = he.bit_mismatches(a, b)
        assert nd.size == 0, (what, "%s differs at" % v, nd[:8].tolist())


# ------------------------------------------------------------------------------------------------ passes
@pytest.mark.parametrize("name", FAMILIES)
def test_jacobi_passes(pkg, name):
    abi = _mods(pkg)[3]
    c = _case(name)
    L = c.levels[0]
    Af, _, perm = gd.folded(c.G["mats"][0], c.G["owners"][0])
    assert np.array_equal(perm, L.own_gid)
    lmin, lmax = given_bounds(Af)
    M = nt.Jacobi(Af)
    x0, r0 = he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0)
    fuses = he.fusable(L)
    g = _handle(pkg, c, dict(degree=3, lambda_min=lmin, lambda_max=lmax))
    try:
        assert g.halo_info(0)["pack_fused"] == fuses
        assert g.sweep_signature(0).endswith(" cheb=3/3")
        if name in ("one-way", "gs-edge"):
            assert not fuses                                 # the option has nothing to switch here: the same bits and launches below
        for m in DEGREES:
            _reset(abi, g, m, lmin, lmax)
            info = g.chebyshev_info(0)
            assert np.isnan(info["lambda_est"]) and (info["degree"], info["lambda_min"], info["lambda_max"]) == (m, lmin, lmax)
            co = cr.coefficients(m, lmin, lmax)
            for x_zero in (False, True):
                xs = np.zeros(L.n_own) if x_zero else x0
                what = (name, m, "x = 0" if x_zero else "x != 0")
                _set_fused(abi, g, 1)
                got, n1 = _profiled_pass(abi, g, xs, r0)
                _set_fused(abi, g, 0)
                got0, n0 = _profiled_pass(abi, g, xs, r0)
                _set_fused(abi, g, 1)
                _same_bits(got, got0, (what, "cheb_pack_fused 0 / 1"))
                assert n0 - n1 == (m if fuses else 0), (what, "launches", n1, n0)
                rx, rr = cr.chebyshev(Af, M, co, xs.copy(), r0.copy())
                dev = (oe.max_rel(got[0], rx), oe.max_rel(got[1], rr))
                print(what, "launches fused / unfused", n1, n0, "max_rel x, r against the global reference:", dev)
                assert max(dev) <= TOL_KERNEL, (what, dev)
                _same_bits(got, cd.twin_pass(L, co, xs, r0, "jacobi"), (what, "float64 twin"))
            z = _precond(abi, g, r0)
            assert np.array_equal(he.bits(z), he.bits(cd.dinv(L) * r0)), (name, m, "gmg_precond_apply")
        # degree 1 is one Richardson sweep with omega = 1/theta: the device's own
        _reset(abi, g, 1, lmin, lmax)
        cheb1 = _smooth(abi, g, x0, r0)
        omega = 1.0 / ((lmax + lmin) / 2.0)
        abi.check(g.h, g._lib.gmg_set_smoother_jacobi(g.h, 0, abi.PRE_AND_POST, 1, omega))
        abi.check(g.h, g._lib.gmg_setup(g.h))
        assert " cheb=" not in g.sweep_signature(0)
        _same_bits(cheb1, _smooth(abi, g, x0, r0), (name, "degree 1 against Richardson(Jacobi, 1, 1/theta)"))
    finally:
        g.close()


def test_patch_passes(pkg):
    """`patches` (fan-out with ragged patches reaching into the ghost dofs of two neighbours): every sweep is consistent!(r), the local
    solves, the gather over all local dofs, assemble!(z) in message order, the update on the owned rows, r -= A d"""
    abi = _mods(pkg)[3]
    c = he.case("patches")
    L, p = c.levels[0], c.patch
    Af, _, perm = gd.folded(c.G["mats"][0], c.G["owners"][0])
    pos = np.empty(perm.size, dtype=np.int64)
    pos[perm] = np.arange(perm.size)
    Mg = nt.Patch(Af, p.pp, pos[p.pd])
    Mt = cd.patch_M(c)
    x0, r0 = he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0)
    tabs = [(p.ptr, p.dofs, p.blocks)] + [None] * (c.nlev - 1)
    lmin, lmax = 0.2, 2.0
    g = _handle(pkg, c, dict(degree=3, lambda_min=lmin, lambda_max=lmax), smoother="patch", patch_tables=tabs)
    try:
        z = _precond(abi, g, r0)
        nd = he.bit_mismatches(z, Mt(r0))
        assert nd.size == 0, ("gmg_precond_apply differs from the assembled z at", nd[:8].tolist())
        for m in DEGREES:
            _reset(abi, g, m, lmin, lmax)
            co = cr.coefficients(m, lmin, lmax)
            for x_zero in (False, True):
                xs = np.zeros(L.n_own) if x_zero else x0
                what = ("patches", m, "x = 0" if x_zero else "x != 0")
                _set_fused(abi, g, 1)
                got, n1 = _profiled_pass(abi, g, xs, r0)
                _set_fused(abi, g, 0)
                got0, n0 = _profiled_pass(abi, g, xs, r0)
                _set_fused(abi, g, 1)
                _same_bits(got, got0, (what, "cheb_pack_fused 0 / 1"))
                assert n0 - n1 == (m if he.fusable(L) else 0), (what, "launches", n1, n0)
                rx, rr = cr.chebyshev(Af, Mg, co, xs.copy(), r0.copy())
                dev = (oe.max_rel(got[0], rx), oe.max_rel(got[1], rr))
                print(what, "max_rel x, r against the global reference:", dev)
                assert max(dev) <= TOL_KERNEL, (what, dev)
                _same_bits(got, cd.twin_pass(L, co, xs, r0, Mt), (what, "float64 twin"))
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ structured partitions
_POISSON = {}


def _poisson(pkg, po, cells, nlev, W, rep=None, order=1):
    """-> (folded local hierarchy, the global hierarchy)"""
    key = (cells, nlev, W, rep, order)
    if key not in _POISSON:
        pa = _mods(pkg)[0]
        grid = pa.rank_grid(W, len(cells))
        locs = [pa.build_local_hierarchy(cells, nlev, grid, r, order, None, rep, None, "jacobi") for r in range(W)]
        _POISSON[key] = (pa.fold_ranks(locs), po.build_hierarchy(cells, nlev, order))
    return _POISSON[key]


def _poisson_handle(pkg, F, cells, nlev, cheb, transport="host_loopback", options=None, **kw):
    mg = _mods(pkg)[1]
    return mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport=transport, local_hierarchy=F, cells_global=cells, options=options,
                             chebyshev=cheb, **kw)


@pytest.mark.parametrize("cells,W", [((16, 16, 16), 8), ((96, 96), 4)])
def test_estimates_on_a_partitioned_level(pkg, po, cells, W):
    """SPD (Q1 Poisson), so Lanczos applies.  The folded handle's start vector is the stacked index: the twin is the single-handle
    estimate of the folded matrix"""
    abi = _mods(pkg)[3]
    F, H = _poisson(pkg, po, cells, 2, W)
    Af = gd.folded_hierarchy(H, F["levels"])[0][0]
    M = nt.Jacobi(Af)
    v0 = cd.start_vector([Af.shape[0]])
    g = _poisson_handle(pkg, F, cells, 2, dict(degree=3))
    try:
        for method in ("power", "lanczos"):
            for steps in (4, 10):
                _reset(abi, g, 3, 0.0, 0.0, method, steps)
                info = g.chebyshev_info(0)
                want = cd.estimate(Af, M, method, steps, v0)
                dev = abs(info["lambda_est"] - want) / want
                print(cells, method, steps, "lambda_est %.12f twin %.12f rel %.2e" % (info["lambda_est"], want, dev))
                assert dev <= TOL_EST, (method, steps, info, want)
                assert (info["eig_method"], info["eig_steps_done"]) == (method, steps)
                assert info["lambda_max"] == 1.1 * info["lambda_est"] and info["lambda_min"] == info["lambda_max"] / 10.0
    finally:
        g.close()


def test_estimates_on_a_replicated_level_are_the_single_gpu_handle_s(pkg, po, S):
    """(32, 32) cells, 4 levels, W = 4, levels 2 and 3 replicated, level 2 smoothed: its estimate is made of local reductions over the
    global matrix -- the bits of the same level on a handle without a communicator"""
    cells, nlev, W, rep = (32, 32), 4, 4, 2
    F, H = _poisson(pkg, po, cells, nlev, W, rep)
    assert [L.replicated for L in F["levels"]] == [False, False, True, True]
    out = {}
    for method in ("power", "lanczos"):
        g = _poisson_handle(pkg, F, cells, nlev, dict(degree=3, eig_method=method))
        try:
            out[method] = g.chebyshev_info(2)
        finally:
            g.close()
        sms = [S.ChebyshevSmoother(S.JacobiLinearSolver(), 3, eig_method=method) for _ in range(nlev - 1)]
        gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sms, post_smoothers=sms, maxiter=1)
        ns = S.numerical_setup(S.symbolic_setup(gmg, gmg.smatrices[0]), gmg.smatrices[0])
        try:
            one = ns.chebyshev_info(2)
        finally:
            ns.close()
        assert out[method] == one, (method, out[method], one)
        assert out[method]["lambda_est"] > 1.0


def test_value_refresh_is_bitwise_a_fresh_setup(pkg):
    """gmg_update_values with scaled values + gmg_setup on a partitioned level: the estimate is made again, with the bits of a fresh
    setup on those values; so is the pass"""
    import copy
    abi = _mods(pkg)[3]
    c = _case("fan-out")
    L = c.levels[0]
    x0, r0 = he.own_vec(c, 0, c.x0), he.own_vec(c, 0, c.r0)
    scaled = np.ascontiguousarray(L.A.val * (1.0 + 0.25 * np.cos(np.arange(L.A.val.size))))
    out = {}
    g = _handle(pkg, c, dict(degree=3))
    try:
        before = (g.chebyshev_info(0), _smooth(abi, g, x0, r0))
        abi.check(g.h, g._lib.gmg_update_values(g.h, 0, C.c_void_p(scaled.ctypes.data)))
        abi.check(g.h, g._lib.gmg_setup(g.h))
        out["refreshed"] = (g.chebyshev_info(0), _smooth(abi, g, x0, r0))
    finally:
        g.close()
    c2, L2 = copy.copy(c), copy.copy(L)
    L2.A = type(L.A)(L.A.shape, L.A.ptr, L.A.idx, scaled)
    c2.levels = [L2] + list(c.levels[1:])
    c2.local = dict(c.local, levels=c2.levels)
    g = _handle(pkg, c2, dict(degree=3))
    try:
        out["fresh"] = (g.chebyshev_info(0), _smooth(abi, g, x0, r0))
    finally:
        g.close()
    assert out["refreshed"][0] == out["fresh"][0] and out["fresh"][0]["lambda_est"] != before[0]["lambda_est"]
    _same_bits(out["refreshed"][1], out["fresh"][1], "refreshed against fresh")


# ------------------------------------------------------------------------------------------------ solves
def _agree(sv, log, ref, x):
    xo, nit, hist = ref
    assert log.num_iters == nit and log.flag == sv.SOLVER_CONVERGED_RTOL, (log.num_iters, nit, log.flag)
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= 1e-10 * hist[0])
    assert rel_err(x, xo) <= 1e-10


CG_CASE = ((16, 16, 16), 3, 8)


def _cg_device(pkg, F, cells, nlev, method, b, transport="host_loopback"):
    import torch
    g = _poisson_handle(pkg, F, cells, nlev, dict(degree=3, eig_method=method), transport=transport)
    try:
        bd = torch.from_numpy(np.ascontiguousarray(b)).cuda()
        x = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
        log = g.cg_solve(bd, x, maxiter=100, atol=1e-14, rtol=1e-8)
        torch.cuda.synchronize()
        return x.cpu().numpy(), log, [g.sweep_signature(l) for l in range(nlev)], [g.chebyshev_info(l)["lambda_est"] for l in range(nlev - 1)]
    finally:
        g.close()


@pytest.mark.parametrize("method", ["power", "lanczos"])
def test_cg_gmg_solve(pkg, po, method):
    sv = _mods(pkg)[2]
    cells, nlev, W = CG_CASE
    F, H = _poisson(pkg, po, cells, nlev, W)
    lv = F["levels"]
    G, mats = cd.gmg_twin(H, lv, ["jacobi"] * (nlev - 1), 3, method)
    b = po.dirichlet_lift_rhs(cells, 1)[lv[0].own_gid]
    ref = cr.cg(mats[0], b, Pl=G.solve, maxiter=100, atol=1e-14, rtol=1e-8)
    assert ref[2][-1] / ref[2][0] < 1e-8
    x, log, sigs, lest = _cg_device(pkg, F, cells, nlev, method, b)
    print(method, "iterations", log.num_iters, "twin", ref[1], "lambda_est", lest, "twin", [ns[3][0] for ns in G.pre_ns])
    for l in range(nlev - 1):
        assert abs(lest[l] - G.pre_ns[l][3][0]) <= TOL_EST * G.pre_ns[l][3][0]
        assert sigs[l].endswith(" cheb=3/3"), sigs
    assert " cheb=" not in sigs[-1]
    _agree(sv, log, ref, x)


def test_fgmres_gmg_patch_solve(pkg, po):
    """Q2 on 8^3 cells, 2 x 2 x 2 folded, two levels (the smallest Q2 partition of tests/test_loopback.py's patch tests): vertex-star
    patches owned per rank with driver-assembled matrices, Chebyshev(patch, 4) with the default estimate, FGMRES(5) outside"""
    import torch
    pa, mg, sv, abi = _mods(pkg)
    cells, nlev, W, order = (8, 8, 8), 2, 8, 2
    F, H = _poisson(pkg, po, cells, nlev, W, order=order)
    lv = F["levels"]
    gid = np.asarray(lv[0].own_gid, dtype=np.int64)
    pos = np.empty(gid.size, dtype=np.int64)
    pos[gid] = np.arange(gid.size)
    pp, rows = po.vertex_star_patches(H["ncells"][0], order)
    G, mats = cd.gmg_twin(H, lv, [("patch", pp, pos[np.asarray(rows, dtype=np.int64)])], 4)
    b = po.dirichlet_lift_rhs(cells, order)[gid]
    ref = cr.fgmres(mats[0], b, Pr=G.solve, m=5, maxiter=100, atol=1e-14, rtol=1e-8)
    assert ref[2][-1] / ref[2][0] < 1e-8
    g = mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport="host_loopback", local_hierarchy=F, cells_global=cells, order=order,
                          smoother="patch", patch_tables=pa.fold_patch_tables(F), chebyshev=dict(degree=4))
    try:
        bd = torch.from_numpy(np.ascontiguousarray(b)).cuda()
        x = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
        log = g.fgmres_solve(bd, x, m=5, maxiter=100, atol=1e-14, rtol=1e-8)
        torch.cuda.synchronize()
        x = x.cpu().numpy()
        lest, sig = g.chebyshev_info(0)["lambda_est"], g.sweep_signature(0)
    finally:
        g.close()
    want = G.pre_ns[0][3][0]
    print("iterations", log.num_iters, "twin", ref[1], "lambda_est %.12f twin %.12f" % (lest, want))
    assert abs(lest - want) <= TOL_EST * want and sig.endswith(" cheb=4/4")
    _agree(sv, log, ref, x)


@pytest.mark.child_process
def test_rccl_loopback_is_bitwise_the_host_loopback(pkg, po):
    cells, nlev, W = CG_CASE
    F, H = _poisson(pkg, po, cells, nlev, W)
    b = po.dirichlet_lift_rhs(cells, 1)[F["levels"][0].own_gid]
    xh, lh, _, eh = _cg_device(pkg, F, cells, nlev, "lanczos", b)
    xr, lr_, _, er = _cg_device(pkg, F, cells, nlev, "lanczos", b, transport="rccl_loopback")
    assert eh == er
    assert lr_.num_iters == lh.num_iters and np.array_equal(xr, xh)
    assert np.array_equal(np.asarray(lr_.residuals[: lr_.num_iters + 1]), np.asarray(lh.residuals[: lh.num_iters + 1]))


# ------------------------------------------------------------------------------------------------ two true ranks
def test_two_true_ranks(pkg, po, tmp_path):
    """Threads of one child process, host transport.  A loopback all-reduce is the identity, so only true ranks show a reduction the
    estimate forgot: lambda_est per level against the twin whose start vector restarts its index on every rank, the CG iteration count
    of that twin, and one pass with given bounds bit for bit the W = 2 folded run."""
    pa, mg, sv, abi = _mods(pkg)
    cells, nlev = (16, 16, 16), 3
    out = os.path.join(str(tmp_path), "ranks.npz")
    env = dict(os.environ, OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "cheb_dist_worker.py"), out, "x".join(map(str, cells)), str(nlev)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    v = np.load(out)
    H = po.build_hierarchy(cells, nlev, 1)
    gids = [np.concatenate([v["gid_%d_0" % l], v["gid_%d_1" % l]]) for l in range(nlev - 1)] + [np.arange(H["mats"][nlev - 1].shape[0])]
    counts = [[v["gid_%d_0" % l].size, v["gid_%d_1" % l].size] for l in range(nlev - 1)]
    levels = [type("L", (), dict(own_gid=q)) for q in gids]
    G, mats = cd.gmg_twin(H, levels, ["jacobi"] * (nlev - 1), cw.DEGREE, "power", counts)
    b = po.dirichlet_lift_rhs(cells, 1)[gids[0]]
    xo, nit, hist = cr.cg(mats[0], b, Pl=G.solve, maxiter=100, atol=1e-14, rtol=1e-8)
    assert np.array_equal(v["lest_0"], v["lest_1"])         # reduced scalars: one estimate on both ranks
    for l in range(nlev - 1):
        want = G.pre_ns[l][3][0]
        stacked = cd.estimate(mats[l], nt.Jacobi(mats[l]), "power", 10, cd.start_vector([mats[l].shape[0]]))
        print("level", l, "lambda_est %.12f twin (per-rank start vector) %.12f twin (stacked) %.12f" % (v["lest_0"][l], want, stacked))
        assert abs(v["lest_0"][l] - want) <= TOL_EST * want, (l, v["lest_0"][l], want)
    x = np.concatenate([v["x_0"], v["x_1"]])
    print("iterations", int(v["iters_0"]), "twin", nit, "x rel", rel_err(x, xo))
    assert int(v["iters_0"]) == int(v["iters_1"]) == nit and np.array_equal(he.bits(v["hist_0"]), he.bits(v["hist_1"]))
    # the pass with given bounds against the W = 2 folded run
    grid = pa.rank_grid(2, 3)
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, None, None, "jacobi") for r in range(2)])
    gid = F["levels"][0].own_gid
    assert np.array_equal(gid, gids[0])
    g = mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport="host_loopback", local_hierarchy=F, cells_global=cells,
                          chebyshev=dict(degree=cw.DEGREE), options=cw.OPTIONS)
    try:
        sx, sr = cw.given_pass(abi, g, gid, int(np.prod([c - 1 for c in cells])))
    finally:
        g.close()
    _same_bits((np.concatenate([v["sx_0"], v["sx_1"]]), np.concatenate([v["sr_0"], v["sr_1"]])), (sx, sr), "two ranks against the folded run")


# ------------------------------------------------------------------------------------------------ errors
def test_errors(pkg, po, S):
    pa, mg, sv, abi = _mods(pkg)
    # (a) a level in the overlapping layout
    cells, nlev, W = (32, 32), 4, 4
    grid = pa.rank_grid(W, 2)
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, 3, [0, 2, 0, 0], "jacobi") for r in range(W)])
    g = mg.DistributedGMG(cells, nlev, 0, 2, transport="host_loopback", local_hierarchy=F, cells_global=cells)
    try:
        abi.check(g.h, g._lib.gmg_set_smoother_chebyshev(g.h, 1, abi.PRE_AND_POST, 3, 0.0, 0.0, 10, 10.0, 1.1))
        rc = g._lib.gmg_setup(g.h)
        assert rc == abi.ERR_UNSUPPORTED
        with pytest.raises(abi.GmgError, match=r"Chebyshev smoother on level 1: the overlapping layout"):
            abi.check(g.h, rc)
    finally:
        g.close()
    # (b) a level of a redistributed rank subset: rank 0 of two by itself, level 1 on the first rank alone
    per_rank = tuple(c // q for c, q in zip((16, 16), pa.rank_grid(2, 2)))
    g = mg.DistributedGMG(per_rank, 3, 0, 2, device_id=0, transport="alone", rep_from=2, sub_from=1, sub_ranks=1)
    try:
        abi.check(g.h, g._lib.gmg_set_smoother_chebyshev(g.h, 1, abi.POST, 3, 0.0, 0.0, 10, 10.0, 1.1))
        rc = g._lib.gmg_setup(g.h)
        assert rc == abi.ERR_UNSUPPORTED
        with pytest.raises(abi.GmgError, match=r"Chebyshev smoother on level 1: a level of a redistributed rank subset"):
            abi.check(g.h, rc)
    finally:
        g.close()
    # (c) a communicator, but no layout was ever declared
    H = po.build_hierarchy((8, 8, 8), 2, 1)
    sms = [S.ChebyshevSmoother(S.JacobiLinearSolver(), 2)]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sms, post_smoothers=sms, maxiter=1)
    ns = S.numerical_setup(S.symbolic_setup(gmg, gmg.smatrices[0]), gmg.smatrices[0])
    xfn = abi.HOST_EXCHANGE_FN(lambda *a: None)
    rfn = abi.HOST_ALLREDUCE_FN(lambda *a: None)
    try:
        abi.check(ns.h, ns._lib.gmg_comm_init_host(ns.h, 0, 1, C.cast(xfn, C.c_void_p), C.cast(rfn, C.c_void_p), None))
        with pytest.raises(abi.GmgError, match=r"Chebyshev smoother on level 0: the handle has a communicator .* no layout") as e:
            ns.setup()
        assert e.value.code == abi.ERR_UNSUPPORTED and "gmg_set_replication" in str(e.value)
    finally:
        ns.close()
