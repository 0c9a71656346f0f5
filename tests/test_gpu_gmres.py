"""GMRESSolver on the device (gmg_gmres_solve / gmg_block_gmres_solve, Krylov/GMRESSolvers.jl:132-210) against the numpy restatement
of the reference (tests/gmres_reference.py) driven by the CPU oracle's pieces: orc.spmv, orc.dot, orc.norm, orc.givens, the oracle
GMG (maxiter = 1), the oracle block preconditioner, orc.jacobi_inv_diag.  Same iteration count and flag, history within
1e-10 hist[0], solution within 1e-10 relative (test_gpu_minres.py::_agree).  Every solve of sections 1 and 2 runs with
gmres_fused = 1 and 0 on fresh handles and the two must agree bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gmres_reference as gr
import minres_reference as mr
from conftest import rel_err

pytestmark = pytest.mark.gpu


def _csr(po, M):
    M = M.tocsr(); M.sort_indices()
    return po.CSR(M.shape, M.indptr, M.indices, M.data)


def _setup(S, solver, A):
    return S.numerical_setup(S.symbolic_setup(solver, A), A)


def _jac(S, nlev, niter=10, omega=2.0 / 3.0):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), niter, omega)] * (nlev - 1)


def _ref(orc, A, b, m, **kw):
    return gr.gmres(lambda v: orc.spmv(A, v), b, m, dot=orc.dot, norm=orc.norm, givens=orc.givens, **kw)


def _agree(log, ref, x, tol=1e-10):
    xo, nit, flag, hist = ref
    print("gmres parity: iters %d / %d, flag %d / %d, max |hist - ref| / hist[0] = %.3e, rel err x = %.3e" % (
        log.num_iters, nit, log.flag, flag,
        np.max(np.abs(np.asarray(log.residuals[: min(nit, log.num_iters) + 1]) - hist[: min(nit, log.num_iters) + 1])) / hist[0],
        rel_err(x, xo) if x is not None else -1.0))
    assert log.num_iters == nit and log.flag == flag, (log.num_iters, nit, log.flag, flag)
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= tol * hist[0])
    if x is not None:
        assert rel_err(x, xo) <= tol


def _gmg(S, H, nlev, fused, pre=None):
    sm = pre if pre is not None else _jac(S, nlev)
    return S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=1,
                             mode="preconditioner", options={"gmres_fused": fused})


def _both(S, H, nlev, A, b, m, sides, kw, x0=None, device=False, pre=None):
    """the solve with gmres_fused = 1 and 0, each on a fresh handle; bitwise equal histories and solutions -> (log, x) of the fused one"""
    out = []
    for fused in (1, 0):
        gmg = _gmg(S, H, nlev, fused, pre)
        solver = S.GMRESSolver(m, **sides(S, gmg), **kw)
        ns = _setup(S, solver, A)
        if device:
            import torch
            xd = torch.from_numpy(np.zeros(b.size) if x0 is None else x0.copy()).cuda()
            S.solve_(xd, ns, torch.from_numpy(b).cuda())
            torch.cuda.synchronize()
            x = xd.cpu().numpy()
        else:
            x = np.zeros(b.size) if x0 is None else x0.copy()
            S.solve_(x, ns, b)
        out.append((solver.log, x, np.array(solver.log.residuals[: solver.log.num_iters + 1])))
        ns.close()
    (l1, x1, h1), (l0, x0_, h0) = out
    assert l1.num_iters == l0.num_iters and l1.flag == l0.flag
    assert np.array_equal(h1, h0) and np.array_equal(x1, x0_)
    return l1, x1


# ---------------------------------------------------------------- 1. KrylovTests.jl:67-75 shapes, no GMG in the preconditioner
SHAPES = {
    "m40-PrPl-jacobi": (40, False, True, True),
    "m10": (10, False, False, False),
    "m10-restart": (10, True, False, False),
    "m10-restart-Pr": (10, True, True, False),
    "m5-restart-Pl": (5, True, False, True),
}
CASES = [(nc, s) for nc in [(16, 16), (8, 8, 8), (16, 16, 16)] for s in SHAPES] + [((32, 32), "m40-PrPl-jacobi")]


@pytest.mark.parametrize("nc,shape", CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_gmres_krylovtests_shapes_poisson(S, po, orc, hierarchy, nc, shape):
    m, restart, jr, jl = SHAPES[shape]
    nlev = 2
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    kw = dict(restart=restart, maxiter=200, atol=1e-14, rtol=1e-8)
    sides = lambda S, gmg: dict(Pr=(S.JacobiLinearSolver() if jr else None, gmg), Pl=(S.JacobiLinearSolver(), gmg) if jl else None)
    log, x = _both(S, H, nlev, A, b, m, sides, kw)
    dinv = orc.jacobi_inv_diag(A)
    jac = lambda r: dinv * r
    ref = _ref(orc, A, b, m, Pr=jac if jr else None, Pl=jac if jl else None, **kw)
    assert ref[2] == gr.CONVERGED_RTOL
    if not restart:
        assert ref[1] > m or shape == "m40-PrPl-jacobi"                    # the unrestarted m = 10 cases outgrow the basis (m_add)
    _agree(log, ref, x)


# ---------------------------------------------------------------- 2. GMG as Pr and as Pl
@pytest.mark.parametrize("side", ["Pr", "Pl"])
def test_gmres_gmg_3d_host_device_guess_and_restart(S, po, orc, hierarchy, side):
    nc, nlev = (32, 32, 32), 3
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    Pg = lambda r: go.solve(r)[0]
    sides = lambda S, gmg: {side: gmg}
    rk = {side: Pg}
    kw = dict(maxiter=100, atol=1e-14, rtol=1e-8)
    # host vectors, x0 = 0
    log, x = _both(S, H, nlev, A, b, 10, sides, kw)
    ref = _ref(orc, A, b, 10, **rk, **kw)
    assert ref[2] == gr.CONVERGED_RTOL
    _agree(log, ref, x)
    # device (torch) vectors and a random initial guess
    x0 = np.random.default_rng(5).uniform(-1.0, 1.0, b.size)
    log, x = _both(S, H, nlev, A, b, 10, sides, kw, x0=x0, device=True)
    _agree(log, _ref(orc, A, b, 10, x0=x0, **rk, **kw), x)
    # m = 5 with restart = true: at least one restart.  rtol = 1e-12 is met by the fifth iteration, the last of the first cycle
    # (6.6e-13 with Pr, 8.9e-13 with Pl), so the tolerance is 1e-13: a sixth iteration, in a second cycle
    kw = dict(restart=True, maxiter=60, atol=1e-30, rtol=1e-13)
    log, x = _both(S, H, nlev, A, b, 5, sides, kw)
    info = {}
    ref = _ref(orc, A, b, 5, info=info, **rk, **kw)
    assert ref[2] == gr.CONVERGED_RTOL and info["cycles"] >= 2
    _agree(log, ref, x)


@pytest.mark.child_process
def test_gmres_gmg_128_cubed_4_levels(S, po, orc, hierarchy):
    nc, nlev = (128, 128, 128), 4
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    kw = dict(maxiter=30, atol=1e-14, rtol=1e-6)
    log, x = _both(S, H, nlev, A, b, 5, lambda S, gmg: dict(Pr=gmg), kw)
    ref = _ref(orc, A, b, 5, Pr=lambda r: go.solve(r)[0], **kw)
    assert ref[2] == gr.CONVERGED_RTOL
    _agree(log, ref, x)


def test_gmres_q2_patch_smoothed_gmg_as_pr(S, po, orc, hierarchy):
    """the hierarchy of test_q2_patch_smoother_parity: Q2 16 x 16, Richardson(PatchSolver, 10, 0.2)"""
    nc, nlev, order = (16, 16), 2, 2
    H = hierarchy(nc, nlev, order)
    pp, pd = po.vertex_star_patches(nc, order)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, order)
    osm = [orc.Smoother(orc.PATCH, 10, 0.2, pp, pd)]
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=osm, post_smoothers=osm, maxiter=1)
    kw = dict(maxiter=40, atol=1e-14, rtol=1e-8)
    log, x = _both(S, H, nlev, A, b, 5, lambda S, gmg: dict(Pr=gmg), kw, pre=[S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2)])
    ref = _ref(orc, A, b, 5, Pr=lambda r: go.solve(r)[0], **kw)
    assert ref[2] == gr.CONVERGED_RTOL
    _agree(log, ref, x)


# ---------------------------------------------------------------- 3. errors
def test_gmres_gmg_on_both_sides_is_invalid(S, po, pkg, hierarchy):
    abi = importlib.import_module(pkg.__name__ + ".abi")
    nc, nlev = (8, 8, 8), 2
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    gmg = _gmg(S, H, nlev, 1)
    with pytest.raises(ValueError):
        _setup(S, S.GMRESSolver(5, Pr=gmg, Pl=gmg), A)
    ns = _setup(S, S.GMRESSolver(5, Pr=gmg), A)
    g = ns.P_ns
    res, hist, x = abi.Result(), np.zeros(11), np.zeros(b.size)
    st = g._lib.gmg_gmres_solve(g.h, C.c_void_p(b.ctypes.data), C.c_void_p(x.ctypes.data), abi.MEM_HOST, 5, 0, 1, 10, 1e-14, 1e-8,
                                1, 1, C.byref(res), C.c_void_p(hist.ctypes.data), hist.size)
    assert st == abi.ERR_INVALID
    with pytest.raises(abi.GmgError) as e:
        abi.check(g.h, st)
    assert e.value.code == abi.ERR_INVALID and "not both" in str(e.value)
    assert not x.any()
    S.solve_(x, ns, b)                                                     # the handle survives
    assert ns.solver.log.flag == gr.CONVERGED_RTOL
    ns.close()


# ---------------------------------------------------------------- 5. slot hygiene on one handle
def test_gmres_fgmres_minres_cg_keep_their_caches_apart_on_one_handle(S, po, orc, pkg, hierarchy):
    """FGMRES, GMRES, FGMRES: the first FGMRES result bitwise; GMRES, MINRES, CG, GMRES likewise; each against its own reference"""
    import torch
    abi = importlib.import_module(pkg.__name__ + ".abi")
    nc, nlev = (32, 32, 32), 3
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    ns = _setup(S, S.GMRESSolver(5, Pr=_gmg(S, H, nlev, 1)), A)
    g = ns.P_ns
    lib = g._lib
    bd = torch.from_numpy(b).cuda()
    kw = dict(maxiter=30, atol=1e-14, rtol=1e-8)
    tol = (30, 1e-14, 1e-8)

    def run(fn, *args):
        x = torch.zeros(b.size, dtype=torch.float64, device="cuda")
        res, hist = abi.Result(), np.zeros(31)
        abi.check(g.h, fn(g.h, C.c_void_p(bd.data_ptr()), C.c_void_p(x.data_ptr()), abi.MEM_DEVICE, *args,
                          C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        torch.cuda.synchronize()
        return x.cpu().numpy(), hist[: res.niters + 1].copy(), res

    def same(u, v):
        return np.array_equal(u[0], v[0]) and np.array_equal(u[1], v[1])

    def agrees(got, ref):
        xo, nit, flag, hist = ref
        return got[2].niters == nit and got[2].flag == flag and np.all(np.abs(got[1] - hist) <= 1e-10 * hist[0]) and rel_err(got[0], xo) <= 1e-10

    fg = lambda: run(lib.gmg_fgmres_solve, 5, 0, 1, *tol, 1)
    gm = lambda: run(lib.gmg_gmres_solve, 5, 0, 1, *tol, 1, 0)
    f1, g1, f2 = fg(), gm(), fg()
    g2, mn, cg, g3 = gm(), run(lib.gmg_minres_solve, *tol, 1), run(lib.gmg_cg_solve, *tol, 0, 1), gm()
    f3 = fg()
    assert same(f1, f2) and same(f1, f3)
    assert same(g1, g2) and same(g1, g3)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    Pg = lambda r: go.solve(r)[0]
    assert agrees(g1, _ref(orc, A, b, 5, Pr=Pg, **kw))
    assert agrees(f1, orc.fgmres_solve(A, b, Pr=go, m=5, **kw))
    assert agrees(mn, mr.minres(lambda v: orc.spmv(A, v), b, Pg, dot=orc.dot, norm=orc.norm, givens=orc.givens, **kw))
    assert agrees(cg, orc.cg_solve(A, b, Pl=go, **kw))
    ns.close()


# ---------------------------------------------------------------- 6. memory
def test_gmres_keeps_m_plus_3_vectors_where_fgmres_keeps_2m(S, po, pkg, hierarchy):
    """GMRES(m; Pr = GMG): V (m + 1), zl, zr.  Measured around the first GMRES / FGMRES solve of a handle that has already run a CG
    solve on device vectors (that allocates what every solver shares: the saved initial guess of an in-place device solve).  The
    allowance is the allocator's, not a vector: every device allocation carries 64 bytes of slack for vector loads -- the m + 3
    vectors and the table of m + 8 basis pointers are m + 4 allocations.  Measured on the 128^3 problem at m = 5: 8 vectors + 680 bytes = 64 (m + 4) + 8 (m + 8)."""
    import torch
    abi = importlib.import_module(pkg.__name__ + ".abi")
    nc, nlev, m = (32, 32, 32), 3, 8
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    kw = dict(maxiter=m, atol=1e-14, rtol=1e-8)
    bd = torch.from_numpy(b).cuda()
    grow = []
    for solver in (S.GMRESSolver(m, Pr=_gmg(S, H, nlev, 1), **kw), S.FGMRESSolver(m, _gmg(S, H, nlev, 1), **kw)):
        ns = _setup(S, solver, A)
        g = ns.P_ns
        xd = torch.zeros(b.size, dtype=torch.float64, device="cuda")
        res = abi.Result()
        abi.check(g.h, g._lib.gmg_cg_solve(g.h, C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), abi.MEM_DEVICE, 1, 1e-14, 1e-8, 0, 1,
                                           C.byref(res), None, 0))
        torch.cuda.synchronize()
        b0 = g.device_bytes()
        xd.zero_()
        S.solve_(xd, ns, bd)
        torch.cuda.synchronize()
        assert solver.log.flag == gr.CONVERGED_RTOL
        grow.append(g.device_bytes() - b0)
        ns.close()
    vec = 8 * b.size
    print("krylov storage: GMRES(%d) %d bytes = %.3f vectors, FGMRES(%d) %d bytes = %.3f vectors" % (m, grow[0], grow[0] / vec, m, grow[1], grow[1] / vec))
    assert 0 < grow[0] <= (m + 3) * vec + 64 * (m + 4) + 8 * (m + 8)
    assert grow[1] >= 2 * m * vec


# ---------------------------------------------------------------- 7. block handle
@pytest.mark.parametrize("side", ["Pr", "Pl"])
def test_gmres_block_triangular_stokes(S, po, orc, monkeypatch, side):
    """GMRES(20; Pr = P) and GMRES(20; Pl = P) on stokes.py at 64^2 with the block-triangular preconditioner of
    test_gpu_block.py::_real_stokes, against gmres_reference driven by the oracle block preconditioner"""
    from test_gpu_block import _real_stokes
    n, nlev = 64, 3
    sysd, Hv, gmg, solver_p, Pd, Po, go = _real_stokes(S, po, orc, n, nlev)
    b = sysd["b"]
    kw = dict(maxiter=100, atol=1e-10, rtol=1e-12)
    solver = S.GMRESSolver(20, **{side: Pd}, **kw)
    ns = _setup(S, solver, sysd["A"])
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    hist1 = np.array(solver.log.residuals[: solver.log.num_iters + 1])
    # a block handle has no option table: the variable is read at every solve.  gmres_fused = 0 on a fresh handle: the same bits
    sysd0, _, _, _, Pd0, _, _ = _real_stokes(S, po, orc, n, nlev)
    solver0 = S.GMRESSolver(20, **{side: Pd0}, **kw)
    ns0 = _setup(S, solver0, sysd0["A"])
    x_unfused = np.zeros(b.size)
    monkeypatch.setenv("GMG_GMRES_FUSED", "0")
    S.solve_(x_unfused, ns0, b)
    monkeypatch.delenv("GMG_GMRES_FUSED")
    ns0.close()
    assert np.array_equal(x, x_unfused) and np.array_equal(hist1, np.array(solver0.log.residuals[: solver0.log.num_iters + 1]))
    K = _csr(po, sysd["K"])
    ref = _ref(orc, K, b, 20, **{side: Po.apply}, **kw)
    assert ref[2] in (gr.CONVERGED_RTOL, gr.CONVERGED_ATOL)
    print("block GMRES(20; %s): ||K x - b|| = %.3e (device) %.3e (reference)" % (side, np.linalg.norm(sysd["K"] @ x - b),
                                                                                np.linalg.norm(sysd["K"] @ ref[0] - b)))
    _agree(solver.log, ref, x)
    assert np.linalg.norm(sysd["K"] @ x - b) < 1e-7                        # StokesGMG.jl:162-165
    ns.close()


def test_gmres_unpreconditioned_on_a_block_diagonal_system(S, po, orc):
    """BlockDiagonalSolversTests.jl:30,38-45: the [[M, 0], [0, M]] system of test_gpu_block.py, GMRES(10; rtol = 1e-10) with no
    preconditioner on the block handle"""
    import scipy.sparse as sp
    M = po.poisson_matrix((8, 8), 1); n = M.shape[0]
    Pd = S.BlockDiagonalSolver([S.LUSolver(), S.LUSolver()])
    kw = dict(maxiter=100, atol=1e-14, rtol=1e-10)
    solver = S.GMRESSolver(10, Pr=(None, Pd), **kw)
    ns = _setup(S, solver, [[M, None], [None, M]])
    b = np.random.default_rng(0).uniform(-1, 1, 2 * n)
    x = np.zeros(2 * n)
    S.solve_(x, ns, b)
    K = _csr(po, sp.bmat([[M.to_scipy(), None], [None, M.to_scipy()]]))
    ref = _ref(orc, K, b, 10, **kw)
    assert ref[2] == gr.CONVERGED_RTOL and ref[1] > 10
    _agree(solver.log, ref, x)
    ns.close()


# ---------------------------------------------------------------- 8. partitioned GMRES + GMG over the loopback communicator
@pytest.mark.child_process
def test_partitioned_gmres_gmg_over_the_loopback(S, pkg, po, orc, hierarchy):
    """W = 8 folded ranks (tests/test_loopback.py): with a communicator the core takes the unfused sequence (all-reduced dots)"""
    import torch
    pa = importlib.import_module(pkg.__name__ + ".partition")
    mg = importlib.import_module(pkg.__name__ + ".multigpu")
    cells, nlev, W = (16, 16, 16), 3, 8
    grid = pa.rank_grid(W, len(cells))
    F = pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, None, None, "jacobi") for r in range(W)])
    H = hierarchy(cells, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(cells, 1)
    kw = dict(maxiter=40, atol=1e-14, rtol=1e-6)
    # the single-handle run
    log1, x1 = _both(S, H, nlev, A, b, 5, lambda S, gmg: dict(Pr=gmg), kw)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    ref = _ref(orc, A, b, 5, Pr=lambda r: go.solve(r)[0], **kw)
    _agree(log1, ref, x1)
    outs = {}
    for transport in ("host_loopback", "rccl_loopback"):
        g = mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport=transport, local_hierarchy=F, cells_global=cells)
        bd = torch.from_numpy(g.rhs_lin()).cuda()
        xd = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
        log = g.gmres_solve(bd, xd, m=5, **kw)
        torch.cuda.synchronize()
        outs[transport] = (log, xd.cpu().numpy(), g.comm_info(), F["levels"][0].own_gid)
        g.close()
    for transport, (log, x, info, gid) in outs.items():
        assert info["transport"] == transport.split("_")[0]
        assert log.num_iters == log1.num_iters and log.flag == log1.flag
        _agree(log, (ref[0][gid], ref[1], ref[2], ref[3]), x)
