"""MINRESSolver on the device (gmg_minres_solve / gmg_block_minres_solve, Krylov/MINRESSolvers.jl:75-148) against the numpy
transcription of the reference (tests/minres_reference.py) driven by the CPU oracle's pieces: orc.spmv, orc.dot, orc.norm, the
oracle GMG (maxiter = 1), the oracle block-diagonal preconditioner, orc.jacobi_inv_diag.  Same iteration count and flag, history
within 1e-10 hist[0], solution within 1e-10 relative."""
import importlib

import numpy as np
import pytest

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


def _ref(orc, A, b, Pl, **kw):
    return mr.minres(lambda v: orc.spmv(A, v), b, Pl, dot=orc.dot, norm=orc.norm, givens=orc.givens, **kw)


def _agree(log, ref, x, tol=1e-10):
    xo, nit, flag, hist = ref
    assert log.num_iters == nit and log.flag == flag, (log.num_iters, nit, log.flag, flag)
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= tol * hist[0])
    if x is not None:
        assert rel_err(x, xo) <= tol


# ---------------------------------------------------------------- 1. KrylovTests.jl:92 problem, no GMG in the preconditioner
@pytest.mark.parametrize("jacobi", [True, False])
def test_minres_poisson_2d_jacobi_and_unpreconditioned(S, po, orc, hierarchy, jacobi):
    nc, nlev = (32, 32), 2
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=_jac(S, nlev),
                            post_smoothers=_jac(S, nlev), maxiter=1, mode="preconditioner")
    solver = S.MINRESSolver(Pl=(S.JacobiLinearSolver() if jacobi else None, gmg), maxiter=1000, atol=1e-14, rtol=1e-8)
    ns = _setup(S, solver, A)
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    dinv = orc.jacobi_inv_diag(A)
    ref = _ref(orc, A, b, (lambda r: dinv * r) if jacobi else None, maxiter=1000, atol=1e-14, rtol=1e-8)
    assert ref[2] == mr.CONVERGED_RTOL and ref[1] > 10
    _agree(solver.log, ref, x)
    ns.P_ns.close()


# ---------------------------------------------------------------- 2. MINRES + GMG on a 3-D Q1 hierarchy
def _gmg_case(S, po, orc, H, nc, nlev, coarse=None):
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=_jac(S, nlev),
                            post_smoothers=_jac(S, nlev), maxiter=1, mode="preconditioner",
                            **({"coarsest_solver": coarse} if coarse is not None else {}))
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    return gmg, go


def test_minres_gmg_3d_host_device_guess_and_smoother(S, po, orc, hierarchy):
    import torch
    nc, nlev = (32, 32, 32), 3
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    gmg, go = _gmg_case(S, po, orc, H, nc, nlev)
    kw = dict(maxiter=100, atol=1e-14, rtol=1e-8)
    Pg = lambda r: go.solve(r)[0]
    # host vectors, x0 = 0
    solver = S.MINRESSolver(Pl=gmg, **kw)
    ns = _setup(S, solver, A)
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    ref = _ref(orc, A, b, Pg, **kw)
    assert ref[2] == mr.CONVERGED_RTOL
    _agree(solver.log, ref, x)
    # device (torch) vectors and a nonzero initial guess
    x0 = np.random.default_rng(5).uniform(-1.0, 1.0, b.size)
    xd = torch.from_numpy(x0.copy()).cuda()
    S.solve_(xd, ns, torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    _agree(solver.log, _ref(orc, A, b, Pg, x0=x0, **kw), xd.cpu().numpy())
    ns.P_ns.close()
    # use_precond = 3: LinearSolverFromSmoother(finest pre-smoother)
    gmg, go = _gmg_case(S, po, orc, H, nc, nlev)
    solver = S.MINRESSolver(Pl=(S.LinearSolverFromSmoother(gmg.pre_smoothers[0]), gmg), **kw)
    ns = _setup(S, solver, A)
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    ref = _ref(orc, A, b, lambda r: go.smooth(0, np.zeros_like(r), r)[0], **kw)
    _agree(solver.log, ref, x)
    ns.P_ns.close()


@pytest.mark.child_process
def test_minres_gmg_128_cubed_4_levels(S, po, orc, hierarchy):
    nc, nlev = (128, 128, 128), 4
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    gmg, go = _gmg_case(S, po, orc, H, nc, nlev)
    kw = dict(maxiter=30, atol=1e-14, rtol=1e-6)
    solver = S.MINRESSolver(Pl=gmg, **kw)
    ns = _setup(S, solver, A)
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    _agree(solver.log, _ref(orc, A, b, lambda r: go.solve(r)[0], **kw), x)
    ns.P_ns.close()


# ---------------------------------------------------------------- 3. block path: Stokes with an SPD block-diagonal preconditioner
def _stokes(S, po, orc, pkg, n, nlev, sign, alpha=1.0e3):
    """velocity GMG made symmetric: patch smoother pre = post, the plain P with R = P^T, one V-cycle; pressure block
    LU(sign * Mp_scaled) (sign = -1: +M_p / alpha, SPD)"""
    st = importlib.import_module(pkg.__name__ + ".stokes")
    sysd = st.stokes_system(n, alpha)
    Hv = st.velocity_hierarchy(n, nlev, alpha)
    Rs = [_csr(po, P.to_scipy().T) for P in Hv["prolongations"]]
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
    gmg = S.GMGLinearSolver(Hv["mats"], Hv["prolongations"], Rs, pre_smoothers=sm, post_smoothers=sm,
                            coarsest_solver=S.LUSolver(), maxiter=1, mode="preconditioner")
    Mp = _csr(po, sign * sysd["Mp_scaled"].to_scipy())
    blocks = [S.LinearSystemBlock(), S.MatrixBlock(Mp)]
    Pd = S.BlockDiagonalSolver(blocks, [gmg, S.LUSolver()])
    osm = [orc.Smoother(orc.PATCH, 10, 0.2, pp, pd) for pp, pd in Hv["star_patches"]]
    go = orc.GMG(Hv["mats"], Hv["prolongations"], Rs, pre_smoothers=osm, post_smoothers=osm, maxiter=1)
    nu, npp = sysd["sizes"]
    Po = orc.BlockPreconditioner([nu, npp], [go, (orc.BD_LU, Mp)], None, orc.DIAGONAL)
    K = _csr(po, sysd["K"])
    return sysd, Pd, Po, K


@pytest.mark.parametrize("n,nlev", [(8, 2), (16, 3)])
def test_minres_block_diagonal_stokes(S, po, orc, pkg, n, nlev):
    sysd, Pd, Po, K = _stokes(S, po, orc, pkg, n, nlev, -1.0)
    b = sysd["b"]
    kw = dict(maxiter=200, atol=1e-12, rtol=1e-10)
    solver = S.MINRESSolver(Pl=Pd, **kw)
    ns = _setup(S, solver, sysd["A"])
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    ref = _ref(orc, K, b, Po.apply, **kw)
    assert ref[2] == mr.CONVERGED_RTOL
    _agree(solver.log, ref, None)
    assert rel_err(x, ref[0]) <= 1e-8
    assert np.linalg.norm(sysd["K"] @ x - b) < 1e-8 * np.linalg.norm(b)
    ns.P_ns.close()


# ---------------------------------------------------------------- 4. errors and scalar-slot hygiene
def test_minres_indefinite_preconditioner_is_an_error_and_the_handle_survives(S, po, orc, pkg):
    abi = importlib.import_module(pkg.__name__ + ".abi")
    sysd, Pd, Po, K = _stokes(S, po, orc, pkg, 8, 2, 1.0)                 # LU on -M_p / alpha: Pl indefinite
    b = sysd["b"]
    with pytest.raises(mr.NotPositiveDefinite):
        _ref(orc, K, b, Po.apply, maxiter=200, atol=1e-12, rtol=1e-10)
    solver = S.MINRESSolver(Pl=Pd, maxiter=200, atol=1e-12, rtol=1e-10)
    ns = _setup(S, solver, sysd["A"])
    x = np.zeros(b.size)
    with pytest.raises(abi.GmgError) as e:
        S.solve_(x, ns, b)
    assert e.value.code == abi.ERR_INVALID and "positive definite" in str(e.value)
    # the same handle, Pl = nothing (gmg_block_minres_solve, use_precond = 0): MINRES on K itself
    import ctypes as C
    g = ns.P_ns
    res, hist = abi.Result(), np.zeros(31)
    x = np.zeros(b.size)
    abi.check_block(g.h, g._lib.gmg_block_minres_solve(g.h, C.c_void_p(b.ctypes.data), C.c_void_p(x.ctypes.data), abi.MEM_HOST,
                                                       30, 1e-12, 1e-8, 0, C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
    xo, nit, flag, ho = _ref(orc, K, b, None, maxiter=30, atol=1e-12, rtol=1e-8)   # (unpreconditioned: a few steps of it)
    assert res.niters == nit and np.all(np.abs(hist[: nit + 1] - ho) <= 1e-9 * ho[0]) and rel_err(x, xo) <= 1e-8
    g.close()


def test_cg_is_bitwise_the_same_before_and_after_minres_on_one_handle(S, po, orc, pkg, hierarchy):
    """MINRES's scalar slots touch neither the CG slots nor those of a CG nested in the preconditioner (coarsest CG-Jacobi)"""
    import ctypes as C
    import torch
    abi = importlib.import_module(pkg.__name__ + ".abi")
    nc, nlev = (32, 32, 32), 3
    H = hierarchy(nc, nlev)
    A, b = H["mats"][0], po.dirichlet_lift_rhs(nc, 1)
    gmg, go = _gmg_case(S, po, orc, H, nc, nlev, coarse=S.CGSolver(S.JacobiLinearSolver(), maxiter=200, atol=1e-14, rtol=1e-10))
    ns = _setup(S, S.CGSolver(gmg, maxiter=30, atol=1e-14, rtol=1e-8), A)
    g = ns.P_ns
    bd = torch.from_numpy(b).cuda()

    def run(fn, *args):
        x = torch.zeros(b.size, dtype=torch.float64, device="cuda")
        res, hist = abi.Result(), np.zeros(31)
        abi.check(g.h, fn(g.h, C.c_void_p(bd.data_ptr()), C.c_void_p(x.data_ptr()), abi.MEM_DEVICE, 30, 1e-14, 1e-8, *args,
                          C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        torch.cuda.synchronize()
        return x.cpu().numpy(), hist[: res.niters + 1].copy(), res

    x1, h1, _ = run(g._lib.gmg_cg_solve, 0, 1)
    xm1, hm1, rm = run(g._lib.gmg_minres_solve, 1)
    x2, h2, _ = run(g._lib.gmg_cg_solve, 0, 1)
    xm2, hm2, _ = run(g._lib.gmg_minres_solve, 1)
    assert np.array_equal(x1, x2) and np.array_equal(h1, h2)
    assert np.array_equal(xm1, xm2) and np.array_equal(hm1, hm2)
    assert rm.flag == mr.CONVERGED_RTOL and rel_err(xm1, x1) < 1e-6
    g.close()


# ---------------------------------------------------------------- 5. partitioned MINRES + GMG over the RCCL loopback
def _folded(pa, cells, nlev, W, depth=None, rep_from=None):
    grid = pa.rank_grid(W, len(cells))
    return pa.fold_ranks([pa.build_local_hierarchy(cells, nlev, grid, r, 1, None, rep_from, depth, "jacobi") for r in range(W)])


def _dist_minres(mg, F, cells, nlev, transport, kw):
    import torch
    g = mg.DistributedGMG(cells, nlev, 0, 2, device_id=0, transport=transport, local_hierarchy=F, cells_global=cells)
    b = torch.from_numpy(g.rhs_lin()).cuda()
    x = torch.zeros(g.n_own, dtype=torch.float64, device="cuda")
    log = g.minres_solve(b, x, **kw)
    torch.cuda.synchronize()
    out = dict(x=x.cpu().numpy(), iters=log.num_iters, flag=log.flag, hist=np.array(log.residuals[: log.num_iters + 1]),
               info=g.comm_info(), gid=F["levels"][0].own_gid)
    g.close()
    return out


@pytest.mark.child_process
@pytest.mark.parametrize("cells,nlev,W,depth,rep", [((16, 16, 16), 3, 8, None, None), ((32, 32), 4, 4, [0, 3, 5, 0], 3)])
def test_partitioned_minres_gmg_over_rccl_loopback(pkg, po, orc, cells, nlev, W, depth, rep):
    pa = importlib.import_module(pkg.__name__ + ".partition")
    mg = importlib.import_module(pkg.__name__ + ".multigpu")
    F = _folded(pa, cells, nlev, W, depth, rep)
    H = po.build_hierarchy(cells, nlev, 1)
    b = po.dirichlet_lift_rhs(cells, 1)
    kw = dict(maxiter=40, atol=1e-14, rtol=1e-6)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    xo, nit, flag, hist = _ref(orc, H["mats"][0], b, lambda r: go.solve(r)[0], **kw)
    host = _dist_minres(mg, F, cells, nlev, "host_loopback", kw)
    rccl = _dist_minres(mg, F, cells, nlev, "rccl_loopback", kw)
    assert host["info"]["transport"] == "host" and rccl["info"]["transport"] == "rccl"
    assert rccl["iters"] == host["iters"] == nit and rccl["flag"] == flag
    assert np.array_equal(rccl["x"], host["x"]) and np.array_equal(rccl["hist"], host["hist"])
    assert np.all(np.abs(rccl["hist"] - hist) <= 1e-10 * hist[0]) and rel_err(rccl["x"], xo[rccl["gid"]]) < 1e-10
