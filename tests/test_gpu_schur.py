"""SchurComplementSolver on the device (block handle of kind GMG_BLOCK_SCHUR, LinearSolvers/SchurComplementSolvers.jl:55-74) against the
numpy restatement of the reference (tests/schur_reference.py) driven by the CPU checkers: scipy's splu for LUSolver(), the oracle GMG,
the oracle's CG-Jacobi (orc.cg_solve with Pl = "jacobi", which takes an initial guess), a Jacobi scaling.

Tolerances are those of tests/test_gpu_block.py for the same shapes and solver kinds: one application <= 1e-11 relative 2-norm with
direct block solvers, <= 1e-9 with a GMG, <= 1e-10 with a 3-iteration CG-Jacobi; outer residual histories <= 1e-6 hist[0],
solutions <= 1e-6, iteration counts and flags identical."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmres_reference as gr
import numpy_twin as nt
import schur_reference as sr
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL_APPLY, TOL_HIST = 1e-11, 1e-6


def _csr(po, M):
    M = M.tocsr(); M.sort_indices()
    return po.CSR(M.shape, M.indptr, M.indices, M.data)


def _setup(S, solver, A):
    return S.numerical_setup(S.symbolic_setup(solver, A), A)


def _oracle_cg_jacobi(orc, M, maxiter, atol, rtol, log=None):
    """CGSolver(JacobiLinearSolver(); ...) as an in-place callable: x on entry is the initial guess"""
    def solve(x, b):
        xo, nit, _flag, _hist = orc.cg_solve(M, np.ascontiguousarray(b), Pl="jacobi", x0=x, maxiter=maxiter, atol=atol, rtol=rtol)
        x[:] = xo
        if log is not None:
            log["num_iters"] = nit
    return solve


def _oracle_gmg(go, log=None):
    def solve(x, b):
        xo, nit, _flag, _hist = go.solve(np.ascontiguousarray(b), x.copy())
        x[:] = xo
        if log is not None:
            log["num_iters"] = nit
    return solve


# ---------------------------------------------------------------- 1, 6: the reference's block test problem, exact factorisation
@pytest.fixture(scope="module")
def lu_problem(po):
    """[[M, -M], [M, M]] (BlockDiagonalSolversTests.jl / BlockTriangularSolversTests.jl): S = M - M M^-1 (-M) = 2 M exactly"""
    M = po.poisson_matrix((8, 8), 1); n = M.shape[0]
    assert n == 49
    Ms = M.to_scipy().tocsr()
    negM, M2 = _csr(po, -Ms), _csr(po, 2.0 * Ms)
    K = sp.bmat([[Ms, -Ms], [Ms, Ms]]).tocsr()
    b = np.random.default_rng(0).uniform(-1, 1, 2 * n)
    x_ref = sr.schur_apply(np.zeros(2 * n), b, sr.exact_solver(Ms), sr.exact_solver(2.0 * Ms), -Ms, Ms, sr.SchurCache(n))
    x_ref.setflags(write=False)
    return dict(M=M, negM=negM, M2=M2, mat=[[M, negM], [M, M]], K=K, b=b, n=n, x_ref=x_ref)


def _lu_solver(S, T):
    return S.SchurComplementSolver((S.LUSolver(), T["M"]), T["negM"], T["M"], (S.LUSolver(), T["M2"]))


def test_schur_exact_factorisation_lu_blocks(S, lu_problem):
    T = lu_problem
    n, b = T["n"], T["b"]
    ns = _setup(S, _lu_solver(S, T), T["mat"])
    x = np.zeros(2 * n)
    S.solve_(x, ns, b)
    exact = spla.splu(T["K"].tocsc()).solve(b)
    print("schur LU blocks: rel err vs reference %.3e, ||x - K^-1 b|| = %.3e" % (rel_err(x, T["x_ref"]), np.linalg.norm(x - exact)))
    assert rel_err(x, T["x_ref"]) <= TOL_APPLY
    assert np.linalg.norm(x - exact) < 1e-8                                # S is exact: BlockDiagonalSolversTests.jl:45
    y = np.zeros(2 * n)
    ns.mul(y, b)
    assert rel_err(y, T["K"] @ b) <= 1e-13
    ns.close()


def test_schur_device_tensors_give_the_bits_of_the_host_path(S, lu_problem):
    import torch
    T = lu_problem
    n, b = T["n"], T["b"]
    ns = _setup(S, _lu_solver(S, T), T["mat"])
    x = np.zeros(2 * n)
    S.solve_(x, ns, b)
    xd = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    bd = torch.from_numpy(b).cuda()
    assert xd.is_contiguous() and bd.is_contiguous()
    S.solve_(xd, ns, bd)
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x)                             # same kernels, same order: bit-identical
    assert rel_err(x, T["x_ref"]) <= TOL_APPLY
    yd = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    ns.mul(yd, bd)
    torch.cuda.synchronize()
    assert rel_err(yd.cpu().numpy(), T["K"] @ b) <= 1e-13
    ns.close()


# ---------------------------------------------------------------- 2: explicit blocks win
def test_schur_uses_its_own_b_and_c_and_mul_uses_the_systems(S, po, lu_problem):
    T = lu_problem
    n, b = T["n"], T["b"]
    Ms = T["M"].to_scipy().tocsr()
    Bs = sp.random(n, n, density=0.05, random_state=3, format="csr")      # the solver's B and C: not the system's (0,1), (1,0)
    Cs = sp.random(n, n, density=0.05, random_state=7, format="csr")
    solver = S.SchurComplementSolver((S.LUSolver(), T["M"]), _csr(po, Bs), _csr(po, Cs), (S.LUSolver(), T["M2"]))
    ns = _setup(S, solver, T["mat"])
    x = np.zeros(2 * n)
    S.solve_(x, ns, b)
    ref = sr.schur_apply(np.zeros(2 * n), b, sr.exact_solver(Ms), sr.exact_solver(2.0 * Ms), Bs, Cs, sr.SchurCache(n))
    assert rel_err(x, ref) <= TOL_APPLY
    assert rel_err(x, T["x_ref"]) > 1e-3                                   # and not the system's blocks
    y = np.zeros(2 * n)
    ns.mul(y, b)
    assert rel_err(y, T["K"] @ b) <= 1e-13                                 # mul! is the system's
    ns.close()


# ---------------------------------------------------------------- 3: GMG + CG-Jacobi, one application
def test_schur_gmg_and_cg_jacobi_one_application(S, po, orc, hierarchy):
    from test_gpu_block import _stokes_like
    T = _stokes_like(S, po, orc, hierarchy, (8, 8, 8), 2, True)            # fresh GMG solver objects (maxiter = 4, preconditioner)
    go, Mp, B10, B01 = T["keep"]                                           # oracle GMG, pressure block, (1,0) block, (0,1) block
    n1, N = T["n1"], T["n"]
    cg = S.CGSolver(S.JacobiLinearSolver(), maxiter=20, atol=1e-14, rtol=1e-6)
    solver = S.SchurComplementSolver((T["gmg"], None), B01, B10, (cg, Mp))
    ns = _setup(S, solver, T["mat"])
    b = np.random.default_rng(5).uniform(-1, 1, N)
    z = np.zeros(N)
    S.solve_(z, ns, b)
    glog, clog = {}, {}
    zo = sr.schur_apply(np.zeros(N), b, _oracle_gmg(go, glog), _oracle_cg_jacobi(orc, Mp, 20, 1e-14, 1e-6, clog),
                        B01.to_scipy(), B10.to_scipy(), sr.SchurCache(n1))
    print("schur GMG + CG-Jacobi: rel err %.3e, GMG iters %d (ref %d), CG iters %d (ref %d)" % (
        rel_err(z, zo), T["gmg"].log.num_iters, glog["num_iters"], cg.log.num_iters, clog["num_iters"]))
    assert rel_err(z, zo) <= 1e-9
    assert 0 < T["gmg"].log.num_iters <= 4 and 0 < cg.log.num_iters <= 20
    ns.close()


# ---------------------------------------------------------------- 4: initial guess and the du cache
def test_schur_initial_guess_and_persistent_du(S, orc, lu_problem):
    T = lu_problem
    n, b, M = T["n"], T["b"], T["M"]
    Ms = M.to_scipy().tocsr()

    def device():
        cg = S.CGSolver(S.JacobiLinearSolver(), maxiter=3, atol=1e-30, rtol=1e-30)
        return _setup(S, S.SchurComplementSolver((cg, M), T["negM"], M, (S.JacobiLinearSolver(), T["M2"])), T["mat"]), cg

    def reference():
        cache = sr.SchurCache(n)
        solveA, solveS = _oracle_cg_jacobi(orc, M, 3, 1e-30, 1e-30), sr.jacobi_solver(2.0 * Ms)
        return lambda x: sr.schur_apply(x, b, solveA, solveS, -Ms, Ms, cache)

    x0 = np.random.default_rng(11).uniform(-1, 1, 2 * n)
    ns, cg = device()
    ref = reference()
    x, xr = x0.copy(), x0.copy()
    for k in range(2):                                                     # x prefilled, then left as returned; du persists
        S.solve_(x, ns, b)
        ref(xr)
        print("schur CG-Jacobi(3) application %d: rel err %.3e" % (k + 1, rel_err(x, xr)))
        assert rel_err(x, xr) <= 1e-10
        assert cg.log.num_iters == 3
        if k == 0:
            first = x.copy()
    # x zeroed, du still warm: not what a fresh setup gives from x = 0
    xw, xwr = np.zeros(2 * n), np.zeros(2 * n)
    S.solve_(xw, ns, b)
    ref(xwr)
    ns.close()
    ns2, _ = device()
    xf, xfr = np.zeros(2 * n), np.zeros(2 * n)
    S.solve_(xf, ns2, b)
    reference()(xfr)
    ns2.close()
    assert rel_err(xw, xwr) <= 1e-10 and rel_err(xf, xfr) <= 1e-10
    assert rel_err(xwr, xfr) > 1e-6                                        # the references tell a warm du from a cold one ...
    assert rel_err(xw, xf) > 1e-6                                          # ... and so does the device: the cache is live, not reset
    assert rel_err(first, xfr) > 1e-6                                      # the prefilled x was used as a guess as well


# ---------------------------------------------------------------- 5: outer solves on real Stokes inputs
@pytest.fixture(scope="module")
def stokes8(S, po, orc):
    """stokes.stokes_system(8), 2-level velocity GMG as test_gpu_block.py::_real_stokes builds it (patch smoothers, patch prolongation
    with the grad-div rhs, LU coarsest, maxiter = 4); S = LU of -1/alpha M_p (191 rows: 3 x 64 cell dofs less the pinned one).  Both block solvers are stateless, so the
    content of the Krylov work vectors does not enter.  The reference Schur preconditioner runs on the oracle GMG and splu."""
    from test_gpu_block import _real_stokes
    sysd, Hv, gmg, _solver_p, _Pd, Po, go = _real_stokes(S, po, orc, 8, 2)
    nu, npp = sysd["sizes"]
    assert sysd["Mp_scaled"].shape == (npp, npp) and npp == 191
    B, Cm, Mp = sysd["A"][0][1], sysd["A"][1][0], sysd["Mp_scaled"]
    solveA, solveS = _oracle_gmg(go), sr.exact_solver(Mp.to_scipy())
    cache = sr.SchurCache(nu)
    Bs, Cs = B.to_scipy().tocsr(), Cm.to_scipy().tocsr()
    Pref = lambda r: sr.schur_apply(np.zeros(r.size), np.asarray(r, dtype=np.float64), solveA, solveS, Bs, Cs, cache)
    Kc = po.CSR(sysd["K"].shape, sysd["K"].indptr, sysd["K"].indices, sysd["K"].data)
    return dict(sysd=sysd, Hv=Hv, Po=Po, go=go, Pref=Pref, Kc=Kc, B=B, C=Cm, Mp=Mp)


def _stokes_schur(S, po, orc):
    """a fresh device GMG solver object + the Schur solver on it"""
    from test_gpu_block import _real_stokes
    sysd, _Hv, gmg, _solver_p, _Pd, _Po, _go = _real_stokes(S, po, orc, 8, 2)
    return S.SchurComplementSolver((gmg, None), sysd["A"][0][1], sysd["A"][1][0], (S.LUSolver(), sysd["Mp_scaled"])), sysd


KW = dict(maxiter=100, atol=1e-10, rtol=1e-12)


def _agree(log, ref, x, K, b, what):
    xo, nit, flag, hist = ref
    k = min(nit, log.num_iters)
    print("%s: iters %d / %d, flag %d / %d, max |hist - ref| / hist[0] = %.3e, rel err x = %.3e, ||K x - b|| = %.3e" % (
        what, log.num_iters, nit, log.flag, flag, np.max(np.abs(np.asarray(log.residuals[: k + 1]) - hist[: k + 1])) / hist[0],
        rel_err(x, xo), np.linalg.norm(K @ x - b)))
    assert log.num_iters == nit and log.flag == flag
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= TOL_HIST * hist[0])
    assert rel_err(x, xo) <= 1e-6
    assert np.linalg.norm(K @ x - b) < 1e-7


def test_schur_as_pr_of_gmres_on_stokes(S, po, orc, stokes8):
    """SchurComplementSolversTests.jl:98-114: GMRESSolver(20; Pr = SchurComplementSolver(A_ns, B, C, PS_ns))"""
    T = stokes8
    b = T["sysd"]["b"]
    P, sysd = _stokes_schur(S, po, orc)
    solver = S.GMRESSolver(20, Pr=P, **KW)
    ns = _setup(S, solver, sysd["A"])
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    ref = gr.gmres(lambda v: orc.spmv(T["Kc"], v), b, 20, Pr=T["Pref"], dot=orc.dot, norm=orc.norm, givens=orc.givens, **KW)
    assert ref[2] in (gr.CONVERGED_RTOL, gr.CONVERGED_ATOL)
    _agree(solver.log, ref, x, T["sysd"]["K"], b, "GMRES(20; Pr = schur)")
    ns.close()


def test_schur_as_pr_of_fgmres_on_stokes(S, po, orc, stokes8):
    """FGMRESSolver(20, schur) against the numpy FGMRES of tests/numpy_twin.py (orc.fgmres_solve takes oracle objects only, and the
    oracle has no Schur preconditioner) with the reference Schur as Pr; its flag follows from the stopping rule of
    SolverTolerances.jl:117-128.  The count is also held against the upper block-triangular preconditioner of _real_stokes on the
    same system: the Schur form needs no more iterations (3 against 4 with the two CPU references at this size)."""
    T = stokes8
    b = T["sysd"]["b"]
    P, sysd = _stokes_schur(S, po, orc)
    solver = S.FGMRESSolver(20, P, **KW)
    ns = _setup(S, solver, sysd["A"])
    x = np.zeros(b.size)
    S.solve_(x, ns, b)
    xo, nit, hist = nt.fgmres(T["sysd"]["K"], b, Pr=T["Pref"], m=20, **KW)
    flag = gr._flag(nit, hist[-1], hist[-1] / hist[0], KW["maxiter"], KW["atol"], KW["rtol"])
    assert flag in (gr.CONVERGED_RTOL, gr.CONVERGED_ATOL)
    _agree(solver.log, (xo, nit, flag, hist), x, T["sysd"]["K"], b, "FGMRES(20, schur)")
    _xt, nit_tri, flag_tri, _ht = orc.fgmres_solve(T["Kc"], b, Pr=T["Po"], m=20, **KW)
    assert flag_tri in (gr.CONVERGED_RTOL, gr.CONVERGED_ATOL)
    print("FGMRES(20) iterations: schur %d (device) / %d (reference), upper block-triangular %d (reference)" % (solver.log.num_iters, nit, nit_tri))
    assert nit <= nit_tri and solver.log.num_iters <= nit_tri
    ns.close()


# ---------------------------------------------------------------- 7: errors
def test_schur_error_behaviour(S, po, orc, pkg, lu_problem):
    abi = importlib.import_module(pkg.__name__ + ".abi")
    lib = abi.load()
    T = lu_problem
    n, b, M = T["n"], T["b"], T["M"]
    idx = M.idx.astype(np.int64); ptr = M.ptr.astype(np.int64)

    def set_block(fn, h, i, j):
        return fn(h, i, j, n, n, M.nnz, ptr.ctypes.data, idx.ctypes.data, M.val.ctypes.data, 0, 0, 8)

    # 3 blocks
    h = C.c_void_p()
    sizes3 = np.array([n, n, n], dtype=np.int64)
    assert lib.gmg_block_create(C.byref(h), 3, sizes3.ctypes.data, abi.BLOCK_SCHUR, 0) == abi.ERR_INVALID
    assert not h.value
    assert lib.gmg_block_create(C.byref(h), 1, sizes3.ctypes.data, abi.BLOCK_SCHUR, 0) == abi.ERR_INVALID
    ns = _setup(S, _lu_solver(S, T), T["mat"])                             # a valid setup still works
    x = np.zeros(2 * n)
    S.solve_(x, ns, b)
    assert rel_err(x, T["x_ref"]) <= TOL_APPLY
    ns.close()
    # C missing: no precond block (1,0) and no system block (1,0)
    sizes = np.array([n, n], dtype=np.int64)
    assert lib.gmg_block_create(C.byref(h), 2, sizes.ctypes.data, abi.BLOCK_SCHUR, 0) == abi.OK
    assert set_block(lib.gmg_block_set_system_block, h, 0, 0) == abi.OK
    assert set_block(lib.gmg_block_set_system_block, h, 1, 1) == abi.OK
    assert set_block(lib.gmg_block_set_precond_block, h, 0, 1) == abi.OK
    for i in range(2):
        assert lib.gmg_block_set_diag_solver(h, i, abi.BLOCK_LU, 0, 0.0, 0.0) == abi.OK
    assert lib.gmg_block_setup(h) == abi.ERR_STATE
    msg = lib.gmg_block_last_error(h)
    assert b"(1,0)" in msg and b"C" in msg
    v = np.zeros(2 * n)
    assert lib.gmg_block_precond_apply(h, b.ctypes.data, v.ctypes.data, abi.MEM_HOST) == abi.ERR_STATE   # not set up
    # the same handle, completed: C from the system this time
    assert set_block(lib.gmg_block_set_system_block, h, 1, 0) == abi.OK
    assert lib.gmg_block_setup(h) == abi.OK
    assert lib.gmg_block_precond_apply(h, b.ctypes.data, v.ctypes.data, abi.MEM_HOST) == abi.OK
    Ms = M.to_scipy().tocsr()
    ref = sr.schur_apply(np.zeros(2 * n), b, sr.exact_solver(Ms), sr.exact_solver(Ms), Ms, Ms, sr.SchurCache(n))
    assert rel_err(v, ref) <= TOL_APPLY
    assert lib.gmg_block_destroy(h) == abi.OK
    # B missing
    assert lib.gmg_block_create(C.byref(h), 2, sizes.ctypes.data, abi.BLOCK_SCHUR, 0) == abi.OK
    assert set_block(lib.gmg_block_set_system_block, h, 1, 0) == abi.OK
    assert lib.gmg_block_setup(h) == abi.ERR_STATE
    assert b"(0,1)" in lib.gmg_block_last_error(h)
    assert lib.gmg_block_destroy(h) == abi.OK
    # a communicator of more than one rank: no partitioned Schur application exists, setup says so (the callbacks are never called)
    xcb, rcb = abi.HOST_EXCHANGE_FN(lambda *a: None), abi.HOST_ALLREDUCE_FN(lambda *a: None)
    assert lib.gmg_block_create(C.byref(h), 2, sizes.ctypes.data, abi.BLOCK_SCHUR, 0) == abi.OK
    assert lib.gmg_block_comm_init_host(h, 0, 2, C.cast(xcb, C.c_void_p), C.cast(rcb, C.c_void_p), None) == abi.OK
    for i in range(2):
        for j in range(2):
            assert set_block(lib.gmg_block_set_system_block, h, i, j) == abi.OK
        assert lib.gmg_block_set_diag_solver(h, i, abi.BLOCK_JACOBI, 0, 0.0, 0.0) == abi.OK
    assert lib.gmg_block_setup(h) == abi.ERR_UNSUPPORTED
    assert b"single-GPU" in lib.gmg_block_last_error(h)
    assert lib.gmg_block_precond_apply(h, b.ctypes.data, v.ctypes.data, abi.MEM_HOST) == abi.ERR_STATE
    assert lib.gmg_block_destroy(h) == abi.OK
    # Pr and Pl both: the existing rule
    P = _lu_solver(S, T)
    with pytest.raises(ValueError, match="not both"):
        _setup(S, S.GMRESSolver(20, Pr=P, Pl=P), T["mat"])
    # (None, schur) as a GMRES side: the unpreconditioned solver on the handle's system
    solver = S.GMRESSolver(10, Pr=(None, P), maxiter=200, atol=1e-14, rtol=1e-10)
    ns = _setup(S, solver, T["mat"])
    x = np.zeros(2 * n)
    S.solve_(x, ns, b)
    Kc = _csr(po, T["K"])
    ref = gr.gmres(lambda u: orc.spmv(Kc, u), b, 10, dot=orc.dot, norm=orc.norm, givens=orc.givens, maxiter=200, atol=1e-14, rtol=1e-10)
    assert ref[2] == gr.CONVERGED_RTOL
    assert solver.log.num_iters == ref[1] and solver.log.flag == ref[2]
    assert np.all(np.abs(np.asarray(solver.log.residuals[: ref[1] + 1]) - ref[3]) <= 1e-10 * ref[3][0])   # test_gpu_gmres.py::_agree
    assert rel_err(x, ref[0]) <= 1e-10
    # and preconditioned on the same kind of handle: one iteration would do with the exact factorisation; a few with rounding
    solver = S.GMRESSolver(10, Pr=P, maxiter=200, atol=1e-14, rtol=1e-10)
    ns2 = _setup(S, solver, T["mat"])
    x2 = np.zeros(2 * n)
    S.solve_(x2, ns2, b)
    assert solver.log.flag == gr.CONVERGED_RTOL and solver.log.num_iters <= 2 < ref[1]
    assert rel_err(x2, x) <= 1e-8
    ns.close(); ns2.close()
