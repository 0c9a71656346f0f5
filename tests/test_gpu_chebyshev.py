"""ChebyshevSmoother on the device (csrc/cheb.inc.hpp) against its numpy restatement (tests/chebyshev_reference.py).

1. whole passes (smooth) within the project's per-kernel gate, x and r, given bounds: Jacobi M on families of gs_edge_problems, patch M
   on Q2 4^3 and Q2 6^2 in every application form; degrees 1, 2, 3, 5; pre and post of different degree; the same pass twice; host
   vectors and (unaligned) device tensors; a pass that starts from x = 0 with x full of NaN
2. degree 1 against the device's own Richardson sweep with omega = 1/theta
3. the estimate: chebyshev_info against the twin's power iteration; a value refresh is bitwise a fresh setup
4. in the solver: CG / FGMRES(5) / V, W, F / mode = :solver / LinearSolverFromSmoother as Pl, iteration count and flag equal to the
   twin's, history within 1e-10 hist[0], solution within 1e-10; the other levels keep their signatures and their bits
5. errors"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp

import chebyshev_reference as cr
import fullsize_reference as fr
import gs_edge_problems as ge
import gs_reference as gr
import numpy_twin as nt
import patch_edge_problems as pe
from conftest import max_rel, rel_err

pytestmark = pytest.mark.gpu

TOL_KERNEL, TOL_HIST = fr.TOL_KERNEL, 1e-8
PLAIN_SELL = dict(pattern=0, vdict=0, idx16=0, opattern=0)   # a layout that stores explicit values: gmg_setup refreshes in place
DEGREE_PAIRS = ((1, 5), (2, 3))                               # (pre, post): degrees 1, 2, 3 and 5 over two handles
JACOBI_BOUNDS = (0.2, 2.0)
PATCH_BOUNDS = (0.88, 8.8)


def _raw(po, M):
    return po.CSR(M.shape, M.indptr, M.indices, M.data)      # raw: `shuffled` keeps its storage order


def _sorted(po, M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return _raw(po, M)


def _setup(S, mats, Ps, Rs, pre, post=None, options=None, **kw):
    post = pre if post is None else post
    kw.setdefault("maxiter", 1)
    gmg = S.GMGLinearSolver(mats, Ps, Rs, pre_smoothers=list(pre), post_smoothers=list(post), options=options, **kw)
    return S.numerical_setup(S.symbolic_setup(gmg, gmg.smatrices[0]), gmg.smatrices[0])


def _ops(po, c, zero_P=False):
    """operators of a gs_edge_problems-style case namespace (A, P, R, Ac)"""
    return [_raw(po, c.A), _raw(po, c.Ac)], [_raw(po, c.P * 0.0 if zero_P else c.P)], [_raw(po, c.R)]


_PROBLEMS = {}


def _q2(po, hierarchy, nc):
    """Q2 Poisson on nc cells, two levels, vertex-star patches -> case namespace with the patch table (pp, pd)"""
    if nc not in _PROBLEMS:
        H = hierarchy(nc, 2, 2)
        A = gr.csr(H["mats"][0].to_scipy())
        pp, pd = po.vertex_star_patches(nc, 2)
        rng = np.random.default_rng([17, A.shape[0]])
        _PROBLEMS[nc] = types.SimpleNamespace(
            name="q2-%s" % "x".join(map(str, nc)), A=A, Ac=gr.csr(H["mats"][1].to_scipy()), P=gr.csr(H["prolongations"][0].to_scipy()),
            R=gr.csr(H["restrictions"][0].to_scipy()), n=A.shape[0], pp=pp, pd=pd, pivot=True,
            x0=rng.uniform(-1, 1, A.shape[0]), r0=rng.uniform(-1, 1, A.shape[0]))
    return _PROBLEMS[nc]


def _big():
    """patch_edge_problems' ragged set with patches of more than 64 dofs (65, 81, 125, 130): patch_apply_big_kernel"""
    if "big" not in _PROBLEMS:
        c = pe.case("big", "nopivot")
        H = pe.two_level(c.A, c.agg)
        _PROBLEMS["big"] = types.SimpleNamespace(name="big", A=gr.csr(c.A), Ac=gr.csr(H["mats"][1]), P=gr.csr(H["prolongations"][0]),
                                                 R=gr.csr(H["restrictions"][0]), n=c.N, pp=c.pp, pd=c.pd, pivot=False, x0=c.x0, r0=c.r)
    return _PROBLEMS["big"]


@functools.lru_cache(maxsize=None)
def _twin_M(key, blocks_shift=None):
    """the twin's M of a patch problem through the explicit inverses the kernels build"""
    c = _PROBLEMS[key]
    blocks = None if blocks_shift is None else pe.blocks_of(c.A, c.pp, c.pd, shift=blocks_shift)
    return cr.PatchInverses(c.A, c.pp, c.pd, pivot=c.pivot, blocks=blocks)


def _smooth(ns, which, x0, r0, device=False):
    """one pass on a copy of (x0, r0) -> (x, r) as numpy arrays.  device: torch tensors that are only 8-byte aligned"""
    if not device:
        x, r = x0.copy(), r0.copy()
        ns.smooth(0, x, r, which)
        return x, r
    import torch
    bx, br = torch.zeros(x0.size + 1, dtype=torch.float64, device="cuda"), torch.zeros(x0.size + 1, dtype=torch.float64, device="cuda")
    x, r = bx[1:], br[1:]
    assert x.data_ptr() % 16 == 8
    x.copy_(torch.from_numpy(x0)); r.copy_(torch.from_numpy(r0))
    ns.smooth(0, x, r, which)
    torch.cuda.synchronize()
    return x.cpu().numpy(), r.cpu().numpy()


def _gate_pass(ns, which, A, M, degree, bnds, c, what, device=False):
    x, r = _smooth(ns, which, c.x0, c.r0, device)
    xo, ro = c.x0.copy(), c.r0.copy()
    cr.chebyshev(A, M, cr.coefficients(degree, *bnds), xo, ro)
    ex, er = max_rel(x, xo), max_rel(r, ro)
    print("%s degree %d%s: max_rel x %.2e r %.2e" % (what, degree, " (device tensors)" if device else "", ex, er))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(r))
    assert ex <= TOL_KERNEL and er <= TOL_KERNEL, (what, degree, ex, er)
    return x, r


def _passes_of_both_slots(S, po, pkg, c, make_M, twin, bnds, what, options=None, device=False):
    for dpre, dpost in DEGREE_PAIRS:
        pre = S.ChebyshevSmoother(make_M(), dpre, lambda_max=bnds[1], lambda_min=bnds[0])
        post = S.ChebyshevSmoother(make_M(), dpost, lambda_max=bnds[1], lambda_min=bnds[0])
        ns = _setup(S, *_ops(po, c), [pre], [post], options=options)
        try:
            for which, d in ((pkg.abi.PRE, dpre), (pkg.abi.POST, dpost)):
                first = _gate_pass(ns, which, c.A, twin, d, bnds, c, what)
                again = _smooth(ns, which, c.x0, c.r0)        # the pass before left its d behind: sweep 0 must not read it
                assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), (what, d, "a second pass differs")
                if device:
                    dev = _gate_pass(ns, which, c.A, twin, d, bnds, c, what, device=True)
                    assert np.array_equal(first[0], dev[0]) and np.array_equal(first[1], dev[1]), (what, d, "device tensors differ")
            assert ns.sweep_signature(0).endswith(" cheb=%d/%d" % (dpre, dpost)), ns.sweep_signature(0)
            info = ns.chebyshev_info(0, "post")
            assert np.isnan(info["lambda_est"]) and (info["degree"], info["lambda_min"], info["lambda_max"]) == (dpost,) + bnds
        finally:
            ns.close()


# ---------------------------------------------------------------- 1. whole passes
@pytest.mark.parametrize("name", ("q1_2d", "blocks", "shuffled"))
def test_whole_passes_jacobi(S, po, pkg, name):
    c = ge.case(name)
    A = gr.csr(c.A)
    cc = types.SimpleNamespace(A=A, Ac=c.Ac, P=c.P, R=c.R, x0=c.x0, r0=c.r0)
    if name == "shuffled":
        cc.A = c.A                                            # the device gets the rows in their stored order
    twin_case = types.SimpleNamespace(**vars(cc))
    twin_case.A = A
    for dpre, dpost in DEGREE_PAIRS:
        pre = S.ChebyshevSmoother(S.JacobiLinearSolver(), dpre, lambda_max=JACOBI_BOUNDS[1], lambda_min=JACOBI_BOUNDS[0])
        post = S.ChebyshevSmoother(S.JacobiLinearSolver(), dpost, lambda_max=JACOBI_BOUNDS[1], lambda_min=JACOBI_BOUNDS[0])
        ns = _setup(S, *_ops(po, cc), [pre], [post])
        try:
            for which, d in ((pkg.abi.PRE, dpre), (pkg.abi.POST, dpost)):
                first = _gate_pass(ns, which, A, nt.Jacobi(A), d, JACOBI_BOUNDS, twin_case, name)
                again = _smooth(ns, which, c.x0, c.r0)
                assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), (name, d, "a second pass differs")
                dev = _gate_pass(ns, which, A, nt.Jacobi(A), d, JACOBI_BOUNDS, twin_case, name, device=True)
                assert np.array_equal(first[0], dev[0]) and np.array_equal(first[1], dev[1]), (name, d, "device tensors differ")
            assert ns.sweep_signature(0).endswith(" cheb=%d/%d" % (dpre, dpost)), ns.sweep_signature(0)
        finally:
            ns.close()


PATCH_OPTIONS = {"operator": None, "operator-off": dict(patch_operator=0), "dedup-off": dict(patch_dedup=0),
                 "both-off": dict(patch_operator=0, patch_dedup=0)}


@pytest.mark.parametrize("form", sorted(PATCH_OPTIONS))
def test_whole_passes_patch_q2_3d(S, po, pkg, hierarchy, form):
    """343 rows, 125 patches of 1 to 27 dofs: de-duplicated blocks and the operator form by default"""
    c = _q2(po, hierarchy, (4, 4, 4))
    assert c.n == 343 and np.diff(c.pp).min() == 1 and np.diff(c.pp).max() == 27
    _passes_of_both_slots(S, po, pkg, c, lambda: S.PatchSolver(c.pp, c.pd), _twin_M((4, 4, 4)), PATCH_BOUNDS, "q2 4^3 " + form,
                          options=PATCH_OPTIONS[form], device=form == "operator")


def test_whole_passes_patch_q2_2d(S, po, pkg, hierarchy):
    """121 rows, 49 patches: fewer than the 64 the de-duplication asks for -> patch_apply_kernel and the contribution buffer"""
    c = _q2(po, hierarchy, (6, 6))
    assert c.n == 121 and c.pp.size - 1 == 49
    _passes_of_both_slots(S, po, pkg, c, lambda: S.PatchSolver(c.pp, c.pd), _twin_M((6, 6)), PATCH_BOUNDS, "q2 6^2", device=True)


def test_whole_passes_patch_caller_blocks(S, po, pkg, hierarchy):
    """gmg_set_smoother_patch_matrices: the blocks are A[p, p] + 0.5 I"""
    c = _q2(po, hierarchy, (4, 4, 4))
    mats = pe.pack_colmajor(pe.blocks_of(c.A, c.pp, c.pd, shift=0.5))
    _passes_of_both_slots(S, po, pkg, c, lambda: S.PatchSolver(c.pp, c.pd, patch_mats=mats), _twin_M((4, 4, 4), 0.5), PATCH_BOUNDS,
                          "q2 4^3 caller blocks")


def test_whole_passes_patch_big(S, po, pkg):
    """patches of 65 .. 130 dofs: patch_apply_big_kernel; dofs sit in 0 .. 9 patches"""
    c = _big()
    assert np.diff(c.pp).max() > 64
    _passes_of_both_slots(S, po, pkg, c, lambda: S.BlockJacobiSolver(c.pp, c.pd), _twin_M("big"), (0.9, 9.9), "big")


@pytest.mark.parametrize("kind", ("jacobi", "patch", "patch-contrib"))
def test_a_pass_from_zero_writes_x_and_the_next_takes_the_internal_r(S, po, hierarchy, kind):
    """mode = :preconditioner hands the first pre-smoothing pass x = 0 (x is written, never read: it arrives full of NaN) and the
    post-smoothing pass the level's own residual buffer.  With P = 0 the coarse correction adds nothing: x is the two passes."""
    if kind == "jacobi":
        g = ge.case("q1_2d")
        c = types.SimpleNamespace(A=gr.csr(g.A), Ac=g.Ac, P=g.P, R=g.R, r0=g.r0)
        make, twin, bnds, options = S.JacobiLinearSolver, nt.Jacobi(c.A), JACOBI_BOUNDS, None
    else:
        c = _q2(po, hierarchy, (4, 4, 4))
        make, twin, bnds = (lambda: S.PatchSolver(c.pp, c.pd)), _twin_M((4, 4, 4)), PATCH_BOUNDS
        options = dict(patch_operator=0) if kind == "patch-contrib" else None
    pre = S.ChebyshevSmoother(make(), 3, lambda_max=bnds[1], lambda_min=bnds[0])
    post = S.ChebyshevSmoother(make(), 2, lambda_max=bnds[1], lambda_min=bnds[0])
    ns = _setup(S, *_ops(po, c, zero_P=True), [pre], [post], options=options)
    try:
        x = np.full(c.A.shape[0], np.nan)
        S.solve_(x, ns, c.r0)
    finally:
        ns.close()
    xo, ro = np.full(c.A.shape[0], np.nan), c.r0.copy()
    cr.chebyshev(c.A, twin, cr.coefficients(3, *bnds), xo, ro, x_zero=True)
    cr.chebyshev(c.A, twin, cr.coefficients(2, *bnds), xo, ro)
    print(kind, "max_rel x %.2e" % max_rel(x, xo))
    assert np.all(np.isfinite(x)) and max_rel(x, xo) <= TOL_KERNEL


# ---------------------------------------------------------------- 2. degree 1 = one Richardson sweep of the device
@pytest.mark.parametrize("kind", ("jacobi", "patch-operator", "patch-contrib", "patch-2d"))
def test_degree_one_is_the_device_richardson_sweep(S, po, hierarchy, kind):
    if kind == "jacobi":
        g = ge.case("q1_2d")
        c = types.SimpleNamespace(A=gr.csr(g.A), Ac=g.Ac, P=g.P, R=g.R, x0=g.x0, r0=g.r0)
        make, bnds, options = S.JacobiLinearSolver, JACOBI_BOUNDS, None
    else:
        c = _q2(po, hierarchy, (6, 6) if kind == "patch-2d" else (4, 4, 4))
        make, bnds = (lambda: S.PatchSolver(c.pp, c.pd)), PATCH_BOUNDS
        options = dict(patch_operator=0) if kind == "patch-contrib" else None
    theta = (bnds[1] + bnds[0]) / 2.0
    out = []
    for sm in (S.ChebyshevSmoother(make(), 1, lambda_max=bnds[1], lambda_min=bnds[0]), S.RichardsonSmoother(make(), 1, 1.0 / theta)):
        ns = _setup(S, *_ops(po, c), [sm], options=options)
        try:
            out.append(_smooth(ns, 0, c.x0, c.r0))
        finally:
            ns.close()
    ex, er = max_rel(out[0][0], out[1][0]), max_rel(out[0][1], out[1][1])
    print(kind, "max_rel x %.2e r %.2e" % (ex, er))
    assert ex <= TOL_KERNEL and er <= TOL_KERNEL


# ---------------------------------------------------------------- 3. the estimate
def _estimate_case(S, po, hierarchy, kind):
    if kind == "jacobi":
        g = ge.case("q1_2d")
        c = types.SimpleNamespace(A=gr.csr(g.A), Ac=g.Ac, P=g.P, R=g.R, x0=g.x0, r0=g.r0)
        return c, S.JacobiLinearSolver, nt.Jacobi(c.A)
    c = _q2(po, hierarchy, (4, 4, 4))
    return c, (lambda: S.PatchSolver(c.pp, c.pd)), _twin_M((4, 4, 4))


@pytest.mark.parametrize("kind", ("jacobi", "patch"))
def test_estimate_is_the_twins_power_iteration(S, po, hierarchy, kind):
    c, make, twin = _estimate_case(S, po, hierarchy, kind)
    for kw in (dict(), dict(eig_steps=4, eig_safety=1.0, eig_ratio=4.0), dict(eig_steps=25, lambda_min=0.05)):
        pre, post = S.ChebyshevSmoother(make(), 3, **kw), S.ChebyshevSmoother(make(), 2, **kw)
        ns = _setup(S, *_ops(po, c), [pre], [post])
        try:
            info, info_post = ns.chebyshev_info(0, "pre"), ns.chebyshev_info(0, "post")
        finally:
            ns.close()
        steps, safety, ratio = kw.get("eig_steps", 10), kw.get("eig_safety", 1.1), kw.get("eig_ratio", 10.0)
        want = cr.power_iteration(c.A, twin, steps)
        dev = abs(info["lambda_est"] - want) / want
        print(kind, kw, "lambda_est %.12f twin %.12f rel %.2e" % (info["lambda_est"], want, dev))
        assert dev <= TOL_HIST
        assert info["lambda_max"] == safety * info["lambda_est"]
        assert info["lambda_min"] == kw.get("lambda_min", info["lambda_max"] / ratio)
        assert (info["degree"], info["eig_steps"], info_post["degree"]) == (3, steps, 2)
        if kind == "jacobi":                                  # pre and post share M = D^-1: one estimate
            assert info_post["lambda_est"] == info["lambda_est"] and info_post["lambda_max"] == info["lambda_max"]
        else:
            assert abs(info_post["lambda_est"] - want) / want <= TOL_HIST
    same = S.ChebyshevSmoother(make(), 3)                     # one object for both slots: one estimate
    ns = _setup(S, *_ops(po, c), [same])
    try:
        assert ns.chebyshev_info(0, "pre") == ns.chebyshev_info(0, "post")
    finally:
        ns.close()


@pytest.mark.parametrize("kind,scaling", [("jacobi", "rows"), ("jacobi", "shifted"), ("patch", "rows")])
def test_value_refresh_is_bitwise_a_fresh_setup(S, po, hierarchy, kind, scaling):
    """the finest matrix scaled row-wise by a smooth positive function (`shifted`: plus a positive diagonal, which moves the spectrum
    of M^-1 A as well): numerical_setup! estimates again, and info, x and r are those of a fresh setup on the new values"""
    c, make, _twin = _estimate_case(S, po, hierarchy, kind)
    n = c.A.shape[0]
    s = 1.0 + 0.5 * np.sin(2.0 * np.pi * np.arange(n) / n)
    A2 = sp.diags(s) @ c.A
    if scaling == "shifted":
        A2 = A2 + sp.diags(0.5 * s * c.A.diagonal())
    A2 = gr.csr(A2)
    assert np.array_equal(A2.indices, c.A.indices) and np.array_equal(A2.indptr, c.A.indptr)
    c2 = types.SimpleNamespace(**vars(c))
    c2.A = A2
    out = []
    for start in (c, c2):
        ns = _setup(S, *_ops(po, start), [S.ChebyshevSmoother(make(), 3)], options=PLAIN_SELL)
        try:
            before = ns.chebyshev_info(0)
            if start is c:
                S.numerical_setup_(ns, _raw(po, A2))
            out.append((ns.chebyshev_info(0), ns.chebyshev_info(0, "post")) + _smooth(ns, 0, c.x0, c.r0))
        finally:
            ns.close()
    print(kind, scaling, "lambda_est before %.12f after %.12f" % (before["lambda_est"], out[0][0]["lambda_est"]))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])
    if scaling == "shifted":
        assert out[0][0]["lambda_est"] < 0.95 * cr.power_iteration(c.A, nt.Jacobi(c.A), 10)


# ---------------------------------------------------------------- 4. in the solver
def _device_smoothers(S, po, H, c):
    kind, degree = c["m"]
    if kind == "jacobi":
        return [S.ChebyshevSmoother(S.JacobiLinearSolver(), degree) for _ in H["ncells"][:-1]]
    return [S.ChebyshevSmoother(S.PatchSolver(*po.vertex_star_patches(cells, c["order"])), degree) for cells in H["ncells"][:-1]]


@pytest.mark.parametrize("name", sorted(cr.SOLVER_CASES))
def test_solver_cases(S, po, hierarchy, name):
    c = cr.SOLVER_CASES[name]
    H = hierarchy(c["nc"], c["nlev"], c["order"])
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    sms = _device_smoothers(S, po, H, c)
    kw = dict(maxiter=100, atol=1e-14, rtol=c["rtol"])
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sms, post_smoothers=sms,
                            cycle_type=c["cycle"] + "_cycle", mode="solver" if c["solver"] == "gmg" else "preconditioner",
                            **(kw if c["solver"] == "gmg" else dict(maxiter=1)))
    if c["solver"] == "cg":
        solver = S.CGSolver(gmg, **kw)
    elif c["solver"] == "fgmres":
        solver = S.FGMRESSolver(5, gmg, **kw)
    elif c["solver"] == "fgmres_pl":
        solver = S.FGMRESSolver(5, gmg, Pl=S.LinearSolverFromSmoother(gmg.pre_smoothers[0]), **kw)
    else:
        solver = gmg
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    gns = ns if solver is gmg else ns.P_ns
    try:
        x = np.zeros(b.size)
        S.solve_(x, ns, b)
        sigs = [gns.sweep_signature(l) for l in range(c["nlev"])]
    finally:
        gns.close()
    xo, nit, hist = cr.solver_reference(po, c)
    log = solver.log
    print(name, "iterations", log.num_iters, "twin", nit, "rel_err x %.2e" % rel_err(x, xo))
    assert hist[-1] / hist[0] < c["rtol"]
    assert log.num_iters == nit and log.flag == S.SOLVER_CONVERGED_RTOL, (log.num_iters, nit, log.flag)
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= 1e-10 * hist[0])
    assert rel_err(x, xo) <= 1e-10
    for sig in sigs[:-1]:
        assert sig.endswith(" cheb=%d/%d" % (c["m"][1], c["m"][1])), sigs
    assert " cheb=" not in sigs[-1]


@pytest.mark.parametrize("other", ("jacobi", "gauss-seidel"))
def test_other_levels_keep_their_signature_and_their_bits(S, po, hierarchy, other):
    """three levels, Chebyshev on level 0 only, against a second handle without it: level 1 is swept by the same kernels to the
    same bits, and only level 0's signature names the Chebyshev slot"""
    H = hierarchy((16, 16, 16), 3, 1)
    lev1 = S.RichardsonSmoother(S.JacobiLinearSolver(), 3, 2.0 / 3.0) if other == "jacobi" else S.SymGaussSeidelSmoother(1, 1.0)
    n1 = H["mats"][1].shape[0]
    rng = np.random.default_rng(5)
    x0, r0 = rng.uniform(-1, 1, n1), rng.uniform(-1, 1, n1)
    b = po.random_rhs(H["mats"][0].shape[0])
    out = []
    for lev0 in (S.ChebyshevSmoother(S.JacobiLinearSolver(), 3), S.RichardsonSmoother(S.JacobiLinearSolver(), 3, 2.0 / 3.0)):
        ns = _setup(S, H["mats"], H["prolongations"], H["restrictions"], [lev0, lev1])
        try:
            x, r = x0.copy(), r0.copy()
            ns.smooth(1, x, r)
            sig1 = ns.sweep_signature(1)                      # (before any cycle: which transfers a cycle folds into level 1's passes
            z = np.zeros(b.size)                              # depends on how level 0 is swept, and the signature lists them)
            S.solve_(z, ns, b)                                # one V-cycle: level 0's sweeps name their kernel
            out.append((x, r, ns.sweep_signature(0), sig1, z))
        finally:
            ns.close()
    (xc, rc, sig0c, sig1c, zc), (xp, rp, sig0p, sig1p, _zp) = out
    assert np.array_equal(xc, xp) and np.array_equal(rc, rp)
    assert sig1c == sig1p and " cheb=" not in sig1c and " cheb=" not in sig0p
    assert sig0c.endswith(" cheb=3/3") and np.all(np.isfinite(zc))


# ---------------------------------------------------------------- 5. errors
def _jacobi_handle(S, po, pre=None):
    c = ge.case("q1_3d-1")
    return _setup(S, *_ops(po, c), [pre or S.RichardsonSmoother(S.JacobiLinearSolver(), 2, 0.8)]), c


def test_setter_checks(S, po, pkg):
    abi = pkg.abi
    ns, c = _jacobi_handle(S, po)
    lib, h = ns._lib, ns.h
    try:
        ok = (3, 0.0, 0.0, 10, 10.0, 1.1)
        bad = ((0,) + ok[1:], (-3,) + ok[1:], (3, 2.0, 2.0, 10, 10.0, 1.1), (3, 3.0, 2.0, 10, 10.0, 1.1), (3, 0.0, 0.0, 10, 1.0, 1.1),
               (3, 0.0, 0.0, 10, 0.5, 1.1), (3, 0.0, 0.0, 10, 10.0, 0.99), (3, 0.0, 0.0, 0, 10.0, 1.1), (3, 0.0, 0.0, -1, 10.0, 1.1))
        for args in bad:
            assert lib.gmg_set_smoother_chebyshev(h, 0, abi.PRE_AND_POST, *args) == abi.ERR_INVALID, args
        assert lib.gmg_set_smoother_chebyshev(h, 1, abi.PRE, *ok) == abi.ERR_INVALID        # the coarsest level
        assert lib.gmg_set_smoother_chebyshev(h, 0, 7, *ok) == abi.ERR_INVALID
        x, r = c.x0.copy(), c.r0.copy()
        ns.smooth(0, x, r)                                    # the refused calls left the handle as it was
        assert " cheb=" not in ns.sweep_signature(0) and np.all(np.isfinite(x))
        with pytest.raises(abi.GmgError) as e:                # a slot without Chebyshev
            ns.chebyshev_info(0)
        assert e.value.code == abi.ERR_STATE
        # lambda_max <= 0 means "estimate", lambda_min <= 0 "from eig_ratio"
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.PRE, 2, -1.0, -1.0, 10, 10.0, 1.1) == abi.OK
        with pytest.raises(abi.GmgError) as e:                # before setup
            ns.chebyshev_info(0)
        assert e.value.code == abi.ERR_STATE
        ns.setup()
        info = ns.chebyshev_info(0)
        assert info["degree"] == 2 and info["lambda_est"] > 0.0 and info["lambda_min"] == info["lambda_max"] / 10.0
        assert ns.sweep_signature(0).endswith(" cheb=2/0")
        with pytest.raises(abi.GmgError) as e:                # the post slot kept its Richardson iteration
            ns.chebyshev_info(0, "post")
        assert e.value.code == abi.ERR_STATE
        # a plain smoother on the slot clears it
        assert lib.gmg_set_smoother_jacobi(h, 0, abi.PRE, 2, 0.8) == abi.OK
        ns.setup()
        with pytest.raises(abi.GmgError) as e:
            ns.chebyshev_info(0)
        assert e.value.code == abi.ERR_STATE and " cheb=" not in ns.sweep_signature(0)
        x2, r2 = c.x0.copy(), c.r0.copy()
        ns.smooth(0, x2, r2)
        assert np.array_equal(x2, x) and np.array_equal(r2, r)
    finally:
        ns.close()


def test_slot_without_smoother_and_gauss_seidel_slot(S, po, pkg):
    abi = pkg.abi
    lib = abi.load()
    h = C.c_void_p()
    abi.check(None, lib.gmg_create(C.byref(h), 2, 0))
    try:
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.PRE_AND_POST, 3, 0.0, 0.0, 10, 10.0, 1.1) == abi.ERR_STATE
        assert lib.gmg_set_smoother_jacobi(h, 0, abi.PRE, 2, 1.0) == abi.OK
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.POST, 3, 0.0, 0.0, 10, 10.0, 1.1) == abi.ERR_STATE
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.PRE, 3, 0.0, 0.0, 10, 10.0, 1.1) == abi.OK
    finally:
        lib.gmg_destroy(h)
    ns, _c = _jacobi_handle(S, po, S.SymGaussSeidelSmoother(1))
    try:
        assert ns._lib.gmg_set_smoother_chebyshev(ns.h, 0, abi.PRE, 3, 0.0, 0.0, 10, 10.0, 1.1) == abi.ERR_UNSUPPORTED
        assert ns.sweep_signature(0).endswith(" gs=F+B")
    finally:
        ns.close()


def test_a_handle_with_a_communicator_is_refused_at_setup(S, po, pkg):
    abi = pkg.abi
    ns, _c = _jacobi_handle(S, po, S.ChebyshevSmoother(S.JacobiLinearSolver(), 2))
    xfn = abi.HOST_EXCHANGE_FN(lambda *a: None)
    rfn = abi.HOST_ALLREDUCE_FN(lambda *a: None)
    try:
        abi.check(ns.h, ns._lib.gmg_comm_init_host(ns.h, 0, 1, C.cast(xfn, C.c_void_p), C.cast(rfn, C.c_void_p), None))
        with pytest.raises(abi.GmgError) as e:
            ns.setup()
        assert e.value.code == abi.ERR_UNSUPPORTED and "Chebyshev" in str(e.value) and "communicator" in str(e.value)
    finally:
        ns.close()
