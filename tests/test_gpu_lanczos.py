"""CG's Lanczos diagnostic (gmg_cg_set_trace / gmg_cg_get_trace, CGSolver(diagnostic=...)) and the Lanczos bounds of ChebyshevSmoother
(eig_method="lanczos") on the device, against tests/lanczos_reference.py.

1. the trace against the twin: count, alpha_k, beta_k for Pl none / Jacobi / GMG / GMG flexible / finest pre-smoother
2. the diagnostic: bitwise the host replay of the fetched trace; estimate_ against the twin's
3. no arithmetic change: x and the history with and without the diagnostic, the trace of two identical solves, the launches
4. edge cases
5. the Chebyshev estimate, and 6. in the solver

Largest deviation of a traced scalar from the twin seen on an MI355X (section 1, printed per case): see DESIGN.md, section 4e."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import chebyshev_reference as cr
import gs_reference as gr
import lanczos_reference as lr
import numpy_twin as nt
from conftest import rel_err
from test_gpu_chebyshev import PATCH_OPTIONS, PLAIN_SELL, _big, _ops, _q2, _raw, _setup, _smooth, _twin_M

pytestmark = pytest.mark.gpu

TOL_HIST = 1e-8
PROBLEMS = {"q1-16^2": ((16, 16), 3), "q1-16^3": ((16, 16, 16), 3)}
PLS = ("none", "jacobi", "gmg", "gmg-flexible", "pre-smoother")
KW = dict(maxiter=60, atol=1e-14, rtol=1e-8)
OMEGA = 2.0 / 3.0


def _rich(S):
    return S.RichardsonSmoother(S.JacobiLinearSolver(), 3, OMEGA)


def _solver(S, H, pl, diag=None, options=None, coarsest=None, **kw):
    kw = dict(KW, **kw)
    sms = [_rich(S) for _ in H["mats"][:-1]]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sms, post_smoothers=sms, maxiter=1,
                            options=options, coarsest_solver=coarsest)
    P = {"none": (None, gmg), "jacobi": (S.JacobiLinearSolver(), gmg), "gmg": gmg, "gmg-flexible": gmg,
         "pre-smoother": (S.LinearSolverFromSmoother(gmg.pre_smoothers[0]), gmg)}[pl]
    return S.CGSolver(P, flexible=pl == "gmg-flexible", diagnostic=diag, **kw)


def _run(S, solver, A, b, x0=None):
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    try:
        x = np.zeros(b.size) if x0 is None else x0.copy()
        S.solve_(x, ns, b)
        trace = ns.P_ns.cg_trace() if solver.diag is not None else None
    finally:
        ns.close()
    return x, solver.log.num_iters, np.array(solver.log.residuals[: solver.log.num_iters + 1]), trace


@functools.lru_cache(maxsize=None)
def _twin(po, name, pl):
    nc, nlev = PROBLEMS[name]
    H = po.build_hierarchy(nc, nlev, 1)
    A = H["mats"][0].to_scipy().tocsr()
    A.sort_indices()
    b = po.random_rhs(A.shape[0])
    if pl == "none":
        Pl = None
    elif pl == "jacobi":
        Pl = nt.Jacobi(A).solve
    elif pl == "pre-smoother":
        Pl = cr.apply_smoother(cr.Rich("jacobi", 3, OMEGA), A, None)
    else:
        Pl = cr.GMG(H["mats"], H["prolongations"], H["restrictions"], [cr.Rich("jacobi", 3, OMEGA) for _ in H["mats"][:-1]]).solve
    return lr.cg(A, b, Pl=Pl, flexible=pl == "gmg-flexible", **KW)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if b.size else 0.0


# ---------------------------------------------------------------- 1. + 2. the trace and the diagnostic against the twin
@pytest.mark.parametrize("pl", PLS)
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_trace_and_diagnostic_against_the_twin(S, po, hierarchy, name, pl):
    nc, nlev = PROBLEMS[name]
    H = hierarchy(nc, nlev, 1)
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    diag = S.LanczosDiagnostic(KW["maxiter"] + 1)
    solver = _solver(S, H, pl, diag)
    x, nit, hist, (alpha, beta) = _run(S, solver, A, b)
    xo, nito, histo, ao, bo = _twin(po, name, pl)
    assert alpha.size == beta.size == nit == nito, (alpha.size, nit, nito)
    ea, eb = _rel(alpha, ao), _rel(beta, bo)
    print(name, pl, "iterations %d  max rel deviation alpha %.2e beta %.2e" % (nit, ea, eb))
    assert ea <= TOL_HIST and eb <= TOL_HIST
    # the diagnostic is bitwise the host replay of the fetched trace (the twin's formulas)
    d, g = lr.diagnostic(alpha, beta, KW["maxiter"] + 1)
    assert diag.k == nit and np.array_equal(diag.delta, d) and np.array_equal(diag.gamma, g, equal_nan=True)
    want = lr.estimate(*lr.diagnostic(ao, bo))
    got = S.estimate_(diag)
    print(name, pl, "estimate %.10f twin %.10f" % (got, want))
    assert abs(got - want) <= TOL_HIST * want


# ---------------------------------------------------------------- 3. no arithmetic change
@pytest.mark.parametrize("options", (None, {"red_fused": 0}, {"cg_split": 1}), ids=("default", "red_fused=0", "cg_split=1"))
def test_tracing_changes_no_arithmetic_and_no_launch(S, po, hierarchy, options):
    H = hierarchy((16, 16, 16), 3, 1)
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    plain = _run(S, _solver(S, H, "gmg", None, options), A, b)
    runs = [_run(S, _solver(S, H, "gmg", S.LanczosDiagnostic(61), options), A, b) for _ in range(2)]
    for x, nit, hist, (alpha, beta) in runs:
        assert nit == plain[1] and np.array_equal(x, plain[0]) and np.array_equal(hist, plain[2])
        assert alpha.size == nit and np.all(np.isfinite(alpha)) and np.all(beta > 0.0)
    assert np.array_equal(runs[0][3][0], runs[1][3][0]) and np.array_equal(runs[0][3][1], runs[1][3][1])
    # launches of level 0's sweeps per iteration: a handle that never traced against one whose tracing was switched off again
    counts = []
    for traced in (False, True):
        solver = _solver(S, H, "gmg", S.LanczosDiagnostic(61) if traced else None, options)
        ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
        try:
            if traced:
                ns.P_ns.cg_set_trace(0)
                solver.diag = None
            ns.P_ns.profile(0, True)
            x = np.zeros(b.size)
            S.solve_(x, ns, b)
            st = ns.P_ns.kernel_stats()
            counts.append((st["launches"], st["fused_passes"], solver.log.num_iters))
            assert np.array_equal(x, plain[0])
        finally:
            ns.close()
    print(options, "launches, one-launch passes, iterations:", counts)
    assert counts[0] == counts[1] and counts[0][0] > 0


# ---------------------------------------------------------------- 4. edge cases
def test_maxiter_zero_and_convergence_at_the_first_iteration(S, po, hierarchy):
    H = hierarchy((16, 16), 3, 1)
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    diag = S.LanczosDiagnostic(1)
    diag.update_(3.0, 3.0)
    x, nit, hist, (alpha, beta) = _run(S, _solver(S, H, "gmg", diag, maxiter=0), A, b)
    assert nit == 0 == alpha.size == beta.size == diag.k and S.estimate_(diag) == 1.0 and not diag.delta.any() and not x.any()
    diag = S.LanczosDiagnostic(5)
    x, nit, hist, (alpha, beta) = _run(S, _solver(S, H, "gmg", diag, maxiter=5, rtol=0.5), A, b)
    xo, nito, histo, ao, bo = lr.cg(A.to_scipy().tocsr(), b, Pl=cr.GMG(H["mats"], H["prolongations"], H["restrictions"],
                                                                       [cr.Rich("jacobi", 3, OMEGA)] * 2).solve, maxiter=5, atol=1e-14, rtol=0.5)
    assert nit == 1 == nito == alpha.size == diag.k and S.estimate_(diag) == 1.0
    assert _rel(alpha, ao) <= TOL_HIST and _rel(beta, bo) <= TOL_HIST
    assert diag.delta[0] == 1.0 / alpha[0] and diag.gamma[0] == 0.0


def test_host_vectors_device_tensors_and_a_second_solve(S, po, hierarchy):
    import torch
    H = hierarchy((16, 16, 16), 3, 1)
    A = H["mats"][0]
    n = A.shape[0]
    b = po.random_rhs(n)
    diag = S.LanczosDiagnostic(61)
    solver = _solver(S, H, "gmg", diag)
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    try:
        x = np.zeros(n)
        S.solve_(x, ns, b)
        host = (x.copy(), solver.log.num_iters, diag.delta.copy(), diag.gamma.copy()) + ns.P_ns.cg_trace()
        bx, bb = torch.zeros(n + 1, dtype=torch.float64, device="cuda"), torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        xd, bd = bx[1:], bb[1:]
        assert xd.data_ptr() % 16 == 8
        bd.copy_(torch.from_numpy(b))
        S.solve_(xd, ns, bd)
        torch.cuda.synchronize()
        al, be = ns.P_ns.cg_trace()
        print("host / device tensors: rel_err x %.2e, alpha %.2e" % (rel_err(xd.cpu().numpy(), host[0]), _rel(al, host[4])))
        assert solver.log.num_iters == host[1] == al.size and rel_err(xd.cpu().numpy(), host[0]) <= 1e-10
        assert _rel(al, host[4]) <= TOL_HIST and _rel(be, host[5]) <= TOL_HIST
        # a second, shorter solve resets the trace and the diagnostic
        solver.log.rtol = 1e-2
        x2 = np.zeros(n)
        S.solve_(x2, ns, b)
        al2, be2 = ns.P_ns.cg_trace()
        k = solver.log.num_iters
        assert 0 < k < host[1] and al2.size == k == diag.k
        assert np.array_equal(al2, host[4][:k]) and np.array_equal(be2, host[5][:k])
        assert np.array_equal(diag.delta[:k], host[2][:k]) and not diag.delta[k:].any() and not diag.gamma[k:].any()
    finally:
        ns.close()


def test_entry_points_buffer_and_refusals(S, po, pkg, hierarchy):
    abi = pkg.abi
    H = hierarchy((16, 16), 3, 1)
    A = H["mats"][0]
    n = A.shape[0]
    b = po.random_rhs(n)
    solver = _solver(S, H, "jacobi", None)
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    g = ns.P_ns
    try:
        k = C.c_int(-1)
        assert g._lib.gmg_cg_get_trace(g.h, C.byref(k), None, None, 0) == abi.ERR_STATE           # tracing is off by default
        assert g._lib.gmg_cg_set_trace(g.h, -1) == abi.ERR_INVALID
        before = g.device_bytes()
        g.cg_set_trace(40)
        assert g.device_bytes() == before + 2 * 40 * 8
        g.setup()                                             # the buffer is not part of a setup: it stays, and stays counted
        assert g.device_bytes() == before + 2 * 40 * 8
        al, be = g.cg_trace()
        assert al.size == 0 == be.size                        # no solve yet
        solver.diag = S.LanczosDiagnostic(60)
        x = np.full(n, 7.0)
        with pytest.raises(abi.GmgError) as e:                # maxiter 60 > capacity 40: refused before any work
            S.solve_(x, ns, b)
        assert e.value.code == abi.ERR_INVALID and "60" in str(e.value) and "40" in str(e.value) and np.all(x == 7.0)
        solver.log.maxiter = 40
        solver.log.residuals = np.zeros(41)
        x = np.zeros(n)
        S.solve_(x, ns, b)
        nit = solver.log.num_iters
        assert 2 < nit <= 40 and solver.diag.k == nit
        buf = np.zeros(nit)
        assert g._lib.gmg_cg_get_trace(g.h, C.byref(k), C.c_void_p(buf.ctypes.data), None, nit - 1) == abi.ERR_INVALID   # cap < count
        assert g._lib.gmg_cg_get_trace(g.h, C.byref(k), None, C.c_void_p(buf.ctypes.data), nit) == abi.OK and k.value == nit
        assert np.array_equal(buf, g.cg_trace()[1])
        g.cg_set_trace(0)                                     # released
        assert g.device_bytes() == before
        assert g._lib.gmg_cg_get_trace(g.h, C.byref(k), None, None, 0) == abi.ERR_STATE
    finally:
        ns.close()


def test_a_nested_cg_leaves_only_the_outer_iterations(S, po, hierarchy):
    H = hierarchy((16, 16, 16), 2, 1)                          # coarsest level 7^3 = 343 rows: the nested CG iterates
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    out = []
    for diag in (None, S.LanczosDiagnostic(61)):
        coarse = S.CGSolver(S.JacobiLinearSolver(), maxiter=200, atol=1e-14, rtol=1e-12)
        out.append(_run(S, _solver(S, H, "gmg", diag, coarsest=coarse), A, b))
    (xp, nitp, histp, _none), (x, nit, hist, (alpha, beta)) = out
    assert nit == nitp and np.array_equal(x, xp) and np.array_equal(hist, histp)
    assert 2 < nit < 30 and alpha.size == nit == beta.size and np.all(alpha > 0.0) and np.all(beta > 0.0)
    # the outer scalars, not the coarse solver's: the twin's coarse solve is an LU.  The nested CG stops at a relative residual of
    # 1e-12, an error of at most kappa(D^-1 A_coarse) 1e-12 ~ 3e-11 in the coarse correction; noise of 1e-13 in every operator moves
    # alpha and beta by 1e-11 on these problems, so 3e-11 moves them by about 3e-9: the gate of 1e-6 keeps two orders over that
    H2 = po.build_hierarchy((16, 16, 16), 2, 1)
    G = cr.GMG(H2["mats"], H2["prolongations"], H2["restrictions"], [cr.Rich("jacobi", 3, OMEGA)])
    xo, nito, histo, ao, bo = lr.cg(A.to_scipy().tocsr(), b, Pl=G.solve, **KW)
    print("nested: iterations %d twin %d  alpha %.2e beta %.2e" % (nit, nito, _rel(alpha, ao), _rel(beta, bo)))
    assert nit == nito and _rel(alpha, ao) <= 1e-6 and _rel(beta, bo) <= 1e-6


# ---------------------------------------------------------------- 5. the Chebyshev estimate
def _estimate_cases(S, po, hierarchy, kind):
    """-> (case namespace, make_M, the twin's M, options)"""
    if kind == "jacobi":
        H = hierarchy((16, 16, 16), 2, 1)
        A = gr.csr(H["mats"][0].to_scipy())
        c = types.SimpleNamespace(A=A, Ac=gr.csr(H["mats"][1].to_scipy()), P=gr.csr(H["prolongations"][0].to_scipy()),
                                  R=gr.csr(H["restrictions"][0].to_scipy()))
        return c, S.JacobiLinearSolver, nt.Jacobi(A), None
    if kind == "block-jacobi":
        c = _big()
        return c, (lambda: S.BlockJacobiSolver(c.pp, c.pd)), _twin_M("big"), None
    c = _q2(po, hierarchy, (4, 4, 4))
    return c, (lambda: S.PatchSolver(c.pp, c.pd)), _twin_M((4, 4, 4)), PATCH_OPTIONS["operator" if kind == "patch-operator" else "both-off"]


@pytest.mark.parametrize("kind", ("jacobi", "patch-operator", "patch-contrib", "block-jacobi"))
def test_estimate_is_the_twins_lanczos(S, po, hierarchy, kind):
    c, make, twin, options = _estimate_cases(S, po, hierarchy, kind)
    for steps, safety in ((4, 1.0), (10, 1.1), (25, 1.1)):
        kw = dict(eig_steps=steps, eig_safety=safety, eig_method="lanczos")
        pre, post = S.ChebyshevSmoother(make(), 3, **kw), S.ChebyshevSmoother(make(), 2, **kw)
        other = S.ChebyshevSmoother(make(), 2, eig_steps=steps, eig_safety=safety)          # the power iteration
        infos = []
        for po_st in (post, other):
            ns = _setup(S, *_ops(po, c), [pre], [po_st], options=options)
            try:
                infos.append((ns.chebyshev_info(0, "pre"), ns.chebyshev_info(0, "post")))
            finally:
                ns.close()
        (info, info_post), (info_b, info_power) = infos
        T, k, gs = lr.lanczos_tridiagonal(c.A, twin, steps, with_gammas=True)
        want = float(np.linalg.eigvalsh(T).max())
        dev = abs(info["lambda_est"] - want) / want
        print(kind, "steps %d done %d twin %d  lambda_est %.12f twin %.12f rel %.2e" % (steps, info["eig_steps_done"], k, info["lambda_est"], want, dev))
        assert dev <= TOL_HIST
        assert info["lambda_max"] == safety * info["lambda_est"] and info["lambda_min"] == info["lambda_max"] / 10.0
        assert (info["eig_method"], info["eig_steps"], info["degree"]) == ("lanczos", steps, 3)
        assert info["eig_steps_done"] <= steps
        if k == steps and gs.min() > 1e-20 * gs[0]:
            assert info["eig_steps_done"] == steps
        assert info == info_b
        # pre and post share the estimate when M and the method are the same
        assert info_post["eig_method"] == "lanczos" and abs(info_post["lambda_est"] - want) / want <= TOL_HIST
        if kind == "jacobi":
            assert info_post["lambda_est"] == info["lambda_est"] and info_post["eig_steps_done"] == info["eig_steps_done"]
        # ... and not when the methods differ
        assert (info_power["eig_method"], info_power["eig_steps_done"]) == ("power", steps)
        pw = cr.power_iteration(c.A, twin, steps)
        assert abs(info_power["lambda_est"] - pw) / pw <= TOL_HIST and info_power["lambda_est"] != info["lambda_est"]


def test_nine_rows_stop_early_with_the_exact_lambda_max(S, po, hierarchy):
    H = hierarchy((4, 4), 2, 1)
    A = gr.csr(H["mats"][0].to_scipy())
    assert A.shape[0] == 9
    c = types.SimpleNamespace(A=A, Ac=gr.csr(H["mats"][1].to_scipy()), P=gr.csr(H["prolongations"][0].to_scipy()),
                              R=gr.csr(H["restrictions"][0].to_scipy()))
    ns = _setup(S, *_ops(po, c), [S.ChebyshevSmoother(S.JacobiLinearSolver(), 3, eig_steps=25, eig_method="lanczos")])
    try:
        info = ns.chebyshev_info(0)
    finally:
        ns.close()
    s = np.sqrt(1.0 / A.diagonal())
    true = np.linalg.eigvalsh(s[:, None] * A.toarray() * s[None, :]).max()
    T, k = lr.lanczos_tridiagonal(A, nt.Jacobi(A), 25)
    print("9 rows: steps done %d twin %d lambda_est %.15f true %.15f" % (info["eig_steps_done"], k, info["lambda_est"], true))
    assert info["eig_steps_done"] < 25 and info["eig_steps_done"] <= 9 and k <= 9
    assert abs(info["lambda_est"] - true) <= 1e-10 * true


@pytest.mark.parametrize("kind", ("jacobi", "patch-operator"))
def test_value_refresh_is_bitwise_a_fresh_setup(S, po, hierarchy, kind):
    c, make, _twin_m, _o = _estimate_cases(S, po, hierarchy, kind)
    c = types.SimpleNamespace(**vars(c))                      # (the patch case is shared with other tests: left as it is)
    n = c.A.shape[0]
    rng = np.random.default_rng(11)
    c.x0, c.r0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    s = 1.0 + 0.5 * np.sin(2.0 * np.pi * np.arange(n) / n)
    A2 = c.A.copy()                                           # rows scaled in place: the stored pattern (explicit zeros too) stays
    A2.data = A2.data * np.repeat(s, np.diff(A2.indptr))
    assert np.array_equal(A2.indices, c.A.indices) and np.array_equal(A2.indptr, c.A.indptr)
    c2 = types.SimpleNamespace(**vars(c))
    c2.A = A2
    out, nbytes = [], {}
    for method in ("power", "lanczos"):                       # the estimate's work vector is gone again: the bytes of a power handle,
        ns = _setup(S, *_ops(po, c), [S.ChebyshevSmoother(make(), 3, eig_method=method)], options=PLAIN_SELL)   # fresh and refreshed
        try:
            nbytes[method] = [ns.device_bytes()]
            S.numerical_setup_(ns, _raw(po, A2))
            nbytes[method].append(ns.device_bytes())
        finally:
            ns.close()
    assert nbytes["lanczos"] == nbytes["power"], nbytes
    for start in (c, c2):
        ns = _setup(S, *_ops(po, start), [S.ChebyshevSmoother(make(), 3, eig_method="lanczos")], options=PLAIN_SELL)
        try:
            before = ns.chebyshev_info(0)
            if start is c:
                S.numerical_setup_(ns, _raw(po, A2))
            out.append((ns.chebyshev_info(0), ns.chebyshev_info(0, "post")) + _smooth(ns, 0, c.x0, c.r0))
        finally:
            ns.close()
    print(kind, "lambda_est before %.12f after %.12f" % (before["lambda_est"], out[0][0]["lambda_est"]))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][0]["eig_method"] == "lanczos"
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


def test_errors_of_the_estimate(S, po, pkg, hierarchy):
    abi = pkg.abi
    c, make, _t, _o = _estimate_cases(S, po, hierarchy, "jacobi")
    neg = types.SimpleNamespace(**vars(c))
    neg.A = gr.csr(-c.A)
    with pytest.raises(abi.GmgError) as e:                    # z . r = r . D^-1 r < 0 in the first step
        _setup(S, *_ops(po, neg), [S.ChebyshevSmoother(make(), 3, eig_method="lanczos")])
    assert e.value.code == abi.ERR_SINGULAR and "level 0" in str(e.value) and "positive definite" in str(e.value)
    assert "power" in str(e.value) and "lambda_max" in str(e.value)
    ns = _setup(S, *_ops(po, c), [S.RichardsonSmoother(make(), 2, 0.8)])
    try:
        lib, h = ns._lib, ns.h
        assert lib.gmg_set_chebyshev_eig_method(h, 0, abi.PRE, abi.CHEB_EIG_LANCZOS) == abi.ERR_STATE      # no Chebyshev slot
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.PRE_AND_POST, 3, 0.0, 0.0, 10, 10.0, 1.1) == abi.OK
        assert lib.gmg_set_chebyshev_eig_method(h, 0, abi.PRE_AND_POST, 2) == abi.ERR_INVALID
        assert lib.gmg_set_chebyshev_eig_method(h, 0, 7, abi.CHEB_EIG_LANCZOS) == abi.ERR_INVALID
        assert lib.gmg_set_chebyshev_eig_method(h, 1, abi.PRE, abi.CHEB_EIG_LANCZOS) == abi.ERR_INVALID    # the coarsest level
        assert lib.gmg_set_chebyshev_eig_method(h, 0, abi.POST, abi.CHEB_EIG_LANCZOS) == abi.OK
        ns.setup()
        pre, post = ns.chebyshev_info(0, "pre"), ns.chebyshev_info(0, "post")
        assert (pre["eig_method"], post["eig_method"]) == ("power", "lanczos") and post["lambda_est"] > pre["lambda_est"]
        # a given lambda_max: the method is ignored
        assert lib.gmg_set_smoother_chebyshev(h, 0, abi.PRE, 3, 0.0, 2.0, 10, 10.0, 1.1) == abi.OK
        assert lib.gmg_set_chebyshev_eig_method(h, 0, abi.PRE, abi.CHEB_EIG_LANCZOS) == abi.OK
        ns.setup()
        pre = ns.chebyshev_info(0, "pre")
        assert np.isnan(pre["lambda_est"]) and pre["lambda_max"] == 2.0 and pre["eig_steps_done"] == 0
        # a handle with a communicator is still refused
        xfn = abi.HOST_EXCHANGE_FN(lambda *a: None)
        rfn = abi.HOST_ALLREDUCE_FN(lambda *a: None)
        abi.check(ns.h, lib.gmg_comm_init_host(h, 0, 1, C.cast(xfn, C.c_void_p), C.cast(rfn, C.c_void_p), None))
        with pytest.raises(abi.GmgError) as e:
            ns.setup()
        assert e.value.code == abi.ERR_UNSUPPORTED and "Chebyshev" in str(e.value) and "communicator" in str(e.value)
    finally:
        ns.close()


# ---------------------------------------------------------------- 6. in the solver
@functools.lru_cache(maxsize=None)
def _solver_reference(po, name):
    c = cr.SOLVER_CASES[name]
    H = po.build_hierarchy(c["nc"], c["nlev"], c["order"])
    A = H["mats"][0].to_scipy().tocsr()
    A.sort_indices()
    b = po.random_rhs(A.shape[0])
    kind, degree = c["m"]
    specs = ["jacobi" if kind == "jacobi" else ("patch",) + po.vertex_star_patches(cells, c["order"]) for cells in H["ncells"][:-1]]
    G = cr.GMG(H["mats"], H["prolongations"], H["restrictions"], [lr.LanczosCheb(s, degree) for s in specs], cycle=c["cycle"])
    return cr.cg(A, b, Pl=G.solve, maxiter=100, atol=1e-14, rtol=c["rtol"])


@pytest.mark.parametrize("name", ("cg-q1-3lev-w", "cg-q2-2lev-v"))
def test_solver_cases_with_lanczos_bounds(S, po, hierarchy, name):
    c = cr.SOLVER_CASES[name]
    H = hierarchy(c["nc"], c["nlev"], c["order"])
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    kind, degree = c["m"]
    if kind == "jacobi":
        sms = [S.ChebyshevSmoother(S.JacobiLinearSolver(), degree, eig_method="lanczos") for _ in H["ncells"][:-1]]
    else:
        sms = [S.ChebyshevSmoother(S.PatchSolver(*po.vertex_star_patches(cells, c["order"])), degree, eig_method="lanczos")
               for cells in H["ncells"][:-1]]
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sms, post_smoothers=sms,
                            cycle_type=c["cycle"] + "_cycle", maxiter=1)
    solver = S.CGSolver(gmg, maxiter=100, atol=1e-14, rtol=c["rtol"])
    ns = S.numerical_setup(S.symbolic_setup(solver, A), A)
    try:
        x = np.zeros(b.size)
        S.solve_(x, ns, b)
        infos = [ns.P_ns.chebyshev_info(l) for l in range(c["nlev"] - 1)]
    finally:
        ns.close()
    xo, nit, hist = _solver_reference(po, name)
    log = solver.log
    print(name, "iterations", log.num_iters, "twin", nit, "rel_err x %.2e" % rel_err(x, xo), [i["lambda_est"] for i in infos])
    assert all(i["eig_method"] == "lanczos" for i in infos)
    assert hist[-1] / hist[0] < c["rtol"]
    assert log.num_iters == nit and log.flag == S.SOLVER_CONVERGED_RTOL, (log.num_iters, nit, log.flag)
    assert np.all(np.abs(np.asarray(log.residuals[: nit + 1]) - hist) <= 1e-10 * hist[0])
    assert rel_err(x, xo) <= 1e-10
