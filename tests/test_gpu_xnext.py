"""GPU tests of the three schedule options that remove work the result does not need:

  pat_xnext  per-sweep passes of an even number of r-gather sweeps add s_k and s_{k+1} to x in sweeps 0, 2, ... -- s_{k+1} from the
             r_{k+1} the sweep holds in registers -- instead of s_{k-1} and s_k in sweeps 1, 3, ... (which re-read r_{k-1});
  pat_close  a post-smoothing pass whose residual nobody reads does not run its last sweep;
  cg_split   CG's x += alpha p runs behind the launch that posts the residual norm.

None of them may change a rounding: everything here is compared bit for bit (np.testing.assert_array_equal) with the same handle
built with the three options off, and the default build against the CPU oracle with the gates of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

OFF = {"pat_xnext": 0, "pat_close": 0, "cg_split": 0}
ON = {"pat_xnext": 1, "pat_close": 1, "cg_split": 1}      # (cg_split is off by default: measured equal)


def jac(S, nlev, niter=10, omega=2.0 / 3.0):
    return [S.RichardsonSmoother(S.JacobiLinearSolver(), niter, omega)] * (nlev - 1)


def make_gmg(S, H, **kw):
    nlev = len(H["mats"])
    kw.setdefault("pre_smoothers", jac(S, nlev))
    kw.setdefault("post_smoothers", kw["pre_smoothers"])
    kw.setdefault("maxiter", 1)
    return S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], **kw)


def setup(S, solver, A):
    return S.numerical_setup(S.symbolic_setup(solver, A), A)


def run_all(S, po, H, nc, niter, options, cycle="v_cycle", signature=None):
    """Everything the options could touch, on one set of handles: smoothing passes of level 0 (x and r returned: r is live there), an
    Inf / -Inf in the residual, V-cycles as a preconditioner, a CG solve from a random guess, a verbose preconditioner under CG and a
    GMG in solver mode (r live in both).  Returns the list of arrays to compare."""
    nlev = len(H["mats"])
    A = H["mats"][0]
    n = A.shape[0]
    b = po.dirichlet_lift_rhs(nc, 1)
    sm = jac(S, nlev, niter)
    out = []
    solver = S.CGSolver(make_gmg(S, H, pre_smoothers=sm, cycle_type=cycle, options=options), maxiter=30, atol=1e-14, rtol=1e-8)
    ns = setup(S, solver, A)
    g = ns.P_ns
    x, r = np.random.default_rng(3).uniform(-1, 1, n), np.random.default_rng(50).uniform(-1, 1, n)
    for _ in range(3):                                             # chained: the pass starts from either residual buffer
        g.smooth(0, x, r)
    out += [x.copy(), r.copy()]
    x, r = np.zeros(n), np.random.default_rng(51).uniform(-1, 1, n)
    for _ in range(3):
        g.smooth(0, x, r)
    out += [x.copy(), r.copy()]
    xi, ri = np.zeros(n), np.random.default_rng(52).uniform(-1, 1, n)
    ri[n // 3], ri[5] = np.inf, -np.inf
    g.smooth(0, xi, ri)
    out += [np.isfinite(xi), np.isfinite(ri), np.where(np.isfinite(xi), xi, 0.0), np.where(np.isfinite(ri), ri, 0.0)]
    if signature is not None:
        assert signature in g.sweep_signature(0), g.sweep_signature(0)
    z = np.zeros(n)
    S.solve_(z, g, np.random.default_rng(100).uniform(-1, 1, n))   # one cycle as a preconditioner: z = 0 on entry
    out.append(z.copy())
    xs = np.random.default_rng(7).uniform(-1, 1, n)
    S.solve_(xs, ns, b)
    out += [xs.copy(), solver.log.residuals[: solver.log.num_iters + 1].copy()]
    g.close()
    # r is NOT dead: the verbose preconditioner takes the post-cycle norm, the solver-mode GMG the norm of every cycle
    gv = make_gmg(S, H, pre_smoothers=sm, cycle_type=cycle, options=options, verbose=1)
    sv = S.CGSolver(gv, maxiter=4, atol=1e-14, rtol=1e-8)
    nv = setup(S, sv, A)
    xv = np.zeros(n)
    S.solve_(xv, nv, b)
    out += [xv.copy(), np.array(gv.log.residuals[:2]), sv.log.residuals[: sv.log.num_iters + 1].copy()]
    assert np.all(np.isfinite(gv.log.residuals[:2]))
    nv.P_ns.close()
    gs = make_gmg(S, H, pre_smoothers=sm, cycle_type=cycle, options=options, mode="solver", maxiter=3, rtol=1e-30)
    nss = setup(S, gs, A)
    xg = np.random.default_rng(8).uniform(-1, 1, n)
    S.solve_(xg, nss, b)
    assert gs.log.num_iters == 3
    out += [xg.copy(), gs.log.residuals[:4].copy()]
    nss.close()
    return out


def same(a, b):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(u, v, err_msg=f"item {i}")


# ---------------------------------------------------------------- per-sweep launches (persist = 0)
@pytest.mark.parametrize("nc,nlev,niter", [
    ((40, 40, 40), 3, 10),      # 59 319 rows: ragged last 126-row slice, clamped first and last slices
    ((130, 66), 2, 4),          # 9-point operator: NR = 3
    ((34, 46, 30), 2, 3),       # odd number of sweeps: the old schedule, must still agree
    ((24, 24, 24), 3, 2),       # with r dead the pass is ONE launch
    ((24, 24, 24), 3, 1),       # single-sweep pass
])
def test_per_sweep_schedule_is_bitwise_the_old_one(S, po, hierarchy, nc, nlev, niter):
    H = hierarchy(nc, nlev)
    new = run_all(S, po, H, nc, niter, dict(ON, persist=0), signature="sells_r2sweep_kernel")
    old = run_all(S, po, H, nc, niter, dict(OFF, persist=0))
    same(new, old)


@pytest.mark.parametrize("name,opts,sig", [
    ("zwalk", {"pat_zwalk": 2}, "sells_zsweep_kernel"),
    ("occ0", {"pat_r2_occ": 0}, "OCC=0"),
    ("occ1", {"pat_r2_occ": 1}, "OCC=1"),
    ("occ2", {"pat_r2_occ": 2, "pat_tile_rows": 1000}, "OCC=2"),
    ("fma", {"pat_fma": 1}, "FM=1"),
])
def test_every_kernel_with_the_new_mode_is_bitwise_the_old_schedule(S, po, hierarchy, name, opts, sig):
    """sells_zsweep_kernel and the three forms of sells_r2sweep_kernel (105 registers, 64 registers, eight-wave workgroups), and the
    fused multiply-add taps (compared with pat_fma = 1 and the new options off: FMA taps are not the default's bits)."""
    nc, nlev, niter = (40, 40, 40), 3, 10
    H = hierarchy(nc, nlev)
    new = run_all(S, po, H, nc, niter, dict(ON, persist=0, **opts), signature=sig)
    old = run_all(S, po, H, nc, niter, dict(OFF, persist=0, **opts), signature=sig)
    same(new, old)


# ---------------------------------------------------------------- one-launch passes (default persist)
@pytest.mark.parametrize("cycle", ["v_cycle", "w_cycle", "f_cycle"])
@pytest.mark.parametrize("niter", [10, 3, 2, 1])
def test_closed_one_launch_pass_is_bitwise_the_full_one(S, po, hierarchy, cycle, niter):
    """sells_smooth_kernel with `close`: niter - 1 sweeps, x += s_{niter-1} from registers, no r store.  25 cycles on one handle (the
    epochs advance by niter although a closed pass publishes one value fewer) and a CG solve (level 0 closes too) against pat_close = 0."""
    nc, nlev = (24, 24, 24), 3
    H = hierarchy(nc, nlev)
    A = H["mats"][0]
    n = A.shape[0]
    b = po.dirichlet_lift_rhs(nc, 1)
    res = []
    for options in (ON, dict(ON, pat_close=0)):
        solver = S.CGSolver(make_gmg(S, H, pre_smoothers=jac(S, nlev, niter), cycle_type=cycle, options=options), maxiter=30, atol=1e-14, rtol=1e-8)
        ns = setup(S, solver, A)
        assert ns.P_ns.persist_retries() == dict(retries=0, persist_active=True)
        out = []
        z = np.zeros(n)
        for rep in range(25):
            S.solve_(z, ns.P_ns, np.random.default_rng(100 + rep % 3).uniform(-1, 1, n))
            if rep < 3:
                out.append(z.copy())
            else:
                np.testing.assert_array_equal(z, out[rep % 3], err_msg=f"cycle {rep} differs from its first run ({options})")
        x = np.random.default_rng(7).uniform(-1, 1, n)
        S.solve_(x, ns, b)
        out += [x.copy(), solver.log.residuals[: solver.log.num_iters + 1].copy()]
        assert ns.P_ns.persist_retries() == dict(retries=0, persist_active=True)
        ns.P_ns.close()
        res.append(out)
    same(res[0], res[1])


# ---------------------------------------------------------------- the sweep is really gone
@pytest.mark.parametrize("close,total", [(1, 19), (0, 20)])
def test_the_dead_sweep_is_not_launched(S, po, hierarchy, close, total):
    """One preconditioner application inside CG (the path on which level 0's post-cycle residual is not read), every level-0 sweep
    launch bracketed: 10 pre + 9 post sweeps, the x-updating form first in every pair -- so one x-untouched launch fewer than
    x-updating ones, none of them after the last x-updating one.  With pat_close = 0: 10 + 10."""
    nc, nlev = (40, 40, 40), 3
    H = hierarchy(nc, nlev)
    A = H["mats"][0]
    b = po.dirichlet_lift_rhs(nc, 1)
    solver = S.CGSolver(make_gmg(S, H, options={"persist": 0, "prof_stride": 1, "pat_close": close}), maxiter=1, atol=1e-14, rtol=1e-8)
    ns = setup(S, solver, A)
    ns.P_ns.profile(0, True)
    S.solve_(np.zeros_like(b), ns, b)
    st = ns.P_ns.kernel_stats()
    ns.P_ns.profile(0, False)
    bv = st["by_variant"]
    assert st["launches"] == total, st
    assert "x_every_sweep" not in bv
    assert bv["x_two_increments"]["launches"] == 10 and bv["x_untouched"]["launches"] == total - 10, bv
    # bytes per launch without the r_{k-1} term: r in + r out (+ x in + x out), 2 B of pattern id per row
    n = A.shape[0]
    assert bv["x_untouched"]["layout_bytes"] == 18.0 * n and bv["x_two_increments"]["layout_bytes"] == 34.0 * n
    ns.P_ns.close()


# ---------------------------------------------------------------- CG's update in two launches
@pytest.mark.parametrize("nc,nlev", [((6, 6), 2), ((40, 40, 40), 3)])
def test_split_cg_update_is_bitwise_the_single_kernel(S, po, hierarchy, nc, nlev):
    """n = 49 (odd, below one reduction block) and n = 59 319 (odd, many blocks); persist = 0 and device vectors: nothing but the end
    of cg_core stands between the last x += alpha p and the caller's read."""
    import torch
    H = hierarchy(nc, nlev)
    A = H["mats"][0]
    n = A.shape[0]
    assert n % 2 == 1
    b = po.dirichlet_lift_rhs(nc, 1)
    bd = torch.from_numpy(b).cuda()
    x0 = np.random.default_rng(7).uniform(-1, 1, n)
    res = []
    for split in (1, 0):
        solver = S.CGSolver(make_gmg(S, H, options={"persist": 0, "cg_split": split}), maxiter=30, atol=1e-14, rtol=1e-8)
        ns = setup(S, solver, A)
        xd = torch.from_numpy(x0).cuda()
        torch.cuda.synchronize()
        S.solve_(xd, ns, bd)
        xh = xd.cpu().numpy()
        res.append([xh, solver.log.residuals[: solver.log.num_iters + 1].copy()])
        ns.P_ns.close()
    same(res[0], res[1])


# ---------------------------------------------------------------- the default build against the CPU oracle
@pytest.mark.parametrize("nc,nlev,persist", [((24, 24, 24), 3, 1), ((40, 40, 40), 3, 0)])
def test_default_options_reproduce_the_oracle(S, po, orc, hierarchy, nc, nlev, persist):
    H = hierarchy(nc, nlev)
    A = H["mats"][0]
    b = po.dirichlet_lift_rhs(nc, 1)
    solver = S.CGSolver(make_gmg(S, H, options={"persist": persist}), maxiter=20, atol=1e-14, rtol=1e-6)
    ns = setup(S, solver, A)
    x = np.zeros_like(b)
    S.solve_(x, ns, b)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    xo, nit, flag, hist = orc.cg_solve(A, b, Pl=go, maxiter=20, atol=1e-14, rtol=1e-6)
    assert solver.log.num_iters == nit
    np.testing.assert_allclose(solver.log.residuals[: nit + 1], hist, rtol=1e-8)
    assert rel_err(x, xo) <= 1e-10
    ns.P_ns.close()
