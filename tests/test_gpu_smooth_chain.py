"""GPU tests of the one-launch smoothing pass with a compile-time run count (sells_smooth_kernel<NS, TD, MK, 0, NR>, option
persist_regs): run offsets in scalar registers, gather indices formed once, every gather of a sweep in flight before the
first tap and -- one slice per wave -- the row's coefficients in registers.  The taps, their order and their roundings are those of the
runtime run count body, so everything here is compared bit for bit (np.testing.assert_array_equal) between three builds of one handle:

    persist_regs = 1   the new instantiation (default)
    persist_regs = 0   the runtime run count body
    persist = 0        per-sweep launches

with the battery of tests/test_gpu_xnext.py (run_all), and the default build against the CPU oracle with the gates of
tests/test_gpu_parity.py.  The text gmg_sweep_signature gives for a level whose passes are one launch names the instantiation that ran.

A run count other than 3 or 9 keeps the runtime run count body whatever persist_regs says: the 2-D Q2 generator gives such levels (25-point
rows in the K = 3 table), test_other_run_counts_keep_the_runtime_body."""
import numpy as np
import pytest

from conftest import rel_err
from test_gpu_xnext import jac, make_gmg, run_all, same, setup

pytestmark = pytest.mark.gpu

# shape, levels, signature of level 0's one-launch pass with persist_regs = 1
SHAPES = {
    "27pt": ((24, 24, 24), 3, "sells_smooth_kernel<NS=1,TD=1,MK=1,NR=9>"),     # 12 167 rows: one-wave workgroups, neighbours +-9, clamped first and last slices, ragged last slice
    "9pt": ((130, 66), 2, "sells_smooth_kernel<NS=1,TD=1,MK=1,NR=3>"),          # NR = 3
    "planes": ((64, 64, 6), 2, "sells_smooth_kernel<NS=1,TD=1,MK=1,NR=9>"),     # a plane of 3969 rows in a level of five: every workgroup is every other one's neighbour
    "two_slices": ((80, 80, 64), 4, "sells_smooth_kernel<NS=2,TD=1,MK=1,NR=9>"),  # 393 183 rows: two slices per wave, coefficients stay in LDS
    "9pt_two_slices": ((528, 512), 5, "sells_smooth_kernel<NS=2,TD=1,MK=1,NR=3>"),  # 269 297 rows of a 9-point operator: NR = 3 at two slices per wave
}

_PER_SWEEP = {}


def per_sweep(S, po, H, key, nc, niter, options):
    """The per-sweep reference of a case: computed once, shared, never written to."""
    if key not in _PER_SWEEP:
        _PER_SWEEP[key] = run_all(S, po, H, nc, niter, dict(options, persist=0))
    return _PER_SWEEP[key]


def three_builds(S, po, hierarchy, name, niter, options, sig=None):
    nc, nlev, sig1 = SHAPES[name]
    sig1 = sig or sig1
    H = hierarchy(nc, nlev)
    new = run_all(S, po, H, nc, niter, dict(options, persist_regs=1), signature=sig1)
    old = run_all(S, po, H, nc, niter, dict(options, persist_regs=0), signature=sig1[: sig1.index("NR=")] + "NR=0>")
    ref = per_sweep(S, po, H, (name, niter, tuple(sorted(options.items()))), nc, niter, options)
    same(new, old)
    same(new, ref)


@pytest.mark.parametrize("niter,close", [(10, 1), (10, 0), (3, 1), (3, 0), (2, 1), (2, 0)])
def test_27_point_one_slice_per_wave(S, po, hierarchy, niter, close):
    three_builds(S, po, hierarchy, "27pt", niter, {"pat_close": close})


@pytest.mark.parametrize("name", ["9pt", "planes", "two_slices", "9pt_two_slices"])
@pytest.mark.parametrize("niter,close", [(10, 1), (3, 0), (2, 1)])
def test_other_geometries(S, po, hierarchy, name, niter, close):
    three_builds(S, po, hierarchy, name, niter, {"pat_close": close})


@pytest.mark.parametrize("name,dinv,strict", [("27pt", 0, 1), ("27pt", 1, 0), ("27pt", 0, 0), ("9pt", 0, 0), ("9pt", 0, 1), ("9pt", 1, 0),
                                              ("two_slices", 0, 1), ("two_slices", 1, 0), ("9pt_two_slices", 0, 1), ("9pt_two_slices", 1, 0)])
def test_row_diagonal_and_unmasked_table(S, po, hierarchy, name, dinv, strict):
    """The kernel's TD (1/diag from the pattern table, pat_dinv) and MK (masked table entries, pat_strict) arguments, both values.  Two
    slices per wave of a 27-point operator without masks keep the runtime run count body (that instantiation would spill): NR=0."""
    sig = SHAPES[name][2].replace("TD=1", f"TD={dinv}").replace("MK=1", f"MK={strict}")
    if name == "two_slices" and not strict:
        sig = sig.replace("NR=9", "NR=0")
    three_builds(S, po, hierarchy, name, 3, {"pat_dinv": dinv, "pat_strict": strict}, sig=sig)


@pytest.mark.parametrize("regs", [1, 0])
def test_epochs_keep_advancing(S, po, hierarchy, regs):
    """25 preconditioner applications on one handle: no pass times out, the cycles repeat bit for bit."""
    nc, nlev, sig = SHAPES["27pt"]
    H = hierarchy(nc, nlev)
    n = H["mats"][0].shape[0]
    g = setup(S, make_gmg(S, H, options={"persist_regs": regs}), H["mats"][0])
    assert g.persist_retries() == dict(retries=0, persist_active=True)
    z, first = np.zeros(n), []
    for rep in range(25):
        S.solve_(z, g, np.random.default_rng(100 + rep % 3).uniform(-1, 1, n))
        if rep < 3:
            first.append(z.copy())
        else:
            np.testing.assert_array_equal(z, first[rep % 3], err_msg=f"cycle {rep} differs from its first run")
    assert g.persist_retries() == dict(retries=0, persist_active=True)
    assert (sig if regs else sig.replace("NR=9", "NR=0")) in g.sweep_signature(0), g.sweep_signature(0)
    g.close()


def test_a_one_launch_pass_of_two_sweeps_counts_as_fused(S, hierarchy):
    """gmg_get_kernel_stats counts the one-launch passes from the mark smooth_persistent leaves on the sample, not from the sample's
    weight: a pass of two sweeps (weight 2, or 1 when its last sweep is closed) is a one-launch pass like any longer one."""
    nc, nlev, _ = SHAPES["9pt"]
    H = hierarchy(nc, nlev)
    n = H["mats"][0].shape[0]
    g = setup(S, make_gmg(S, H, pre_smoothers=jac(S, nlev, 2), options={"prof_stride": 1}), H["mats"][0])
    g.profile(0, True)
    x, r = np.zeros(n), np.random.default_rng(50).uniform(-1, 1, n)
    g.smooth(0, x, r)
    st = g.kernel_stats()
    g.profile(0, False)
    assert "sells_smooth_kernel" in g.sweep_signature(0), g.sweep_signature(0)
    assert st["fused_passes"] > 0, st
    g.close()


@pytest.mark.parametrize("name", ["27pt", "9pt"])
def test_default_options_reproduce_the_oracle(S, po, orc, hierarchy, name):
    nc, nlev, sig = SHAPES[name]
    H = hierarchy(nc, nlev)
    A = H["mats"][0]
    b = po.dirichlet_lift_rhs(nc, 1)
    solver = S.CGSolver(make_gmg(S, H), maxiter=20, atol=1e-14, rtol=1e-6)
    ns = setup(S, solver, A)
    x = np.zeros_like(b)
    S.solve_(x, ns, b)
    assert sig in ns.P_ns.sweep_signature(0), ns.P_ns.sweep_signature(0)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    xo, nit, flag, hist = orc.cg_solve(A, b, Pl=go, maxiter=20, atol=1e-14, rtol=1e-6)
    assert solver.log.num_iters == nit and solver.log.flag == flag
    np.testing.assert_allclose(solver.log.residuals[: nit + 1], hist, rtol=1e-8)
    assert rel_err(x, xo) <= 1e-10
    ns.P_ns.close()



def test_other_run_counts_keep_the_runtime_body(S, po, hierarchy):
    """2-D Q2, 63^2 = 3969 rows: qualifies for the one-launch pass with a run count that is neither 3 nor 9 -- NR=0 with either value of
    persist_regs, and the same bits as the per-sweep launches."""
    nc, nlev = (32, 32), 3
    H = hierarchy(nc, nlev, 2)
    n = H["mats"][0].shape[0]
    res = []
    for options in ({"persist_regs": 1}, {"persist_regs": 0}, {"persist": 0}):
        g = setup(S, make_gmg(S, H, options=options), H["mats"][0])
        x, r = np.random.default_rng(3).uniform(-1, 1, n), np.random.default_rng(50).uniform(-1, 1, n)
        for _ in range(3):
            g.smooth(0, x, r)
        z = np.zeros(n)
        S.solve_(z, g, np.random.default_rng(100).uniform(-1, 1, n))
        if "persist" not in options:
            assert "sells_smooth_kernel<NS=1,TD=1,MK=1,NR=0>" in g.sweep_signature(0), g.sweep_signature(0)
        res.append([x, r, z])
        g.close()
    same(res[0], res[1])
    same(res[0], res[2])
