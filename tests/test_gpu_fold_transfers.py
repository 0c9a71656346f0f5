"""GPU tests of the transfers that run as the head of a one-launch smoothing pass (option persist_fold):

  bit 1  the restriction  rH = R rh  is the head of the coarse level's pre-smoothing pass (r and s_0 formed per owned row);
  bit 2  dxh = P dxH ; xh += dxh ; rh -= Ah dxh  is one more step in front of the sweeps of the post-smoothing pass;
  bit 4  bit 1 also where the finer level is no one-launch level itself.

No fold adds arithmetic or changes a rounding: everything is compared bit for bit (np.testing.assert_array_equal) between the default
value of persist_fold, persist_fold = 0 (the separate transfer kernels) and persist = 0 (per-sweep launches) on the same hierarchy, and
gmg_sweep_signature says which folds ran on a level (`folds=R+P`, `folds=R`, `folds=P`, `folds=none` behind the one-launch pass)."""
import numpy as np
import pytest

from conftest import rel_err
from test_gpu_xnext import jac, make_gmg, run_all, same, setup

pytestmark = pytest.mark.gpu

DEFAULT_FOLD = 7     # the library's default persist_fold

# shape -> (levels, extra options, {level: folds with every bit of persist_fold set})
SHAPES = {
    "27pt": ((24, 24, 24), 3, {}, {0: "P", 1: "R+P"}),          # one-wave workgroups, ragged last slice, clamped first and last slices, neighbours +-9
    "headline": ((40, 40, 40), 4, {"persist_max_slices": 400}, {1: "R+P", 2: "R+P"}),   # level 0 per-sweep (sells_r2sweep_kernel), levels 1 and 2 one launch: bit 4
    "9pt": ((130, 66), 2, {}, {0: "P"}),                         # 9-point rows, NR = 3 (130 cells halve once: two levels, prolongation fold only)
    "9pt_3lev": ((132, 68), 3, {}, {0: "P", 1: "R+P"}),          # ... and with a restriction fold: 131 x 67 and 65 x 33 rows
    "planes": ((64, 64, 6), 2, {}, {0: "P"}),                    # every workgroup is every other one's neighbour; prolongation fold only
    "two_slices": ((80, 80, 64), 4, {}, {0: "P", 1: "R+P", 2: "R+P"}),   # two slices per wave
    "unequal": ((34, 46, 30), 2, {}, {0: "P"}),                  # unequal extents
}

_REF = {}


def folds_for(name, mask):
    """What gmg_sweep_signature reports per level for a value of persist_fold: R needs bit 1 -- and bit 4 where the finer level is no
    one-launch level (the first level of SHAPES[name][3] that is not level 0) --, P needs bit 2."""
    full = SHAPES[name][3]
    first = min(full)
    out = {}
    for lev, f in full.items():
        got = [c for c in f.split("+") if (c == "R" and mask & 1 and (lev - 1 >= first or mask & 4)) or (c == "P" and mask & 2)]
        if got:
            out[lev] = "+".join(got)
    return out


def check_folds(g, want):
    for lev, folds in want.items():
        sig = g.sweep_signature(lev)
        assert "sells_smooth_kernel" in sig and sig.endswith("folds=" + folds), (lev, sig)


def run_case(S, po, hierarchy, name, niter, options, cycle="v_cycle", want=None):
    """run_all with the default persist_fold, with persist_fold = 0 and (once per case, shared) with persist = 0: the same bits."""
    nc, nlev, extra, folds = SHAPES[name]
    H = hierarchy(nc, nlev)
    options = dict(extra, **options)
    want = folds_for(name, options.get("persist_fold", DEFAULT_FOLD)) if want is None else want

    def grab(g_options):
        # the folds of every level after a V-cycle and a CG solve on a fresh handle of the same options
        g = setup(S, make_gmg(S, H, pre_smoothers=jac(S, nlev, niter), cycle_type=cycle, options=g_options), H["mats"][0])
        n = H["mats"][0].shape[0]
        S.solve_(np.zeros(n), g, np.random.default_rng(100).uniform(-1, 1, n))
        out = {lev: g.sweep_signature(lev) for lev in range(nlev - 1)}
        g.close()
        return out

    new = run_all(S, po, H, nc, niter, options, cycle=cycle)
    old = run_all(S, po, H, nc, niter, dict(options, persist_fold=0), cycle=cycle)
    key = (name, niter, cycle, tuple(sorted(options.items())))
    if key not in _REF:
        _REF[key] = run_all(S, po, H, nc, niter, dict(options, persist=0), cycle=cycle)
    same(new, old)
    same(new, _REF[key])
    on, off = grab(options), grab(dict(options, persist_fold=0))
    for lev in range(nlev - 1):
        if "sells_smooth_kernel" in off[lev]:
            assert off[lev].endswith("folds=none"), (lev, off[lev])
        if lev in want:
            assert "sells_smooth_kernel" in on[lev] and on[lev].endswith("folds=" + want[lev]), (lev, on[lev])
        else:
            assert "folds=R" not in on[lev] and "folds=P" not in on[lev], (lev, on[lev])


@pytest.mark.parametrize("name", ["27pt", "9pt", "9pt_3lev", "planes", "two_slices", "unequal"])
def test_folds_are_bitwise_the_separate_kernels(S, po, hierarchy, name):
    run_case(S, po, hierarchy, name, 10, {})


@pytest.mark.parametrize("mask,want", [(7, {1: "R+P", 2: "R+P"}), (3, {1: "P", 2: "R+P"}), (1, {2: "R"}), (2, {1: "P", 2: "P"}), (5, {1: "R", 2: "R"})])
def test_every_bit_on_the_headline_arrangement(S, po, hierarchy, mask, want):
    """Level 0 sweeps launch by launch, levels 1 and 2 run as one launch: the restriction 0 -> 1 folds only with bit 4."""
    assert folds_for("headline", mask) == want
    run_case(S, po, hierarchy, "headline", 10, {"persist_fold": mask}, want=want)


def test_default_mask_on_the_headline_arrangement(S, po, hierarchy):
    run_case(S, po, hierarchy, "headline", 3, {})


@pytest.mark.parametrize("close", [1, 0])
@pytest.mark.parametrize("niter", [10, 3, 2, 1])
def test_sweep_counts_and_closed_passes(S, po, hierarchy, niter, close):
    """niter = 1 is no one-launch pass: the separate kernels run and no fold is reported."""
    run_case(S, po, hierarchy, "27pt", niter, {"pat_close": close}, want=None if niter > 1 else {})


@pytest.mark.parametrize("cycle", ["w_cycle", "f_cycle"])
@pytest.mark.parametrize("niter", [3, 2])
def test_w_and_f_cycles(S, po, hierarchy, cycle, niter):
    """The re-smooth takes the fold of the first correction and keeps its residual live (a restriction follows)."""
    run_case(S, po, hierarchy, "27pt", niter, {}, cycle=cycle)


@pytest.mark.parametrize("options", [{"pat_dinv": 0}, {"pat_strict": 0}, {"persist_regs": 0}, {"persist_fenced": 1}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_kernel_arguments(S, po, hierarchy, options):
    run_case(S, po, hierarchy, "27pt", 3, options)


def test_two_slices_without_masks(S, po, hierarchy):
    run_case(S, po, hierarchy, "two_slices", 3, {"pat_strict": 0})


@pytest.mark.parametrize("name", ["27pt", "headline"])
def test_non_finite_residual(S, po, hierarchy, name):
    """+Inf and -Inf in the input residual of one preconditioner cycle: the same entries are finite, with the same values, with and
    without the folds -- the padded-entry rule of both prologues and the strict-mask rule of r -= A dx."""
    nc, nlev, extra, folds = SHAPES[name]
    H = hierarchy(nc, nlev)
    n = H["mats"][0].shape[0]
    r = np.random.default_rng(52).uniform(-1, 1, n)
    r[n // 3], r[5], r[n - 7] = np.inf, -np.inf, np.inf
    res = []
    for options in (dict(extra, persist_fold=7), dict(extra, persist_fold=0), dict(extra, persist=0)):
        g = setup(S, make_gmg(S, H, options=options), H["mats"][0])
        z = np.zeros(n)
        S.solve_(z, g, r.copy())
        res.append([np.isfinite(z), np.where(np.isfinite(z), z, 0.0)])
        g.close()
    assert not res[0][0].all()
    same(res[0], res[1])
    same(res[0], res[2])


@pytest.mark.parametrize("name", ["27pt", "headline"])
def test_epochs_keep_advancing(S, po, hierarchy, name):
    """25 preconditioner applications on one handle, gmg_smooth calls (no fold: niter publications) on the same progress words in
    between: every cycle repeats its first run, no pass times out."""
    nc, nlev, extra, folds = SHAPES[name]
    H = hierarchy(nc, nlev)
    n = H["mats"][0].shape[0]
    n1 = H["mats"][1].shape[0]
    g = setup(S, make_gmg(S, H, options=dict(extra, persist_fold=7)), H["mats"][0])
    assert g.persist_retries() == dict(retries=0, persist_active=True)
    z, first, firsts = np.zeros(n), [], []
    for rep in range(25):
        S.solve_(z, g, np.random.default_rng(100 + rep % 3).uniform(-1, 1, n))
        xs, rs = np.random.default_rng(7).uniform(-1, 1, n1), np.random.default_rng(8).uniform(-1, 1, n1)
        g.smooth(1, xs, rs)
        if rep < 3:
            first.append(z.copy())
            firsts.append((xs, rs))
        else:
            np.testing.assert_array_equal(z, first[rep % 3], err_msg=f"cycle {rep} differs from its first run")
            np.testing.assert_array_equal(xs, firsts[0][0])
            np.testing.assert_array_equal(rs, firsts[0][1])
    assert g.persist_retries() == dict(retries=0, persist_active=True)
    check_folds(g, {1: "R+P"})
    g.close()


def test_forced_timeout_reruns_the_solve_with_the_separate_kernels(S, po, hierarchy):
    nc, nlev, extra, folds = SHAPES["27pt"]
    H = hierarchy(nc, nlev)
    A = H["mats"][0]
    b = po.dirichlet_lift_rhs(nc, 1)
    res = []
    for options, force in (({}, 1), ({"persist": 0}, 0)):
        solver = S.CGSolver(make_gmg(S, H, options=options), maxiter=30, atol=1e-14, rtol=1e-8)
        ns = setup(S, solver, A)
        if force:
            ns.P_ns.set_option("persist_force_timeout", 1)
        x = np.random.default_rng(7).uniform(-1, 1, b.size)
        S.solve_(x, ns, b)
        if force:
            assert ns.P_ns.persist_retries() == dict(retries=1, persist_active=False)
        res.append([x, solver.log.residuals[: solver.log.num_iters + 1].copy()])
        ns.P_ns.close()
    same(res[0], res[1])


@pytest.mark.parametrize("name", ["27pt", "9pt", "9pt_3lev"])
def test_default_options_reproduce_the_oracle(S, po, orc, hierarchy, name):
    nc, nlev, extra, folds = SHAPES[name]
    H = hierarchy(nc, nlev)
    A = H["mats"][0]
    b = po.dirichlet_lift_rhs(nc, 1)
    solver = S.CGSolver(make_gmg(S, H), maxiter=20, atol=1e-14, rtol=1e-6)
    ns = setup(S, solver, A)
    x = np.zeros_like(b)
    S.solve_(x, ns, b)
    check_folds(ns.P_ns, folds_for(name, DEFAULT_FOLD))
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    xo, nit, flag, hist = orc.cg_solve(A, b, Pl=go, maxiter=20, atol=1e-14, rtol=1e-6)
    assert solver.log.num_iters == nit
    np.testing.assert_allclose(solver.log.residuals[: nit + 1], hist, rtol=1e-8)
    assert rel_err(x, xo) <= 1e-10
    ns.P_ns.close()


def test_q2_runtime_run_count_and_wide_tables(S, po, hierarchy):
    """2-D Q2, 63^2 rows on level 0 and 31^2 on level 1: the runtime run count body (25-point rows), transfer tables with wide rows.
    Whether a fold applies is the launcher's answer (tables in the LDS form that fit next to the pass's own); the signature reports
    it and the bits agree either way."""
    nc, nlev = (32, 32), 3
    H = hierarchy(nc, nlev, 2)
    n = H["mats"][0].shape[0]
    res = []
    for options in ({}, {"persist_fold": 0}, {"persist": 0}):
        g = setup(S, make_gmg(S, H, pre_smoothers=jac(S, nlev, 3), options=options), H["mats"][0])
        out = []
        for rep in range(3):
            z = np.zeros(n)
            S.solve_(z, g, np.random.default_rng(100 + rep).uniform(-1, 1, n))
            out.append(z)
        if "persist" not in options:
            for lev in (0, 1):
                sig = g.sweep_signature(lev)
                assert "NR=0>" in sig and "folds=" in sig, sig
                if options:
                    assert sig.endswith("folds=none"), sig
        res.append(out)
        g.close()
    same(res[0], res[1])
    same(res[0], res[2])
