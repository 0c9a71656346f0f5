"""GPU tests at default options and full size against the sequential oracle and the exact references of tests/fullsize_reference.py:
a ragged, anisotropic Q1 problem whose levels land between the size gates of the big-level kernels (walk sweeps with a ragged last
chain, the pair sweep in its eight-wave shape, the 64-wide Gauss-Jordan coarse inverse with a ragged last panel), the dot at edge
lengths, and problem P-rand."""
import time

import numpy as np
import pytest

import fullsize_reference as fr
from conftest import rel_err
from fullsize_reference import RAGGED_NC, RAGGED_NLEV

pytestmark = pytest.mark.gpu
TOL_HIST = 1e-8


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


# the sweep kernel family the default options pick per level (include/gmg_amd.h gates; the bands are checked by
# tests/test_fullsize_reference.py::test_ragged_problem_lands_in_the_gate_bands): level 0, 1.1e7 rows >= pat_zwalk_rows (9e6) -> the
# walk; level 1, 1.35e6 rows < pat_tile_rows (3.5e6: the pair sweep's eight-wave form starts there) and above the one-launch pass
# (~5e5 rows) -> the pair sweep, four waves per workgroup; level 2 runs one-launch passes (no sweep signature)
RAGGED_FAMILIES = {0: "sells_zsweep_kernel", 1: ("sells_r2sweep_kernel<", "OCC=1")}


@pytest.mark.child_process
def test_ragged_anisotropic_fullsize_every_kernel_against_the_oracle(S, po, orc):
    """Q1 on (240, 232, 200) cells of the unit cube, 4 levels, default options: 239 x 231 x 199 nodes (three different stencil
    coefficients per axis, no axis a multiple of 64, 199 planes = 16 walk chains of 12 + a ragged chain of 7), levels between the
    gates, a 19 488-dof coarsest level inverted by the device 64-wide Gauss-Jordan (304 full panels + a ragged one of 32 columns).
    Every kernel of every level against the oracle and the exact row reference, the coarse inverse against the oracle's pivoted LU
    (random right-hand side and unit vectors inside the ragged last panel), the dot at the level-0 length, and CG + GMG against the
    sequential oracle: iterations, flag, history, solution."""
    import torch
    from gridapsolvers_jl_amd import abi
    t0 = time.time()
    H = po.build_hierarchy(RAGGED_NC, RAGGED_NLEV, 1)
    A = H["mats"][0]
    n = A.shape[0]
    assert n == 10986591
    b = po.dirichlet_lift_rhs(RAGGED_NC, 1)
    solver = S.CGSolver(make_gmg(S, H), maxiter=20, atol=1e-14, rtol=1e-8)
    ns = setup(S, solver, A)
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    torch.cuda.synchronize()
    S.solve_(xd, ns, bd)
    torch.cuda.synchronize()
    x = xd.cpu().numpy()
    del xd, bd
    g = ns.P_ns
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    report = fr.check_q1_levels(g, H, go, orc, RAGGED_FAMILIES, seed=240, post_levels=(0,))
    nL = H["mats"][-1].shape[0]
    for j in (nL - 1, nL - 17, nL - 32, nL - 33, 64 * 152):
        e = np.zeros(nL); e[j] = 1.0
        xc = np.zeros(nL)
        g.coarse_solve(e, xc)
        xo = go.coarse_solve(e)
        assert fr.max_rel(xc, xo) <= 1e-12, (j, fr.max_rel(xc, xo))
    report.append(f"dot n={n}: |d - exact| <= {fr.check_dot(g, n, 240):.3g} of the bound")
    t1 = time.time()
    xo, nit, flag, hist = orc.cg_solve(A, b, Pl=go, maxiter=20, atol=1e-14, rtol=1e-8)
    report.append(f"oracle CG + GMG: {time.time() - t1:.1f} s, {nit} iterations; whole test {time.time() - t0:.1f} s")
    assert (solver.log.num_iters, solver.log.flag) == (nit, flag) and flag == abi.CONVERGED_RTOL
    np.testing.assert_allclose(solver.log.residuals[: nit + 1], hist, rtol=TOL_HIST)
    assert rel_err(x, xo) <= 1e-10
    print("\n".join(["ragged (240, 232, 200):"] + report))
    g.close()


DOT_EDGE_N = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097, (1 << 20) + 3]


def test_dot_edge_lengths_against_the_exact_dot(S, po):
    """gmg_dot (dot_partial_kernel + reduce_final_kernel) on device vectors at lengths around the wave, the workgroup, the two-element
    vector loads and the grid size, on random data and with heavy cancellation (b = -a + 1e-12 noise), within the bound of its
    summation order (fullsize_reference.dot_depth).  The 288^3 length is checked inside test_weak_anchor_288cubed_properties."""
    H = po.build_hierarchy((8, 8, 8), 2, 1)
    ns = setup(S, make_gmg(S, H), H["mats"][0])
    worst = {n: fr.check_dot(ns, n, 1000 + n) for n in DOT_EDGE_N}
    print("dot |d - exact| / bound:", {n: f"{v:.3g}" for n, v in worst.items()})
    ns.close()


def test_dot_edge_lengths_unaligned_against_the_exact_dot(S, po):
    """The same on vectors 8 bytes off a 16-byte boundary (views buf[1 : n + 1] of device tensors; both operands, and a alone):
    dot_partial_kernel then takes its one-element path, whose order of summation differs -- the bound is
    fullsize_reference.dot_depth(n, vec=False), which tests/test_fullsize_reference.py checks against an emulation of that order.
    Also at 131074 (the first length with 257 partials) and 524289 (the odd length after which the grid stops growing)."""
    H = po.build_hierarchy((8, 8, 8), 2, 1)
    ns = setup(S, make_gmg(S, H), H["mats"][0])
    for offset in ((1, 1), (1, 0)):
        worst = {n: fr.check_dot(ns, n, 2000 + n, offset=offset) for n in DOT_EDGE_N + [131074, 524289]}
        print("dot, offsets %s: |d - exact| / bound:" % (offset,), {n: f"{v:.3g}" for n, v in worst.items()})
    ns.close()


def test_prand_64cubed_cg_gmg_against_the_oracle(S, po, orc):
    """Problem P-rand (b ~ U(-1,1), po.random_rhs) on Q1 64^3, 4 levels, CG + GMG to rtol 1e-8: the oracle's iteration count and
    flag, its residual history within TOL_HIST, its solution within 1e-10."""
    nc, nlev = (64, 64, 64), 4
    H = po.build_hierarchy(nc, nlev, 1)
    A = H["mats"][0]
    b = po.random_rhs(A.shape[0])
    solver = S.CGSolver(make_gmg(S, H), maxiter=60, atol=1e-14, rtol=1e-8)
    ns = setup(S, solver, A)
    x = np.zeros_like(b)
    S.solve_(x, ns, b)
    go = orc.GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=1)
    xo, nit, flag, hist = orc.cg_solve(A, b, Pl=go, maxiter=60, atol=1e-14, rtol=1e-8)
    assert (solver.log.num_iters, solver.log.flag) == (nit, flag) and nit < 60
    np.testing.assert_allclose(solver.log.residuals[: nit + 1], hist, rtol=TOL_HIST)
    assert rel_err(x, xo) <= 1e-10
