"""GPU tests of the launchers' option -> template argument dispatch (csrc/dispatch.hpp: with_value, with_bool, with_bools).

Every kernel family that takes the x-update mode XM, the masked / unmasked table MK, the fused multiply-add taps FM or the 1/diag
source TD as template arguments is launched with each value of the options behind them.  Two constants passed in the wrong order
reach a kernel that exists and runs, so the results are what is compared:

  (a) pat_strict = 0 and 1 (MK) give the same bits at equal pat_fma, and pat_dinv = 0 and 1 (TD) the same bits where a form takes it;
  (b) with pat_fma = 0 the result is bit for bit the per-sweep reference (default options, persist = 0: what tests/test_gpu_xnext.py
      and tests/test_gpu_smooth_chain.py compare with) -- a wrong XM is another x or another r; with pat_fma = 1 it is inside the
      per-kernel parity gate (tests/test_gpu_parity.py: TOL_KERNEL) and NOT the reference's bits (FM really arrived);
  (c) the level's sweep signature names the kernel family and the MK / FM / TD values.

A pass of four sweeps (pre slot) and one of three (post slot) per handle: x modes 1 and 3 where the form has mode 3 (z-walk, pair
sweep), 1 and 2 elsewhere, and 1, 2, 0 in the odd pass.

Operators: the 27-point one of hierarchy((24, 24, 24), 3) (12 167 rows: 97 slices of 126 rows, the last one ragged) and the 9-point
one of hierarchy((130, 66), 2) (NR = 3).  Pairs that do not exist: the z-walk needs nine runs (3 x 3 offsets a plane
apart), so the 9-point operator does not have it, nor the eight-wave pair mat-vec.  The mat-vec kernels leave no signature: (c) is for the
sweeps.  sells_sweep_kernel (the form that takes TD) has no FM argument: pat_fma = 0 only."""
import numpy as np
import pytest

from conftest import max_rel
from test_gpu_parity import TOL_KERNEL
from test_gpu_xnext import jac, make_gmg, setup

pytestmark = pytest.mark.gpu

SHAPES = {"27pt": ((24, 24, 24), 3), "9pt": ((130, 66), 2)}

# r-gather sweep forms of level 0: options that force them, the family the signature names
SWEEP_FORMS = {
    "zwalk": ({"pat_zwalk": 2}, "sells_zsweep_kernel"),
    "pair": ({"pat_zwalk": 0}, "sells_r2sweep_kernel"),
    "row": ({"pat_r2": 0}, "sells_rsweep_kernel"),
}
SWEEP_CASES = [("27pt", f) for f in SWEEP_FORMS] + [("9pt", f) for f in ("pair", "row")]

MV_FORMS = {
    "r2mv": {"pat_zwalk": 0, "pat_r2mv_min": 1, "pat_r2mv_dot": 0},
    "r2mv_occ2": {"pat_zwalk": 0, "pat_tile_rows": 0, "pat_r2mv_min": 1, "pat_r2mv_dot": 0},
    "zwalk": {"pat_zwalk": 2, "pat_r2mv_min": 1, "pat_r2mv_dot": 0},
}
MV_CASES = [("27pt", f) for f in MV_FORMS] + [("9pt", "r2mv")]

_REF = {}


def passes(S, H, options):
    """Level 0 of one handle: the four-sweep pass from a given x, twice (chained: either residual buffer), and from x = 0, then the
    three-sweep pass.  Returns the arrays and the signature the last pass left."""
    nlev = len(H["mats"])
    n = H["mats"][0].shape[0]
    from gridapsolvers_jl_amd.abi import POST, PRE
    g = setup(S, make_gmg(S, H, pre_smoothers=jac(S, nlev, 4), post_smoothers=jac(S, nlev, 3), options=dict(options, persist=0)), H["mats"][0])
    out = []
    for which in (PRE, POST):
        x, r = np.random.default_rng(3).uniform(-1, 1, n), np.random.default_rng(50).uniform(-1, 1, n)
        for _ in range(2):
            g.smooth(0, x, r, which)
        out += [x, r]
        x, r = np.zeros(n), np.random.default_rng(51).uniform(-1, 1, n)
        g.smooth(0, x, r, which)
        out += [x, r]
    sig = g.sweep_signature(0)
    g.close()
    return out, sig


def reference(S, hierarchy, shape):
    """The per-sweep reference of a shape: computed once, shared, never written to."""
    if shape not in _REF:
        _REF[shape] = passes(S, hierarchy(*SHAPES[shape]), {})[0]
    return _REF[shape]


def check(out, ref, fma, what):
    """(b): the reference's bits without FMA taps, inside the gate -- and not the same bits -- with them"""
    assert len(out) == len(ref)
    for i, (u, v) in enumerate(zip(out, ref)):
        print(f"{what} item {i}: max_rel = {max_rel(u, v):.3e}")
        if fma:
            assert max_rel(u, v) <= TOL_KERNEL, (what, i)
        else:
            np.testing.assert_array_equal(u, v, err_msg=f"{what} item {i}")
    if fma:
        assert not all(np.array_equal(u, v) for u, v in zip(out, ref)), what


@pytest.mark.parametrize("shape,form", SWEEP_CASES)
def test_gather_sweep_forms_take_their_options(S, hierarchy, shape, form):
    H = hierarchy(*SHAPES[shape])
    ref = reference(S, hierarchy, shape)
    opts, family = SWEEP_FORMS[form]
    res = {}
    for strict in (0, 1):
        for fma in (0, 1):
            out, sig = passes(S, H, dict(opts, pat_strict=strict, pat_fma=fma))
            assert family in sig and f"MK={strict}" in sig and f"FM={fma}" in sig, sig      # (c)
            check(out, ref, fma, f"{shape} {form} strict={strict} fma={fma}")                # (b)
            res[strict, fma] = out
    for fma in (0, 1):                                                                     # (a)
        for i, (u, v) in enumerate(zip(res[0, fma], res[1, fma])):
            np.testing.assert_array_equal(u, v, err_msg=f"pat_strict 0 / 1 differ at pat_fma={fma}, item {i}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_gather_sweep_takes_the_diagonal_and_the_table(S, hierarchy, shape):
    """sells_sweep_kernel<XM, NB, TD, MK> (pat_rsweep = 0): 1/diag from the pattern table or from the vector, masked or unmasked table."""
    H = hierarchy(*SHAPES[shape])
    ref = reference(S, hierarchy, shape)
    for dinv in (0, 1):
        for strict in (0, 1):
            out, sig = passes(S, H, {"pat_rsweep": 0, "pat_dinv": dinv, "pat_strict": strict})
            assert "sells_sweep_kernel" in sig and f"TD={dinv}" in sig and f"MK={strict}" in sig, sig
            check(out, ref, 0, f"{shape} one-gather dinv={dinv} strict={strict}")          # (a) and (b): all four are the reference's bits


@pytest.mark.parametrize("shape,form", MV_CASES)
def test_matvec_forms_take_their_options(S, orc, hierarchy, shape, form):
    """y = A x of level 0 through sells_r2mv_kernel (four- and eight-wave workgroups) and sells_zsweep_kernel<1, MK, FM, EPI_SET>
    against the oracle's mul! (rows summed in CSR order: the same bits without FMA taps)."""
    from gridapsolvers_jl_amd.abi import OP_A
    H = hierarchy(*SHAPES[shape])
    A = H["mats"][0]
    n = A.shape[0]
    v = np.random.default_rng(9).uniform(-1, 1, n)
    ref = [orc.spmv(A, v)]
    res = {}
    for strict in (0, 1):
        for fma in (0, 1):
            g = setup(S, make_gmg(S, H, options=dict(MV_FORMS[form], pat_strict=strict, pat_fma=fma, persist=0)), A)
            y = np.zeros(n)
            g.op_apply(0, OP_A, v, y)
            g.close()
            check([y], ref, fma, f"{shape} mat-vec {form} strict={strict} fma={fma}")
            res[strict, fma] = y
    for fma in (0, 1):
        np.testing.assert_array_equal(res[0, fma], res[1, fma], err_msg=f"pat_strict 0 / 1 differ at pat_fma={fma}")
