"""Host tests of numerical_setup! for block solvers (no GPU): the mirror's NonlinearSystemBlock, the x argument of
numerical_setup_, the four C entry points as the binding declares them, and the problem builders of the device tests
(tests/block_refresh_problems.py): every pair has identical ptr / idx and different values."""
import os
import re

import numpy as np
import pytest

import block_refresh_problems as bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nonlinear_system_block_is_a_system_block(S, po):
    """BlockSolverInterfaces.jl:206-214: NonlinearSystemBlock(ids); accepted wherever LinearSystemBlock is."""
    assert "NonlinearSystemBlock" in S.__all__
    assert S.NonlinearSystemBlock().ids == ()
    assert S.NonlinearSystemBlock((1, 2)).ids == (1, 2) and S.NonlinearSystemBlock([2]).ids == (2,) and S.NonlinearSystemBlock(1).ids == (1,)
    assert isinstance(S.NonlinearSystemBlock(), S.LinearSystemBlock) and not isinstance(S.LinearSystemBlock(), S.NonlinearSystemBlock)
    nl, li = S.NonlinearSystemBlock, S.LinearSystemBlock
    t = S.BlockTriangularSolver([[nl([1]), li()], [li(), nl()]], [S.LUSolver(), S.JacobiLinearSolver()], half="lower")
    assert isinstance(t.blocks[0][0], nl) and isinstance(t.blocks[1][1], nl) and not isinstance(t.blocks[0][1], nl)
    d = S.BlockDiagonalSolver([nl(), li()], [S.LUSolver(), S.JacobiLinearSolver()])
    assert isinstance(d.blocks[0][0], nl) and not isinstance(d.blocks[1][1], nl)
    M = po.poisson_matrix((4, 4), 1)
    sc = S.SchurComplementSolver((S.LUSolver(), M), M, M, (S.JacobiLinearSolver(), M))
    assert all(isinstance(b, S.MatrixBlock) for row in sc.blocks for b in row)     # the Schur solver's blocks are its own matrices


def test_numerical_setup_accepts_x(S):
    import inspect
    sig = inspect.signature(S.numerical_setup_)
    assert list(sig.parameters) == ["ns", "A", "smatrices", "x"] and sig.parameters["x"].default is None
    with pytest.raises(TypeError):
        S.numerical_setup_(object(), None, x=np.zeros(3))                          # x is accepted; the setup type is still checked
    assert hasattr(S.BlockNumericalSetup, "update") and hasattr(S.BlockNumericalSetup, "setup_info")


def test_abi_declares_the_block_refresh_entry_points(pkg):
    """argument counts of abi.SYMBOLS against the declarations of include/gmg_amd.h"""
    txt = open(os.path.join(ROOT, "include", "gmg_amd.h")).read()
    for name in ("gmg_block_update_values", "gmg_block_update_values_csc", "gmg_block_refresh_diag_solver", "gmg_block_get_setup_info"):
        m = re.search(r"GMG_API\s+int\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name
        assert len(pkg.abi.SYMBOLS[name]) == len(m.group(1).split(",")), name
    assert (pkg.abi.BLOCK_SLOT_SYSTEM, pkg.abi.BLOCK_SLOT_PRECOND, pkg.abi.BLOCK_SLOT_DIAG_MATRIX) == (0, 1, 2)
    assert re.search(r"GMG_BLOCK_SLOT_SYSTEM = 0, GMG_BLOCK_SLOT_PRECOND = 1, GMG_BLOCK_SLOT_DIAG_MATRIX = 2", txt)


def test_stokes_like_sequences_share_their_patterns(po):
    for explicit in (True, False):
        seq = bp.stokes_like(po, (8, 8, 8), 2, nsteps=4, explicit=explicit)
        assert len(seq) == 4 and seq[0]["n1"] == 343 and seq[0]["n2"] == 27
        for a, b in zip(seq[:-1], seq[1:]):
            bp.assert_same_patterns(a["mat"], b["mat"], fixed=((1, 1),))
        B = seq[0]["mat"][1][0]
        assert B.shape == (27, 343)
        # explicit: no value twice (no dictionary, no row pattern); constant coefficients: a handful of values
        assert (np.unique(B.val).size == B.val.size) == explicit
        assert np.unique(seq[0]["mat"][0][0].val).size > 256                        # variable coefficients: no value dictionary


def test_reference_pair_and_edge_systems(po):
    M, M2 = bp.reference_pair(po)
    assert M.shape == (49, 49) and bp.same_pattern(M, M2)
    r = M2.to_scipy().diagonal() / M.to_scipy().diagonal()
    assert r.min() > 1.1                                                           # old and new diagonal blocks differ by far more than 1e-3
    for name in bp.EDGE_NAMES:
        seq = bp.edge_system(po, name)
        assert len(seq) == 3
        bp.assert_same_patterns(seq[0], seq[1]); bp.assert_same_patterns(seq[1], seq[2])
    assert [bp.edge_system(po, "ragged-%d" % n)[0][0][0].shape[0] for n in (1, 63, 64, 65, 4283)] == [1, 63, 64, 65, 4283]
    R = bp.edge_system(po, "aggregation")[0][1][0]
    assert R.shape == (97, 4283) and np.diff(R.ptr).max() == 3000
    P, R = bp.edge_system(po, "rect-257x63")[0][0][1], bp.edge_system(po, "rect-257x63")[0][1][0]
    assert P.shape == (257, 63) and R.shape == (63, 257) and (np.diff(P.ptr) == 0).any() and (np.diff(R.ptr) == 0).any()
    assert np.diff(bp.edge_system(po, "long")[0][0][0].ptr).max() == 3000
    assert bp.edge_system(po, "offsets")[0][0][0].shape[0] % 64 == 29
