"""Host side of the Krylov solvers around a GMG as block solvers (FGMRESSolver(m, gmg) / GMRESSolver(m; Pr | Pl = gmg) / CGSolver(gmg)
on a diagonal block, GMG_BLOCK_KRYLOV_GMG): the Python constructors, the declared ABI, and the composed CPU reference of
tests/krylov_block_reference.py -- its self-consistency and the fixture conditions the device tests rely on.  No GPU."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import krylov_block_reference as kb
import numpy_twin as nt
from conftest import ROOT, rel_err


@pytest.fixture(scope="module")
def small(S, po):
    H = po.build_hierarchy((8, 8), 2, 1)
    gmg = S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"])
    M, R = H["mats"][0], po.poisson_matrix((4, 4), 1)
    import scipy.sparse as sp
    n, m = M.shape[0], R.shape[0]
    B = sp.random(n, m, density=0.2, random_state=1, format="csr")
    Cm = sp.random(m, n, density=0.2, random_state=2, format="csr")
    return dict(H=H, gmg=gmg, M=M, R=R, B=B, C=Cm)


# ---------------------------------------------------------------- (a) constructors
def _accepted(S, gmg):
    return [S.FGMRESSolver(5, gmg), S.FGMRESSolver(5, gmg, restart=True, m_add=2, maxiter=7), S.GMRESSolver(4, Pr=gmg),
            S.GMRESSolver(4, Pl=gmg), S.CGSolver(gmg), S.CGSolver(gmg, flexible=True)]


def _rejected(S, gmg):
    return [S.FGMRESSolver(5, gmg, Pl=S.JacobiLinearSolver()),                  # an FGMRES with a Pl
            S.GMRESSolver(4, Pr=gmg, Pl=gmg),                                   # both sides of GMRES
            S.GMRESSolver(4, Pr=gmg, Pl=(S.JacobiLinearSolver(), gmg)),
            S.FGMRESSolver(5, S.JacobiLinearSolver()),                          # a preconditioner that is not a GMGLinearSolver
            S.FGMRESSolver(5, (None, gmg)),
            S.GMRESSolver(4, Pr=S.LUSolver()),
            S.CGSolver(S.LUSolver()),
            S.CGSolver((None, gmg))]


def test_constructors_accept_krylov_around_gmg(S, small):
    T = small
    gmg, cg = T["gmg"], S.CGSolver(S.JacobiLinearSolver(), maxiter=20)
    # the form of the issue: the Schur constructor raised TypeError for this before
    P = S.SchurComplementSolver((S.FGMRESSolver(5, gmg), None), T["B"], T["C"], (cg, T["R"]))
    assert P.A[1] is T["H"]["mats"][0] and P.blocks[0][0].mat is T["H"]["mats"][0]       # matrix = None: the GMG's own finest matrix
    for sv in _accepted(S, gmg):
        assert S._is_block_diag_solver(sv)
        assert S.SchurComplementSolver((sv, None), T["B"], T["C"], (cg, T["R"])).solvers[0] is sv
        assert S.SchurComplementSolver((sv, T["M"]), T["B"], T["C"], (cg, T["R"])).A[1] is T["M"]
        assert S.SchurComplementSolver((S.LUSolver(), T["R"]), T["C"], T["B"], (sv, None)).solvers[1] is sv    # S as well
        for half in ("upper", "lower"):
            assert S.BlockTriangularSolver([sv, cg], half=half).solvers[0] is sv
        assert S.BlockDiagonalSolver([sv, cg]).solvers[0] is sv
    spec = S._krylov_gmg_spec
    abi = importlib.import_module(S.__name__.rsplit(".", 1)[0] + ".abi")
    assert spec(S.FGMRESSolver(5, gmg, restart=True, m_add=2)) == (gmg, abi.KRYLOV_FGMRES, 5, True, 2, False, 0)
    assert spec(S.GMRESSolver(4, Pr=gmg))[1:] == (abi.KRYLOV_GMRES, 4, False, 1, False, 0)
    assert spec(S.GMRESSolver(4, Pl=gmg))[-1] == 1
    assert spec(S.CGSolver(gmg, flexible=True))[1] == abi.KRYLOV_CG and spec(S.CGSolver(gmg, flexible=True))[-2:] == (True, 1)
    assert spec(S.CGSolver(S.JacobiLinearSolver())) is None and spec(S.LUSolver()) is None and spec(gmg) is None


def test_constructors_reject_other_krylov_forms(S, small):
    T = small
    gmg, cg = T["gmg"], S.CGSolver(S.JacobiLinearSolver(), maxiter=20)
    for bad in _rejected(S, gmg):
        with pytest.raises(NotImplementedError, match=r"FGMRESSolver\(m, gmg\).*GMRESSolver\(m, Pr=gmg\).*CGSolver\(gmg"):
            S.SchurComplementSolver((bad, T["M"]), T["B"], T["C"], (cg, T["R"]))
        with pytest.raises(NotImplementedError):
            S.SchurComplementSolver((S.LUSolver(), T["M"]), T["B"], T["C"], (bad, T["R"]))
        with pytest.raises(NotImplementedError):
            S.BlockTriangularSolver([bad, cg], half="upper")
        with pytest.raises(NotImplementedError):
            S.BlockDiagonalSolver([bad, cg])
    # a Krylov solver without any preconditioner was never a block solver and is refused as before
    for bare in (S.CGSolver(None), S.FGMRESSolver(5, None), S.GMRESSolver(4)):
        assert not S._is_block_diag_solver(bare)
        with pytest.raises(TypeError):
            S.SchurComplementSolver((bare, T["M"]), T["B"], T["C"], (cg, T["R"]))


# ---------------------------------------------------------------- (b) the declared ABI
def test_abi_constants_and_prototypes(pkg):
    abi = importlib.import_module(pkg.__name__ + ".abi")
    hdr = open(os.path.join(ROOT, "include", "gmg_amd.h")).read()
    jl = open(os.path.join(ROOT, "gridapsolvers.jl_amd", "julia", "GridapSolversAMD.jl")).read()
    assert abi.BLOCK_KRYLOV_GMG == 5 and (abi.KRYLOV_CG, abi.KRYLOV_FGMRES, abi.KRYLOV_GMRES) == (1, 2, 3)
    assert re.search(r"GMG_BLOCK_KRYLOV_GMG\s*=\s*5", hdr)
    assert re.search(r"enum gmg_krylov_kind\s*\{\s*GMG_KRYLOV_CG = 1, GMG_KRYLOV_FGMRES = 2, GMG_KRYLOV_GMRES = 3\s*\}", hdr)
    proto = re.search(r"GMG_API int gmg_block_set_diag_krylov_gmg\(([^;]*)\);", hdr).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["h", "i", "g", "krylov", "m", "restart", "m_add", "flexible", "side",
                                                                      "maxiter", "atol", "rtol"]
    assert re.search(r"GMG_API int gmg_block_diag_stats\(gmg_block_handle_t h, int i, int64_t \*napplies, int64_t \*total_iters\);", hdr)
    assert "fgmres_fused" in hdr and "NavierStokesGMG.jl:159-169" in hdr
    assert abi.SYMBOLS["gmg_block_set_diag_krylov_gmg"] == [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 7 + [C.c_double] * 2
    assert abi.SYMBOLS["gmg_block_diag_stats"] == [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert "gmg_block_set_diag_krylov_gmg" in jl and re.search(r"GMG_BLOCK_KRYLOV_GMG\s*=\s*Cint\(5\)", jl)
    lib = abi.load()                                                             # the built library exports both
    assert lib.gmg_block_set_diag_krylov_gmg and lib.gmg_block_diag_stats
    docs = {n: open(os.path.join(ROOT, n)).read() for n in ("INTEGRATION.md", "DESIGN.md", "README.md")}
    assert "gmg_block_set_diag_krylov_gmg" in docs["INTEGRATION.md"] and "GMG_BLOCK_KRYLOV_GMG" in docs["DESIGN.md"]
    assert "FGMRESSolver(m, gmg)" in docs["README.md"]


# ---------------------------------------------------------------- (c) the composition is self-consistent
@pytest.mark.parametrize("m,restart,m_add", [(2, False, 1), (2, True, 2)])
def test_oracle_fgmres_with_initial_guess_agrees_with_numpy_restatement(orc, m, restart, m_add):
    """orc.fgmres_solve(A, b, Pr = GMG, x0) against numpy_twin.fgmres, which starts from zero: FGMRES from x0 on b is x0 + FGMRES
    from zero on b - A x0 (the same r0, the same basis, the same stopping rule relative to |r0|)"""
    H = kb.q1((8, 8, 8), 2)
    A = [a.to_scipy().tocsr() for a in H["mats"]]
    b = np.random.default_rng(1).uniform(-1, 1, A[0].shape[0])
    x0 = np.random.default_rng(2).uniform(-1, 1, A[0].shape[0])
    go = kb.oracle_q1_gmg(H)
    tw = nt.GMG(H["mats"], H["prolongations"], H["restrictions"], [(nt.Jacobi(A[0]), 10, 2.0 / 3.0)])
    kw = dict(m=m, restart=restart, m_add=m_add, maxiter=12, atol=1e-14, rtol=1e-10)
    xo, nit, flag, hist = orc.fgmres_solve(H["mats"][0], b, Pr=go, x0=x0, **kw)
    dx, nit_t, hist_t = nt.fgmres(A[0], b - A[0] @ x0, Pr=tw.solve, **kw)
    assert nit == nit_t and nit > m and flag == kb.flag_of(nit, hist, 12, 1e-14, 1e-10)
    np.testing.assert_allclose(hist, hist_t, rtol=1e-7, atol=1e-15 * hist[0])   # tests/test_oracle.py: the same comparison from x0 = 0
    assert rel_err(xo, x0 + dx) <= 1e-9
    assert rel_err(xo, x0) > 1e-2 and abs(hist[0] - np.linalg.norm(b - A[0] @ x0)) <= 1e-12 * hist[0]   # the guess was read
    # and the in-place callable of the composition is that solve
    inner = kb.Inner(H["mats"][0], go, kb.spec("fgmres", **kw))
    x = x0.copy()
    inner(x, b)
    assert np.array_equal(x, xo) and inner.calls[0][0] == nit


def test_block_glue_with_persistent_caches_restates_numpy_twin(po):
    """BlockApply with stateless block solvers is numpy_twin.block_apply; with a stateful one the second application starts from y"""
    M = po.poisson_matrix((8, 8), 1); n = M.shape[0]
    Ms = M.to_scipy().tocsr()
    b = np.random.default_rng(0).uniform(-1, 1, 2 * n)
    import schur_reference as sr
    ex = sr.exact_solver(Ms)
    for half in ("upper", "lower", "diagonal"):
        coeffs = [[1.0, -2.5], [0.5, 1.0]]
        P = kb.BlockApply(half, [ex, ex], {(0, 1): -Ms, (1, 0): Ms}, coeffs, [n, n])
        ref = nt.block_apply(half, [lambda w: ex_out(ex, w)] * 2, {(0, 1): -Ms, (1, 0): Ms}, coeffs, [n, n], b)
        assert np.array_equal(P(b), ref) and np.array_equal(P(b), ref)
    seen = []

    def stateful(x, w):
        seen.append(x.copy())
        x += 1.0
    P = kb.BlockApply("diagonal", [stateful], {}, [[1.0]], [3])
    P(np.zeros(3)); P(np.zeros(3))
    assert np.array_equal(seen[0], np.zeros(3)) and np.array_equal(seen[1], np.ones(3))


def ex_out(ex, w):
    x = np.zeros_like(w)
    ex(x, w)
    return x


def test_margin_rule():
    ok = kb.margin_ok
    assert ok([1.0, 1e-1, 1e-4], 2, 10, 1e-30, 1e-3)                        # stops a decade under, the entry before two decades over
    assert not ok([1.0, 1.5e-3, 1e-4], 2, 10, 1e-30, 1e-3)                  # an entry that did not stop within a factor 2 of rtol
    assert not ok([1.0, 1e-1, 6e-4], 2, 10, 1e-30, 1e-3)                    # the stopping entry within a factor 2
    assert ok([1.0, 1e-1, 6e-4], 2, 2, 1e-30, 1e-3)                         # the same run ending at maxiter: its last entry is exempt
    assert not ok([1.0, 1.5e-3, 6e-4], 2, 2, 1e-30, 1e-3)                   # ... the earlier ones are not
    assert ok([1e-3, 1e-9], 1, 10, 1e-6, 1e-30) and not ok([1e-3, 7e-7], 1, 10, 1e-6, 1e-30)   # the absolute threshold
    assert ok([0.0], 0, 10, 1e-12, 1e-6) and not ok([8e-13], 0, 10, 1e-12, 1e-6)              # init!


# ---------------------------------------------------------------- (d) the fixture conditions, on the reference alone
@pytest.mark.parametrize("name", kb.all_case_names())
def test_fixture_conditions_hold_for_the_reference(name):
    c = kb.case(name)
    for label, good in c["checks"]:
        assert good, (name, label, "a stop-deciding residual of the reference is within a factor 2 of its threshold: change the parameters")
    for n, _flag, hist in c["inner"]:
        assert n >= 1 and np.all(np.isfinite(hist))
    if name.startswith("outer:"):
        assert c["flag"] in (kb.gr.CONVERGED_RTOL, kb.gr.CONVERGED_ATOL) and 0 < c["nit"] < 20
        T = kb.stokes8(name.split("/")[1])
        true_res = np.linalg.norm(T["K"] @ c["x"] - T["b"])
        print("%s: %d iterations, estimate %.3e, ||K x - b|| = %.3e" % (name, c["nit"], c["hist"][-1], true_res))
        assert true_res < 1e-7                              # under GMRES too: its nested solve is tight (krylov_block_reference.SPECS)
        assert len(c["inner"]) >= c["nit"] and len(c["cg"]) == len(c["inner"])


def test_reference_tells_a_warm_cache_from_a_cold_one():
    """2, 7: the references started from the previous y / du and from zero differ by at least 100 x the tolerance of the comparison,
    so a device that ignores the guess cannot pass"""
    g = kb.case("guess:nonsym")
    assert rel_err(g["x2"], g["x1"]) >= 100 * kb.TOL_X
    s = kb.case("schur:nonsym")
    assert rel_err(s["x2"], s["x1"]) >= 100 * kb.TOL_X                      # the second application: x and du are warm
    assert rel_err(s["xz"], s["x1"]) >= 100 * kb.TOL_X                      # x on entry was read
    a = kb.case("apply:nonsym")
    assert rel_err(a["x2"], a["x1"]) >= 100 * kb.TOL_X


def test_nonsymmetric_variant_is_a_weak_block_solve_for_one_gmg(orc):
    """the reason for the wrapper: on the perturbed velocity block one GMG application leaves a residual the Krylov wrapper removes"""
    for variant, most in (("sym", 3), ("nonsym", 12)):
        T = kb.stokes8(variant)
        w = np.random.default_rng(3).uniform(-1, 1, T["nu"])
        _x, nit, flag, _h = orc.fgmres_solve(T["A"][0][0], w, Pr=kb.oracle_velocity_gmg(T), m=20, maxiter=20, atol=1e-30, rtol=1e-10)
        assert flag == kb.gr.CONVERGED_RTOL and nit <= most
        if variant == "nonsym":
            assert nit >= 5
