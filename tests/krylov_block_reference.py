"""Reference of the Krylov solvers around a GMG as block solvers (GMG_BLOCK_KRYLOV_GMG: FGMRESSolver(m, gmg) / GMRESSolver(m; Pr | Pl
= gmg) / CGSolver(gmg) on a diagonal block, test/Applications/NavierStokesGMG.jl:159-169), a COMPOSITION of the checkers the suite
already has -- the oracle's library is not extended:

  inner solve   orc.fgmres_solve(A_u, w, Pr = oracle GMG, x0 = y_prev, ...) / orc.cg_solve(..., Pl = oracle GMG, x0 = ...) /
                tests/gmres_reference.gmres on the oracle's spmv, dot, norm and Givens (Inner)
  block glue    BlockTriangularSolvers.jl:186-242 / BlockDiagonalSolvers.jl:165-177 restated with PERSISTENT y caches (BlockApply:
                numpy_twin.block_apply solves into a fresh vector; the reference's ns.work_caches keep y_i, the initial guess of an
                iterative block solver), tests/schur_reference.schur_apply for the Schur form
  outer solve   numpy_twin.fgmres / gmres_reference.gmres with the composed application as Pr

Test infrastructure only; plain helper (no fixtures, no collection hooks), nothing read from outside the repository.  Every case is
computed once per process (cases()) and shared, read-only, by tests/test_krylov_block_host.py (which checks the fixture conditions on
the CPU) and tests/test_gpu_krylov_blocks.py.

Fixture condition (margin_ok): iteration counts of the device are held to the reference's only where the reference's own history keeps
every stop-deciding residual a factor 2 away from its threshold -- a residual that did not stop the solve is >= 2 x the threshold, the
one that did is <= threshold / 2; a solve that ends at maxiter is exempt for its last entry.  The parameters below were chosen so that
every inner and outer solve of every case satisfies it."""
import numpy as np
import scipy.sparse as sp

import __graft_entry__ as entry
import block_refresh_problems as bp
import gmres_reference as gr
import numpy_twin as nt
import schur_reference as sr

TOL_X = 1e-6                  # tests/test_gpu_schur.py::_agree: rel err of x
TOL_HIST = 1e-6               # the same: |hist - ref| <= TOL_HIST * hist[0]
REL_NONSYM = 1.0e-3           # relative size of the seeded perturbation of every velocity entry (same pattern): with alpha = 1e3 in the
                              # grad-div term this is an O(1) nonsymmetric change against the viscous part -- GMG(4 cycles) then takes 8
                              # FGMRES iterations to 1e-10 where the symmetric block takes 2 (5e-2 leaves no convergence at all)
ALPHA = 1.0e3
NONSYM_SEED = 55              # seed of that perturbation, chosen so that every solve of every case below keeps the factor-2 margins (with
                              # most seeds some inner FGMRES(5; rtol = 1e-2) of the outer solves stops within a factor 2 of its threshold)
OUTER = dict(maxiter=100, atol=1e-10, rtol=1e-12)            # tests/test_gpu_schur.py::KW
CG_P = dict(maxiter=20, atol=1e-14, rtol=1e-6)               # CGSolver(JacobiLinearSolver(); ...) on the pressure mass matrix


def _pkg():
    return entry.import_package()


def _orc():
    return entry.import_oracle()


def csr(M):
    po = _pkg().poisson
    M = sp.csr_matrix(M); M.sort_indices()
    return po.CSR(M.shape, M.indptr, M.indices, M.data)


# ---------------------------------------------------------------- the fixture condition
def margin_ok(hist, nit, maxiter, atol, rtol, factor=2.0):
    """every stop-deciding residual of one solve a factor `factor` away from its threshold (the last entry of a solve that ends at
    maxiter is exempt: the count is then decided by maxiter, not by a residual)"""
    hist = np.asarray(hist, dtype=np.float64)
    assert hist.size == nit + 1
    r0 = hist[0]
    if nit == 0:                                             # stopped at init!: by atol (e_r = 1 there)
        return maxiter == 0 or r0 <= atol / factor
    for k in range(nit):                                     # did not stop: well above both thresholds
        e_r = 1.0 if k == 0 else hist[k] / r0
        if not (e_r >= factor * rtol and hist[k] >= factor * atol):
            return False
    if nit >= maxiter:
        return True
    return hist[nit] / r0 <= rtol / factor or hist[nit] <= atol / factor


def flag_of(nit, hist, maxiter, atol, rtol):
    return gr._flag(nit, hist[-1], hist[-1] / hist[0], maxiter, atol, rtol)


# ---------------------------------------------------------------- block solvers as in-place callables with a record
class Inner:
    """spec = dict(kind = "fgmres" | "gmres-pr" | "gmres-pl" | "cg" | "fcg", m, restart, m_add, maxiter, atol, rtol): the Krylov solver
    around the oracle GMG `go` on the matrix A (po.CSR), solve!(x, ns, b) in place -- x on entry is the initial guess.  calls =
    [(niters, flag, hist)] of every application."""

    def __init__(self, A, go, spec):
        self.A, self.go, self.spec, self.calls = A, go, dict(spec), []

    def __call__(self, x, b):
        orc, s = _orc(), self.spec
        b = np.ascontiguousarray(b, dtype=np.float64)
        kw = dict(maxiter=s["maxiter"], atol=s["atol"], rtol=s["rtol"])
        if s["kind"] == "fgmres":
            ref = orc.fgmres_solve(self.A, b, Pr=self.go, x0=x, m=s["m"], restart=s.get("restart", False), m_add=s.get("m_add", 1), **kw)
        elif s["kind"] in ("cg", "fcg"):
            ref = orc.cg_solve(self.A, b, Pl=self.go, x0=x, flexible=(s["kind"] == "fcg"), **kw)
        else:
            P = lambda r: self.go.solve(np.ascontiguousarray(r, dtype=np.float64))[0]
            side = dict(Pr=P) if s["kind"] == "gmres-pr" else dict(Pl=P)
            ref = gr.gmres(lambda v: orc.spmv(self.A, np.ascontiguousarray(v)), b, s["m"], x0=x, restart=s.get("restart", False),
                           m_add=s.get("m_add", 1), dot=orc.dot, norm=orc.norm, givens=orc.givens, **side, **kw)
        x[:] = ref[0]
        self.calls.append((ref[1], ref[2], np.array(ref[3])))

    def margins_ok(self):
        s = self.spec
        return all(margin_ok(h, n, s["maxiter"], s["atol"], s["rtol"]) for n, _f, h in self.calls)


class CgJacobi:
    """CGSolver(JacobiLinearSolver(); maxiter, atol, rtol) through the oracle, in place, x on entry the initial guess"""

    def __init__(self, M, maxiter, atol, rtol):
        self.M, self.kw, self.calls = M, dict(maxiter=maxiter, atol=atol, rtol=rtol), []

    def __call__(self, x, b):
        xo, nit, flag, hist = _orc().cg_solve(self.M, np.ascontiguousarray(b, dtype=np.float64), Pl="jacobi", x0=x, **self.kw)
        x[:] = xo
        self.calls.append((nit, flag, np.array(hist)))

    def margins_ok(self):
        return all(margin_ok(h, n, **self.kw) for n, _f, h in self.calls)


class Jacobi:
    def __init__(self, M):
        self.dinv, self.calls = 1.0 / M.to_scipy().diagonal(), []

    def __call__(self, x, b):
        x[:] = self.dinv * b

    def margins_ok(self):
        return True


class BlockApply:
    """solve!(x, ns, b) of BlockDiagonalSolverNS / BlockTriangularSolverNS with the y caches of the numerical setup: solves[i](y_i, w_i)
    works in place on y_i, which persists between applications (zero before the first); offd[(i, j)] = scipy matrices."""

    def __init__(self, kind, solves, offd, coeffs, sizes):
        self.kind, self.solves, self.offd, self.coeffs = kind, solves, offd, coeffs
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.y = [np.zeros(int(n)) for n in sizes]

    def __call__(self, b):
        nb, off = len(self.y), self.off
        b = np.asarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        order = range(nb - 1, -1, -1) if self.kind == "upper" else range(nb)
        for i in order:
            w = b[off[i]:off[i + 1]].copy()
            if self.kind != "diagonal":
                for j in (range(i + 1, nb) if self.kind == "upper" else range(i)):
                    if (i, j) in self.offd and self.coeffs[i][j] != 0.0:
                        w -= self.coeffs[i][j] * (self.offd[(i, j)] @ x[off[j]:off[j + 1]])
            self.solves[i](self.y[i], w)
            x[off[i]:off[i + 1]] = self.y[i]
        return x


# ---------------------------------------------------------------- problems
_PROBLEMS = {}


def stokes8(variant):
    """stokes.stokes_system(8) with the 2-level patch-smoothed velocity hierarchy of tests/test_gpu_schur.py::stokes8; variant "nonsym":
    the velocity block with a seeded relative perturbation of every entry (block_refresh_problems.perturbed, same pattern)."""
    if ("stokes8", variant) in _PROBLEMS:
        return _PROBLEMS[("stokes8", variant)]
    import importlib
    pkg = _pkg()
    po, st = pkg.poisson, importlib.import_module(pkg.__name__ + ".stokes")
    sysd = st.stokes_system(8, ALPHA)
    Hv = st.velocity_hierarchy(8, 2, ALPHA)
    A = [list(r) for r in sysd["A"]]
    if variant == "nonsym":
        A[0][0] = bp.perturbed(po, A[0][0], NONSYM_SEED, rel=REL_NONSYM)
        assert bp.same_pattern(A[0][0], sysd["A"][0][0])
        d = A[0][0].to_scipy(); assert abs(d - d.T).max() > 0.1 * REL_NONSYM * abs(d).max()
    elif variant != "sym":
        raise ValueError(variant)
    mats = [A[0][0]] + list(Hv["mats"][1:])
    K = sp.bmat([[None if m is None else m.to_scipy() for m in row] for row in A]).tocsr()
    K.sort_indices()
    nu, npp = (int(v) for v in sysd["sizes"])
    T = dict(A=A, K=K, Kc=csr(K), b=np.array(sysd["b"], dtype=np.float64), Hv=Hv, mats=mats, nu=nu, np=npp, n=nu + npp, Mp=sysd["Mp_scaled"],
             B=A[0][1], C=A[1][0])
    T["b"].setflags(write=False)
    _PROBLEMS[("stokes8", variant)] = T
    return T


def oracle_velocity_gmg(T, maxiter=4):
    orc, Hv = _orc(), T["Hv"]
    osm = [orc.Smoother(orc.PATCH, 10, 0.2, pp, pd) for pp, pd in Hv["star_patches"]]
    nlev = len(T["mats"])
    return orc.GMG(T["mats"], Hv["prolongations"], Hv["restrictions"], pre_smoothers=osm, maxiter=maxiter, rtol=1e-8,
                   prolongation_patches=[(orc.PATCH, *Hv["interior_patches"][l], Hv["graddiv"][l]) for l in range(nlev - 1)])


def device_velocity_gmg(S, T, maxiter=4, options=None):
    """the device twin of oracle_velocity_gmg (tests/test_gpu_block.py::_real_stokes)"""
    Hv = T["Hv"]
    nlev = len(T["mats"])
    sm = [S.RichardsonSmoother(S.PatchSolver(pp, pd), 10, 0.2) for pp, pd in Hv["star_patches"]]
    interp = [S.PatchProlongationOperator(Hv["prolongations"][l], *Hv["interior_patches"][l], pivoting=True, rhs=Hv["graddiv"][l])
              for l in range(nlev - 1)]
    return S.GMGLinearSolver(T["mats"], interp, Hv["restrictions"], pre_smoothers=sm, post_smoothers=sm, coarsest_solver=S.LUSolver(),
                             maxiter=maxiter, mode="preconditioner", options=options)


def q1(nc=(16, 16, 16), nlev=3):
    """the suite's small Q1 Poisson hierarchy: 3375, 343 and 27 rows"""
    key = ("q1", tuple(nc), nlev)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = _pkg().poisson.build_hierarchy(nc, nlev, 1)
    return _PROBLEMS[key]


def oracle_q1_gmg(H, maxiter=1):
    return _orc().GMG(H["mats"], H["prolongations"], H["restrictions"], maxiter=maxiter)


def device_q1_gmg(S, H, maxiter=1, options=None):
    nlev = len(H["mats"])
    sm = [S.RichardsonSmoother(S.JacobiLinearSolver(), 10, 2.0 / 3.0)] * (nlev - 1)
    return S.GMGLinearSolver(H["mats"], H["prolongations"], H["restrictions"], pre_smoothers=sm, post_smoothers=sm, maxiter=maxiter,
                             mode="preconditioner", options=options)


def unaligned_system():
    """lower triangular, block 0 = 343 rows (ODD: block 1 of every block vector starts 8 bytes off a 16-byte boundary), block 1 = the
    3375-row finest Q1 matrix, block (1,0) = 0.05 x the prolongation between the two"""
    if "unaligned" in _PROBLEMS:
        return _PROBLEMS["unaligned"]
    H = q1()
    A0, A1 = H["mats"][1], H["mats"][0]
    C10 = csr(0.05 * H["prolongations"][0].to_scipy())
    assert A0.shape[0] == 343 and C10.shape == (A1.shape[0], 343)
    mat = [[A0, None], [C10, A1]]
    K = sp.bmat([[A0.to_scipy(), None], [C10.to_scipy(), A1.to_scipy()]]).tocsr()
    b = np.random.default_rng(17).uniform(-1, 1, K.shape[0])
    b.setflags(write=False)
    T = dict(H=H, mat=mat, K=K, b=b, sizes=[343, A1.shape[0]], C10=C10)
    _PROBLEMS["unaligned"] = T
    return T


# ---------------------------------------------------------------- solver specs (shared by the reference and the device tests)
def spec(kind, m=1, restart=False, m_add=1, maxiter=100, atol=1e-12, rtol=1e-6):
    return dict(kind=kind, m=m, restart=restart, m_add=m_add, maxiter=maxiter, atol=atol, rtol=rtol)


SPECS = {
    # 1, 2: FGMRES(3, gmg; maxiter = 2) -- the defaults of FGMRESSolver otherwise
    "apply": spec("fgmres", m=3, maxiter=2),
    # 2: one iteration only, so that the initial guess shows in the result
    "guess": spec("fgmres", m=3, maxiter=1),
    # 3: basis growth and restart inside the nested solve
    "grow": spec("fgmres", m=2, restart=False, m_add=1, maxiter=5, atol=1e-30, rtol=1e-30),
    "restart": spec("fgmres", m=2, restart=True, m_add=1, maxiter=5, atol=1e-30, rtol=1e-30),
    # 4: kinds
    # 4: kinds, fixed counts (GMRES: the fifth column grows the basis of 4; the symmetric block converges by 1e-7 per iteration, so
    # longer runs would only iterate on rounding noise -- and hand the GMG of a CG residuals under its own atol)
    "gmres-pr": spec("gmres-pr", m=4, maxiter=5, atol=1e-30, rtol=1e-30),
    "gmres-pl": spec("gmres-pl", m=4, maxiter=5, atol=1e-30, rtol=1e-30),
    "cg": spec("cg", maxiter=2, atol=1e-30, rtol=1e-30),
    "fcg": spec("fcg", maxiter=2, atol=1e-30, rtol=1e-30),
    # 5: the unaligned sub-vector
    "unaligned": spec("fgmres", m=4, maxiter=3, atol=1e-30, rtol=1e-30),
    # 6: outer solves -- FGMRES(5, gmg; rtol = 1e-2)
    "outer": spec("fgmres", m=5, maxiter=100, atol=1e-12, rtol=1e-2),
    # 6, under GMRES: x = x0 + Pr(sum g_i V_i) takes Pr for LINEAR, and a nested Krylov solve that stops at rtol = 1e-2 from its previous
    # solution is not -- with the spec above the reference's estimate reports convergence at a true residual of 1.5e-4 (symmetric) and
    # 1.25 (perturbed).  GMRES outside therefore gets the nested solve to 1e-13: linear to the outer tolerance, ||K x - b|| < 1e-7 for
    # the reference (1e-10 .. 1e-12 leave some nested solve within a factor 2 of its threshold on one of the two systems)
    "outer-gmres": spec("fgmres", m=5, maxiter=100, atol=1e-30, rtol=1e-13),
    # 7: Schur -- FGMRES(5, gmg)
    "schur": spec("fgmres", m=5, maxiter=2, atol=1e-30, rtol=1e-30),
}


def device_inner(S, gmg, s):
    """the device solver object of a spec"""
    kw = dict(maxiter=s["maxiter"], atol=s["atol"], rtol=s["rtol"])
    if s["kind"] == "fgmres":
        return S.FGMRESSolver(s["m"], gmg, restart=s["restart"], m_add=s["m_add"], **kw)
    if s["kind"] == "gmres-pr":
        return S.GMRESSolver(s["m"], Pr=gmg, restart=s["restart"], m_add=s["m_add"], **kw)
    if s["kind"] == "gmres-pl":
        return S.GMRESSolver(s["m"], Pl=gmg, restart=s["restart"], m_add=s["m_add"], **kw)
    return S.CGSolver(gmg, flexible=(s["kind"] == "fcg"), **kw)


def device_stokes_solver(S, T, s, half="upper", options=None):
    """-> (block solver, inner solver, CG-Jacobi) on the Stokes system T: [inner(spec s) around the velocity GMG, CG-Jacobi on
    -1/alpha M_p]; upper: coefficients [[1, 1], [0, 1]] (StokesGMG.jl:151-157), lower: [[1, 0], [1, 1]], diagonal"""
    inner = device_inner(S, device_velocity_gmg(S, T, options=options), s)
    cg = S.CGSolver(S.JacobiLinearSolver(), **CG_P)
    blocks = [[S.LinearSystemBlock(), S.LinearSystemBlock()], [S.LinearSystemBlock(), S.MatrixBlock(T["Mp"])]]
    if half == "diagonal":
        return S.BlockDiagonalSolver([blocks[0][0], blocks[1][1]], [inner, cg]), inner, cg
    coeffs = [[1.0, 1.0], [0.0, 1.0]] if half == "upper" else [[1.0, 0.0], [1.0, 1.0]]
    return S.BlockTriangularSolver(blocks, [inner, cg], coeffs=coeffs, half=half), inner, cg


def reference_stokes_apply(T, s, half="upper"):
    """-> (BlockApply, Inner, CgJacobi): the composed reference of device_stokes_solver"""
    inner = Inner(T["A"][0][0], oracle_velocity_gmg(T), s)
    cg = CgJacobi(T["Mp"], **CG_P)
    coeffs = [[1.0, 1.0], [0.0, 1.0]] if half == "upper" else [[1.0, 0.0], [1.0, 1.0]]
    offd = {(0, 1): T["B"].to_scipy().tocsr(), (1, 0): T["C"].to_scipy().tocsr()}
    return BlockApply(half, [inner, cg], offd, coeffs, [T["nu"], T["np"]]), inner, cg


# ---------------------------------------------------------------- the cases: computed once, shared, read-only
_CASES = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _rec(solver):
    return [(n, f, h) for n, f, h in solver.calls]


def case(name):
    """name -> dict of the reference results of one case (see the builders below); `checks` = [(label, margins hold?)]"""
    if name in _CASES:
        return _CASES[name]
    kind, _, arg = name.partition(":")
    out = _BUILDERS[kind](arg)
    _CASES[name] = _freeze(out)
    return out


def _case_apply(variant):
    """1, 2: two applications of upper([FGMRES(3, gmg; maxiter = 2), CG-Jacobi]) on one setup (same b), and the second application
    from a cold cache"""
    T = stokes8(variant)
    P, inner, cg = reference_stokes_apply(T, SPECS["apply"])
    x1 = P(T["b"]); x2 = P(T["b"])
    Pc, inner_c, cg_c = reference_stokes_apply(T, SPECS["apply"])
    xc = Pc(T["b"])
    assert np.array_equal(xc, x1)
    return dict(x1=x1, x2=x2, inner=_rec(inner), cg=_rec(cg), checks=[("inner", inner.margins_ok()), ("cg", cg.margins_ok())])


def _case_one(arg):
    """3, 4: one application of half([inner(spec), CG-Jacobi]); arg = "<spec>/<half>/<variant>" """
    sname, half, variant = arg.split("/")
    T = stokes8(variant)
    P, inner, cg = reference_stokes_apply(T, SPECS[sname], half)
    x = P(T["b"])
    return dict(x=x, inner=_rec(inner), cg=_rec(cg), checks=[("inner", inner.margins_ok()), ("cg", cg.margins_ok())])


def _case_unaligned(_arg):
    """5: lower([Jacobi (343 rows), FGMRES(4, gmg) on the Q1 hierarchy]), two applications"""
    T = unaligned_system()
    inner = Inner(T["H"]["mats"][0], oracle_q1_gmg(T["H"]), SPECS["unaligned"])
    P = BlockApply("lower", [Jacobi(T["mat"][0][0]), inner], {(1, 0): T["C10"].to_scipy().tocsr()}, [[1.0, 0.0], [1.0, 1.0]], T["sizes"])
    x1 = P(T["b"]); x2 = P(T["b"])
    return dict(x1=x1, x2=x2, inner=_rec(inner), checks=[("inner", inner.margins_ok())])


def _case_outer(arg):
    """6: FGMRESSolver(20, P), P = upper([FGMRES(5, gmg; rtol = 1e-2), CG-Jacobi]) / GMRESSolver(20; Pr = P), P = upper([FGMRES(5, gmg;
    rtol = 1e-13), CG-Jacobi]) (outer_spec); arg = "<outer>/<variant>" """
    outer, variant = arg.split("/")
    T = stokes8(variant)
    orc = _orc()
    P, inner, cg = reference_stokes_apply(T, outer_spec(outer))
    if outer == "fgmres":
        x, nit, hist = nt.fgmres(T["K"], T["b"], Pr=P, m=20, **OUTER)
        flag = flag_of(nit, hist, **OUTER)
    else:
        x, nit, flag, hist = gr.gmres(lambda v: orc.spmv(T["Kc"], np.ascontiguousarray(v)), T["b"], 20, Pr=P, dot=orc.dot, norm=orc.norm,
                                      givens=orc.givens, **OUTER)
    return dict(x=x, nit=nit, flag=flag, hist=np.array(hist), inner=_rec(inner), cg=_rec(cg),
                checks=[("inner", inner.margins_ok()), ("cg", cg.margins_ok()), ("outer", margin_ok(hist, nit, **OUTER))])


def outer_spec(outer):
    """the nested solver of the outer solves: SPECS["outer"] under FGMRES, SPECS["outer-gmres"] under GMRES (see there)"""
    return SPECS["outer" if outer == "fgmres" else "outer-gmres"]


def schur_x0(T):
    return np.random.default_rng(23).uniform(-1, 1, T["n"])


def _case_schur(variant):
    """7: SchurComplementSolver((FGMRES(5, gmg), None), B, C, (CG-Jacobi, Mp)): one application with a nonzero x on entry, a second one on
    the x it returned (du persists), and the first from a zero x"""
    T = stokes8(variant)

    def make():
        inner = Inner(T["A"][0][0], oracle_velocity_gmg(T), SPECS["schur"])
        cg = CgJacobi(T["Mp"], **CG_P)
        cache = sr.SchurCache(T["nu"])
        Bs, Cs = T["B"].to_scipy().tocsr(), T["C"].to_scipy().tocsr()
        return (lambda x: sr.schur_apply(x, T["b"], inner, cg, Bs, Cs, cache)), inner, cg

    ap, inner, cg = make()
    x = schur_x0(T)
    x1 = ap(x).copy(); x2 = ap(x).copy()
    ap0, _i0, _c0 = make()
    xz = ap0(np.zeros(T["n"])).copy()
    return dict(x1=x1, x2=x2, xz=xz, inner=_rec(inner), cg=_rec(cg), checks=[("inner", inner.margins_ok()), ("cg", cg.margins_ok())])


def guess_rhs(T):
    return np.random.default_rng(29).uniform(-1, 1, T["n"])


def _case_guess(variant):
    """2: two applications of upper([FGMRES(3, gmg; maxiter = 1), CG-Jacobi]) to one seeded right-hand side: the second starts from the
    first's y.  x1 is also what a cold cache (x0 = 0) gives for that right-hand side."""
    T = stokes8(variant)
    P, inner, cg = reference_stokes_apply(T, SPECS["guess"])
    b = guess_rhs(T)
    x1 = P(b); x2 = P(b)
    return dict(x1=x1, x2=x2, inner=_rec(inner), cg=_rec(cg), checks=[("inner", inner.margins_ok()), ("cg", cg.margins_ok())])


_BUILDERS = {"guess": _case_guess, "apply": _case_apply, "one": _case_one, "unaligned": _case_unaligned, "outer": _case_outer, "schur": _case_schur}

VARIANTS = ("sym", "nonsym")
KINDS = ("gmres-pr", "gmres-pl", "cg", "fcg")
HALVES = ("diagonal", "lower", "upper")


def all_case_names():
    names = ["apply:" + v for v in VARIANTS] + ["guess:nonsym"]
    names += ["one:%s/upper/nonsym" % s for s in ("grow", "restart")]
    names += ["one:%s/%s/sym" % (k, h) for k in KINDS for h in HALVES]
    names += ["unaligned:"]
    names += ["outer:%s/%s" % (o, v) for o in ("fgmres", "gmres") for v in VARIANTS]
    names += ["schur:nonsym"]
    return names


# ---------------------------------------------------------------- edge lengths: a two-level GMG on a matrix of ANY length
def edge_hierarchy(N):
    """krylov_edge_problems.problem(N, "nonsym") as the finest matrix of a 2-level hierarchy: piecewise-constant aggregation onto
    min(N, 8) coarse rows, Galerkin coarse matrix.  -> (mats, prolongations, restrictions, b)"""
    import krylov_edge_problems as kp
    A, b = kp.problem(N, "nonsym")
    nH = min(int(N), 8)
    agg = (np.arange(N, dtype=np.int64) * nH) // N
    P = sp.csr_matrix((np.ones(N), (np.arange(N), agg)), shape=(N, nH))
    R = P.T.tocsr()
    Ac = (R @ A @ P).tocsr()
    return [csr(A), csr(Ac)], [csr(P)], [csr(R)], b
