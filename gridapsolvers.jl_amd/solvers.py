"""Host-side mirror of the reference's Gridap.Algebra surface for the GMG path.

The reference's host language (Julia) is not available in this image, so the
layer a GridapSolvers user touches is mirrored here in Python with the same
names, argument meaning, defaults and error behaviour, on top of the C ABI
(include/gmg_amd.h).  The Julia binding of the same ABI lives in
julia/GridapSolversAMD.jl.

    reference (src/LinearSolvers)                      here
    ------------------------------------------------   ---------------------------
    JacobiLinearSolver()            JacobiLinearSolvers.jl:6        JacobiLinearSolver
    RichardsonSmoother(M,niter,w)   RichardsonSmoothers.jl:21-30    RichardsonSmoother
    PatchSolver / BlockJacobiSolver PatchBasedSmoothers/*.jl        PatchSolver / BlockJacobiSolver
    (none: an addition of the device library)                       ChebyshevSmoother(M, degree, ...)
    (none: SchwarzLinearSolvers.jl:3,13 names it as a TODO)         MultiplicativePatchSmoother(M, niter, omega, type, coloring)
    GMGLinearSolver(mats,P,R;...)   GMGLinearSolvers.jl:48-69       GMGLinearSolver
    CGSolver(Pl;...)                Krylov/CGSolvers.jl:19          CGSolver
    LanczosDiagnostic(n) / estimate!  Krylov/KrylovUtils.jl:58-90   LanczosDiagnostic / estimate_ (the replay of the device's trace)
    FGMRESSolver(m,Pr;...)          Krylov/FGMRESSolvers.jl:26      FGMRESSolver
    MINRESSolver(;Pl,...)           Krylov/MINRESSolvers.jl:16      MINRESSolver
    GMRESSolver(m;Pr,Pl,...)        Krylov/GMRESSolvers.jl:25       GMRESSolver
    BlockDiagonalSolver(blocks,solvers)   BlockSolvers/BlockDiagonalSolvers.jl:20-45     BlockDiagonalSolver
    BlockTriangularSolver(blocks,solvers,coeffs,half)  BlockTriangularSolvers.jl:55-85    BlockTriangularSolver
    SchurComplementSolver(A,B,C,S)  SchurComplementSolvers.jl:11-26 SchurComplementSolver (A, S = (solver, matrix) pairs)
    NullSpace(V) / NullspaceSolver(solver,N;constrain_matrix)  SolverInterfaces/NullSpaces.jl, NullspaceSolvers.jl:30-43   same names (f! = f_)
    LinearSystemBlock / NonlinearSystemBlock / MatrixBlock BlockSolvers/BlockSolverInterfaces.jl   same names
    symbolic_setup / numerical_setup / numerical_setup! / solve!    same names (solve_ = solve!)
    ConvergenceLog                  SolverInterfaces/ConvergenceLogs.jl:42   ConvergenceLog

All arithmetic happens in libgmgamd.so on the GPU.  Vectors may be numpy arrays
(host memory, copied in/out per call) or CUDA/HIP torch tensors (used in place).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time

import numpy as np

from . import abi

__all__ = [
    "JacobiLinearSolver", "RichardsonSmoother", "ChebyshevSmoother", "GaussSeidelSmoother", "SymGaussSeidelSmoother", "multicolor_order", "MultiplicativePatchSmoother", "patch_multicolor", "PatchSolver", "BlockJacobiSolver", "LUSolver",
    "GMGLinearSolver", "CGSolver", "LanczosDiagnostic", "estimate_", "FGMRESSolver", "MINRESSolver", "GMRESSolver", "ConvergenceLog", "PatchProlongationOperator",
    "RichardsonLinearSolver", "BlockDiagonalSolver", "BlockTriangularSolver", "SchurComplementSolver", "LinearSystemBlock", "NonlinearSystemBlock", "MatrixBlock", "LinearSolverFromSmoother",
    "NullSpace", "NullspaceSolver", "is_orthonormal", "is_orthogonal", "make_orthonormal_", "gram_schmidt_", "modified_gram_schmidt_",
    "project", "project_", "make_orthogonal_", "reconstruct", "reconstruct_",
    "symbolic_setup", "numerical_setup", "numerical_setup_", "solve_", "mul_",
    "SOLVER_CONVERGED_ATOL", "SOLVER_CONVERGED_RTOL", "SOLVER_DIVERGED_MAXITER", "SOLVER_DIVERGED_BREAKDOWN",
]

SOLVER_CONVERGED_ATOL, SOLVER_CONVERGED_RTOL, SOLVER_DIVERGED_MAXITER, SOLVER_DIVERGED_BREAKDOWN = 0, 1, 2, 3


# ----------------------------------------------------------------------------
# small solver description objects (constructors only hold parameters)
# ----------------------------------------------------------------------------
class JacobiLinearSolver:
    """struct JacobiLinearSolver <: LinearSolver (JacobiLinearSolvers.jl:6)."""


class LUSolver:
    """Gridap.Algebra.LUSolver(): the default coarsest_solver (GMGLinearSolvers.jl:54)."""


class HostCallbackSolver:
    """coarsest_solver implemented by the host language: `fn(r) -> x` on numpy vectors (GMG_COARSE_HOST_CALLBACK).
    In Julia this is an `@cfunction` around `solve!(x, ns_coarse, r)` of any Gridap LinearSolver."""

    def __init__(self, fn):
        self.fn = fn


class PatchSolver:
    """PatchBasedSmoothers.PatchSolver restricted to what reaches solve!: the
    patch dof tables (patch_rows == patch_cols for :star assembly) -- PatchSolvers.jl:18-54."""
    kind = abi.PATCH_LU

    def __init__(self, patch_ptr, patch_dofs, patch_cols=None, patch_mats=None, factors=None, pivots=None):
        """patch_dofs = patch_rows.  Optional, as held by the reference's PatchNS (PatchSolvers.jl:100-150):
        patch_cols (separate column table), patch_mats (the solver's own assembled patch matrices, column-major,
        concatenated) or factors (+ 1-based LAPACK pivots) = the output of lu!(patch_mat)."""
        self.patch_ptr = np.ascontiguousarray(patch_ptr, dtype=np.int64)
        self.patch_dofs = np.ascontiguousarray(patch_dofs, dtype=np.int32)
        if self.patch_ptr.ndim != 1 or self.patch_ptr.size < 1:
            raise ValueError("patch_ptr must have npatch+1 entries")
        self.patch_cols = None if patch_cols is None else np.ascontiguousarray(patch_cols, dtype=np.int32)
        if patch_mats is not None and factors is not None:
            raise ValueError("give patch_mats or factors, not both")
        self.patch_mats = None if patch_mats is None else np.ascontiguousarray(patch_mats, dtype=np.float64)
        self.factors = None if factors is None else np.ascontiguousarray(factors, dtype=np.float64)
        self.pivots = None if pivots is None else np.ascontiguousarray(pivots, dtype=np.int32)


class BlockJacobiSolver(PatchSolver):
    """BlockJacobiSolver(patch_rows, patch_cols) -- BlockJacobiSolvers.jl:2-16 (NoPivot LU, :162)."""
    kind = abi.PATCH_NOPIVOT


class PatchProlongationOperator:
    """PatchProlongationOperator (PatchTransferOperators.jl:2-60,153-172) reduced to what its mul! needs: the
    plain prolongation matrix P and the patch dof tables; y = P x - sum_p A_pp^-1 (A P x)_p."""

    def __init__(self, P, patch_ptr, patch_dofs, pivoting=True, rhs=None):
        """rhs: assembled rhs form of the local problems when it is not the level operator (StokesGMG.jl:125-127 passes graddiv)."""
        self.P = P
        self.rhs = rhs
        self.patch_ptr = np.ascontiguousarray(patch_ptr, dtype=np.int64)
        self.patch_dofs = np.ascontiguousarray(patch_dofs, dtype=np.int64)
        self.kind = abi.PATCH_LU if pivoting else abi.PATCH_NOPIVOT


class RichardsonSmoother:
    """RichardsonSmoother(M, niter=1, omega=1.0) -- RichardsonSmoothers.jl:21-30."""

    def __init__(self, M, niter=1, omega=1.0):
        if not isinstance(M, (JacobiLinearSolver, PatchSolver)):
            raise TypeError("RichardsonSmoother: M must be JacobiLinearSolver, PatchSolver or BlockJacobiSolver")
        self.M, self.niter, self.omega = M, int(niter), float(omega)


class ChebyshevSmoother:
    """ChebyshevSmoother(M, degree=3, lambda_max=None, lambda_min=None, eig_ratio=10.0, eig_safety=1.1, eig_steps=10,
    eig_method="power"): a Chebyshev
    polynomial of `degree` in M^-1 A where RichardsonSmoother(M, niter, omega) runs niter damped sweeps (gmg_set_smoother_chebyshev).
    No reference counterpart.  On partitioned handles: multigpu.DistributedGMG(..., chebyshev={...}).

    lambda_max given: the interval is [lambda_min, lambda_max], lambda_min defaulting to lambda_max / eig_ratio.  Otherwise the setup
    estimates lambda_max(M^-1 A) per level by eig_steps power steps and takes lambda_max = eig_safety * estimate (PETSc's
    convention); see GMGNumericalSetup.chebyshev_info.  A few power steps under-estimate a clustered top of the spectrum: pass
    lambda_max, raise eig_steps, or take eig_method="lanczos" where that matters: eig_steps steps of CG with preconditioner M from the
    same start vector, the estimate being the largest eigenvalue of the Lanczos tridiagonal CG builds (gmg_set_chebyshev_eig_method).
    At the same cost plus one dot per step it gives a much better top Ritz value (Jacobi on Q1 32^3, 10 steps: 1.455 against 1.336,
    true 1.494), so the default safety factor covers lambda_max.  The gain is a robust default interval, not a faster solve."""
    _EIG_METHODS = {"power": abi.CHEB_EIG_POWER, "lanczos": abi.CHEB_EIG_LANCZOS}

    def __init__(self, M, degree=3, lambda_max=None, lambda_min=None, eig_ratio=10.0, eig_safety=1.1, eig_steps=10, eig_method="power"):
        if not isinstance(M, (JacobiLinearSolver, PatchSolver)):
            raise TypeError("ChebyshevSmoother: M must be JacobiLinearSolver, PatchSolver or BlockJacobiSolver")
        if not int(degree) >= 1:
            raise ValueError("The degree must be a positive integer.")
        if lambda_max is not None and not float(lambda_max) > 0.0:
            raise ValueError("lambda_max must be a positive real number (or None: estimated by the setup).")
        if lambda_min is not None and not float(lambda_min) > 0.0:
            raise ValueError("lambda_min must be a positive real number (or None: lambda_max / eig_ratio).")
        if lambda_max is not None and lambda_min is not None and not float(lambda_min) < float(lambda_max):
            raise ValueError("lambda_min must be smaller than lambda_max.")
        if not float(eig_ratio) > 1.0:
            raise ValueError("eig_ratio must be greater than 1.")
        if not float(eig_safety) >= 1.0:
            raise ValueError("eig_safety must be at least 1.")
        if not int(eig_steps) >= 1:
            raise ValueError("eig_steps must be a positive integer.")
        if eig_method not in self._EIG_METHODS:
            raise ValueError('eig_method must be "power" or "lanczos".')
        self.eig_method = eig_method
        self.M, self.degree = M, int(degree)
        self.lambda_max = None if lambda_max is None else float(lambda_max)
        self.lambda_min = None if lambda_min is None else float(lambda_min)
        self.eig_ratio, self.eig_safety, self.eig_steps = float(eig_ratio), float(eig_safety), int(eig_steps)


class GaussSeidelSmoother:
    """GaussSeidelSmoother(niter=1, omega=1.0, type=:symmetric) -- SymGaussSeidelSmoothers.jl:105-118.

    ordering: the visiting order of the sweeps on the smoother's level (gmg_set_gs_ordering) -- "natural" (the reference's), "multicolor"
    (greedy first-fit colouring of the symmetrised stored pattern, rows sorted stably by colour) or a 1-D integer array: order[k] is the
    row the forward sweep visits k-th.  One order per level: pre- and post-smoother of a level must name the same."""
    _TYPES = {"symmetric": abi.GS_SYMMETRIC, "forward": abi.GS_FORWARD, "backward": abi.GS_BACKWARD}
    _ORDERINGS = {"natural": abi.GS_ORDER_NATURAL, "multicolor": abi.GS_ORDER_MULTICOLOR}

    def __init__(self, niter=1, omega=1.0, type="symmetric", ordering="natural"):
        if type not in self._TYPES:
            raise ValueError("The type must be :symmetric, :forward or :backward.")
        if not int(niter) > 0:
            raise ValueError("The number of iterations must be a positive integer.")
        if not float(omega) > 0.0:
            raise ValueError("The relaxation parameter must be a positive real number.")
        self.niter, self.omega, self.type = int(niter), float(omega), type
        self.ordering = self._check_ordering(ordering)

    @classmethod
    def _check_ordering(cls, ordering):
        if isinstance(ordering, str):
            if ordering not in cls._ORDERINGS:
                raise ValueError('The ordering must be "natural", "multicolor" or a 1-D integer array.')
            return ordering
        if isinstance(ordering, (bytes, dict, set)) or ordering is None:
            raise ValueError('The ordering must be "natural", "multicolor" or a 1-D integer array.')
        a = np.asarray(ordering)
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
            raise ValueError('The ordering must be "natural", "multicolor" or a 1-D integer array.')
        return np.ascontiguousarray(a, dtype=np.int32)

    def _same_ordering(self, other):
        a, b = self.ordering, other.ordering
        if isinstance(a, str) or isinstance(b, str):
            return isinstance(a, str) and isinstance(b, str) and a == b
        return np.array_equal(a, b)


def SymGaussSeidelSmoother(niter=1, omega=1.0, ordering="natural"):
    """SymGaussSeidelSmoother(niter, omega) = GaussSeidelSmoother(niter, omega, :symmetric) -- SymGaussSeidelSmoothers.jl:121."""
    return GaussSeidelSmoother(niter, omega, "symmetric", ordering)


def multicolor_order(A):
    """gmg_gs_multicolor_order on the stored pattern of a square matrix (poisson.CSR, scipy CSR, ...; explicit zeros count) ->
    (order, color): the visiting order ordering="multicolor" uses and the colour of every row.  Host only: no handle, no GPU."""
    shape, ptr, idx, _val, layout, base = _csr_fields(A)
    if shape[0] != shape[1]:
        raise ValueError("multicolor_order: the matrix must be square")
    # (the colouring symmetrises the pattern, so a CSC pattern gives the same answer as its CSR form)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64) - base
    idx = np.ascontiguousarray(idx, dtype=np.int32) - np.int32(base)
    n = int(shape[0])
    order, color, nc = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), C.c_int64(0)
    abi.check(None, abi.load().gmg_gs_multicolor_order(n, C.c_void_p(ptr.ctypes.data), C.c_void_p(idx.ctypes.data),
                                                       C.c_void_p(order.ctypes.data), C.c_void_p(color.ctypes.data), C.byref(nc)))
    return order, color


class MultiplicativePatchSmoother:
    """MultiplicativePatchSmoother(M, niter=1, omega=1.0, type="symmetric", coloring="greedy"): block Gauss-Seidel over the patches of
    M = PatchSolver / BlockJacobiSolver (multiplicative Schwarz, Vanka), swept colour by colour on the device
    (gmg_set_smoother_patch_multiplicative).  The reference has the additive patch solver only (SchwarzLinearSolvers.jl:3,13: TODO).

    One pass: dx = 0; niter times, forward over the colours (types forward, symmetric) and backward (backward, symmetric), every patch p
    solves its block against the fresh residual (r - A dx)[rows_p] and adds omega times the result to dx[rows_p]; x += dx; r -= A dx.
    No damping parameter has to be found: omega = 1 is the method.

    coloring: "greedy" (first-fit in patch order; patches of one colour share no dof and no stored entry of A couples them) or a 1-D
    integer array with the colour (>= 0) of every patch, which the setup validates.  GMGNumericalSetup.patch_coloring reports it.
    One GPU, patch_cols == patch_rows, a level matrix handed over whole."""
    _TYPES = {"symmetric": abi.PMULT_SYMMETRIC, "forward": abi.PMULT_FORWARD, "backward": abi.PMULT_BACKWARD}

    def __init__(self, M, niter=1, omega=1.0, type="symmetric", coloring="greedy"):
        if not isinstance(M, PatchSolver):
            raise TypeError("MultiplicativePatchSmoother: M must be PatchSolver or BlockJacobiSolver")
        if type not in self._TYPES:
            raise ValueError("The type must be :symmetric, :forward or :backward.")
        if not int(niter) > 0:
            raise ValueError("The number of iterations must be a positive integer.")
        if not float(omega) > 0.0:
            raise ValueError("The relaxation parameter must be a positive real number.")
        self.M, self.niter, self.omega, self.type = M, int(niter), float(omega), type
        self.coloring = self._check_coloring(coloring, M.patch_ptr.size - 1)

    @staticmethod
    def _check_coloring(coloring, npatch):
        msg = 'The coloring must be "greedy" or a 1-D integer array with one colour >= 0 per patch.'
        if isinstance(coloring, str):
            if coloring != "greedy":
                raise ValueError(msg)
            return coloring
        if isinstance(coloring, (bytes, dict, set)) or coloring is None:
            raise ValueError(msg)
        a = np.asarray(coloring)
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < 0 or a.max() >= 2 ** 31)):
            raise ValueError(msg)
        if a.size != npatch:
            raise ValueError("The coloring has %d entries, M has %d patches." % (a.size, npatch))
        return np.ascontiguousarray(a, dtype=np.int32)


def patch_multicolor(A, patch_ptr, patch_dofs):
    """gmg_patch_multicolor on the stored pattern of a square matrix (poisson.CSR, scipy CSR, ...; explicit zeros count) and a patch
    table -> (color, ncolors): the colouring coloring="greedy" uses.  Host only: no handle, no GPU."""
    shape, ptr, idx, _val, layout, base = _csr_fields(A)
    if shape[0] != shape[1]:
        raise ValueError("patch_multicolor: the matrix must be square")
    # (the conflict rule symmetrises the pattern, so a CSC pattern gives the same answer as its CSR form)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64) - base
    idx = np.ascontiguousarray(idx, dtype=np.int32) - np.int32(base)
    pp = np.ascontiguousarray(patch_ptr, dtype=np.int64)
    pd = np.ascontiguousarray(patch_dofs, dtype=np.int32)
    if pp.ndim != 1 or pp.size < 1:
        raise ValueError("patch_ptr must have npatch+1 entries")
    color, nc = np.empty(pp.size - 1, dtype=np.int32), C.c_int64(0)
    abi.check(None, abi.load().gmg_patch_multicolor(int(shape[0]), C.c_void_p(ptr.ctypes.data), C.c_void_p(idx.ctypes.data), pp.size - 1,
                                                    C.c_void_p(pp.ctypes.data), C.c_void_p(pd.ctypes.data), C.c_void_p(color.ctypes.data),
                                                    C.byref(nc)))
    return color, nc.value


class Galerkin:
    """Galerkin(): marker for an entry of smatrices[1:] -- the matrix of that level is R (A P) of the finer level, formed on the device
    at the numerical setup (gmg_set_galerkin) instead of being assembled by the caller:
        GMGLinearSolver([A0, Galerkin(), Galerkin()], interp, restrict, ...)
    The reference has the caller's matrices only (GMGLinearSolverFromMatrices, GMGLinearSolvers.jl:336-340).  One GPU; the finer
    level's operators handed over whole.  GMGNumericalSetup.level_matrix(lev) returns the product."""

    def __repr__(self):
        return "Galerkin()"


class Aggregation:
    """Aggregation(theta=0.25, smooth=True, omega=None, seed=0): marker for an entry of interp -- the prolongation of that level is built
    on the device from the level's matrix by smoothed aggregation at the numerical setup (gmg_set_aggregation); the next entry of
    smatrices must be Galerkin():
        GMGLinearSolver([A0, Galerkin(), Galerkin()], [Aggregation(), Aggregation()])
    theta: strength threshold against the largest off-diagonal entry of the row; smooth=False: the tentative (piecewise constant)
    prolongation; omega=None: (4/3) / the infinity-norm bound of D^-1 A; seed: of the priorities of the independent set.  The reference
    has the caller's transfers only.  One GPU; constant near-null space.  GMGNumericalSetup.aggregates / prolongation / aggregation_info
    return what was built."""

    def __init__(self, theta=0.25, smooth=True, omega=None, seed=0):
        if not 0.0 <= float(theta) <= 1.0:
            raise ValueError("theta must lie in [0, 1]")
        if omega is not None and not float(omega) > 0.0:
            raise ValueError("omega must be positive (None: automatic)")
        if int(seed) < 0:
            raise ValueError("seed must not be negative")
        self.theta, self.smooth, self.omega, self.seed = float(theta), bool(smooth), None if omega is None else float(omega), int(seed)

    def __repr__(self):
        return f"Aggregation(theta={self.theta}, smooth={self.smooth}, omega={self.omega}, seed={self.seed})"


def _level_size(smatrices, interp, l):
    """rows of level l: of its matrix, or, for a Galerkin level, the columns of the prolongation onto the finer level; None (unknown
    until the setup) where that prolongation is an Aggregation()"""
    if not isinstance(smatrices[l], Galerkin):
        return int(smatrices[l].shape[0])
    ip = interp[l - 1]
    if isinstance(ip, Aggregation):
        return None
    return int((ip.P if isinstance(ip, PatchProlongationOperator) else ip).shape[1])


def _is_patch_smoother(sm):
    if isinstance(sm, (ChebyshevSmoother, MultiplicativePatchSmoother)):
        return not isinstance(sm.M, JacobiLinearSolver)
    return isinstance(sm, RichardsonSmoother) and not isinstance(sm.M, JacobiLinearSolver)


def galerkin_pattern(R, A, P):
    """gmg_galerkin_pattern on the stored patterns of R (nc x nf), A (nf x nf), P (nf x nc) (poisson.CSR, scipy CSR, ...; explicit zeros
    count, rows in any order) -> ((tptr, tcol), (cptr, ccol)): the patterns of T = A P and of R A P, columns ascending, as the
    symbolic phase of a Galerkin level builds them.  Host only: no handle, no GPU."""
    pats = []
    for M in (R, A, P):
        shape, ptr, idx, _val, layout, base = _csr_fields(M)
        if layout != abi.CSR:
            raise ValueError("galerkin_pattern: CSR operands")
        pats.append((shape, np.ascontiguousarray(ptr, dtype=np.int64) - base, np.ascontiguousarray(idx, dtype=np.int32) - np.int32(base)))
    (rs, rp, rc), (as_, ap, ac), (ps, pp, pc) = pats
    nc, nf = int(rs[0]), int(as_[0])
    if not (as_[0] == as_[1] == rs[1] == ps[0] and ps[1] == nc):
        raise ValueError("galerkin_pattern: the shapes of R, A and P do not chain to a square matrix")
    lib = abi.load()
    args = [nc, nf] + [C.c_void_p(a.ctypes.data) for a in (rp, rc, ap, ac, pp, pc)]
    tn, cn = C.c_int64(0), C.c_int64(0)
    abi.check(None, lib.gmg_galerkin_pattern(*args, None, None, 0, C.byref(tn), None, None, 0, C.byref(cn)))
    tptr, tcol = np.empty(nf + 1, dtype=np.int64), np.empty(tn.value, dtype=np.int32)
    cptr, ccol = np.empty(nc + 1, dtype=np.int64), np.empty(cn.value, dtype=np.int32)
    abi.check(None, lib.gmg_galerkin_pattern(*args, C.c_void_p(tptr.ctypes.data), C.c_void_p(tcol.ctypes.data), tn.value, C.byref(tn),
                                             C.c_void_p(cptr.ctypes.data), C.c_void_p(ccol.ctypes.data), cn.value, C.byref(cn)))
    return (tptr, tcol), (cptr, ccol)


class LinearSolverFromSmoother:
    """LinearSolverFromSmoother(smoother) -- LinearSolverFromSmoothers.jl:2-4: x = 0; r = copy(b); solve!(x,smoother,r)."""

    def __init__(self, smoother):
        if not isinstance(smoother, (RichardsonSmoother, GaussSeidelSmoother, ChebyshevSmoother, MultiplicativePatchSmoother)):
            raise TypeError("smoother must be a RichardsonSmoother, a GaussSeidelSmoother, a ChebyshevSmoother or a MultiplicativePatchSmoother")
        self.smoother = smoother


class ConvergenceLog:
    """ConvergenceLog{Float64}: name, tols, num_iters, residuals (ConvergenceLogs.jl:42-60)."""

    def __init__(self, name, maxiter, atol, rtol):
        self.name, self.maxiter, self.atol, self.rtol = name, int(maxiter), float(atol), float(rtol)
        self.num_iters = 0
        self.residuals = np.zeros(self.maxiter + 1)
        self.flag = None

    def _fill(self, res, hist):
        self.num_iters = int(res.niters)
        self.residuals[:] = 0.0
        self.residuals[: self.num_iters + 1] = hist[: self.num_iters + 1]
        self.flag = int(res.flag)

    def summary(self):
        r = self.residuals[self.num_iters]
        return (f"Convergence[{self.name}]: conv_flag={self.flag}, niter={self.num_iters}, "
                f"r_abs={r}, r_rel={r / self.residuals[0] if self.residuals[0] else float('nan')}")


_MODES = {"preconditioner": abi.MODE_PRECONDITIONER, "solver": abi.MODE_SOLVER}
_CYCLES = {"v_cycle": abi.V_CYCLE, "w_cycle": abi.W_CYCLE, "f_cycle": abi.F_CYCLE}
_CYCLE_VALUES = ("float64", "float32")


class GMGLinearSolver:
    """GMGLinearSolver(smatrices, interp, restrict; pre_smoothers, post_smoothers,
    coarsest_solver, mode, cycle_type, maxiter, atol, rtol) -- GMGLinearSolvers.jl:48-69.

    smatrices / interp / restrict are sequences of CSR-like objects with fields
    (shape, ptr, idx, val), 0-based (e.g. poisson.CSR or scipy.sparse.csr_matrix
    via `from_scipy`).  restrict=None means R = P^T (the :residual-mode transfer of
    GridTransferOperators.jl:202-209 on nested meshes).  An entry of smatrices[1:] may be Galerkin(): that level's matrix is
    R (A P) of the finer level, formed on the device.

    cycle_values (no reference counterpart): "float64" (default) or "float32".  With "float32" the cycle streams the matrices of the
    levels stored as SELL-64 / SELL-O from float32 copies: the preconditioner is exactly the fp64 cycle on the matrices rounded to
    float32, while the Krylov solver around it keeps A in fp64 (include/gmg_amd.h, gmg_level_values).  Preconditioner mode only."""

    def __init__(self, smatrices, interp, restrict=None, pre_smoothers=None, post_smoothers=None,
                 coarsest_solver=None, mode="preconditioner", cycle_type="v_cycle",
                 maxiter=100, atol=1.0e-14, rtol=1.0e-8, verbose=False, options=None, pin_vectors=False, cycle_values="float64"):
        nlev = len(smatrices)
        if pre_smoothers is None:  # Fill(RichardsonSmoother(JacobiLinearSolver(),10),nlev-1)
            pre_smoothers = [RichardsonSmoother(JacobiLinearSolver(), 10) for _ in range(nlev - 1)]
        if post_smoothers is None:
            post_smoothers = pre_smoothers
        if restrict is None:
            restrict = [None] * (nlev - 1)
        # @check length(smatrices)-1 == length(interp) == ... (GMGLinearSolvers.jl:59)
        if not (nlev - 1 == len(interp) == len(restrict) == len(pre_smoothers) == len(post_smoothers)):
            raise ValueError("length(smatrices)-1 must equal the number of transfer operators and smoothers")
        if nlev and isinstance(smatrices[0], Galerkin):
            raise ValueError("smatrices[0]: the finest level has no finer level to form a Galerkin product from")
        if mode not in _MODES:          # :60
            raise ValueError("mode must be 'preconditioner' or 'solver'")
        if cycle_type not in _CYCLES:   # :61
            raise ValueError("cycle_type must be 'v_cycle', 'w_cycle' or 'f_cycle'")
        if cycle_values not in _CYCLE_VALUES:
            raise ValueError("cycle_values must be 'float64' or 'float32'")
        if cycle_values == "float32":
            # what gmg_setup refuses and this constructor can already see
            if mode != "preconditioner":
                raise ValueError("cycle_values='float32' needs mode='preconditioner': as a solver the cycle would converge to the solution "
                                 "of the rounded system")
            if any(isinstance(A, Galerkin) for A in smatrices):
                raise ValueError("cycle_values='float32' does not take a Galerkin() level")
            if any(isinstance(ip, PatchProlongationOperator) for ip in interp):
                raise ValueError("cycle_values='float32' does not take a PatchProlongationOperator")
        # Aggregation() entries of interp: what gmg_setup refuses and this constructor can already see
        for l, ip in enumerate(interp):
            if not isinstance(ip, Aggregation):
                continue
            if not isinstance(smatrices[l + 1], Galerkin):
                raise ValueError(f"interp[{l}] is Aggregation(): smatrices[{l + 1}] must be Galerkin(), a matrix of the caller's cannot "
                                 f"match the aggregates of level {l}")
            if restrict[l] is not None:
                raise ValueError(f"interp[{l}] is Aggregation(): level {l} takes no explicit restriction (restrict[{l}]), R = P^T")
            if hasattr(smatrices[l], "row_blocks"):
                raise ValueError(f"interp[{l}] is Aggregation(): the matrix of level {l} is streamed, the aggregation needs its rows")
            if l + 1 < nlev - 1:
                if _is_patch_smoother(pre_smoothers[l + 1]) or _is_patch_smoother(post_smoothers[l + 1]):
                    raise ValueError(f"level {l + 1} takes its size from the aggregation of level {l}: a patch-based smoother there is "
                                     f"refused, its tables cannot match")
                if isinstance(interp[l + 1], PatchProlongationOperator):
                    raise ValueError(f"level {l + 1} takes its size from the aggregation of level {l}: a PatchProlongationOperator there "
                                     f"is refused, its tables cannot match")
        # coarsest_solver: LUSolver() (default, GMGLinearSolvers.jl:54), CGSolver(JacobiLinearSolver();...) on the device, or any
        # host-side solver wrapped in HostCallbackSolver (the analogue of passing PETSc / UMFPACK objects in Julia)
        if isinstance(coarsest_solver, NullspaceSolver):
            # NullspaceSolver(LUSolver(), N_coarse): the :constrained mode (NullspaceSolvers.jl:59-107) inside the dense coarsest solve
            if not (coarsest_solver.constrain_matrix and isinstance(coarsest_solver.solver, LUSolver)):
                raise NotImplementedError("coarsest_solver: NullspaceSolver(LUSolver(), N_coarse) with constrain_matrix=True "
                                          "(an iterative coarsest solver needs no constraint: CGSolver(JacobiLinearSolver()))")
            if _level_size(smatrices, interp, nlev - 1) is None:
                raise ValueError(f"coarsest_solver: a null space cannot be given for level {nlev - 1}, whose size comes from an Aggregation()")
            if coarsest_solver.nullspace.size()[1] != _level_size(smatrices, interp, nlev - 1):
                raise ValueError(f"coarsest_solver: the null space has vectors of length {coarsest_solver.nullspace.size()[1]}, "
                                 f"the coarsest matrix {_level_size(smatrices, interp, nlev - 1)} rows")
        elif coarsest_solver is not None and not isinstance(coarsest_solver, (LUSolver, HostCallbackSolver)):
            if not (isinstance(coarsest_solver, CGSolver) and isinstance(coarsest_solver.Pl, JacobiLinearSolver)
                    and not coarsest_solver.flexible):
                raise NotImplementedError("coarsest_solver on the device: LUSolver(), CGSolver(JacobiLinearSolver()) or HostCallbackSolver(fn)")
        self.coarsest_solver = coarsest_solver
        self.smatrices, self.interp, self.restrict = list(smatrices), list(interp), list(restrict)
        self.pre_smoothers, self.post_smoothers = list(pre_smoothers), list(post_smoothers)
        self.mode, self.cycle_type = mode, cycle_type
        self.cycle_values = cycle_values
        self.verbose = int(verbose)
        self.log = ConvergenceLog("GMG", maxiter, atol, rtol)
        # device-side policy (no reference counterpart): `options` = {key: number} handed to gmg_set_option before the operators are
        # set (storage layout, sweep kernels, one-launch passes, x0_zero, ...; keys in include/gmg_amd.h); `pin_vectors` = the
        # numerical setup page-locks the host vectors it is called with, once (the pattern of ext/GridapPETScExt/PETScCaches.jl:23-36)
        self.options = dict(options or {})
        self.pin_vectors = bool(pin_vectors)

    def num_levels(self):
        return len(self.smatrices)


class LanczosDiagnostic:
    """LanczosDiagnostic(max_iters) -- KrylovUtils.jl:58-81: the Lanczos tridiagonal that CG builds as a by-product, diagonal `delta`
    and off-diagonal `gamma` (gamma[0] unused), `k` entries filled.  Pass it as CGSolver(..., diagnostic=...); estimate_ turns it
    into a condition-number estimate of the preconditioned operator."""

    def __init__(self, max_iters):
        if not int(max_iters) >= 0:
            raise ValueError("max_iters must not be negative.")
        self.k = 0
        self.delta = np.zeros(int(max_iters))
        self.gamma = np.zeros(int(max_iters))

    def reset_(self):
        """reset! (KrylovUtils.jl:69-74)"""
        self.k = 0
        self.delta[:] = 0.0
        self.gamma[:] = 0.0
        return self

    def update_(self, delta, gamma):
        """update! (KrylovUtils.jl:76-81)"""
        self.k += 1
        self.delta[self.k - 1] = delta
        self.gamma[self.k - 1] = gamma
        return self

    def replay_(self, alpha, beta):
        """what solve! does to the diagnostic (CGSolvers.jl:87,114-115,128-138) for the recorded alpha_k, beta_k, in double and in the
        reference's order of operations.  VERBATIM the reference: the off-diagonal is sqrt(beta_k)/alpha_k where the textbook Lanczos
        matrix has sqrt(beta_k)/alpha_{k-1}.  A negative beta_k (flexible=True or an indefinite Pl only) stores NaN."""
        self.reset_()                                          # :87
        alpha_last = 1.0                                       # :83
        for ak, bk in zip(np.asarray(alpha, dtype=np.float64).tolist(), np.asarray(beta, dtype=np.float64).tolist()):
            if self.k == 0:                                    # :130-132
                d, g = 1.0 / ak, 0.0
            else:                                              # :134-135
                d = (1.0 / ak) + (bk / alpha_last)
                g = (math.sqrt(bk) if bk >= 0.0 else math.nan) / ak
            self.update_(d, g)                                 # :137
            alpha_last = ak                                    # :115
        return self


def estimate_(diag):
    """estimate! (KrylovUtils.jl:83-90): |lambda_max / lambda_min| of the symmetric tridiagonal (delta[0:k], gamma[1:k]); 1.0 for k < 2."""
    k = diag.k
    if k < 2:
        return 1.0
    T = np.diag(diag.delta[:k]) + np.diag(diag.gamma[1:k], 1) + np.diag(diag.gamma[1:k], -1)
    lam = np.linalg.eigvalsh(T)
    return abs(lam.max() / lam.min())


class CGSolver:
    """CGSolver(Pl; maxiter=1000, atol=1e-12, rtol=1e-6, diagnostic=nothing, flexible=false) -- CGSolvers.jl:19.

    diagnostic: a LanczosDiagnostic.  The device records alpha_k and beta_k of the solve (gmg_cg_set_trace, allocated by
    numerical_setup); solve_ fetches them and replays CGSolvers.jl:87,114-115,128-138 on the host, so that afterwards
    diagnostic.k == log.num_iters.  The reference would hit a BoundsError in the iteration that outgrows the diagnostic; here
    numerical_setup refuses max_iters < maxiter with a ValueError before any work."""

    def __init__(self, Pl=None, maxiter=1000, atol=1e-12, rtol=1.0e-6, flexible=False, verbose=0, name="CG", diagnostic=None):
        if diagnostic is not None and not isinstance(diagnostic, LanczosDiagnostic):
            raise TypeError("diagnostic must be a LanczosDiagnostic (or None)")
        self.Pl, self.flexible = Pl, bool(flexible)
        self.diag = diagnostic
        self.log = ConvergenceLog(name, maxiter, atol, rtol)


class RichardsonLinearSolver:
    """RichardsonLinearSolver(omega, maxiter; Pl=nothing, rtol=1e-10, atol=1e-6) -- RichardsonLinearSolvers.jl:13-23
    (scalar omega on the device path)."""

    def __init__(self, omega, maxiter, Pl=None, rtol=1e-10, atol=1e-6, verbose=True, name="RichardsonLinearSolver"):
        if not np.isscalar(omega):
            raise NotImplementedError("vector-valued omega is not on the device path")
        self.omega, self.Pl = float(omega), Pl
        self.log = ConvergenceLog(name, maxiter, atol, rtol)


class FGMRESSolver:
    """FGMRESSolver(m, Pr; Pl=nothing, restart=false, m_add=1, maxiter=100, atol=1e-12,
    rtol=1e-6) -- FGMRESSolvers.jl:26."""

    def __init__(self, m, Pr, Pl=None, restart=False, m_add=1, maxiter=100, atol=1e-12, rtol=1.0e-6,
                 verbose=False, name="FGMRES"):
        # Pl (KrylovUtils.jl:14-18,46-50): None | JacobiLinearSolver() | LinearSolverFromSmoother(finest pre-smoother) on the
        # matrix of Pr's handle; the GMG itself serves on one side only
        if Pl is not None and not isinstance(Pl, (JacobiLinearSolver, LinearSolverFromSmoother)):
            raise NotImplementedError("FGMRES Pl on the device: JacobiLinearSolver() or LinearSolverFromSmoother(...)")
        self.Pl = Pl
        self.m, self.Pr, self.restart, self.m_add = int(m), Pr, bool(restart), int(m_add)
        self.log = ConvergenceLog(name, maxiter, atol, rtol)


class MINRESSolver:
    """MINRESSolver(; Pl=nothing, maxiter=1000, atol=1e-12, rtol=1e-6) -- MINRESSolvers.jl:16.  Pl must be symmetric positive
    definite (the reference's docstring): a GMGLinearSolver, (None | JacobiLinearSolver() | LinearSolverFromSmoother, gmg) as for
    CGSolver, or a BlockDiagonalSolver (a BlockTriangularSolver is accepted, as by the reference, but is outside MINRES's
    assumptions)."""

    def __init__(self, Pl=None, maxiter=1000, atol=1e-12, rtol=1.0e-6, verbose=0, name="MINRES"):
        self.Pl = Pl
        self.log = ConvergenceLog(name, maxiter, atol, rtol)


class GMRESSolver:
    """GMRESSolver(m; Pr=nothing, Pl=nothing, restart=false, m_add=1, maxiter=100, atol=1e-12, rtol=1e-6) --
    GMRESSolvers.jl:25.  Each side is None, a GMGLinearSolver, a BlockDiagonalSolver / BlockTriangularSolver / SchurComplementSolver, or the tuple
    (None | JacobiLinearSolver() | LinearSolverFromSmoother(finest pre-smoother), gmg) that CGSolver and MINRESSolver accept for
    "the matrix of this handle, but not its GMG"; (None, block_solver) names a block system without preconditioning it.  Both
    sides live on one handle, and its GMG (or block preconditioner) serves on one side only.  At least one side must name the
    handle: GMRESSolver(10, Pr=(None, gmg)) is the unpreconditioned solver on gmg's finest matrix."""

    def __init__(self, m, Pr=None, Pl=None, restart=False, m_add=1, maxiter=100, atol=1e-12, rtol=1.0e-6,
                 verbose=False, name="GMRES"):
        self.m, self.Pr, self.Pl, self.restart, self.m_add = int(m), Pr, Pl, bool(restart), int(m_add)
        self.log = ConvergenceLog(name, maxiter, atol, rtol)


class LinearSystemBlock:
    """LinearSystemBlock(): the block is taken from the system matrix (BlockSolverInterfaces.jl)."""


class NonlinearSystemBlock(LinearSystemBlock):
    """NonlinearSystemBlock(ids=()) -- BlockSolverInterfaces.jl:206-214: a block taken from the system matrix whose solver is set
    up again by numerical_setup!(ns, A, x) (:232-236); a LinearSystemBlock keeps its first set-up (:104-109).  `ids` names the
    blocks of x the block depends on (the reference's `I`); the device takes assembled matrices, so it is stored only."""

    def __init__(self, ids=()):
        self.ids = tuple(ids) if isinstance(ids, (tuple, list)) else (ids,)


class MatrixBlock:
    """MatrixBlock(mat): an explicit matrix (also what a BiformBlock assembles to)."""

    def __init__(self, mat):
        self.mat = mat


class BlockDiagonalSolver:
    """BlockDiagonalSolver(blocks, solvers) / BlockDiagonalSolver(solvers) -- BlockDiagonalSolvers.jl:20-45.
    solvers[i]: GMGLinearSolver | CGSolver(JacobiLinearSolver()) | LUSolver() | JacobiLinearSolver() | a Krylov solver around a
    GMGLinearSolver: FGMRESSolver(m, gmg) | GMRESSolver(m, Pr=gmg) | GMRESSolver(m, Pl=gmg) | CGSolver(gmg, flexible=...)."""

    half = "diagonal"

    def __init__(self, blocks, solvers=None):
        if solvers is None:
            blocks, solvers = None, blocks
        self.solvers = list(solvers)
        for sv in self.solvers:
            _krylov_gmg_spec(sv)               # NotImplementedError: a Krylov solver around something that is not a GMG
        nb = len(self.solvers)
        diag = [LinearSystemBlock() for _ in range(nb)] if blocks is None else list(blocks)
        if len(diag) != nb:
            raise ValueError("blocks and solvers must have the same length")   # @check :27
        self.blocks = [[diag[i] if i == j else LinearSystemBlock() for j in range(nb)] for i in range(nb)]
        self.coeffs = np.ones((nb, nb))


class BlockTriangularSolver:
    """BlockTriangularSolver(blocks, solvers, coeffs=fill(1.0,size(blocks)), half=:upper) /
    BlockTriangularSolver(solvers; coeffs, half) -- BlockTriangularSolvers.jl:55-85."""

    def __init__(self, blocks, solvers=None, coeffs=None, half="upper"):
        if solvers is None:
            blocks, solvers = None, blocks
        self.solvers = list(solvers)
        for sv in self.solvers:
            _krylov_gmg_spec(sv)               # NotImplementedError: a Krylov solver around something that is not a GMG
        nb = len(self.solvers)
        if blocks is None:
            blocks = [[LinearSystemBlock() for _ in range(nb)] for _ in range(nb)]
        self.blocks = [list(row) for row in blocks]
        if len(self.blocks) != nb or any(len(r) != nb for r in self.blocks):
            raise ValueError("blocks must be a square matrix matching solvers")  # @check :63-64
        if half not in ("upper", "lower"):
            raise ValueError("half must be :upper or :lower")                     # @check :65
        self.coeffs = np.ones((nb, nb)) if coeffs is None else np.asarray(coeffs, dtype=np.float64)
        if self.coeffs.shape != (nb, nb):
            raise ValueError("coeffs must match blocks")
        self.half = half


_KRYLOV_GMG_FORMS = ("a Krylov solver on a diagonal block wraps a GMGLinearSolver: FGMRESSolver(m, gmg) (Pl=None), "
                     "GMRESSolver(m, Pr=gmg) or GMRESSolver(m, Pl=gmg) (one side), CGSolver(gmg, flexible=...); "
                     "or CGSolver(JacobiLinearSolver())")


def _krylov_gmg_spec(sv):
    """FGMRESSolver(m, gmg) | GMRESSolver(m, Pr=gmg) | GMRESSolver(m, Pl=gmg) | CGSolver(gmg) as a diagonal-block solver
    (test/Applications/NavierStokesGMG.jl:159-169) -> (gmg, krylov, m, restart, m_add, flexible, side) for
    gmg_block_set_diag_krylov_gmg.  None: not one of these solvers, or one without any preconditioner (never a block solver);
    NotImplementedError: a Krylov solver around something the device cannot nest."""
    if isinstance(sv, FGMRESSolver):
        if sv.Pr is None and sv.Pl is None:
            return None
        if sv.Pl is not None or not isinstance(sv.Pr, GMGLinearSolver):
            raise NotImplementedError(_KRYLOV_GMG_FORMS)
        return sv.Pr, abi.KRYLOV_FGMRES, sv.m, sv.restart, sv.m_add, False, 0
    if isinstance(sv, GMRESSolver):
        if sv.Pr is None and sv.Pl is None:
            return None
        if sv.Pr is not None and sv.Pl is not None:
            raise NotImplementedError(_KRYLOV_GMG_FORMS)
        P, side = (sv.Pr, 0) if sv.Pr is not None else (sv.Pl, 1)
        if not isinstance(P, GMGLinearSolver):
            raise NotImplementedError(_KRYLOV_GMG_FORMS)
        return P, abi.KRYLOV_GMRES, sv.m, sv.restart, sv.m_add, False, side
    if isinstance(sv, CGSolver):
        if sv.Pl is None or isinstance(sv.Pl, JacobiLinearSolver):
            return None
        if not isinstance(sv.Pl, GMGLinearSolver):
            raise NotImplementedError(_KRYLOV_GMG_FORMS)
        return sv.Pl, abi.KRYLOV_CG, 1, False, 1, sv.flexible, 1
    return None


def _is_block_diag_solver(sv):
    """what BlockNumericalSetup can put on a diagonal block"""
    return isinstance(sv, (GMGLinearSolver, LUSolver, JacobiLinearSolver)) or \
        (isinstance(sv, CGSolver) and isinstance(sv.Pl, JacobiLinearSolver) and not sv.flexible) or \
        _krylov_gmg_spec(sv) is not None


class SchurComplementSolver:
    """SchurComplementSolver(A, B, C, S) -- SchurComplementSolvers.jl:11-26: the block factorisation of [A B; C D] with
    S ~ D - C A^-1 B (solve!: :55-74).  The reference receives A and S as numerical setups; here each is the pair
    (solver, matrix) that stands for numerical_setup(symbolic_setup(solver, matrix), matrix), with solver one of
    GMGLinearSolver | CGSolver(JacobiLinearSolver()) | LUSolver() | JacobiLinearSolver() | FGMRESSolver(m, gmg) |
    GMRESSolver(m, Pr=gmg) | GMRESSolver(m, Pl=gmg) | CGSolver(gmg); matrix may be None for a GMGLinearSolver or a Krylov
    solver around one (the GMG's own smatrices[0]).  B and C are CSR-like matrices of shape (n_A, n_S) and (n_S, n_A).
    The matrix given to numerical_setup (2 x 2 nested) serves mul! and the outer Krylov residual only, as in the reference."""

    half = "schur"

    def __init__(self, A, B, C, S):
        sizes = []
        for name, pair in (("A", A), ("S", S)):
            if not (isinstance(pair, (tuple, list)) and len(pair) == 2):
                raise TypeError(f"SchurComplementSolver: {name} must be a (solver, matrix) pair")
            sv, M = pair
            if not _is_block_diag_solver(sv):
                raise TypeError(f"SchurComplementSolver: the solver of {name} must be a GMGLinearSolver, CGSolver(JacobiLinearSolver()), "
                                "LUSolver() or JacobiLinearSolver()")
            if M is None:
                spec = _krylov_gmg_spec(sv)
                if not isinstance(sv, GMGLinearSolver) and spec is None:
                    raise ValueError(f"SchurComplementSolver: {name} needs a matrix (only a GMGLinearSolver brings its own)")
                M = (sv if spec is None else spec[0]).smatrices[0]
            if M.shape[0] != M.shape[1]:
                raise ValueError(f"SchurComplementSolver: the matrix of {name} must be square")
            sizes.append((sv, M))
        (sA, MA), (sS, MS) = sizes
        nA, nS = int(MA.shape[0]), int(MS.shape[0])
        if tuple(B.shape) != (nA, nS):
            raise ValueError(f"SchurComplementSolver: B has shape {tuple(B.shape)}, expected {(nA, nS)}")
        if tuple(C.shape) != (nS, nA):
            raise ValueError(f"SchurComplementSolver: C has shape {tuple(C.shape)}, expected {(nS, nA)}")
        self.A, self.B, self.C, self.S = (sA, MA), B, C, (sS, MS)
        # the fields BlockNumericalSetup reads: every block is the solver's own (MatrixBlock), none is taken from the system
        self.solvers = [sA, sS]
        self.blocks = [[MatrixBlock(MA), MatrixBlock(B)], [MatrixBlock(C), MatrixBlock(MS)]]
        self.coeffs = np.ones((2, 2))          # not consulted by the Schur application


_BLOCK_SOLVERS = (BlockDiagonalSolver, BlockTriangularSolver, SchurComplementSolver)


# ----------------------------------------------------------------------------
# vector / matrix marshalling
# ----------------------------------------------------------------------------
def _is_device(v):
    return hasattr(v, "data_ptr") and getattr(v, "is_cuda", False)


def _vec(v, n=None, writable=False):
    """-> (pointer, memspace, keepalive)."""
    if _is_device(v):
        import torch
        if v.dtype != torch.float64 or not v.is_contiguous():
            raise TypeError("device vectors must be contiguous float64 tensors")
        if n is not None and v.numel() != n:
            raise ValueError(f"vector length {v.numel()} != {n}")
        return C.c_void_p(v.data_ptr()), abi.MEM_DEVICE, v
    if not isinstance(v, np.ndarray) or v.dtype != np.float64 or not v.flags.c_contiguous:
        if writable:
            raise TypeError("output vectors must be contiguous float64 numpy arrays (or CUDA tensors)")
        v = np.ascontiguousarray(v, dtype=np.float64)
    if n is not None and v.size != n:
        raise ValueError(f"vector length {v.size} != {n}")
    return C.c_void_p(v.ctypes.data), abi.MEM_HOST, v


def _csr_fields(M):
    """Accept poisson.CSR, scipy.sparse CSR/CSC, or any object with shape/ptr/idx/val."""
    if hasattr(M, "indptr"):  # scipy
        layout = abi.CSC if M.format == "csc" else abi.CSR
        if M.format not in ("csr", "csc"):
            M = M.tocsr(); layout = abi.CSR
        return M.shape, np.ascontiguousarray(M.indptr), np.ascontiguousarray(M.indices), \
            np.ascontiguousarray(M.data, dtype=np.float64), layout, 0
    base = getattr(M, "index_base", 0)
    layout = getattr(M, "layout", abi.CSR)
    return M.shape, np.ascontiguousarray(M.ptr), np.ascontiguousarray(M.idx), \
        np.ascontiguousarray(M.val, dtype=np.float64), layout, base


def _set_op(fn, h, lev, M):
    if hasattr(M, "row_blocks"):
        # an operator delivered as consecutive row blocks (poisson.StreamedCSR): gmg_set_operator_rows per block, the block
        # is dropped right after -- the host never holds the whole CSR
        lib = abi.load()
        op = {"gmg_set_matrix": abi.OP_A, "gmg_set_prolongation": abi.OP_P, "gmg_set_restriction": abi.OP_R}[fn.__name__]
        seen = 0
        plan = M.row_plan() if (hasattr(M, "row_plan") and os.environ.get("GMG_STREAM_REPEAT", "1") != "0") else (("block", r0, B) for r0, B in M.row_blocks())
        for item in plan:
            if item[0] == "repeat":                         # the last nrows_block rows recur: no arrays, nothing hashed
                _, nrb, count, cshift = item
                abi.check(h, lib.gmg_set_operator_rows_repeat(h, lev, op, nrb, count, cshift))
                seen += nrb * count
                continue
            _, row0, B = item
            if row0 != seen:
                raise ValueError("row-block stream out of order")
            ptr = np.ascontiguousarray(B.ptr, dtype=np.int64)
            idx = np.ascontiguousarray(B.idx, dtype=np.int64)
            val = np.ascontiguousarray(B.val, dtype=np.float64)
            abi.check(h, lib.gmg_set_operator_rows(h, lev, op, M.shape[0], M.shape[1], row0, B.shape[0], C.c_void_p(ptr.ctypes.data),
                                                   C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data), 0, 8))
            seen = row0 + B.shape[0]
        if seen != M.shape[0]:
            raise ValueError("row-block stream ended early")
        return
    shape, ptr, idx, val, layout, base = _csr_fields(M)
    if ptr.dtype != idx.dtype:
        if idx.dtype == np.int32 and val.size < 2 ** 31 - 1:   # narrow the (short) pointer array instead of widening the index array
            ptr = ptr.astype(np.int32)
        else:
            ptr = ptr.astype(np.int64); idx = idx.astype(np.int64)
    if ptr.dtype not in (np.int32, np.int64):
        raise TypeError("index arrays must be int32 or int64")
    nnz = int(val.size)
    abi.check(h, fn(h, lev, shape[0], shape[1], nnz, C.c_void_p(ptr.ctypes.data), C.c_void_p(idx.ctypes.data),
                    C.c_void_p(val.ctypes.data), layout, base, ptr.dtype.itemsize))


# ----------------------------------------------------------------------------
# setups
# ----------------------------------------------------------------------------
class GMGSymbolicSetup:
    """GMGLinearSolvers.jl:160-170: no work."""

    def __init__(self, solver):
        self.solver = solver


class GMGNumericalSetup:
    """GMGNumericalSetup (GMGLinearSolvers.jl:172-210) backed by a native handle;
    released by a finalizer like ext/PardisoExt.jl:54-61."""

    def __init__(self, solver, mat, device_id=None):
        lib = abi.load()
        self.solver = solver
        self._lib = lib
        if device_id is None:
            device_id = 0
            try:
                import torch
                if torch.cuda.is_available():
                    device_id = torch.cuda.current_device()
            except Exception:
                pass
        h = C.c_void_p()
        abi.check(None, lib.gmg_create(C.byref(h), solver.num_levels(), device_id))
        self.h = h
        self._pinned = []          # host arrays registered with the handle, kept alive while they are (LRU, at most 8)
        try:
            for k, v in solver.options.items():
                self.set_option(k, v)
            if getattr(solver, "cycle_values", "float64") == "float32":
                self.set_option("values_f32", 1)
            self._upload(mat)
        except Exception:
            self.close()
            raise

    # -- per-handle policy (gmg_set_option) and page-locked host vectors (gmg_host_register)
    def set_option(self, key, value):
        abi.check(self.h, self._lib.gmg_set_option(self.h, str(key).encode(), float(value)))

    def get_option(self, key):
        """-> (effective value or None when the built-in default applies, source: 'default' | 'handle' | 'environment')"""
        v, src = C.c_double(), C.c_int()
        abi.check(self.h, self._lib.gmg_get_option(self.h, str(key).encode(), C.byref(v), C.byref(src)))
        return (None if v.value != v.value else v.value), ("default", "handle", "environment")[src.value]

    def set_stream(self, stream=None):
        """gmg_set_stream: issue the handle's work on the caller's HIP stream (an integer hipStream_t, a torch.cuda.Stream, or None for
        the handle's own) -- ordered with the caller's kernels on that stream, no device synchronisation in between."""
        abi.check(self.h, self._lib.gmg_set_stream(self.h, abi.stream_arg(stream)))

    def get_stream(self):
        out = C.c_void_p()
        abi.check(self.h, self._lib.gmg_get_stream(self.h, C.byref(out)))
        return out.value or 0

    def setup(self):
        """gmg_setup again (after set_option changed a layout option)."""
        abi.check(self.h, self._lib.gmg_setup(self.h))

    def register_host(self, arr):
        abi.check(self.h, self._lib.gmg_host_register(self.h, C.c_void_p(arr.ctypes.data), arr.nbytes))

    def unregister_host(self, arr):
        abi.check(self.h, self._lib.gmg_host_unregister(self.h, C.c_void_p(arr.ctypes.data)))

    def pin(self, *arrays):
        """Page-lock host vectors for the life of this setup (or until 8 newer ones displaced them); holds a reference to each.
        Keyed by address range, as the C registry is: two views of one buffer are one registration."""
        for a in arrays:
            if not isinstance(a, np.ndarray) or a.nbytes == 0:
                continue
            key = (a.ctypes.data, a.nbytes)
            hit = next((i for i, (k, _q) in enumerate(self._pinned) if k == key), None)
            if hit is not None:
                self._pinned.append(self._pinned.pop(hit))          # most recently used last
                continue
            if len(self._pinned) >= 8:
                _k, old = self._pinned.pop(0)
                try:
                    self.unregister_host(old)
                except abi.GmgError:                                 # (a range another view had already released)
                    pass
            self.register_host(a)
            self._pinned.append((key, a))

    def host_io_stats(self):
        up, down, nreg = C.c_int64(), C.c_int64(), C.c_int64()
        abi.check(self.h, self._lib.gmg_get_host_io_stats(self.h, C.byref(up), C.byref(down), C.byref(nreg)))
        return dict(bytes_up=up.value, bytes_down=down.value, registered=nreg.value)

    def persist_retries(self):
        r, a = C.c_int64(), C.c_int()
        abi.check(self.h, self._lib.gmg_get_persist_retries(self.h, C.byref(r), C.byref(a)))
        return dict(retries=r.value, persist_active=bool(a.value))

    def _upload(self, mat):
        lib, h, s = self._lib, self.h, self.solver
        nlev = s.num_levels()
        mats = list(s.smatrices)
        if mat is not None:
            mats[0] = mat  # smatrices[1] = mat, GMGLinearSolvers.jl:338
        for l, A in enumerate(mats):
            if isinstance(A, Galerkin):
                abi.check(h, lib.gmg_set_galerkin(h, l))
            else:
                _set_op(lib.gmg_set_matrix, h, l, A)
        for l in range(nlev - 1):
            ip = s.interp[l]
            if isinstance(ip, Aggregation):
                abi.check(h, lib.gmg_set_aggregation(h, l, ip.theta, 1 if ip.smooth else 0, 0.0 if ip.omega is None else ip.omega, ip.seed))
            elif isinstance(ip, PatchProlongationOperator):
                _set_op(lib.gmg_set_prolongation, h, l, ip.P)
                abi.check(h, lib.gmg_set_prolongation_patch_correction(
                    h, l, ip.kind, ip.patch_ptr.size - 1, C.c_void_p(ip.patch_ptr.ctypes.data),
                    C.c_void_p(ip.patch_dofs.ctypes.data), 0, 8))
                if ip.rhs is not None:
                    shape, ptr, idx, val, layout, base = _csr_fields(ip.rhs)
                    if ptr.dtype != idx.dtype:
                        ptr = ptr.astype(np.int64); idx = idx.astype(np.int64)
                    abi.check(h, lib.gmg_set_prolongation_patch_correction_rhs(
                        h, l, shape[0], int(val.size), C.c_void_p(ptr.ctypes.data), C.c_void_p(idx.ctypes.data),
                        C.c_void_p(val.ctypes.data), layout, base, ptr.dtype.itemsize))
            else:
                _set_op(lib.gmg_set_prolongation, h, l, ip)
            if s.restrict[l] is not None:
                _set_op(lib.gmg_set_restriction, h, l, s.restrict[l])
            pre, post = s.pre_smoothers[l], s.post_smoothers[l]
            self._set_gs_ordering(l, pre, post)
            if post is pre:
                self._set_smoother(l, abi.PRE_AND_POST, pre)
            else:
                self._set_smoother(l, abi.PRE, pre)
                self._set_smoother(l, abi.POST, post)
        abi.check(h, lib.gmg_set_options(h, _MODES[s.mode], _CYCLES[s.cycle_type], s.log.maxiter, s.log.atol, s.log.rtol))
        abi.check(h, lib.gmg_set_verbose(h, s.verbose))
        cs = s.coarsest_solver
        if isinstance(cs, CGSolver):
            abi.check(h, lib.gmg_set_coarse_solver(h, abi.COARSE_CG_JACOBI, cs.log.maxiter, cs.log.atol, cs.log.rtol, None, None))
        elif isinstance(cs, HostCallbackSolver):
            def _cb(ctx, n, r, x, fn=cs.fn):
                try:
                    out = np.asarray(fn(np.ctypeslib.as_array(r, shape=(n,)).copy()), dtype=np.float64)
                    np.ctypeslib.as_array(x, shape=(n,))[:] = out
                    return 0
                except Exception:      # never unwind through the C frames
                    return 1
            self._coarse_cb = abi.COARSE_SOLVE_FN(_cb)
            abi.check(h, lib.gmg_set_coarse_solver(h, abi.COARSE_HOST_CALLBACK, 0, 0.0, 0.0, C.cast(self._coarse_cb, C.c_void_p), None))
        elif isinstance(cs, NullspaceSolver):
            Kc = np.ascontiguousarray(cs.nullspace.matrix_representation().T)      # vector q at Kc + q*n_L
            abi.check(h, lib.gmg_set_coarse_nullspace(h, Kc.shape[0], C.c_void_p(Kc.ctypes.data), Kc.shape[1]))
        self.n = int(mats[0].shape[0])
        self.sizes = [_level_size(mats, s.interp, l) for l in range(nlev)]
        abi.check(h, lib.gmg_setup(h))
        self.sizes = [self.level_size(l) if n is None else n for l, n in enumerate(self.sizes)]

    def _set_gs_ordering(self, l, pre, post):
        """one visiting order per level (gmg_set_gs_ordering): the one its Gauss-Seidel smoother(s) name"""
        gs = [sm for sm in (pre, post) if isinstance(sm, GaussSeidelSmoother)]
        if not gs:
            return
        if len(gs) == 2 and not gs[0]._same_ordering(gs[1]):
            raise ValueError(f"level {l}: the pre- and the post-smoother name different orderings (one order per level)")
        o = gs[0].ordering
        if isinstance(o, str):
            abi.check(self.h, self._lib.gmg_set_gs_ordering(self.h, l, GaussSeidelSmoother._ORDERINGS[o], None, 0))
        else:
            abi.check(self.h, self._lib.gmg_set_gs_ordering(self.h, l, abi.GS_ORDER_GIVEN, C.c_void_p(o.ctypes.data), o.size))

    def _set_smoother(self, l, which, sm):
        lib, h = self._lib, self.h
        if isinstance(sm, GaussSeidelSmoother):
            abi.check(h, lib.gmg_set_smoother_gauss_seidel(h, l, which, sm.niter, sm.omega, sm._TYPES[sm.type]))
            return
        if isinstance(sm, ChebyshevSmoother):
            # the slot's M through its own setter (niter and omega are unused), then the Chebyshev iteration over it
            self._set_smoother(l, which, RichardsonSmoother(sm.M, 1, 1.0))
            abi.check(h, lib.gmg_set_smoother_chebyshev(h, l, which, sm.degree, 0.0 if sm.lambda_min is None else sm.lambda_min,
                                                        0.0 if sm.lambda_max is None else sm.lambda_max, sm.eig_steps, sm.eig_ratio,
                                                        sm.eig_safety))
            if sm.eig_method != "power":
                abi.check(h, lib.gmg_set_chebyshev_eig_method(h, l, which, sm._EIG_METHODS[sm.eig_method]))
            return
        if isinstance(sm, MultiplicativePatchSmoother):
            # the slot's patch tables and blocks through M's own setter, then the multiplicative sweep over them
            self._set_smoother(l, which, RichardsonSmoother(sm.M, 1, 1.0))
            abi.check(h, lib.gmg_set_smoother_patch_multiplicative(h, l, which, sm.niter, sm.omega, sm._TYPES[sm.type]))
            if not isinstance(sm.coloring, str):
                abi.check(h, lib.gmg_set_patch_coloring(h, l, which, abi.PATCH_COLORING_GIVEN, C.c_void_p(sm.coloring.ctypes.data),
                                                        sm.coloring.size))
            return
        if not isinstance(sm, RichardsonSmoother):
            raise TypeError("smoothers must be RichardsonSmoother, GaussSeidelSmoother, ChebyshevSmoother or MultiplicativePatchSmoother objects")
        if isinstance(sm.M, JacobiLinearSolver):
            abi.check(h, lib.gmg_set_smoother_jacobi(h, l, which, sm.niter, sm.omega))
        else:
            M = sm.M
            pp = M.patch_ptr
            if M.patch_cols is None and M.patch_mats is None and M.factors is None:
                if M.patch_dofs.dtype == np.int32 and int(pp[-1]) < 2 ** 31 - 1:
                    # int32 tables as they are (1.7e7 vertex-star patches of a 256^3 Q2 level: 4.6e8 entries), the short pointer array narrowed
                    pp32, pd = np.ascontiguousarray(pp, dtype=np.int32), np.ascontiguousarray(M.patch_dofs)
                    abi.check(h, lib.gmg_set_smoother_patch(h, l, which, sm.niter, sm.omega, M.kind, pp.size - 1,
                                                            C.c_void_p(pp32.ctypes.data), C.c_void_p(pd.ctypes.data), 0, 4))
                    return
            pp, pd = np.ascontiguousarray(pp, dtype=np.int64), M.patch_dofs.astype(np.int64)
            if M.patch_cols is None and M.patch_mats is None and M.factors is None:
                abi.check(h, lib.gmg_set_smoother_patch(h, l, which, sm.niter, sm.omega, M.kind, pp.size - 1,
                                                        C.c_void_p(pp.ctypes.data), C.c_void_p(pd.ctypes.data), 0, 8))
            else:
                pc = None if M.patch_cols is None else M.patch_cols.astype(np.int64)
                blk = M.patch_mats if M.patch_mats is not None else M.factors
                abi.check(h, lib.gmg_set_smoother_patch_matrices(
                    h, l, which, sm.niter, sm.omega, M.kind, pp.size - 1, C.c_void_p(pp.ctypes.data), C.c_void_p(pd.ctypes.data),
                    None if pc is None else C.c_void_p(pc.ctypes.data), 0, 8,
                    None if blk is None else C.c_void_p(blk.ctypes.data), 1 if M.factors is not None else 0,
                    None if M.pivots is None else C.c_void_p(M.pivots.ctypes.data)))

    # -- numerical_setup!(ns, A): FromMatrices variant is unsupported in the reference
    #    (GMGLinearSolvers.jl:249-258 logs @error); here new values on the same pattern are accepted.
    def update(self, mat, smatrices=None):
        """numerical_setup!(ns, A): new values on the same sparsity.  `smatrices` (optional) = the re-assembled matrices of ALL
        levels, as the FromWeakform variant recomputes them (GMGLinearSolvers.jl:260-297); default: only the finest changes.
        Galerkin levels follow the new values of the levels above them; their entry of `smatrices` is None or Galerkin()."""
        mats = [mat] if smatrices is None else [mat] + list(smatrices[1:])
        for l, M in enumerate(mats):
            if M is not None and not isinstance(M, Galerkin) and isinstance(self.solver.smatrices[l], Galerkin):
                raise ValueError(f"smatrices[{l}]: level {l} is a Galerkin level, its matrix is formed from the finer level's")
        for l, M in enumerate(mats):
            if M is None or isinstance(M, Galerkin):
                continue
            shape, ptr, idx, val, layout, base = _csr_fields(M)
            if layout == abi.CSC:           # values in the caller's CSC order (the level was set in CSC layout): scattered by the library
                st = self._lib.gmg_update_values_csc(self.h, l, C.c_void_p(ptr.ctypes.data), C.c_void_p(idx.ctypes.data),
                                                     C.c_void_p(val.ctypes.data), base, ptr.dtype.itemsize)
            else:
                st = self._lib.gmg_update_values(self.h, l, C.c_void_p(val.ctypes.data))
            if st == abi.ERR_UNSUPPORTED:       # level held in row-pattern form only: hand the whole matrix over again
                _set_op(self._lib.gmg_set_matrix, self.h, l, M)
            else:
                abi.check(self.h, st)
        abi.check(self.h, self._lib.gmg_setup(self.h))
        return self

    def close(self):
        if getattr(self, "h", None):
            self._lib.gmg_destroy(self.h)      # unregisters what is still page-locked (never frees caller memory)
            self.h = None
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- operator-level helpers (duck-typed mul! / smoother solve!)
    def op_apply(self, lev, op, x, y):
        px, ms, _k1 = _vec(x)
        py, ms2, _k2 = _vec(y, writable=True)
        if ms != ms2:
            raise TypeError("x and y must live in the same memory space")
        abi.check(self.h, self._lib.gmg_op_apply(self.h, lev, op, px, py, ms))
        return y

    def smooth(self, lev, x, r, which=abi.PRE):
        px, ms, _k1 = _vec(x, self.sizes[lev], writable=True)
        pr, ms2, _k2 = _vec(r, self.sizes[lev], writable=True)
        if ms != ms2:
            raise TypeError("x and r must live in the same memory space")
        abi.check(self.h, self._lib.gmg_smooth(self.h, lev, which, px, pr, ms))
        return x, r

    def precond(self, lev, r, dx, which=abi.PRE):
        pr, ms, _k1 = _vec(r, self.sizes[lev])
        pd, ms2, _k2 = _vec(dx, self.sizes[lev], writable=True)
        if ms != ms2:
            raise TypeError("r and dx must live in the same memory space")
        abi.check(self.h, self._lib.gmg_precond_apply(self.h, lev, which, pr, pd, ms))
        return dx

    def coarse_solve(self, r, x):
        pr, ms, _k1 = _vec(r, self.sizes[-1])
        px, ms2, _k2 = _vec(x, self.sizes[-1], writable=True)
        if ms != ms2:
            raise TypeError("r and x must live in the same memory space")
        abi.check(self.h, self._lib.gmg_coarse_solve(self.h, pr, px, ms))
        return x

    def coarse_info(self):
        """gmg_get_coarse_info: how the setup built the dense inverse of LUSolver() on the coarsest level ->
        dict(built_by ("none" / "host_lu" / "device_gj" / "host_constrained"), panel (0, 32 or 64), mfma, device_rejected)"""
        v = [C.c_int(0) for _ in range(4)]
        abi.check(self.h, self._lib.gmg_get_coarse_info(self.h, *[C.byref(q) for q in v]))
        return dict(built_by=("none", "host_lu", "device_gj", "host_constrained")[v[0].value], panel=v[1].value,
                    mfma=bool(v[2].value), device_rejected=bool(v[3].value))

    def dot(self, a, b):
        pa, ms, _k1 = _vec(a)
        pb, ms2, _k2 = _vec(b)
        out = C.c_double(0.0)
        n = a.numel() if _is_device(a) else _k1.size
        abi.check(self.h, self._lib.gmg_dot(self.h, n, pa, pb, ms, C.byref(out)))
        return out.value

    def coarse_log(self):
        res = abi.Result()
        abi.check(self.h, self._lib.gmg_get_coarse_log(self.h, C.byref(res)))
        return dict(niters=int(res.niters), flag=int(res.flag), res0=res.res0, res=res.res)

    def fill_log(self):
        """ns.solver.log of the GMG after it ran inside a Krylov call (gmg_get_log)."""
        log = self.solver.log
        res = abi.Result()
        hist = np.zeros(log.maxiter + 1)
        abi.check(self.h, self._lib.gmg_get_log(self.h, C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return log

    def profile(self, lev=0, enable=True):
        abi.check(self.h, self._lib.gmg_profile_enable(self.h, lev, 1 if enable else 0))

    def kernel_stats(self):
        st = abi.KernelStats()
        abi.check(self.h, self._lib.gmg_get_kernel_stats(self.h, C.byref(st)))
        ms, nl, lb = (C.c_double * 3)(), (C.c_int64 * 3)(), (C.c_double * 3)()
        abi.check(self.h, self._lib.gmg_get_kernel_stats_by_variant(self.h, ms, nl, lb))
        names = ("x_every_sweep", "x_untouched", "x_two_increments")
        by_variant = {names[v]: dict(launches=int(nl[v]), total_ms=float(ms[v]), avg_ms=float(ms[v]) / nl[v], layout_bytes=float(lb[v]))
                      for v in range(3) if nl[v]}
        return dict(launches=st.launches, total_ms=st.total_ms, alg_bytes=st.alg_bytes, rows=st.rows, nnz=st.nnz,
                    layout_bytes=st.layout_bytes, fused_passes=st.fused_passes, by_variant=by_variant)

    def stream_probe(self, nbytes=1 << 30, reps=10):
        v = C.c_double(0.0)
        abi.check(self.h, self._lib.gmg_stream_probe(self.h, nbytes, reps, C.byref(v)))
        return v.value

    def stream_probe_read(self, nbytes=1 << 30, reps=10):
        v = C.c_double(0.0)
        abi.check(self.h, self._lib.gmg_stream_probe_read(self.h, nbytes, reps, C.byref(v)))
        return v.value

    def model_bytes(self):
        a, b = C.c_double(0.0), C.c_double(0.0)
        abi.check(self.h, self._lib.gmg_model_bytes(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def level_format(self, lev=0):
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        d, e = C.c_double(0.0), C.c_double(0.0)
        abi.check(self.h, self._lib.gmg_level_format(self.h, lev, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        return dict(layout=("CSR-stream", "SELL-64", "SELL-P", "SELL-O")[a.value], row_patterns=(a.value == 2),
                    value_dictionary=bool(b.value), idx16=bool(c.value), stream_bytes_per_nnz=d.value, padding=e.value)

    def level_values(self, lev=0):
        """gmg_level_values: what the cycle streams of this level's matrix -> dict(dtype ("float64" / "float32"),
        cycle_stream_bytes_per_nnz)"""
        f, d = C.c_int(0), C.c_double(0.0)
        abi.check(self.h, self._lib.gmg_level_values(self.h, lev, C.byref(f), C.byref(d)))
        return dict(dtype="float32" if f.value else "float64", cycle_stream_bytes_per_nnz=d.value)

    def level_matrix(self, lev):
        """gmg_get_galerkin_matrix: the matrix of a Galerkin level as the last setup formed it -> (shape, ptr, idx, val), 0-based CSR
        with int64 pointers and int32 columns."""
        n, nnz = C.c_int64(), C.c_int64()
        abi.check(self.h, self._lib.gmg_get_galerkin_matrix(self.h, lev, C.byref(n), C.byref(nnz), None, None, None, 0))
        ptr, idx, val = np.empty(n.value + 1, dtype=np.int64), np.empty(nnz.value, dtype=np.int32), np.empty(nnz.value)
        abi.check(self.h, self._lib.gmg_get_galerkin_matrix(self.h, lev, C.byref(n), C.byref(nnz), C.c_void_p(ptr.ctypes.data),
                                                            C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data), nnz.value))
        return (n.value, n.value), ptr, idx, val

    def level_size(self, lev):
        """gmg_get_level_size: rows of a level after the setup (levels below an Aggregation() have no size before)"""
        n = C.c_int64()
        abi.check(self.h, self._lib.gmg_get_level_size(self.h, lev, C.byref(n)))
        return n.value

    def aggregates(self, lev):
        """gmg_get_aggregates: -> (agg, nagg): the aggregate 0 .. nagg-1 of every row of an Aggregation() level (int32)"""
        nagg, n = C.c_int64(), self.sizes[lev]
        if n is None:
            n = self.level_size(lev)
        agg = np.empty(n, dtype=np.int32)
        abi.check(self.h, self._lib.gmg_get_aggregates(self.h, lev, C.byref(nagg), C.c_void_p(agg.ctypes.data), agg.size))
        return agg, nagg.value

    def prolongation(self, lev):
        """gmg_get_prolongation: the prolongation of an Aggregation() level as the last setup formed it -> (shape, ptr, idx, val),
        0-based CSR with int64 pointers and int32 columns"""
        nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        abi.check(self.h, self._lib.gmg_get_prolongation(self.h, lev, C.byref(nr), C.byref(nc), C.byref(nnz), None, None, None, 0, 0))
        ptr, idx, val = np.empty(nr.value + 1, dtype=np.int64), np.empty(nnz.value, dtype=np.int32), np.empty(nnz.value)
        abi.check(self.h, self._lib.gmg_get_prolongation(self.h, lev, C.byref(nr), C.byref(nc), C.byref(nnz), C.c_void_p(ptr.ctypes.data),
                                                         C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data), ptr.size, nnz.value))
        return (nr.value, nc.value), ptr, idx, val

    def aggregation_info(self, lev):
        """gmg_get_aggregation_info: what the last aggregation of the level did -> dict(rounds, omega, rho, strong_edges, strength_ms,
        mis_ms, assign_ms, p_ms)"""
        r, om, rho, se, ms = C.c_int(), C.c_double(), C.c_double(), C.c_int64(), (C.c_double * 4)()
        abi.check(self.h, self._lib.gmg_get_aggregation_info(self.h, lev, C.byref(r), C.byref(om), C.byref(rho), C.byref(se), ms))
        return dict(rounds=r.value, omega=om.value, rho=rho.value, strong_edges=se.value, strength_ms=ms[0], mis_ms=ms[1], assign_ms=ms[2],
                    p_ms=ms[3])

    def galerkin_timing(self, lev):
        """gmg_get_galerkin_timing: what the last product of a Galerkin level cost, in ms"""
        s, a, r = C.c_double(), C.c_double(), C.c_double()
        abi.check(self.h, self._lib.gmg_get_galerkin_timing(self.h, lev, C.byref(s), C.byref(a), C.byref(r)))
        return dict(symbolic_ms=s.value, ap_ms=a.value, rt_ms=r.value)

    def sweep_signature(self, lev=0):
        buf = C.create_string_buffer(256)
        abi.check(self.h, self._lib.gmg_sweep_signature(self.h, lev, buf, 256))
        return buf.value.decode()

    def device_bytes(self):
        v = C.c_int64(0)
        abi.check(self.h, self._lib.gmg_device_bytes(self.h, C.byref(v)))
        return v.value

    def chebyshev_info(self, lev=0, which="pre"):
        """gmg_get_chebyshev_info: what the setup fixed for the ChebyshevSmoother of a slot (which = "pre" / "post") ->
        dict(degree, lambda_est (NaN where the bounds were given), lambda_min, lambda_max, eig_steps, eig_method ("power" / "lanczos"),
        eig_steps_done (power: eig_steps; lanczos: <= eig_steps, fewer where the Krylov space was exhausted; 0 where the bounds were
        given)); GmgError (ERR_STATE) on a slot without one."""
        if which not in ("pre", "post"):
            raise ValueError('which must be "pre" or "post"')
        deg, steps = C.c_int(0), C.c_int(0)
        v = [C.c_double(0.0) for _ in range(3)]
        abi.check(self.h, self._lib.gmg_get_chebyshev_info(self.h, lev, abi.PRE if which == "pre" else abi.POST, C.byref(deg),
                                                           C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(steps)))
        meth, done = C.c_int(0), C.c_int(0)
        abi.check(self.h, self._lib.gmg_get_chebyshev_eig(self.h, lev, abi.PRE if which == "pre" else abi.POST, C.byref(meth), C.byref(done)))
        return dict(degree=deg.value, lambda_est=v[0].value, lambda_min=v[1].value, lambda_max=v[2].value, eig_steps=steps.value,
                    eig_method=("power", "lanczos")[meth.value], eig_steps_done=done.value)

    def patch_coloring(self, level=0, which="pre"):
        """gmg_get_patch_coloring: the colouring the setup of the slot's MultiplicativePatchSmoother uses -> (ncolors, color);
        GmgError (ERR_STATE) on a slot without one."""
        if which not in ("pre", "post"):
            raise ValueError('which must be "pre" or "post"')
        w, nc = abi.PRE if which == "pre" else abi.POST, C.c_int64(0)
        abi.check(self.h, self._lib.gmg_get_patch_coloring(self.h, level, w, C.byref(nc), None, 0))
        sm = (self.solver.pre_smoothers if which == "pre" else self.solver.post_smoothers)[level]
        color = np.empty(sm.M.patch_ptr.size - 1, dtype=np.int32)
        abi.check(self.h, self._lib.gmg_get_patch_coloring(self.h, level, w, C.byref(nc), C.c_void_p(color.ctypes.data), color.size))
        return nc.value, color

    def cg_set_trace(self, capacity):
        """gmg_cg_set_trace: capacity > 0 makes the outermost CG of gmg_cg_solve record alpha_k, beta_k; 0 releases the buffer."""
        abi.check(self.h, self._lib.gmg_cg_set_trace(self.h, int(capacity)))

    def cg_trace(self):
        """gmg_cg_get_trace -> (alpha, beta) of the iterations of the last gmg_cg_solve; GmgError (ERR_STATE) while tracing is off."""
        k = C.c_int(0)
        abi.check(self.h, self._lib.gmg_cg_get_trace(self.h, C.byref(k), None, None, 0))
        alpha, beta = np.zeros(k.value), np.zeros(k.value)
        abi.check(self.h, self._lib.gmg_cg_get_trace(self.h, C.byref(k), C.c_void_p(alpha.ctypes.data), C.c_void_p(beta.ctypes.data), k.value))
        return alpha, beta

    def gs_schedule(self, lev=0, forward=True):
        """gmg_get_gs_schedule: what the setup of the level's Gauss-Seidel smoother built for one direction ->
        dict(nsets, max_set_rows, nlaunches, nwide); GmgError (ERR_STATE) when no smoother of the level uses that direction."""
        v = [C.c_int64(0) for _ in range(4)]
        abi.check(self.h, self._lib.gmg_get_gs_schedule(self.h, lev, 0 if forward else 1, *[C.byref(q) for q in v]))
        return dict(zip(("nsets", "max_set_rows", "nlaunches", "nwide"), (q.value for q in v)))


    def gs_ordering(self, lev=0):
        """gmg_get_gs_ordering: the visiting order the setup of the level's Gauss-Seidel smoother used ->
        dict(kind ("natural" / "multicolor" / "given"), ncolors (0 unless multicolor), order)"""
        kind, nc = C.c_int(0), C.c_int64(0)
        order = np.empty(self.sizes[lev], dtype=np.int32)
        abi.check(self.h, self._lib.gmg_get_gs_ordering(self.h, lev, C.byref(kind), C.byref(nc), C.c_void_p(order.ctypes.data), order.size))
        return dict(kind=("natural", "multicolor", "given")[kind.value], ncolors=nc.value, order=order)


def _set_block(fn, h, i, j, M):
    shape, ptr, idx, val, layout, base = _csr_fields(M)
    if ptr.dtype != idx.dtype:
        if idx.dtype == np.int32 and val.size < 2 ** 31 - 1:   # narrow the (short) pointer array instead of widening the index array
            ptr = ptr.astype(np.int32)
        else:
            ptr = ptr.astype(np.int64); idx = idx.astype(np.int64)
    abi.check_block(h, fn(h, i, j, shape[0], shape[1], int(val.size), C.c_void_p(ptr.ctypes.data),
                          C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data), layout, base, ptr.dtype.itemsize))


class BlockSymbolicSetup:
    def __init__(self, solver):
        self.solver = solver


class BlockNumericalSetup:
    """BlockDiagonalSolverNS / BlockTriangularSolverNS (BlockTriangularSolvers.jl:132-152) / SchurComplementNumericalSetup
    (SchurComplementSolvers.jl:36-53) on a native handle.  `mat` is the block system matrix as a nested list (None = zero block)."""

    _HALF = {"diagonal": abi.BLOCK_DIAGONAL, "lower": abi.BLOCK_LOWER, "upper": abi.BLOCK_UPPER, "schur": abi.BLOCK_SCHUR}

    def __init__(self, solver, mat, device_id=None):
        lib = abi.load()
        self.solver, self._lib = solver, lib
        nb = len(solver.solvers)
        if len(mat) != nb or any(len(r) != nb for r in mat):
            raise ValueError("block matrix does not match the number of solvers")
        sizes = np.zeros(nb, dtype=np.int64)
        for i in range(nb):
            row = [m for m in mat[i] if m is not None]
            if not row:
                raise ValueError(f"block row {i} is empty")
            sizes[i] = int(_csr_fields(row[0])[0][0])
        self.sizes, self.n = sizes, int(sizes.sum())
        if device_id is None:
            device_id = 0
            try:
                import torch
                if torch.cuda.is_available():
                    device_id = torch.cuda.current_device()
            except Exception:
                pass
        h = C.c_void_p()
        abi.check_block(None, lib.gmg_block_create(C.byref(h), nb, C.c_void_p(sizes.ctypes.data), self._HALF[solver.half], device_id))
        self.h = h
        self.block_ns = [None] * nb
        try:
            for i in range(nb):
                for j in range(nb):
                    if mat[i][j] is not None:
                        _set_block(lib.gmg_block_set_system_block, h, i, j, mat[i][j])
                    blk = solver.blocks[i][j]
                    if i != j:
                        if isinstance(blk, MatrixBlock):
                            _set_block(lib.gmg_block_set_precond_block, h, i, j, blk.mat)
                        abi.check_block(h, lib.gmg_block_set_coeff(h, i, j, float(solver.coeffs[i][j])))
            for i, sv in enumerate(solver.solvers):
                blk = solver.blocks[i][i]
                Mi = blk.mat if isinstance(blk, MatrixBlock) else mat[i][i]
                if isinstance(sv, GMGLinearSolver):
                    g = GMGNumericalSetup(sv, Mi, device_id)
                    self.block_ns[i] = g
                    abi.check_block(h, lib.gmg_block_set_diag_gmg(h, i, g.h))
                    continue
                spec = _krylov_gmg_spec(sv)
                if spec is not None:               # FGMRESSolver(m, gmg) & co.: the GMG is set up on the block's matrix as a bare one
                    gmg, krylov, m, restart, m_add, flexible, side = spec
                    g = GMGNumericalSetup(gmg, Mi, device_id)
                    self.block_ns[i] = g
                    abi.check_block(h, lib.gmg_block_set_diag_krylov_gmg(h, i, g.h, krylov, m, int(restart), m_add, int(flexible), side,
                                                                         sv.log.maxiter, sv.log.atol, sv.log.rtol))
                    continue
                if isinstance(sv, CGSolver) and isinstance(sv.Pl, JacobiLinearSolver) and not sv.flexible:
                    kind, (mi, at, rt) = abi.BLOCK_CG_JACOBI, (sv.log.maxiter, sv.log.atol, sv.log.rtol)
                elif isinstance(sv, LUSolver):
                    kind, (mi, at, rt) = abi.BLOCK_LU, (0, 0.0, 0.0)
                elif isinstance(sv, JacobiLinearSolver):
                    kind, (mi, at, rt) = abi.BLOCK_JACOBI, (0, 0.0, 0.0)
                else:
                    raise NotImplementedError("block solvers on the device: GMGLinearSolver, CGSolver(JacobiLinearSolver()), "
                                              "LUSolver(), JacobiLinearSolver(); " + _KRYLOV_GMG_FORMS)
                abi.check_block(h, lib.gmg_block_set_diag_solver(h, i, kind, mi, at, rt))
                if isinstance(blk, MatrixBlock):
                    shape, ptr, idx, val, layout, base = _csr_fields(blk.mat)
                    if ptr.dtype != idx.dtype:
                        ptr = ptr.astype(np.int64); idx = idx.astype(np.int64)
                    abi.check_block(h, lib.gmg_block_set_diag_matrix(h, i, shape[0], int(val.size), C.c_void_p(ptr.ctypes.data),
                                                                     C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data),
                                                                     layout, base, ptr.dtype.itemsize))
            abi.check_block(h, lib.gmg_block_setup(h))
        except Exception:
            self.close()
            raise

    # -- numerical_setup!(ns, A, x): BlockTriangularSolvers.jl:156-186, BlockDiagonalSolvers.jl:153-163
    def update(self, mat, smatrices=None):
        """numerical_setup!(ns, A): new values on the same patterns.  Every present system block is handed over again; the solver
        of a NonlinearSystemBlock diagonal block is set up again (a GMGLinearSolver first refreshes its own handle from mat[i][i];
        `smatrices[i]`, optional, = the re-assembled matrices of all its levels), LinearSystemBlock and MatrixBlock solvers keep
        theirs (BlockSolverInterfaces.jl:104-118,232-236)."""
        lib, h = self._lib, self.h
        nb = len(self.solver.solvers)
        if len(mat) != nb or any(len(r) != nb for r in mat):
            raise ValueError("block matrix does not match the number of solvers")
        t0 = time.perf_counter()
        for i in range(nb):
            for j in range(nb):
                if mat[i][j] is None:
                    continue
                shape, ptr, idx, val, layout, base = _csr_fields(mat[i][j])
                if layout == abi.CSC:
                    st = lib.gmg_block_update_values_csc(h, abi.BLOCK_SLOT_SYSTEM, i, j, C.c_void_p(ptr.ctypes.data),
                                                         C.c_void_p(idx.ctypes.data), C.c_void_p(val.ctypes.data), base, ptr.dtype.itemsize)
                else:
                    st = lib.gmg_block_update_values(h, abi.BLOCK_SLOT_SYSTEM, i, j, C.c_void_p(val.ctypes.data))
                abi.check_block(h, st)
        t1 = time.perf_counter()
        for i, sv in enumerate(self.solver.solvers):
            if not isinstance(self.solver.blocks[i][i], NonlinearSystemBlock):
                continue
            if isinstance(sv, GMGLinearSolver) or _krylov_gmg_spec(sv) is not None:
                self.block_ns[i].update(mat[i][i], None if smatrices is None else smatrices[i])
            abi.check_block(h, lib.gmg_block_refresh_diag_solver(h, i))
        t2 = time.perf_counter()
        abi.check_block(h, lib.gmg_block_setup(h))
        # seconds of the last update: values recorded on the host copies / the GMG handles' own refresh / gmg_block_setup
        self.update_seconds = dict(record=t1 - t0, gmg=t2 - t1, block_setup=time.perf_counter() - t2)
        return self

    def setup_info(self):
        """what the last gmg_block_setup did: kind (1 full, 2 in place), blocks_refreshed, value_bytes, device_bytes"""
        k, v = C.c_int(0), [C.c_int64(0) for _ in range(3)]
        abi.check_block(self.h, self._lib.gmg_block_get_setup_info(self.h, C.byref(k), *[C.byref(q) for q in v]))
        return dict(zip(("kind", "blocks_refreshed", "value_bytes", "device_bytes"), (k.value,) + tuple(q.value for q in v)))

    def _fill_logs(self):
        """copy the block solvers' ConvergenceLogs back (their last application)"""
        for i, sv in enumerate(self.solver.solvers):
            # (a Krylov solver around a GMG: the wrapper's own log; the GMG's stays as the GMG leaves it)
            if isinstance(sv, (GMGLinearSolver, CGSolver)) or _krylov_gmg_spec(sv) is not None:
                res = abi.Result()
                abi.check_block(self.h, self._lib.gmg_block_diag_log(self.h, i, C.byref(res)))
                sv.log.num_iters, sv.log.flag = int(res.niters), int(res.flag)

    def diag_stats(self, i):
        """gmg_block_diag_stats: (applications, iterations in all) of the iterative solver of block i since the last setup"""
        a, t = C.c_int64(0), C.c_int64(0)
        abi.check_block(self.h, self._lib.gmg_block_diag_stats(self.h, i, C.byref(a), C.byref(t)))
        return int(a.value), int(t.value)

    def mul(self, y, x):
        """mul!(y, A, x) on the block system"""
        px, ms, _k1 = _vec(x, self.n)
        py, ms2, _k2 = _vec(y, self.n, writable=True)
        if ms != ms2:
            raise TypeError("x and y must live in the same memory space")
        abi.check_block(self.h, self._lib.gmg_block_apply_system(self.h, px, py, ms))
        return y

    def close(self):
        if getattr(self, "h", None):
            self._lib.gmg_block_destroy(self.h)       # before the GMG handles it borrows
            self.h = None
        for g in getattr(self, "block_ns", []):
            if g is not None:
                g.close()
        self.block_ns = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _KrylovSymbolicSetup:
    def __init__(self, solver):
        self.solver = solver


class _KrylovNumericalSetup:
    """CGNumericalSetup / FGMRESNumericalSetup / MINRESNumericalSetup / GMRESNumericalSetup: holds the preconditioner's numerical
    setup (CGSolvers.jl:50-55, FGMRESSolvers.jl:96-102)."""

    def __init__(self, solver, A, device_id=None):
        self.solver = solver
        if isinstance(solver, GMRESSolver):
            self._init_gmres(solver, A, device_id)
            return
        P = solver.Pr if isinstance(solver, FGMRESSolver) else solver.Pl
        diag = getattr(solver, "diag", None) if isinstance(solver, CGSolver) else None
        if diag is not None:
            if isinstance(P, _BLOCK_SOLVERS):
                raise ValueError("CGSolver(diagnostic=...) over a block system is not supported (gmg_block_cg_solve records no trace)")
            if diag.delta.size < solver.log.maxiter:
                raise ValueError(f"the LanczosDiagnostic holds {diag.delta.size} iterations, the solver may take {solver.log.maxiter} "
                                 "(LanczosDiagnostic(maxiter + 1) as the reference's tests build it)")
        if isinstance(P, _BLOCK_SOLVERS):
            self.pc_kind = 1
            self.P_ns = BlockNumericalSetup(P, A, device_id)
            self.n = self.P_ns.n
            return
        if isinstance(P, GMGLinearSolver):
            self.pc_kind, gmg = 1, P
        elif isinstance(P, tuple) and len(P) == 2 and isinstance(P[1], GMGLinearSolver) and \
                (P[0] is None or isinstance(P[0], (JacobiLinearSolver, LinearSolverFromSmoother))):
            # (None | JacobiLinearSolver() | LinearSolverFromSmoother(gmg.pre_smoothers[0]), gmg):
            # Krylov on the handle's finest matrix with Pl = nothing / Jacobi / the finest pre-smoother
            if isinstance(P[0], LinearSolverFromSmoother):
                if P[0].smoother is not P[1].pre_smoothers[0]:
                    raise ValueError("LinearSolverFromSmoother must wrap the GMG's finest pre-smoother")
                self.pc_kind, gmg = 3, P[1]
            else:
                self.pc_kind, gmg = (0 if P[0] is None else 2), P[1]
        else:
            raise NotImplementedError("the device Krylov solvers take a GMGLinearSolver preconditioner "
                                      "(or (None|JacobiLinearSolver(), gmg) to reuse its finest matrix)")
        self.P_ns = GMGNumericalSetup(gmg, A, device_id)   # numerical_setup(symbolic_setup(Pl,A),A)
        self.n = self.P_ns.n
        if diag is not None:
            self.P_ns.cg_set_trace(max(diag.delta.size, 1))    # the allocation happens here, never in a solve

    @staticmethod
    def _side(P):
        """one side of GMRESSolver -> (selector, the solver object that owns the handle | None)"""
        if P is None:
            return 0, None
        if isinstance(P, (GMGLinearSolver,) + _BLOCK_SOLVERS):
            return 1, P
        if isinstance(P, tuple) and len(P) == 2:
            if isinstance(P[1], _BLOCK_SOLVERS) and P[0] is None:
                return 0, P[1]
            if isinstance(P[1], GMGLinearSolver):
                if P[0] is None:
                    return 0, P[1]
                if isinstance(P[0], JacobiLinearSolver):
                    return 2, P[1]
                if isinstance(P[0], LinearSolverFromSmoother):
                    if P[0].smoother is not P[1].pre_smoothers[0]:
                        raise ValueError("LinearSolverFromSmoother must wrap the GMG's finest pre-smoother")
                    return 3, P[1]
        raise NotImplementedError("a GMRES side is None, a GMGLinearSolver, a block solver, or (None | JacobiLinearSolver() | "
                                  "LinearSolverFromSmoother(...), gmg)")

    def _init_gmres(self, solver, A, device_id):
        (self.pr_kind, hr), (self.pl_kind, hl) = self._side(solver.Pr), self._side(solver.Pl)
        if hr is not None and hl is not None and hr is not hl:
            raise ValueError("Pr and Pl of GMRESSolver must name the same GMGLinearSolver / block solver (one device handle)")
        host = hr if hr is not None else hl
        if host is None:
            raise ValueError("GMRESSolver needs a device handle: pass Pr=(None, gmg) for the unpreconditioned solver")
        if self.pr_kind == 1 and self.pl_kind == 1:
            raise ValueError("the handle's preconditioner serves as Pr or as Pl of GMRESSolver, not both")
        self.pc_kind = self.pr_kind
        # numerical_setup(symbolic_setup(Pr,A),A) and the same for Pl (GMRESSolvers.jl:96-97): one handle holds both sides
        self.P_ns = (GMGNumericalSetup if isinstance(host, GMGLinearSolver) else BlockNumericalSetup)(host, A, device_id)
        self.n = self.P_ns.n

    def close(self):
        """releases the preconditioner's numerical setup (GMRES: the one handle that holds Pr and Pl)"""
        self.P_ns.close()


# ----------------------------------------------------------------------------
# null spaces (SolverInterfaces/NullSpaces.jl, LinearSolvers/NullspaceSolvers.jl)
# ----------------------------------------------------------------------------
class NullSpace:
    """struct NullSpace (NullSpaces.jl:1-31): `V` is a list of k vectors of equal length n.  NullSpace(list of vectors),
    NullSpace(n x k array) (the columns; what matrix_representation returns), NullSpace(vector) (:21).  The vectors are host copies;
    the algebra below runs on the device, on the copy `bind(ns)` uploads to the handle of a numerical setup."""

    def __init__(self, V):
        if isinstance(V, np.ndarray) and V.ndim == 2:
            vecs = [V[:, q] for q in range(V.shape[1])]
        elif isinstance(V, np.ndarray) and V.ndim == 1:
            vecs = [V]                                                           # :21
        else:
            vecs = list(V)
            if vecs and np.isscalar(vecs[0]):
                vecs = [vecs]
        if not vecs:
            raise ValueError("NullSpace: at least one vector")
        self.V = [np.array(v, dtype=np.float64).reshape(-1) for v in vecs]
        n = self.V[0].size
        if not all(v.size == n for v in self.V):                                 # @assert :7
            raise ValueError("NullSpace: all vectors must have the same length")
        self._ns = None

    @classmethod
    def from_matrix(cls, A):
        """NullSpace(A::Matrix) (:23-26): the columns of LinearAlgebra.nullspace(A) -- the right singular vectors whose singular value
        is <= min(size(A)) * eps * sigma_max.  On the host (setup only)."""
        A = np.asarray(A, dtype=np.float64)
        if A.ndim != 2:
            raise ValueError("NullSpace.from_matrix: a dense matrix is expected")
        _u, sv, vt = np.linalg.svd(A, full_matrices=True)
        tol = min(A.shape) * np.finfo(np.float64).eps * (sv[0] if sv.size else 0.0)
        r = int(np.sum(sv > tol))
        if r == A.shape[1]:
            raise ValueError("NullSpace.from_matrix: the matrix has a trivial null space")
        return cls([vt[i].copy() for i in range(r, A.shape[1])])

    def size(self, i=None):
        """Base.size(N) = (k, n) (:13-14)"""
        sz = (len(self.V), self.V[0].size)
        return sz if i is None else sz[i]

    def merge(self, other):
        """Base.merge(a, b) (:15)"""
        return NullSpace([v.copy() for v in self.V] + [v.copy() for v in other.V])

    def matrix_representation(self):
        """stack(N.V) (:17-19): n x k"""
        return np.stack(self.V, axis=1)

    # -- the device copy
    def bind(self, ns):
        """Upload the vectors to the handle behind `ns` (a GMG, block, Krylov or NullspaceSolver numerical setup); the algebra functions
        then run there.  Bind again after changing N.V on the host."""
        tgt = _ns_target(ns)
        k, n = self.size()
        if n != tgt.n:
            raise ValueError(f"NullSpace.bind: vectors of length {n}, the numerical setup has {tgt.n}")
        Vp = np.ascontiguousarray(np.stack(self.V, axis=0))
        _ns_call(tgt, "set", n, k, C.c_void_p(Vp.ctypes.data), n, abi.MEM_HOST)
        self._ns = tgt
        return self

    def unbind(self):
        """Remove the device copy (gmg_nullspace_set with k = 0: its storage is freed)."""
        if self._ns is not None and getattr(self._ns, "h", None):
            _ns_call(self._ns, "set", 0, 0, None, 0, abi.MEM_HOST)
        self._ns = None
        return self

    def gram(self):
        """G[i, j] = dot(w_i, w_j) on the device: what is_orthonormal / is_orthogonal(N) compare"""
        k = self.size(0)
        G = np.zeros((k, k))
        _ns_call(self._bound(), "gram", C.c_void_p(G.ctypes.data))
        return G

    def dots(self, v):
        """[dot(v, w_k) for w_k in N.V] on the device: what is_orthogonal(N, v) compares"""
        k, n = self.size()
        out = np.zeros(k)
        pv, ms, _k = _vec(v, n)                                                  # @assert NullSpaces.jl:50
        _ns_call(self._bound(), "dots", pv, C.c_void_p(out.ctypes.data), ms)
        return out

    def _bound(self):
        if self._ns is None or not getattr(self._ns, "h", None):
            raise RuntimeError("this NullSpace is not bound to a numerical setup: call N.bind(ns) first (the algebra runs on the device)")
        return self._ns

    def _download(self):
        k, n = self.size()
        Vp = np.zeros((k, n))
        _ns_call(self._bound(), "get", C.c_void_p(Vp.ctypes.data), n, abi.MEM_HOST)
        for q in range(k):
            self.V[q][:] = Vp[q]


def _ns_target(ns):
    """the numerical setup that owns the native handle"""
    while not isinstance(ns, (GMGNumericalSetup, BlockNumericalSetup)):
        if isinstance(ns, NullspaceNumericalSetup):
            ns = ns.ns
        elif isinstance(ns, _KrylovNumericalSetup):
            ns = ns.P_ns
        else:
            raise TypeError(f"a null space lives on a GMG, block or Krylov numerical setup, not {type(ns).__name__}")
    return ns


def _ns_call(tgt, name, *args):
    if isinstance(tgt, BlockNumericalSetup):
        return abi.check_block(tgt.h, getattr(tgt._lib, "gmg_block_nullspace_" + name)(tgt.h, *args))
    return abi.check(tgt.h, getattr(tgt._lib, "gmg_nullspace_" + name)(tgt.h, *args))


def is_orthogonal(N, other=None, tol=1.0e-12):
    """is_orthogonal(N) (NullSpaces.jl:40-47), is_orthogonal(N, v) (:49-55), is_orthogonal(N, A) (:57-65) with A given as
    (ns, A): the operator of the numerical setup N is bound to."""
    tgt = N._bound()
    k, n = N.size()
    if other is None:
        G = N.gram()
        return all(abs(G[i, j]) < tol for i in range(k) for j in range(i + 1, k))
    if isinstance(other, tuple):
        ns, A = other
        if _ns_target(ns) is not tgt:
            raise ValueError("is_orthogonal(N, (ns, A)): N is bound to another numerical setup")
        if A is not None and hasattr(A, "shape") and int(A.shape[1]) != n:       # @assert :58
            raise ValueError("is_orthogonal: size(A,2) != size(N,2)")
        out = np.zeros(k)
        _ns_call(tgt, "image_norms", C.c_void_p(out.ctypes.data))
    else:
        out = N.dots(other)
    return all(abs(a) < tol for a in out)


def is_orthonormal(N, tol=1.0e-12):
    """is_orthonormal(N) (NullSpaces.jl:33-38)"""
    k = N.size(0)
    G = N.gram()
    if not all(abs(np.sqrt(G[i, i]) - 1.0) < tol for i in range(k)):
        return False
    return all(abs(G[i, j]) < tol for i in range(k) for j in range(i + 1, k))


_ORTHO_METHODS = {"gram_schmidt": 0, "modified_gram_schmidt": 1}


def make_orthonormal_(N, method="gram_schmidt"):
    """make_orthonormal!(N; method) (NullSpaces.jl:67-76) on the device; N.V receives the orthonormal vectors."""
    if method not in _ORTHO_METHODS:
        raise ValueError(f"Unknown method: {method}")                            # :73
    _ns_call(N._bound(), "orthonormalize", _ORTHO_METHODS[method])
    N._download()
    return N


def gram_schmidt_(N):
    """gram_schmidt!(N.V) (NullSpaces.jl:78-88) -> N.V"""
    return make_orthonormal_(N, "gram_schmidt").V


def modified_gram_schmidt_(N):
    """modified_gram_schmidt!(N.V) (NullSpaces.jl:90-100) -> N.V"""
    return make_orthonormal_(N, "modified_gram_schmidt").V


def _like(v):
    if _is_device(v):
        import torch
        return torch.empty_like(v)
    return np.zeros(np.asarray(v).size)


def project_(p, N, v, subtract=False):
    """project!(p, N, v) (NullSpaces.jl:107-116) -> (p, alpha).  subtract=True also performs v .-= p in the same pass
    (NullspaceSolvers.jl:116); p may then be None."""
    tgt = N._bound()
    k, n = N.size()
    pv, ms, _kv = _vec(v, n, writable=bool(subtract))
    pp = None
    if p is not None:
        pp, ms2, _kp = _vec(p, n, writable=True)
        if ms != ms2:
            raise TypeError("p and v must live in the same memory space")
    alpha = np.zeros(k)
    _ns_call(tgt, "project", pv, pp, C.c_void_p(alpha.ctypes.data), ms, 1 if subtract else 0)
    return p, alpha


def project(N, v):
    """project(N, v) (NullSpaces.jl:102-105) -> (p, alpha)"""
    return project_(_like(v), N, v)


def make_orthogonal_(N, v):
    """make_orthogonal!(N, v) (NullSpaces.jl:118-126) -> (v, alpha)"""
    tgt = N._bound()
    k, n = N.size()
    pv, ms, _kv = _vec(v, n, writable=True)
    alpha = np.zeros(k)
    _ns_call(tgt, "make_orthogonal", pv, C.c_void_p(alpha.ctypes.data), ms)
    return v, alpha


def reconstruct_(N, v, alpha):
    """reconstruct!(N, v, alpha) (NullSpaces.jl:134-139) -> v"""
    tgt = N._bound()
    k, n = N.size()
    pv, ms, _kv = _vec(v, n, writable=True)
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    if a.size != k:
        raise ValueError(f"reconstruct!: {a.size} coefficients for {k} vectors")
    _ns_call(tgt, "reconstruct", pv, C.c_void_p(a.ctypes.data), ms)
    return v


def reconstruct(N, v, alpha):
    """reconstruct(N, v, alpha) (NullSpaces.jl:128-132) -> a new vector"""
    w = v.clone() if _is_device(v) else np.array(v, dtype=np.float64)
    return reconstruct_(N, w, alpha)


_KRYLOV_SOLVERS = (CGSolver, FGMRESSolver, MINRESSolver, GMRESSolver, RichardsonLinearSolver)


class NullspaceSolver:
    """NullspaceSolver(solver, nullspace; constrain_matrix=true) -- NullspaceSolvers.jl:30-43.
    constrain_matrix=False (:projected, :109-120): `solver` is any of the device Krylov solvers, on a GMG or a block handle; the
    numerical setup orthonormalises `nullspace` (Gram-Schmidt, :68 -- nullspace.V receives the result) and every solve starts from the
    initial guess with its kernel component removed.
    constrain_matrix=True (:constrained, :59-107): the augmented matrix needs a direct solver, and the device has one only on the
    coarsest level of a GMG: accepted as GMGLinearSolver(..., coarsest_solver=NullspaceSolver(LUSolver(), N_coarse))."""

    def __init__(self, solver, nullspace, constrain_matrix=True):
        if not isinstance(nullspace, NullSpace):
            raise TypeError("NullspaceSolver: nullspace must be a NullSpace")
        if not isinstance(solver, _KRYLOV_SOLVERS + (LUSolver,)):
            raise TypeError("NullspaceSolver: solver must be a Krylov solver of this package or LUSolver()")
        self.solver, self.nullspace, self.constrain_matrix = solver, nullspace, bool(constrain_matrix)


class NullspaceSymbolicSetup:
    """NullspaceSolverSS (NullspaceSolvers.jl:45-51)"""

    def __init__(self, solver):
        self.solver = solver


class NullspaceNumericalSetup:
    """NullspaceSolverNS{:projected} (NullspaceSolvers.jl:53-75): the inner solver's numerical setup, the null space on its handle."""

    def __init__(self, solver, A, device_id=None):
        self.solver = solver
        N = solver.nullspace
        self.ns = numerical_setup(symbolic_setup(solver.solver, A), A, device_id)
        self.n = self.ns.n
        try:
            if N.size(1) != self.n:                                              # @assert :63
                raise ValueError(f"NullspaceSolver: null-space vectors of length {N.size(1)}, the matrix has {self.n} rows")
            N.bind(self.ns)
            make_orthonormal_(N)                                                 # :68
            _ns_call(N._bound(), "project_guess", 1)
        except Exception:
            self.close()
            raise

    def close(self):
        self.ns.close()


def symbolic_setup(solver, A=None):
    """Gridap.Algebra.symbolic_setup(solver, A)."""
    if isinstance(solver, GMGLinearSolver):
        return GMGSymbolicSetup(solver)
    if isinstance(solver, (CGSolver, FGMRESSolver, MINRESSolver, GMRESSolver, RichardsonLinearSolver)):
        return _KrylovSymbolicSetup(solver)
    if isinstance(solver, _BLOCK_SOLVERS):
        return BlockSymbolicSetup(solver)
    if isinstance(solver, NullspaceSolver):
        if solver.constrain_matrix:
            raise NotImplementedError("NullspaceSolver(constrain_matrix=True) needs a direct solver for [A K; K' 0] and the device has no "
                                      "top-level direct solver: pass it as GMGLinearSolver(..., coarsest_solver=NullspaceSolver(LUSolver(), "
                                      "N_coarse)), or use the projected mode, NullspaceSolver(krylov_solver, N, constrain_matrix=False)")
        if not isinstance(solver.solver, _KRYLOV_SOLVERS):
            raise NotImplementedError("NullspaceSolver(constrain_matrix=False) wraps a Krylov solver (CG, FGMRES, MINRES, GMRES, Richardson)")
        return NullspaceSymbolicSetup(solver)
    raise TypeError(f"no symbolic_setup for {type(solver).__name__}")


def numerical_setup(ss, A=None, device_id=None):
    """Gridap.Algebra.numerical_setup(ss, A)."""
    if isinstance(ss, GMGSymbolicSetup):
        return GMGNumericalSetup(ss.solver, A, device_id)
    if isinstance(ss, _KrylovSymbolicSetup):
        return _KrylovNumericalSetup(ss.solver, A, device_id)
    if isinstance(ss, BlockSymbolicSetup):
        return BlockNumericalSetup(ss.solver, A, device_id)
    if isinstance(ss, NullspaceSymbolicSetup):
        return NullspaceNumericalSetup(ss.solver, A, device_id)
    raise TypeError(f"no numerical_setup for {type(ss).__name__}")


def numerical_setup_(ns, A, smatrices=None, x=None):
    """Gridap.Algebra.numerical_setup!(ns, A[, x]) (smatrices: re-assembled matrices of all levels, optional; for a block solver one
    list per diagonal block).  `x`, the linearisation point, is accepted and unused: the device takes assembled matrices
    (GridapExtras.jl:12-14 falls back to numerical_setup!(ns, A) in the same way)."""
    if isinstance(ns, (GMGNumericalSetup, BlockNumericalSetup)):
        return ns.update(A, smatrices)
    if isinstance(ns, _KrylovNumericalSetup):                  # FGMRESSolvers.jl:112-128: forwarded to the preconditioner
        ns.P_ns.update(A, smatrices)
        return ns
    if isinstance(ns, NullspaceNumericalSetup):                # NullspaceSolvers.jl:77-90: forwarded; the null space stays on the handle
        numerical_setup_(ns.ns, A, smatrices, x)
        return ns
    raise TypeError(f"no numerical_setup! for {type(ns).__name__}")


def solve_(x, ns, b):
    """Gridap.Algebra.solve!(x, ns, b): in place on x, returns x."""
    if isinstance(ns, NullspaceNumericalSetup):                # NullspaceSolvers.jl:109-120: the handle projects the initial guess
        return solve_(x, ns.ns, b)
    if isinstance(ns, GMGNumericalSetup):
        log = ns.solver.log
        pb, ms, _kb = _vec(b, ns.n)
        px, ms2, _kx = _vec(x, ns.n, writable=True)
        if ms != ms2:
            raise TypeError("x and b must live in the same memory space")
        if ms == abi.MEM_HOST and ns.solver.pin_vectors:
            ns.pin(*(k for k, u in ((_kb, b), (_kx, x)) if k is u))       # the caller's own arrays only, never a conversion copy
        res = abi.Result()
        hist = np.zeros(log.maxiter + 1)
        abi.check(ns.h, ns._lib.gmg_apply(ns.h, pb, px, ms, C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        return x
    if isinstance(ns, BlockNumericalSetup):
        pb, ms, _kb = _vec(b, ns.n)
        px, ms2, _kx = _vec(x, ns.n, writable=True)
        if ms != ms2:
            raise TypeError("x and b must live in the same memory space")
        abi.check_block(ns.h, ns._lib.gmg_block_precond_apply(ns.h, pb, px, ms))
        ns._fill_logs()
        return x
    if isinstance(ns, _KrylovNumericalSetup) and isinstance(ns.P_ns, BlockNumericalSetup):
        s, g = ns.solver, ns.P_ns
        log = s.log
        pb, ms, _kb = _vec(b, ns.n)
        px, ms2, _kx = _vec(x, ns.n, writable=True)
        if ms != ms2:
            raise TypeError("x and b must live in the same memory space")
        res = abi.Result()
        hist = np.zeros(log.maxiter + 1)
        if isinstance(s, CGSolver):
            abi.check_block(g.h, g._lib.gmg_block_cg_solve(g.h, pb, px, ms, log.maxiter, log.atol, log.rtol, int(s.flexible),
                                                           ns.pc_kind, C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        elif isinstance(s, MINRESSolver):
            abi.check_block(g.h, g._lib.gmg_block_minres_solve(g.h, pb, px, ms, log.maxiter, log.atol, log.rtol, ns.pc_kind,
                                                               C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        elif isinstance(s, GMRESSolver):
            abi.check_block(g.h, g._lib.gmg_block_gmres_solve(g.h, pb, px, ms, s.m, int(s.restart), s.m_add, log.maxiter,
                                                              log.atol, log.rtol, ns.pr_kind, ns.pl_kind, C.byref(res),
                                                              C.c_void_p(hist.ctypes.data), hist.size))
        else:
            abi.check_block(g.h, g._lib.gmg_block_fgmres_solve(g.h, pb, px, ms, s.m, int(s.restart), s.m_add, log.maxiter,
                                                               log.atol, log.rtol, ns.pc_kind, C.byref(res),
                                                               C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        g._fill_logs()
        return x
    if isinstance(ns, _KrylovNumericalSetup):
        s, g = ns.solver, ns.P_ns
        log = s.log
        pb, ms, _kb = _vec(b, ns.n)
        px, ms2, _kx = _vec(x, ns.n, writable=True)
        if ms != ms2:
            raise TypeError("x and b must live in the same memory space")
        if ms == abi.MEM_HOST and g.solver.pin_vectors:
            g.pin(*(k for k, u in ((_kb, b), (_kx, x)) if k is u))
        res = abi.Result()
        hist = np.zeros(log.maxiter + 1)
        if isinstance(s, CGSolver):
            abi.check(g.h, g._lib.gmg_cg_solve(g.h, pb, px, ms, log.maxiter, log.atol, log.rtol, int(s.flexible), ns.pc_kind,
                                               C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        elif isinstance(s, MINRESSolver):
            abi.check(g.h, g._lib.gmg_minres_solve(g.h, pb, px, ms, log.maxiter, log.atol, log.rtol, ns.pc_kind,
                                                   C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        elif isinstance(s, GMRESSolver):
            abi.check(g.h, g._lib.gmg_gmres_solve(g.h, pb, px, ms, s.m, int(s.restart), s.m_add, log.maxiter, log.atol,
                                                  log.rtol, ns.pr_kind, ns.pl_kind, C.byref(res),
                                                  C.c_void_p(hist.ctypes.data), hist.size))
        elif isinstance(s, RichardsonLinearSolver):
            abi.check(g.h, g._lib.gmg_richardson_solve(g.h, pb, px, ms, s.omega, log.maxiter, log.atol, log.rtol, ns.pc_kind,
                                                       C.byref(res), C.c_void_p(hist.ctypes.data), hist.size))
        else:
            pl = getattr(s, "Pl", None)
            pl_kind = 0 if pl is None else (2 if isinstance(pl, JacobiLinearSolver) else 3)
            abi.check(g.h, g._lib.gmg_fgmres_solve_pl(g.h, pb, px, ms, s.m, int(s.restart), s.m_add, log.maxiter,
                                                      log.atol, log.rtol, ns.pc_kind, pl_kind, C.byref(res),
                                                      C.c_void_p(hist.ctypes.data), hist.size))
        log._fill(res, hist)
        if isinstance(s, CGSolver) and s.diag is not None:
            s.diag.replay_(*g.cg_trace())
        if ns.pc_kind == 1 or getattr(ns, "pl_kind", 0) == 1:
            g.fill_log()
        return x
    raise TypeError(f"no solve! for {type(ns).__name__}")


def mul_(y, op, x):
    """LinearAlgebra.mul!(y, op, x) for op = (ns, lev, 'A'|'P'|'R')."""
    ns, lev, which = op
    return ns.op_apply(lev, {"A": abi.OP_A, "P": abi.OP_P, "R": abi.OP_R}[which], x, y)
