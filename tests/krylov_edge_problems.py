"""Inputs and references of the Krylov edge-length tests (tests/test_krylov_edge_problems.py on the host,
tests/test_gpu_krylov_edges.py on the device).  Plain helper: no fixtures, no collection hooks.

problem(N, kind, seed)  banded, strictly diagonally dominant matrices of any length N (so the vector length is free, which
                        the Poisson problems' (nc-1)^d is not) whose Krylov iteration counts do not depend on N
split(A, N)             the 2 x 2 nested block list with an ODD first block: block 1 of every block vector starts 8 bytes
                        off a 16-byte boundary
reference(key, N, orc)  the sequential reference of one solver on the monolithic matrix (cached per (key, N))

LENGTHS, checked against the launch geometry of csrc/gmg_amd.hip and csrc/kernels.hpp (kBlock = 256, kRedBlocks = 1024):

  dot_grid(n) = clamp((n/2 + 255) / 256, 1, 1024)   dot_partial_kernel, gmres_mgs_kernel (n2 = n >> 1 double2 elements per vector)
  grid_for(n) = clamp((n + 255) / 256, 1, 2048)     element-wise kernels; gmres_normalize_kernel / gmres_combine_kernel run their
                                                    n >> 1 double2 elements on this grid
  nb          = clamp((n + 255) / 256, 1, 1024)     cg_update_kernel, xpby_dev_kernel, minres_lanczos_kernel, minres_update_kernel
                                                    (cg_core / minres_core; one double per lane)

  1, 2, 3          n2 = 0 or 1: every element of the double2 kernels goes through the odd-tail branch, or none does
  63, 64, 65       around one wave
  511, 512, 513    dot_grid = 1 with n2 = 255, 256, 256: 512 is exactly one workgroup of the double2 path, 513 adds the tail
  1023, 1024       grid_for = nb = 4, ragged and full
  65536, 65537     nb goes 256 -> 257 partials: the stride of sum_partials_all / reduce_final_kernel for the kernels on the nb
                   grid.  ADDED to the list of the issue, which names only dot_grid's crossing:
  131072, 131074, 131075   dot_grid = 256, 257, 257 (131074 is the first length with 257 dot partials), even and odd
  262144, 262145   nb = 1024 saturates at 262144 elements: 262145 is the first second trip of the grid-stride loops of the
                   kernels on the nb grid.  ADDED (the issue's list has no length between 131075 and 524287).
  524287, 524288, 524289   grid_for = 2048 saturates at 524288 elements: 524288 is the last one-trip length of the element-wise
                   kernels and 524289 their first second trip (the issue calls 524287 the last one-trip length; it is the last
                   ragged one).  dot_grid saturates earlier, at n = 523778, but its double2 loop covers 2 * 1024 * 256 = 524288
                   elements per trip, the odd tail making 524289 still one trip:
  524290           the first second trip of dot_partial_kernel's and gmres_mgs_kernel's double2 loop.  ADDED.
  1048578          even; n2 = 524289: the first second trip of gmres_normalize_kernel / gmres_combine_kernel (double2 on grid_for),
                   two full trips plus two elements of the element-wise kernels, two trips plus one double2 of the dot
  1572867          odd; three full trips plus 3 elements (element-wise), three full trips plus one double2 plus the tail (dot)
"""
import numpy as np
import scipy.sparse as sp

import __graft_entry__ as entry
import gmres_reference as gr
import minres_reference as mr

SMALL = [1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 65536, 65537, 131072, 131074, 131075, 262144, 262145]
LARGE = [524287, 524288, 524289, 524290, 1048578, 1572867]
LENGTHS = SMALL + LARGE

KINDS = ("spd", "indefinite", "nonsym")
TOL = dict(maxiter=100, atol=1e-30, rtol=1e-8)          # atol out of the picture: every stop is the relative one
# MINRES on the indefinite matrices contracts about half as fast per iteration as CG on the SPD ones (the runs of 5 rows put the
# spectrum on both sides of 0): rtol = 1e-8 takes 43 .. 68 iterations, above the 60 the host test allows, rtol = 1e-6 at most 51
TOL_OF = {"minres": dict(TOL, rtol=1e-6)}


def tol(key):
    return TOL_OF.get(key, TOL)


M_GMRES = 10

# (kind, N) -> seed, where the default seed 0 leaves a deciding residual within 1 % of rtol * hist[0] for one of the solvers on
# that matrix (tests/test_krylov_edge_problems.py asserts the margin for every pair)
SEEDS = {}


def seed_of(kind, N):
    return SEEDS.get((kind, N), 0)


def problem(N, kind, seed=None):
    """-> (A scipy CSR with sorted indices, b).  Bands +-1 (N < 9) or +-1 and +-(N // 3); off-diagonal entries U(-1, 1), mirrored
    for "spd" and "indefinite", independent for "nonsym"; |d_i| = 1 + sum_j |a_ij| + U(0, 1), sign + ("spd", "nonsym") or
    alternating in runs of 5 rows ("indefinite"): every Gershgorin disc stays at modulus >= 1.  b ~ U(-1, 1) without a zero."""
    N = int(N)
    if kind not in KINDS:
        raise ValueError(kind)
    if seed is None:
        seed = seed_of(kind, N)
    rng = np.random.default_rng([int(seed), N, KINDS.index(kind)])
    offsets = [k for k in ([1] if N < 9 else [1, N // 3]) if k < N]
    rowsum = np.zeros(N)
    diags, where = [], []
    for k in offsets:
        up = rng.uniform(-1.0, 1.0, N - k)                          # a[i, i + k]
        lo = up if kind != "nonsym" else rng.uniform(-1.0, 1.0, N - k)   # a[i + k, i]
        rowsum[: N - k] += np.abs(up)
        rowsum[k:] += np.abs(lo)
        diags += [up, lo]
        where += [k, -k]
    d = 1.0 + rowsum + rng.uniform(0.0, 1.0, N)
    if kind == "indefinite":
        d = np.where((np.arange(N) // 5) % 2 == 0, d, -d)
    A = sp.diags([d] + diags, [0] + where, shape=(N, N), format="csr")
    A.sort_indices()
    b = rng.uniform(-1.0, 1.0, N)
    b[b == 0.0] = 0.5
    return A, b


def _po():
    return entry.import_package().poisson


def csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return _po().CSR(M.shape, M.indptr, M.indices, M.data)


def first_block(N):
    """n1 of split(): odd, so block 1 starts at an odd element offset"""
    return (int(N) // 2) | 1


def split(A, N):
    """the 2 x 2 nested block list of po.CSR with n1 = (N // 2) | 1 (N >= 4), or [[A]] (N < 4)"""
    if N < 4:
        return [[csr(A)]]
    n1 = first_block(N)
    A = A.tocsr()
    top, bot = A[:n1], A[n1:]
    return [[csr(top[:, :n1]), csr(top[:, n1:])], [csr(bot[:, :n1]), csr(bot[:, n1:])]]


def abs_diag_blocks(A, N):
    """diag(|a_ii|) per block of split(): the matrices a Jacobi block solver turns into the SPD preconditioner r / |d|"""
    d = np.abs(A.diagonal())
    cuts = [0, N] if N < 4 else [0, first_block(N), N]
    return [csr(sp.diags([d[i:j]], [0], format="csr")) for i, j in zip(cuts[:-1], cuts[1:])]


# ---------------------------------------------------------------- solvers: key -> (matrix kind, lengths)
# A pair may be missing only where the reference itself produces a non-finite value (the Krylov space is exhausted at N <= 3);
# each such drop is named here with what the reference does.
SOLVERS = {
    "cg": "spd",
    "fcg": "spd",
    "minres": "indefinite",
    "fgmres": "nonsym",
    "gmres-none": "nonsym",
    "gmres-pr": "nonsym",
    "gmres-pl": "nonsym",
}
# minres, N = 2: the Lanczos space is exhausted in iteration 2, dot(Znew, Vnew) is rounding noise and comes out negative --
#   minres_reference raises NotPositiveDefinite("beta_p = -2.5453014913383256e-30 in iteration 2"), the sqrt(beta_p) DomainError
#   of MINRESSolvers.jl:116 (a NaN gamma_new in plain arithmetic).  N = 1 and N = 3 stay: their noise comes out positive.
DROPPED = {"minres": (2,)}


def lengths(key, which=None):
    return [N for N in (LENGTHS if which is None else which) if N not in DROPPED.get(key, ())]


INNER_CG_LENGTHS = [65, 513, 131075, 524289]            # the extra CG case: CG(Jacobi, maxiter = 3) on block 1, odd lengths
INNER_CG = dict(maxiter=3, atol=1e-30, rtol=1e-30)      # never converges: always three inner iterations


_REF = {}


def reference(key, N, orc):
    """-> (x, niters, flag, hist) of the sequential reference on the monolithic matrix; orc = the CPU oracle module.  The
    returned arrays are shared: do not write to them."""
    if (key, N) in _REF:
        return _REF[(key, N)]
    kind = "spd" if key == "cg-inner" else SOLVERS[key]
    A, b = problem(N, kind)
    K = csr(A)
    mul = lambda v: orc.spmv(K, v)
    red = dict(dot=orc.dot, norm=orc.norm, givens=orc.givens)
    with np.errstate(all="ignore"):
        if key == "cg":
            ref = orc.cg_solve(K, b, Pl="jacobi", **tol(key))
        elif key == "fcg":
            ref = orc.cg_solve(K, b, Pl="jacobi", flexible=True, **tol(key))
        elif key == "cg-inner":
            n1 = first_block(N)
            blocks = split(A, N)
            P = orc.BlockPreconditioner([n1, N - n1], [(orc.BD_JACOBI, blocks[0][0]),
                                                       (orc.BD_CG_JACOBI, blocks[1][1], INNER_CG["maxiter"], INNER_CG["atol"], INNER_CG["rtol"])],
                                        None, orc.DIAGONAL)
            ref = orc.cg_solve(K, b, Pl=P, **tol(key))
        elif key == "minres":
            dinv = 1.0 / np.abs(A.diagonal())
            ref = mr.minres(mul, b, lambda r: dinv * r, **red, **tol(key))
        elif key == "fgmres":
            ref = orc.fgmres_solve(K, b, Pr="jacobi", m=M_GMRES, restart=True, **tol(key))
        else:
            dinv = orc.jacobi_inv_diag(K)
            jac = lambda r: dinv * r
            sides = {"gmres-none": {}, "gmres-pr": dict(Pr=jac), "gmres-pl": dict(Pl=jac)}[key]
            ref = gr.gmres(mul, b, M_GMRES, restart=True, **sides, **red, **tol(key))
    for a in (ref[0], ref[3]):
        a.setflags(write=False)
    _REF[(key, N)] = ref
    return ref
