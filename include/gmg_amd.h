/*
 * gmg_amd.h -- C ABI of libgmgamd.so, the MI355X (gfx950) geometric-multigrid
 * V-cycle / CG / FGMRES hot path for GridapSolvers.jl.
 *
 * The reference (GridapSolvers.jl v0.7.1) is pure Julia and has no FFI for this
 * path; its drop-in boundary is the Gridap.Algebra interface
 *     LinearSolver -> symbolic_setup -> numerical_setup(!) -> solve!
 * Each entry point below names the reference method(s) (file:line) whose work
 * it takes over; the Julia wrapper that binds them with `ccall` is in
 * gridapsolvers.jl_amd/julia/GridapSolversAMD.jl and INTEGRATION.md.
 *
 * Conventions
 *   - every function returns an int status (GMG_OK == 0); nothing throws or
 *     longjmps across the boundary; gmg_last_error() gives the message.
 *   - all pointers passed to setters are HOST pointers borrowed for the call
 *     only.  Vector arguments of the solve / operator calls are host or device
 *     pointers according to `memspace`.
 *   - one handle = one HIP device + one HIP stream; not thread-safe per handle.
 *   - levels are numbered 0 .. nlevels-1, level 0 = finest (reference: 1 = finest).
 *   - fp64 values; integer indices int32 or int64, 0- or 1-based, CSR or CSC.
 */
#ifndef GMG_AMD_H
#define GMG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMG_API __attribute__((visibility("default")))

typedef struct gmg_solver *gmg_handle_t;

enum gmg_status {
  GMG_OK = 0,
  GMG_ERR_INVALID = 1,     /* bad argument / inconsistent sizes (reference: @check failures) */
  GMG_ERR_HIP = 2,         /* a HIP runtime call failed */
  GMG_ERR_STATE = 3,       /* call order violated (e.g. solve before setup) */
  GMG_ERR_ALLOC = 4,
  GMG_ERR_COMM = 5,        /* RCCL failure */
  GMG_ERR_UNSUPPORTED = 6,
  GMG_ERR_SINGULAR = 7     /* zero pivot / zero diagonal */
};

enum gmg_layout { GMG_CSR = 0, GMG_CSC = 1 };
enum gmg_memspace { GMG_MEM_HOST = 0, GMG_MEM_DEVICE = 1 };
/* GMGLinearSolvers.jl:56 mode ; :57 cycle_type */
enum gmg_mode { GMG_MODE_PRECONDITIONER = 0, GMG_MODE_SOLVER = 1 };
enum gmg_cycle { GMG_V_CYCLE = 0, GMG_W_CYCLE = 1, GMG_F_CYCLE = 2 };
/* SolverInterfaces/SolverTolerances.jl:11-16 SolverConvergenceFlag */
enum gmg_conv_flag {
  GMG_CONVERGED_ATOL = 0,
  GMG_CONVERGED_RTOL = 1,
  GMG_DIVERGED_MAXITER = 2,
  GMG_DIVERGED_BREAKDOWN = 3
};
enum gmg_which { GMG_PRE = 0, GMG_POST = 1, GMG_PRE_AND_POST = 2 };
enum gmg_patch_kind {
  GMG_PATCH_LU = 0,        /* PatchSolver: lu!(A[p,p]) with partial pivoting, PatchSolvers.jl:176 */
  GMG_PATCH_NOPIVOT = 1    /* BlockJacobiSolver: lu!(A[p,p],NoPivot()), BlockJacobiSolvers.jl:162 */
};
enum gmg_op { GMG_OP_A = 0, GMG_OP_P = 1, GMG_OP_R = 2 };

/* Result of an iterative solve: mirrors ConvergenceLog (ConvergenceLogs.jl:42-60). */
typedef struct {
  int32_t niters;          /* log.num_iters */
  int32_t flag;            /* finalize!(log,res) -> gmg_conv_flag */
  double res0;             /* log.residuals[1] */
  double res;              /* last residual */
} gmg_result;

/* Timing / traffic statistics of the profiled kernel class (gmg_profile_enable). */
typedef struct {
  int64_t launches;        /* sweeps measured (one per launch, except on levels that run a whole smoothing pass as ONE
                              launch -- see fused_passes -- where a pass of niter sweeps counts niter) */
  double total_ms;         /* sum of HIP-event durations on the handle's stream */
  double alg_bytes;        /* algorithmic bytes of ONE launch (SURVEY 8d byte model) */
  int64_t rows, nnz;       /* shape of the operator the kernel streams */
  double layout_bytes;     /* bytes ONE launch moves with the storage layout chosen at setup (matrix stream as
                              stored + row-wise vectors, each once): equals alg_bytes only for the plain 12 B/nnz
                              layouts; far smaller for the row-pattern / dictionary layouts */
  int64_t fused_passes;    /* measured smoothing passes that ran as one launch (sells_smooth_kernel: small single-GPU
                              levels in the row-pattern layout); 0 on levels swept launch by launch */
} gmg_kernel_stats;

/* ---- lifetime ------------------------------------------------------------- */
/* GMGLinearSolver(...) constructor, GMGLinearSolvers.jl:48-69 (allocates nothing on device yet). */
GMG_API int gmg_create(gmg_handle_t *h, int nlevels, int device_id);
/* finalizer of the numerical setup (pattern: ext/PardisoExt.jl:54-61). */
GMG_API int gmg_destroy(gmg_handle_t h);
GMG_API const char *gmg_last_error(gmg_handle_t h); /* h may be NULL: last global error */
GMG_API int gmg_version(void);

/* ---- operators (numerical_setup inputs) ------------------------------------ */
/* smatrices[lev+1], GMGLinearSolvers.jl:183-185,336-340.  Square. */
GMG_API int gmg_set_matrix(gmg_handle_t h, int lev, int64_t nrows, int64_t ncols, int64_t nnz,
                           const void *ptr, const void *idx, const double *val,
                           int layout, int index_base, int index_bytes);
/* The same operators (op = GMG_OP_A, GMG_OP_P or GMG_OP_R of level lev) handed over as a STREAM of consecutive row blocks,
 * for hierarchies whose CSR the host cannot or need not hold at once (BASELINE config 3: 8.5e9 nonzeros on the finest level).
 * Each call passes rows [row0, row0 + nrows_block) as a standalone CSR (ptr has nrows_block+1 entries starting at
 * index_base, columns are global, sorted and duplicate-free); row0 = 0 (re)starts the stream, blocks arrive in order, the
 * operator is complete when row0 + nrows_block = nrows_total.  The library keeps only the row-pattern form (a pattern id
 * per row + the dictionary of distinct rows): host memory is O(block).  Operators with more than 4096 distinct rows
 * (variable coefficients, unstructured meshes) are rejected with GMG_ERR_UNSUPPORTED -- pass those whole.
 * A streamed P needs a streamed R (R = P^T is not formed from a stream); the coarsest matrix is passed whole unless the
 * coarse solver is iterative / a callback.  Several ranks: levels that are laid out like a single-GPU level -- the overlapping
 * layout (gmg_set_partition_overlap: one square local operator over the extended box) and the replicated levels -- keep the stream
 * form, transfers included; the matrix of an own | ghost level (gmg_set_partition, called BEFORE the first block) is streamed with
 * its local shape n_own x (n_own + n_ghost): every block is split into the own x own part, which goes to the stream, and the
 * entries in ghost columns, which become the small CSR the boundary fix-up applies once the halo has arrived. */
GMG_API int gmg_set_operator_rows(gmg_handle_t h, int lev, int op, int64_t nrows_total, int64_t ncols, int64_t row0,
                                  int64_t nrows_block, const void *ptr, const void *idx, const double *val,
                                  int index_base, int index_bytes);
/* Structured operators: append `count` further copies of the LAST nrows_block rows handed over, copy k with all its column
 * indices shifted by k * col_shift (uniform meshes: every interior node plane repeats the previous one).  No arrays cross the
 * boundary and nothing is hashed again; for level matrices col_shift must equal nrows_block.  No reference counterpart (the
 * reference assembles every row, GMGLinearSolvers.jl:342-353). */
GMG_API int gmg_set_operator_rows_repeat(gmg_handle_t h, int lev, int op, int64_t nrows_block, int64_t count, int64_t col_shift);
/* numerical_setup!(ns,A): same pattern, new values in the handle's 0-based CSR order (GMGLinearSolvers.jl:249-297;
 * JacobiLinearSolvers.jl:25-27), any level.  Requires gmg_setup to be called again; when nothing but values changed
 * since the last setup and the refreshed levels are stored with explicit values (SELL-64 / CSR-stream: what
 * variable-coefficient operators get), that gmg_setup keeps every layout, table and work vector and only rewrites the
 * value arrays, D^-1, the patch inverse blocks and the coarse inverse on the device -- bit-identical to a fresh setup.
 * Dictionary / row-pattern layouts depend on the values themselves: those levels trigger a full setup. */
GMG_API int gmg_update_values(gmg_handle_t h, int lev, const double *val);
/* The same for a level whose matrix was handed to gmg_set_matrix in GMG_CSC layout (Julia's SparseMatrixCSC, Gridap's default):
 * `val` = the new nzval in CSC order.  The first call on a level also takes the (unchanged) colptr / rowidx and records where
 * the transposition of gmg_set_matrix put every entry; later calls may pass NULL for both and cost one parallel scatter -- no
 * `sparse(transpose(A))` on the caller's side.  numerical_setup!(ns,A) of the weak-form variant refreshes EVERY level this way
 * (GMGLinearSolvers.jl:260-297: smatrices, smoothers and the coarsest solver are all recomputed). */
GMG_API int gmg_update_values_csc(gmg_handle_t h, int lev, const void *colptr, const void *rowidx, const double *val,
                                  int index_base, int index_bytes);
/* interp[lev+1] : level lev+1 -> lev, `mul!(dxh,interp,dxH)` GMGLinearSolvers.jl:491
 * (y = P x, GridTransferOperators.jl:391-401).  nrows = n(lev), ncols = n(lev+1). */
GMG_API int gmg_set_prolongation(gmg_handle_t h, int lev, int64_t nrows, int64_t ncols, int64_t nnz,
                                 const void *ptr, const void *idx, const double *val,
                                 int layout, int index_base, int index_bytes);
/* restrict[lev+1] : level lev -> lev+1, `mul!(rH,restrict,rh)` :484.  Optional:
 * when absent R = P^T is built (GridTransferOperators.jl:202-209,536-547). */
GMG_API int gmg_set_restriction(gmg_handle_t h, int lev, int64_t nrows, int64_t ncols, int64_t nnz,
                                const void *ptr, const void *idx, const double *val,
                                int layout, int index_base, int index_bytes);

/* Galerkin coarse matrices: level lev (1 .. nlevels-1) takes A_lev = R (A P) of level lev-1 instead of a matrix of the caller's --
 * the algebraic alternative of hypre / AMGX / PETSc PCMG to GMGLinearSolverFromMatrices (GMGLinearSolvers.jl:336-340), which needs
 * the assembled matrix of every level.  No reference counterpart.  In two stages, bit for bit:
 *   T = A P        T(i, J) = sum over k ascending of A(i, k) * P(k, J)
 *   A_lev = R T    A_lev(I, J) = sum over i ascending of R(I, i) * T(i, J)
 * every sum from 0.0, every product and every sum rounded separately, only stored entries contribute.  The patterns are the structural
 * products pattern(A) pattern(P) and pattern(R) pattern(T): explicit zeros of the inputs count, an entry whose terms cancel to 0.0
 * stays stored, columns ascend in every row.  R is the restriction of level lev-1 if one was set, else P^T.  Inputs with unsorted rows
 * are sorted in temporary copies (a column stored twice in a row: GMG_ERR_INVALID at gmg_setup).  Levels chain: level 2 from a
 * Galerkin level 1.
 * gmg_set_galerkin clears a matrix set earlier on the level; a later gmg_set_matrix / gmg_set_operator_rows on it clears the mark.
 * Level 0: GMG_ERR_INVALID.  gmg_update_values[_csc] on such a level: GMG_ERR_STATE.
 * The products are formed at the start of gmg_setup, finest first: patterns on the host, once per structure (kept until an operator
 * the product reads is set again), values on the device by two launches of a gather kernel, one lane per stored entry, no atomics.
 * The level is then treated exactly as if the caller had passed that matrix to gmg_set_matrix (layout choice included), the device
 * temporaries are freed: gmg_device_bytes equals that of a handle given the same matrices.  After gmg_update_values[_csc] on a finer
 * level the next gmg_setup forms the values again (numeric phase only) and hands them on as gmg_update_values would, so the usual
 * rule decides between the in-place value refresh and a full setup.  The values pass through the host.
 * Refused at gmg_setup with GMG_ERR_UNSUPPORTED, naming the level: a communicator of more than one rank, real or loopback (the local
 * rows do not hold the off-rank terms); a matrix or transfer of the finer level that the caller streamed with gmg_set_operator_rows
 * (no rows to take; a matrix gmg_set_matrix keeps in row-pattern form gives its rows back).  A missing prolongation: GMG_ERR_STATE. */
GMG_API int gmg_set_galerkin(gmg_handle_t h, int lev);
/* The matrix of a Galerkin level after gmg_setup, 0-based CSR: ptr[nrows + 1], col[nnz], val[nnz].  All three arrays NULL: size
 * query.  cap_nnz < nnz: GMG_ERR_INVALID.  A level that is not Galerkin: GMG_ERR_STATE.  Any output may be NULL. */
GMG_API int gmg_get_galerkin_matrix(gmg_handle_t h, int lev, int64_t *nrows, int64_t *nnz, int64_t *ptr, int32_t *col, double *val,
                                    int64_t cap_nnz);
/* What the last product of the level cost: host time of the symbolic phase (0 where the patterns were kept) and the HIP-event times
 * of the two launches (T = A P, A_lev = R T), in ms.  Any output may be NULL. */
GMG_API int gmg_get_galerkin_timing(gmg_handle_t h, int lev, double *symbolic_ms, double *ap_ms, double *rt_ms);
/* The symbolic phase itself, without a handle and without a GPU: 0-based CSR patterns of R (nc x nf), A (nf x nf), P (nf x nc), rows in
 * any order -> the patterns of T = A P (tptr[nf + 1], tcol) and of R A P (cptr[nc + 1], ccol), columns ascending.  *tnnz / *cnnz: the
 * entry counts; all four arrays NULL: size query; tcap / ccap smaller than that: GMG_ERR_INVALID.  gmg_setup calls the same code. */
GMG_API int gmg_galerkin_pattern(int64_t nc, int64_t nf, const int64_t *rptr, const int32_t *rcol, const int64_t *aptr,
                                 const int32_t *acol, const int64_t *pptr, const int32_t *pcol, int64_t *tptr, int32_t *tcol,
                                 int64_t tcap, int64_t *tnnz, int64_t *cptr, int32_t *ccol, int64_t ccap, int64_t *cnnz);

/* Smoothed-aggregation prolongations: level lev (0 .. nlevels-2) takes P_lev built from A_lev on the device at gmg_setup instead of a
 * prolongation of the caller's -- with gmg_set_galerkin on the levels below, a hierarchy without any mesh hierarchy (what the reference
 * leaves to PETSc GAMG).  No reference counterpart.  The construction is fixed, bit for bit (tests/aggregation_reference.py):
 *   strength    m_i = max over stored k != i of |a_ik|; (i, j), j != i, a_ij != 0, is row-strong iff |a_ij| >= theta * m_i; {i, j} is an
 *               edge iff (i, j) or (j, i) is row-strong; w_ij = max(|a_ij|, |a_ji|).  Explicit zeros are legal and never strong.
 *   MIS-2       priorities (key_i, i), key_i = the splitmix64 finaliser of i + 0x9E3779B97F4A7C15 (seed + 1); synchronous rounds
 *               until no node is undecided: the undecided node that is the maximum of its distance-2 neighbourhood becomes a root,
 *               undecided nodes within distance 2 of a root become covered
 *   aggregates  roots numbered in ascending row index; a root's neighbours join it; every other node joins the aggregate of the
 *               neighbour assigned so far with the largest w_ij, ties to the smallest index
 *   P           smooth = 0: one 1.0 per row at column agg(i).  smooth != 0: (I - omega D^-1 A) T, row i over {agg(k) : (i, k) stored}
 *               ascending, P(i, J) = [J == agg(i)] - (omega (1 / a_ii)) * (sum over stored k ascending with agg(k) = J of a_ik),
 *               every product and sum rounded separately
 *   omega       the argument if > 0, else (4/3) / rho with rho = max_i (sum_k |a_ik|) / |a_ii|, the infinity-norm bound of D^-1 A: the
 *               same bits on every run, and an under-smoothing against the true largest eigenvalue
 * theta in [0, 1] (0.25 is the usual choice), seed >= 0.  The near-null space is the constant vector; vector-valued candidates
 * (rigid-body modes), filtered matrices and partitioned handles are not built.
 * A_lev needs a stored nonzero diagonal in every row (GMG_ERR_SINGULAR at gmg_setup, naming the row) and a structurally symmetric
 * stored pattern (checked on the device; GMG_ERR_INVALID naming the first offending (i, j)).
 * At gmg_setup, finest level first: A_lev (the caller's, or the Galerkin product just formed) is aggregated, P_lev is installed exactly
 * as gmg_set_prolongation installs a caller's matrix, the product of level lev+1 follows; every size below is taken from the result.
 * The device temporaries are freed and never part of gmg_device_bytes.  After gmg_update_values on a finer level the next gmg_setup
 * keeps the aggregates, the pattern of P and the Galerkin patterns and forms rho, omega, the values of P and the products again -- the
 * strength of connection is NOT evaluated again; gmg_set_matrix aggregates afresh.  A later gmg_set_prolongation clears the mark.
 * Refused at gmg_setup with GMG_ERR_UNSUPPORTED or GMG_ERR_INVALID, naming the level: a communicator of more than one rank, real or
 * loopback; a level matrix streamed with gmg_set_operator_rows; a patch-corrected prolongation or an explicit restriction on the
 * level; level lev+1 not marked with gmg_set_galerkin; values_f32 (refuses the Galerkin level); a level that does not coarsen
 * (as many aggregates as rows); a patch-based smoother or prolongation on level lev+1, whose tables cannot match. */
GMG_API int gmg_set_aggregation(gmg_handle_t h, int lev, double theta, int smooth, double omega, int64_t seed);
/* The aggregate of every row of the level, 0 .. *nagg-1, as the last gmg_setup formed them (also after a gmg_setup that refused the
 * level because it does not coarsen).  agg NULL: size query; cap < rows: GMG_ERR_INVALID.  No aggregates yet: GMG_ERR_STATE. */
GMG_API int gmg_get_aggregates(gmg_handle_t h, int lev, int64_t *nagg, int32_t *agg, int64_t cap);
/* The prolongation of an aggregated level after gmg_setup, 0-based CSR: ptr[nrows + 1], col[nnz], val[nnz].  All three arrays NULL:
 * size query.  ptr_cap < nrows + 1 or nnz_cap < nnz: GMG_ERR_INVALID.  A level without aggregation: GMG_ERR_STATE. */
GMG_API int gmg_get_prolongation(gmg_handle_t h, int lev, int64_t *nrows, int64_t *ncols, int64_t *nnz, int64_t *ptr, int32_t *col,
                                 double *val, int64_t ptr_cap, int64_t nnz_cap);
/* What the last aggregation of the level did: rounds of the independent set, omega and rho in use, edges of the strength graph, and
 * the HIP-event times in ms of ms[0] strength (+ rho), ms[1] independent set, ms[2] assignment, ms[3] P.  Any output may be NULL. */
GMG_API int gmg_get_aggregation_info(gmg_handle_t h, int lev, int *rounds, double *omega, double *rho, int64_t *strong_edges, double *ms);
/* Rows of a level after gmg_setup (levels below an aggregated one have no size before). */
GMG_API int gmg_get_level_size(gmg_handle_t h, int lev, int64_t *n);

/* ---- smoothers ------------------------------------------------------------- */
/* RichardsonSmoother(JacobiLinearSolver(),niter,omega): RichardsonSmoothers.jl:84-98,
 * JacobiLinearSolvers.jl:20-23,43-47. */
GMG_API int gmg_set_smoother_jacobi(gmg_handle_t h, int lev, int which, int niter, double omega);
/* RichardsonSmoother(PatchSolver|BlockJacobiSolver,niter,omega): PatchSolvers.jl:279-300,
 * BlockJacobiSolvers.jl:141-170.  patch_ptr has npatch+1 entries; patch_dofs lists
 * the rows(=cols) of each patch; blocks A[p,p] are extracted and factorised on the device. */
GMG_API int gmg_set_smoother_patch(gmg_handle_t h, int lev, int which, int niter, double omega,
                                   int kind, int64_t npatch, const void *patch_ptr,
                                   const void *patch_dofs, int index_base, int index_bytes);

/* The same smoother with the patch data the reference's numerical setup holds (PatchSolvers.jl:137-150,175-188):
 *   patch_rows / patch_cols  separate index tables (b[rows_p] is the local rhs, x[cols_p] += x_p; PatchSolvers.jl:237-240,296);
 *                            patch_cols = NULL means patch_cols = patch_rows;
 *   blocks                   NULL: blocks A[rows_p, cols_p] are gathered from the level matrix on the device (BlockJacobiSolvers.jl:160);
 *                            else the caller's own n_p x n_p patch matrices, COLUMN-major (Julia Matrix{Float64}), concatenated in
 *                            patch order -- assemble_matrix(biform, assem, trial, test) of the SOLVER'S weak form, which need not equal A[p,p];
 *   blocks_are_factors = 1   `blocks` hold the packed output of lu!(patch_mat) and `pivots` its 1-based LAPACK ipiv (patch_ptr layout;
 *                            NULL for NoPivot factors): the library forms F \ I exactly as ldiv! would and never re-factorises.
 * kind (GMG_PATCH_LU / GMG_PATCH_NOPIVOT) selects the pivoting of the device factorisation when matrices are given. */
GMG_API int gmg_set_smoother_patch_matrices(gmg_handle_t h, int lev, int which, int niter, double omega, int kind,
                                            int64_t npatch, const void *patch_ptr, const void *patch_rows,
                                            const void *patch_cols, int index_base, int index_bytes,
                                            const double *blocks, int blocks_are_factors, const int32_t *pivots);

/* GaussSeidelSmoother(niter, omega, type), SymGaussSeidelSmoothers.jl:105-121 (SymGaussSeidelSmoother(niter, omega) is the symmetric
 * type).  solve!, :175-208, repeats niter times: forward pass (types forward, symmetric) dx = L \ r ; dx .= omega dx ; x .+= dx ;
 * r .-= A dx, then the same backward pass with U (types backward, symmetric); L / U = lower / upper triangle with the diagonal.
 * niter <= 0, omega <= 0 or an unknown type: GMG_ERR_INVALID (the constructor's @check, :113-115).
 * The triangular solves run on the device over the level sets of the dependency graph, one row per lane, each row summed in the
 * order of the reference's forward_sub! / backward_sub! and divided by the stored diagonal: bit for bit the sequential loops.
 * gmg_setup sorts the columns inside the rows if need be, builds the level sets and the tables of the directions the level's
 * smoothers use (one copy for pre and post; counted by gmg_device_bytes) and fixes the launch plan from the set sizes: consecutive
 * sets of at most 1024 rows share one launch of one workgroup, a larger set gets a launch of its own.  No launch waits on another
 * workgroup.  A missing or zero diagonal entry: GMG_ERR_SINGULAR at gmg_setup (SingularException, :31-33).  gmg_update_values +
 * gmg_setup keep the schedule and refill the values where the level's layout refreshes in place (any other path is a full setup
 * that rebuilds them; the results are the same bits).  gmg_smooth is solve!; gmg_precond_apply is ldiv!, :210-214 (x = 0, a copy
 * of r, all niter iterations).
 * Several ranks (a communicator of more than one rank, real or loopback): RANK-BLOCK Gauss-Seidel, the reference's distributed form
 * (:155-165, :71-75, :93-97: DiagonalIndices of the local matrix over the owned indices, forward_sub! / backward_sub! on
 * own_values(x), mul!(Adx, A, dx) the distributed product).  On an own | ghost level (gmg_set_partition; also the levels of a
 * redistributed subset on its member ranks) level sets, colouring, given order and tables are those of the rank's OWN x OWN BLOCK --
 * rows [0, n_own), stored columns < n_own -- the triangular solves need no communication, and r -= A dx exchanges dx and applies
 * the ghost columns; the diagonal test applies to the owned rows, a given order has n_own entries, gmg_get_gs_schedule /
 * gmg_get_gs_ordering report the own-block schedule.  With one rank per block the sweep is the one-rank sweep; with more it is
 * another (weaker) smoother, by construction.  A replicated level (gmg_set_replication) sweeps its global matrix on every rank.
 * The overlapping layout (gmg_set_partition_overlap) is refused: GMG_ERR_UNSUPPORTED at gmg_setup, naming level and layout.
 * On an own | ghost level whose pack can fuse (every sent row is a boundary row: pack_fused of gmg_get_halo_info) the update launch
 * dx = omega dx ; x += dx also fills the send buffer of dx's exchange (gs_update_pack_kernel; option gs_pack_fused, same bits).
 * gmg_model_bytes is not extended: on a handle with such a smoother its byte model still counts Jacobi sweeps.
 * gmg_sweep_signature of a level with such a smoother ends in " gs=F+B", " gs=F" or " gs=B" (the directions that have tables). */
enum gmg_gs_type { GMG_GS_SYMMETRIC = 0, GMG_GS_FORWARD = 1, GMG_GS_BACKWARD = 2 };
GMG_API int gmg_set_smoother_gauss_seidel(gmg_handle_t h, int lev, int which, int niter, double omega, int type);
/* The schedule gmg_setup built: dir 0 forward, 1 backward (GMG_ERR_STATE if no smoother of the level uses that direction):
 * number of level sets, rows of the largest, launches per triangular solve and how many of them are one-set launches. */
GMG_API int gmg_get_gs_schedule(gmg_handle_t h, int lev, int dir, int64_t *nsets, int64_t *max_set_rows,
                                int64_t *nlaunches, int64_t *nwide);

/* The visiting order of a level's Gauss-Seidel sweeps.  order[k] is the row the forward sweep visits k-th, pos its inverse.
 * Forward: for k = 0 .. n-1, i = order[k]: dx_i = (r_i - sum a_ij dx_j) / a_ii over the stored j with pos(j) < k in ascending pos(j),
 * one rounded product and one rounded subtraction per term, the division last; backward: k = n-1 .. 0 over pos(j) > k in descending
 * pos(j).  That is forward_sub! / backward_sub! on B = A[order, order] applied to r[order] and scattered back; the rest of a pass
 * (dx = omega dx, x += dx, r -= A dx in the level's own numbering) is unchanged.
 *   GMG_GS_ORDER_NATURAL     (default) order[k] = k.
 *   GMG_GS_ORDER_MULTICOLOR  greedy first-fit colouring of the symmetrised STORED pattern (explicit zeros count, the diagonal does
 *                            not): rows in natural order, each takes the smallest colour no already-coloured neighbour holds; the
 *                            order is the rows sorted stably by colour.  Rows of one colour share no stored entry, so the solve has
 *                            at most as many level sets as colours (exactly as many on a structurally symmetric pattern).
 *                            Deterministic, built on the host at gmg_setup from the pattern only: a value refresh keeps it.
 *                            Greedy, not optimal.
 *   GMG_GS_ORDER_GIVEN       the caller's permutation (copied): n entries, every row exactly once.
 * gmg_set_gs_ordering takes effect at the next gmg_setup, which then rebuilds everything; one order per level, shared by its pre- and
 * post-smoother.  Legal on any smoothed level and inert where no smoother of the level is Gauss-Seidel.  An unknown kind, `order`
 * given with another kind than GIVEN, n different from the level's rows or a bad permutation: GMG_ERR_INVALID, the message names the
 * level and the first offending position.  gmg_get_gs_schedule reports the sets and launches of the order in use.  On a level with an
 * order of its own the one-set launches run gs_wide_kernel (one wave per slice of 64 permuted rows); where omega == 1 and every
 * launch of the direction's plan is a one-set launch, that kernel also updates x and the update launch is not made (same rounding).
 * With profiling enabled on the level (gmg_profile_enable), gmg_kernel_stats.launches counts the launches of the triangular solves
 * and of the x updates of its Gauss-Seidel passes (r -= A dx is not counted).
 * gmg_get_gs_ordering returns what the last gmg_setup used: kind, the number of colours (0 unless MULTICOLOR) and, if `order` is not
 * NULL, the n entries of the order (the identity for NATURAL); cap < n: GMG_ERR_INVALID.  GMG_ERR_STATE if no smoother of the level
 * is Gauss-Seidel.  Any of the outputs may be NULL. */
enum gmg_gs_order { GMG_GS_ORDER_NATURAL = 0, GMG_GS_ORDER_MULTICOLOR = 1, GMG_GS_ORDER_GIVEN = 2 };
GMG_API int gmg_set_gs_ordering(gmg_handle_t h, int lev, int kind, const int32_t *order, int64_t n);
GMG_API int gmg_get_gs_ordering(gmg_handle_t h, int lev, int *kind, int64_t *ncolors, int32_t *order, int64_t cap);
/* The colouring itself, without a handle and without a GPU: 0-based CSR pattern of a square matrix (ptr[nrows + 1], col[ptr[nrows]];
 * columns in any order, duplicates allowed) -> order[nrows], color[nrows] (either may be NULL), *ncolors.  gmg_setup calls this
 * function.  A column outside [0, nrows) or a non-monotone ptr: GMG_ERR_INVALID. */
GMG_API int gmg_gs_multicolor_order(int64_t nrows, const int64_t *ptr, const int32_t *col, int32_t *order, int32_t *color,
                                    int64_t *ncolors);

/* ChebyshevSmoother(M, degree) over the preconditioner M of a smoother slot, M = JacobiLinearSolver / PatchSolver / BlockJacobiSolver.
 * The reference has no such smoother; it is an addition of this library (like the Gauss-Seidel orderings), on one GPU and on the
 * own | ghost and replicated levels of a partitioned handle (SEVERAL RANKS below).
 * Call it AFTER gmg_set_smoother_jacobi / gmg_set_smoother_patch[_matrices] on the same slot: it turns that slot's Richardson
 * iteration into the Chebyshev one (the slot's niter and omega are then unused).  Setting a plain smoother on the slot again clears it.
 * One pass of degree m on (x, r), with z = M^-1 r the un-relaxed preconditioner (Saad, Alg. 12.1, residual form):
 *   theta = (lmax + lmin)/2 ; delta = (lmax - lmin)/2 ; sigma = theta/delta ; rho_0 = 1/sigma
 *   sweep 0:           d = (1/theta) z                               ; x += d ; r -= A d
 *   sweep k = 1..m-1:  rho_k = 1/(2 sigma - rho_{k-1}) ; d = (rho_k rho_{k-1}) d + (2 rho_k/delta) z ; x += d ; r -= A d
 * The coefficients are computed on the host in double in this order, once per setup; the kernels round each product, then the sum.
 * Bounds: lambda_max > 0 is used as it is, with lambda_min > 0 or, for lambda_min <= 0, lambda_max / eig_ratio.  lambda_max <= 0:
 * gmg_setup estimates lambda_est = lambda_max(M^-1 A) per level and slot (pre and post share it when they share M) by eig_steps power
 * steps w = M^-1 (A v) ; lambda_est = ||w||_2 ; v = w / lambda_est from v_i = 1 + ((i * 2654435761) mod 1024)/1024 (0-based row i,
 * unsigned 64-bit), normalised; then lambda_max = eig_safety * lambda_est and lambda_min as above.  A few power steps UNDER-estimate a
 * clustered top of the spectrum (Jacobi on Q1 32^3: 1.336 after 10 steps, true 1.494): pass lambda_max or raise eig_steps where that
 * matters.  The reference-style defaults of the host layers: degree 3, eig_steps 10, eig_safety 1.1, eig_ratio 10.
 * gmg_update_values[_csc] + gmg_setup estimate again where the bound was not given.
 * Errors: GMG_ERR_STATE if the slot has no smoother yet; GMG_ERR_UNSUPPORTED on a Gauss-Seidel slot; GMG_ERR_INVALID for degree < 1,
 * lambda_min >= lambda_max when both are given, eig_ratio <= 1, eig_safety < 1 or eig_steps < 1.
 * SEVERAL RANKS (communicator of several ranks, real or loopback).  A Chebyshev slot runs on own | ghost levels (gmg_set_partition) and on
 * the replicated levels (>= the level of gmg_set_replication).  On an own | ghost level the recurrence runs on the n_own owned rows;
 * patch M is consistent!(r), the patch solves, the gather over all local dofs, assemble!(z), then the update; r -= A d is the distributed
 * product with its halo exchange.  Where the level's pack can fuse, the update also fills the send buffer of d's exchange
 * (cheb_update_pack_kernel; option cheb_pack_fused, same bits).  The estimates use the distributed product and all-reduced dot / norm
 * (local on replicated levels), so every rank takes the same stops and GMG_ERR_SINGULAR decisions.  The start vector is the formula
 * above with i the 0-based index of the row among THE HANDLE'S OWN ROWS, normalised in the global norm: a folded (loopback) handle
 * gets the single-GPU estimate of the folded matrix, while between true ranks the vector -- and therefore lambda_est after a few steps --
 * DEPENDS ON THE PARTITION (gmg_get_chebyshev_info reports the value; pass lambda_max where that matters).
 * Refused at gmg_setup with GMG_ERR_UNSUPPORTED, naming the level: a level in the overlapping layout (gmg_set_partition_overlap); a level
 * of a redistributed rank subset (gmg_set_redistribution); a handle that has a communicator (gmg_comm_init_*) but no declared layout
 * (gmg_set_replication never called).
 * gmg_smooth runs one pass; gmg_precond_apply on such a slot returns z = M^-1 r, the operator whose spectrum is estimated;
 * gmg_sweep_signature of a level with such a slot ends in " cheb=<pre degree>/<post degree>" (0 for a slot without).  The one-launch
 * passes, folded transfers and the other shortcuts of the Richardson-Jacobi passes do not apply to such a slot. */
GMG_API int gmg_set_smoother_chebyshev(gmg_handle_t h, int lev, int which, int degree, double lambda_min, double lambda_max,
                                       int eig_steps, double eig_ratio, double eig_safety);
/* What the last gmg_setup fixed for the slot (which = GMG_PRE or GMG_POST): lambda_est is NaN where the bounds were given.  Any of the
 * outputs may be NULL.  GMG_ERR_STATE before gmg_setup or on a slot without a Chebyshev smoother. */
GMG_API int gmg_get_chebyshev_info(gmg_handle_t h, int lev, int which, int *degree, double *lambda_est, double *lambda_min,
                                   double *lambda_max, int *eig_steps);
/* How lambda_est is computed where lambda_max is not given.  Call after gmg_set_smoother_chebyshev (which resets the slot to POWER);
 * ignored where lambda_max is given.
 *   GMG_CHEB_EIG_POWER   (0, default) the power iteration above.
 *   GMG_CHEB_EIG_LANCZOS (1) eig_steps steps of CG on A with preconditioner M from r = the same normalised start vector; lambda_est is
 *     the largest eigenvalue of the Lanczos tridiagonal that CG builds:
 *       r = v ; gamma_old = 1 ; k = 0
 *       while k < eig_steps:
 *         z = M^-1 r ; gamma = dot(z, r)   stop unless gamma is finite and > 0 ; for k > 0 also stop if gamma < 1e-24 * gamma_0
 *         beta = gamma / gamma_old ; p = z + beta p  (k = 0: p = z)
 *         w = A p ; pw = dot(p, w)         stop unless pw is finite and > 0
 *         alpha = gamma / pw ; r -= alpha w ; record (alpha, beta) ; gamma_old = gamma ; k += 1
 *       T (k x k): T[i,i] = 1/alpha_i + (i > 0 ? beta_i/alpha_{i-1} : 0) ; T[i,i+1] = T[i+1,i] = sqrt(beta_{i+1}) / alpha_i
 *     (the textbook Lanczos matrix; its largest eigenvalue by Sturm bisection on the host).  The 1e-24 stop is a condition, not a
 *     tolerance: the residual has dropped twelve digits in the M^-1 norm, the Krylov space is exhausted in double.  The same cost per
 *     step as the power iteration plus one dot, and a much better top Ritz value on a clustered spectrum (Jacobi on Q1 32^3: 1.455
 *     after 10 steps against 1.336, true 1.494, so 1.1 lambda_est covers lambda_max).  What it buys is a robust default interval, not
 *     a faster solve.  A stop with no step recorded (M^-1 A not positive definite) is GMG_ERR_SINGULAR at gmg_setup.
 * Pre and post share one estimate when they share M, eig_steps and the method.
 * gmg_get_chebyshev_eig (after gmg_setup): the slot's method and the steps the estimate took (POWER: eig_steps; LANCZOS: <= eig_steps;
 * 0 where lambda_max was given).  GMG_ERR_STATE on a slot without a Chebyshev smoother, GMG_ERR_INVALID for an unknown method. */
enum gmg_cheb_eig { GMG_CHEB_EIG_POWER = 0, GMG_CHEB_EIG_LANCZOS = 1 };
GMG_API int gmg_set_chebyshev_eig_method(gmg_handle_t h, int lev, int which, int method);
GMG_API int gmg_get_chebyshev_eig(gmg_handle_t h, int lev, int which, int *method, int *steps_done);

/* MultiplicativePatchSmoother(M, niter, omega, type) over the patch blocks of a smoother slot, M = PatchSolver / BlockJacobiSolver:
 * block Gauss-Seidel over the patches (multiplicative Schwarz, Vanka), swept colour by colour.  The reference has only the additive
 * patch solver and names this form as a TODO (SchwarzLinearSolvers.jl:3,13); it is an addition of this library, on one GPU.
 * Call it AFTER gmg_set_smoother_patch[_matrices] on the same slot: it turns that slot's additive Richardson iteration into the
 * multiplicative one with this call's niter and omega.  Setting a plain smoother on the slot again clears it.
 * One pass on (x, r):
 *   dx = 0 ; r0 = r
 *   repeat niter times:
 *     forward  (types forward, symmetric): for c = 0 .. ncolors-1, for every patch p of colour c:
 *     backward (types backward, symmetric): for c = ncolors-1 .. 0, for every patch p of colour c:
 *       t_i = r0[rows_p[i]] - sum_k a(rows_p[i], k) dx[k]    the row in its stored order, summed from 0.0, product and sum rounded
 *       d_i = sum_j inv(A_pp)[i, j] t_j                      j = 0 .. n_p-1, as the additive patch solve sums
 *       dx[rows_p[i]] = dx[rows_p[i]] + omega d_i
 *   x = x + dx ; r = r - A dx                                the level's operator application
 * inv(A_pp) is the inverse block the patch setup builds (from the level matrix, the caller's patch matrices or the caller's factors,
 * pivoting or not, de-duplicated or not).  A patch without dofs is skipped; a dof in no patch keeps dx = 0.
 * COLOURING.  Two patches may share a colour only if they share no dof AND the stored pattern of A, symmetrised and with explicit
 * zeros counting, couples no dof of one to a dof of the other.  The patches of a colour then read and write disjoint entries of dx
 * and run in parallel; the result is bit for bit the sequential loop over the patches sorted stably by (colour, patch index).
 * gmg_set_patch_coloring (after gmg_set_smoother_patch_multiplicative, or on any patch slot): kind 0 = greedy first-fit in patch
 * order on that conflict graph (the default; deterministic; 2^d colours on vertex stars of a Cartesian mesh), kind 1 = the caller's
 * color[npatch], every entry >= 0 (copied); npatch different from the slot's patch count, a negative colour, an unknown kind or a
 * colour array with kind 0: GMG_ERR_INVALID.  gmg_setup ALWAYS validates the colouring in use on the host -- that check is what makes
 * the launches race-free -- and a conflict is GMG_ERR_INVALID naming the level and the two patches.  gmg_get_patch_coloring (after
 * gmg_setup; which = GMG_PRE or GMG_POST): the number of colours and, if `color` is not NULL, the colour of every patch (cap < npatch:
 * GMG_ERR_INVALID); GMG_ERR_STATE on a slot without such a smoother.
 * gmg_patch_multicolor is the colouring itself, without a handle and without a GPU: the 0-based CSR pattern of the square level matrix
 * and the patch table -> color[npatch], *ncolors.  It works from a dof -> patch incidence and never forms the patch x patch graph.
 * gmg_setup calls it.  An index out of range or a non-monotone pointer array: GMG_ERR_INVALID.
 * KERNELS.  One launch per non-empty colour and direction: patch_mult_kernel (one wave per patch of at most 64 dofs, four patches per
 * workgroup) and, for the patches of a colour with more than 64 dofs, patch_mult_big_kernel (one workgroup per patch); on small levels
 * the whole pass is ONE launch of ONE workgroup, patch_mult_pass_kernel, with a workgroup barrier between colours.  No kernel waits on
 * another workgroup.  Option pmult_one_launch (live): 1 (default) = levels of at most pmult_one_launch_max patches (default 32, from profiles/patch_mult_timing.md), 0 =
 * never, 2 = every level; the same bits in all settings.  The sweeps read rows of A from the level's CSR, which such a level keeps on
 * the device next to its sweep layout (counted by gmg_device_bytes).
 * gmg_update_values[_csc] + gmg_setup keep the colouring and rebuild the blocks: the bits of a fresh setup.
 * Errors of gmg_set_smoother_patch_multiplicative: GMG_ERR_STATE if the slot holds no patch smoother; GMG_ERR_INVALID for niter <= 0,
 * omega <= 0 or an unknown type; GMG_ERR_UNSUPPORTED if the slot is a Chebyshev slot (and gmg_set_smoother_chebyshev on a
 * multiplicative slot is GMG_ERR_UNSUPPORTED: Chebyshev over the multiplicative sweep is not built).
 * Refused at gmg_setup with GMG_ERR_UNSUPPORTED, naming the level: a level whose operator was streamed (gmg_set_operator_rows) and
 * so has no CSR to read rows from; patch_cols != patch_rows (the sweep needs one dof set per patch); a communicator of more than one
 * rank, real or loopback (the colours of a partitioned level would have to be agreed across ranks); a patch of more than 4096 dofs
 * (the workgroup kernel stages t_p in LDS).
 * gmg_smooth runs one pass; gmg_precond_apply runs it with x = 0 on a copy of r, so z = dx; the slot works as the finest pre-smoother
 * behind LinearSolverFromSmoother and inside a GMG that is a block of a block solver.  gmg_sweep_signature of such a level ends in
 * " pmult=F+B/<ncolors>" (" pmult=F/...", " pmult=B/..." for the one-direction types).  With profiling enabled on the level,
 * gmg_kernel_stats.launches counts the colour launches and the x update of its passes (r -= A dx is not counted).
 * gmg_model_bytes is not extended: on a handle with such a smoother its byte model still counts Jacobi sweeps. */
enum gmg_pmult_type { GMG_PMULT_SYMMETRIC = 0, GMG_PMULT_FORWARD = 1, GMG_PMULT_BACKWARD = 2 };
GMG_API int gmg_set_smoother_patch_multiplicative(gmg_handle_t h, int lev, int which, int niter, double omega, int type);
GMG_API int gmg_set_patch_coloring(gmg_handle_t h, int lev, int which, int kind, const int32_t *color, int64_t npatch);
GMG_API int gmg_get_patch_coloring(gmg_handle_t h, int lev, int which, int64_t *ncolors, int32_t *color, int64_t cap);
GMG_API int gmg_patch_multicolor(int64_t nrows, const int64_t *ptr, const int32_t *col, int64_t npatch, const int64_t *patch_ptr,
                                 const int32_t *patch_dofs, int32_t *color, int64_t *ncolors);

/* Patch-corrected prolongation y = P x - sum_p R_p^T A_pp^-1 R_p (A P x)  over the given patches
 * (PatchProlongationOperator, PatchBasedSmoothers/PatchTransferOperators.jl:153-172 with rhs = lhs = the
 * level operator; used by the reference for grad-div problems, test/Applications/StokesGMG.jl:125-133).
 * Same patch-table format as gmg_set_smoother_patch. */
GMG_API int gmg_set_prolongation_patch_correction(gmg_handle_t h, int lev, int kind, int64_t npatch,
                                                  const void *patch_ptr, const void *patch_dofs,
                                                  int index_base, int index_bytes);

/* rhs form of that correction when it differs from the level operator: PatchProlongationOperator(lev,sh,ptopo,lhs,rhs)
 * solves lhs(u_i,v_i) = rhs(uH,v_i) (PatchTransferOperators.jl:30-50); the Stokes application passes lhs = the velocity
 * form and rhs = the grad-div term only (test/Applications/StokesGMG.jl:125-127).  G = the assembled rhs form on level lev
 * (square, same format options as gmg_set_matrix); lhs patch blocks: A[p,p], or the caller's via the patch tables.   On a distributed level (gmg_set_partition first) the matrix holds this rank's rows
 * with [own | ghost] columns, and every correction patch must lie inside the owned dofs (coarse-cell interiors do). */
GMG_API int gmg_set_prolongation_patch_correction_rhs(gmg_handle_t h, int lev, int64_t n, int64_t nnz, const void *ptr,
                                                      const void *idx, const double *val, int layout, int index_base,
                                                      int index_bytes);

/* ---- coarsest solver ---------------------------------------------------------- */
/* kwarg `coarsest_solver` (GMGLinearSolvers.jl:54; cache :423-434; applied at :474).  The reference accepts any LinearSolver:
 * default LUSolver(); its MPI tests / applications pass iterative or PETSc solvers (joss_paper/scalability/src/stokes_gmg.jl:41-63). */
enum gmg_coarse_kind {
  GMG_COARSE_DENSE_INVERSE = 0,  /* LUSolver(): exact; dense inverse built at setup, one GEMV per cycle (default) */
  GMG_COARSE_CG_JACOBI = 1,      /* CGSolver(JacobiLinearSolver(); maxiter, atol, rtol) on the device, x0 = 0 (CGSolvers.jl:73-120) */
  GMG_COARSE_HOST_CALLBACK = 2   /* the host language's own solver: fn(ctx, n, r, x) on HOST vectors, x pre-zeroed; returns 0 on success */
};
typedef int (*gmg_coarse_solve_fn)(void *ctx, int64_t n, const double *r, double *x);
/* maxiter/atol/rtol: CG_JACOBI only.  fn/ctx: HOST_CALLBACK only (must stay valid while the handle is used; it is called
 * from the thread that calls the solve entry point, once per cycle visit of the coarsest level). */
GMG_API int gmg_set_coarse_solver(gmg_handle_t h, int kind, int maxiter, double atol, double rtol,
                                  gmg_coarse_solve_fn fn, void *ctx);
/* ConvergenceLog summary of the last iterative coarse solve (GMG_COARSE_CG_JACOBI). */
GMG_API int gmg_get_coarse_log(gmg_handle_t h, gmg_result *res);
/* How the last gmg_setup built the dense inverse of GMG_COARSE_DENSE_INVERSE (read-only; no reference counterpart: LUSolver() has
 * one path).  built_by: see below.  panel: width of the device Gauss-Jordan panels, 32 or 64 (gj_wide_min), 0 on the host.
 * mfma: 1 when the device trailing update ran on the FP64 matrix cores (gj_mfma), else 0.  device_rejected: 1 when the device
 * inversion was tried, refused the matrix with GMG_ERR_SINGULAR (zero pivot, or its own A*(Ainv*v) == v check) and the host's
 * pivoted banded LU took over (n <= coarse_host_fallback_max).  Any output may be NULL.  GMG_ERR_STATE before a setup. */
enum gmg_coarse_built_by {
  GMG_COARSE_BUILT_NONE = 0,            /* the coarsest solver is not a dense inverse (CG_JACOBI, HOST_CALLBACK, or chosen by coarse_auto_cg_min) */
  GMG_COARSE_BUILT_HOST_LU = 1,         /* banded LU with partial pivoting on the host (n <= coarse_host_max, or the fallback) */
  GMG_COARSE_BUILT_DEVICE_GJ = 2,       /* blocked Gauss-Jordan without pivoting on the device, result verified */
  GMG_COARSE_BUILT_HOST_CONSTRAINED = 3 /* inv([A K; K' 0]) on the host (gmg_set_coarse_nullspace) */
};
GMG_API int gmg_get_coarse_info(gmg_handle_t h, int *built_by, int *panel, int *mfma, int *device_rejected);

/* ---- solver options --------------------------------------------------------- */
/* kwargs of GMGLinearSolver: mode, cycle_type, maxiter, atol, rtol (GMGLinearSolvers.jl:56-58). */
GMG_API int gmg_set_options(gmg_handle_t h, int mode, int cycle, int maxiter, double atol, double rtol);

/* Layout / schedule policy of ONE handle.  The reference configures a solver by constructor keywords only
 * (GMGLinearSolvers.jl:48-58); every switch this library used to read from the environment is therefore a per-handle option:
 *     gmg_set_option(h, "pat_r2", 0)          ("PAT_R2", "GMG_PAT_R2" name the same option; unknown keys -> GMG_ERR_INVALID)
 * Options take effect at the next gmg_setup (setting one after a setup invalidates it, like a new operator would), except the
 * "live" ones marked (*) which act at the next call.  The environment variable GMG_<KEY>, when set, still OVERRIDES the handle's
 * value -- a debugging / A-B device, not the configuration interface.  Keys (default):
 *   storage layout   pattern (1) pat_shared (1) opattern (1) sell (1) sell_maxpad (1.25) vdict (1) idx16 (1) force_ptr64 (0)
 *                    pat_coded_min_rows (500000) eager* (1) eager_min_rows* (20000) refresh* (1)
 *   cycle precision  values_f32 (0; 1: the cycle streams float32 level values, see gmg_level_values) values_f32_nt (-1: non-temporal
 *                    loads of the float stream by its size, with the thresholds of the fp64 stream; 0 never; 1 always; 2 always, the
 *                    row-wise operands too -- float32 launches only, same bits in every setting)
 *   measurement      prof_stride (7: HIP events on every n-th sweep launch of the profiled level)
 *   sweep kernels    pat_rsweep (1) pat_r2 (1: two rows per lane in the r-gather sweep) pat_r2_occ (2: its 64-register form, eight waves per SIMD, in workgroups of eight waves on big levels; 1: four waves; 0: off) pat_r2_wgs (0 = one round of workgroups)
 *                    pat_tile_rows (3500000: the size, in rows, from which the pair sweep and the pair mat-vec take that eight-wave form, one slice per wave)
 *                    pat_strict (1) pat_fma (0: products and sums rounded separately, as the
 *                    reference's mul!; 1: fused multiply-add taps in the row-pattern sweeps -- not bit-identical)
 *                    pat_xnext (1: per-sweep passes of an even number of r-gather sweeps on one rank add s_k and s_{k+1} to x in sweeps
 *                    0, 2, ... -- s_{k+1} from the r_{k+1} the sweep holds in registers, no r_{k-1} re-read; 0: x = (x + s_{k-1}) + s_k in
 *                    sweeps 1, 3, ....  Same bits) pat_close (1: the last sweep of a post-smoothing pass whose residual nobody reads --
 *                    the final post pass of levels >= 1, and of level 0 in a one-cycle, non-verbose preconditioner application -- is
 *                    not run; per-sweep passes need pat_xnext, one-launch passes stop one sweep early.  Same bits in x; 0: every sweep)
 *                    pat_defer (1) pat_dinv (1) pat_emit (1) pat_nb (0 = auto) pat_rb (3) pat_un (9) pat_wgs (2048) pat_batched (1)
 *                    pat_small_wpb (4) pat_small_wpb2 (2) pat_wide (1) pat_wide_lds (73728) pat_wide_rounds (1) one_gather (1)
 *                    sell_un (6) sell_block (0 = auto) sell_defer (1) nt (1) nt_rowwise (1) big_rows (4000000) xcd_remap (1)
 *                    xcd_remap_big (-1: chunks two gather reaches deep per XCD; 0 launch order; 1 contiguous eighths; n chunk of n workgroups)
 *                    lanes_log2 (-1 = auto)
 *                    pat_r2mv (1: y = A x, y -= A x, y = b - A x of row-pattern levels with two rows per lane) pat_r2mv_min (100000:
 *                    smallest level, in rows, that takes it and the pair prolongation) pat_r2mv_dot (1: dot(p, A p) of CG formed by
 *                    the mat-vec kernel) pat_pair_p (1: prolongation + correction with two rows per lane)
 *                    pat_zwalk (1: levels of >= pat_zwalk_rows (9000000: where the vectors of a sweep outgrow the 256 MB Infinity Cache) rows sweep as a walk up the grid planes -- an interval of a plane
 *                    per wave, three new windows per step, pat_zwalk_t (12) planes per chain; 2: every level; 0: off) pat_zwalk_mv (1: their
 *                    mat-vecs too) pat_zwalk_wide (1: the wide-row (Q2) operator applications of levels of >= pat_zwalk_wide_rows (1000000) rows in the same form, 25 windows in registers)
 *   reductions       red_fused (1: inside CG the second stage of every dot is done by the kernel that consumes the scalar and the
 *                    norm is reduced + posted to the host by one launch; 0: one reduce launch per dot.  Same bits either way)
 *                    cg_split* (0: measured equal, profiles/xnext_ab_128.md; where red_fused applies: 1 = CG's x += alpha p runs in a kernel of its own behind the launch that posts
 *                    the residual norm -- cg_update_r_kernel, cg_update_x_kernel -- and the stream is synchronised once at the end of
 *                    the outermost solve; 0 = one cg_update_kernel.  Same bits either way)
 *                    gmres_fused* (1: where red_fused applies, a GMRES Arnoldi column runs as gmres_mgs_kernel launches -- each sums the
 *                    previous dot's partials, subtracts the projection and accumulates the next dot's partials in one pass -- and
 *                    gmres_normalize_kernel, the solution update as one gmres_combine_kernel; 0: a dot, a reduce and an axmy launch
 *                    per coefficient and an axpy per basis vector.  Same bits either way)
 *                    fgmres_fused* (-1: an FGMRES nested in a block preconditioner (gmg_block_set_diag_krylov_gmg) runs its Arnoldi
 *                    column with the kernels of gmres_fused on V and x += sum g_i Z_i as one gmres_combine_kernel over the table of
 *                    Z, the entry points gmg_fgmres_solve[_pl] / gmg_block_fgmres_solve keep a dot, a reduce and an axmy launch per
 *                    coefficient; 1: all of them fused; 0: none.  Where red_fused applies.  Same bits either way)
 *                    nullspace_fused* (1: where red_fused applies, the dots of a null-space projection are one pass over v for up to
 *                    8 basis vectors, nullspace_dots_kernel, the combination and the subtraction from x another,
 *                    nullspace_project_kernel, and make_orthogonal! / Gram-Schmidt chain nullspace_mgs_kernel; 0: a dot per
 *                    vector, axpy_kernel / axmy_dev_kernel per term.  Same bits either way)
 *   one-launch pass  persist (1) persist_fenced (0) persist_max_slices (0 = one workgroup per CU) persist_shared (0)
 *                    persist_wpb (1: smallest workgroup, in waves) persist_regs (1: passes of 9- / 27-point operators run
 *                    sells_smooth_kernel with a compile-time run count -- run offsets, gather indices and, at one slice per wave, the
 *                    row's coefficients in registers, one load round trip per sweep; 0 = the runtime run count body.  Same bits either
 *                    way; gmg_sweep_signature names the instantiation that ran)
 *                    persist_fold (7: bit mask of the transfers that run as the head of the one-launch pass they feed instead of
 *                    as launches of their own -- 1 the restriction in front of a pre-smoothing pass, 2 prolongation + correction +
 *                    r -= A dx in front of a post-smoothing pass, 4 bit 1 also where the finer level is no one-launch level; one
 *                    rank, transfer tables in the LDS form that fit next to the pass's own; 0 = separate launches.  Same bits
 *                    either way; gmg_sweep_signature ends in folds=R+P / R / P / none for a level with a one-launch pass)
 *   Gauss-Seidel     gs_wide* (1: on a level with a visiting order of its own (gmg_set_gs_ordering) the one-set launches run
 *                    gs_wide_kernel and fold the x update where they may; 0: they run gs_sets_kernel with the update launch, as the
 *                    natural order does.  Same bits either way: the A/B switch of tools/gs_timing.py)
 *                    gs_pack_fused* (1: on an own | ghost level whose pack can fuse, the x update of a Gauss-Seidel direction and the
 *                    pack of dx's send entries are one launch, gs_update_pack_kernel; 0: gs_update_kernel, then halo_pack_kernel.
 *                    Inert where the update folds into gs_wide_kernel or the pack cannot fuse.  Same bits either way: the A/B
 *                    switch of tools/gs_dist_timing.py)
 *   Chebyshev        cheb_pack_fused* (1: on an own | ghost level whose pack can fuse, the pointwise update of a Chebyshev sweep and the
 *                    pack of d's send entries are one launch, cheb_update_pack_kernel; 0: cheb_update_kernel, then halo_pack_kernel.
 *                    Inert where the pack cannot fuse.  Same bits either way: the A/B switch of tools/chebyshev_dist_timing.py)
 *   coarsest level   coarse_host_max (1500) coarse_host_fallback_max (6000) coarse_auto_cg_min (20000: a dense-inverse request on a
 *                    coarsest level of at least this many dofs is served by the device CG-Jacobi solver instead) gj_mfma (1) gj_wide_min (4096)
 *   patch smoother   patch_dedup (1) patch_source_dedup (1) patch_operator (1)
 *                    pmult_one_launch* (1: the pass of a multiplicative patch slot runs as one launch of one workgroup,
 *                    patch_mult_pass_kernel, on levels of at most pmult_one_launch_max* patches; 0: never, one launch per colour and
 *                    direction; 2: on every level.  Same bits in all settings: the A/B switch of tools/patch_mult_timing.py)
 *   distributed      overlap (1) halo_fuse_pack (1) host_async (0)
 *   host round trip  host_poll* (1: the residual norm of every Krylov iteration is posted into page-locked host memory and polled; 0: copy +
 *                    hipStreamSynchronize)
 *   host vectors     x0_zero* (0: the solve entry points read x as the initial guess, CGSolvers.jl:79; 1: x is taken as zero on
 *                    entry and never uploaded) host_chunk_bytes* (4194304: staging chunk of unregistered host vectors)
 *   diagnostics      prof_stride (8) setup_timing* (0) dbg_nogather (0) host_timeline* (0: 1 = host-side duration of every step of
 *                    the cycles on stderr when the handle is destroyed) persist_force_timeout* (0: test hook, the next n solves
 *                    behave as if a one-launch pass had timed out) */
GMG_API int gmg_set_option(gmg_handle_t h, const char *key, double value);
/* Effective value of an option (NaN: the built-in default applies); *source (may be NULL) = 0 default, 1 gmg_set_option, 2 environment. */
GMG_API int gmg_get_option(gmg_handle_t h, const char *key, double *value, int *source);

/* Host-memory callers (GMG_MEM_HOST: what the Julia binding passes for Vector{Float64}).  Registering the caller's arrays ONCE
 * page-locks and maps them, so every later solve moves b / x by DMA straight from / into the caller's pages at the PCIe link rate
 * instead of through the staging path for pageable memory -- the pattern of ext/GridapPETScExt/PETScCaches.jl:23-36, which pins
 * the exact x / b objects of a solve.  The range must stay allocated until gmg_host_unregister (or gmg_destroy, which unregisters
 * what is left; it never frees caller memory).  Vectors inside a registered range are recognised by address. */
GMG_API int gmg_host_register(gmg_handle_t h, const void *ptr, int64_t nbytes);
GMG_API int gmg_host_unregister(gmg_handle_t h, const void *ptr);
/* Bytes moved host -> device / device -> host for host-memory callers since gmg_create, and the number of registered ranges. */
GMG_API int gmg_get_host_io_stats(gmg_handle_t h, int64_t *bytes_up, int64_t *bytes_down, int64_t *nregistered);
/* One-launch smoothing passes: solves that were re-run per sweep after a pass timed out, and whether the passes are still on. */
GMG_API int gmg_get_persist_retries(gmg_handle_t h, int64_t *retries, int *persist_active);

/* kwarg `verbose` of GMGLinearSolver (GMGLinearSolvers.jl:58).  The library never prints; verbose > 0 makes the GMG's own
 * ConvergenceLog complete on every path: as a preconditioner with maxiter = 1 inside gmg_cg_solve / gmg_fgmres_solve the
 * post-cycle norm(rh) of GMGLinearSolvers.jl:639 only feeds that log (update! returns true at maxiter regardless), so
 * with verbose = 0 (default) it is not evaluated and residuals[2] of the GMG log reads NaN. */
/* The HIP stream (hipStream_t, passed as void*) the handle issues ALL its work on -- kernels, copies, the RCCL collectives.  By
 * default every handle owns a non-blocking stream (gmg_create).  A caller that produces b and consumes x with its own kernels
 * (a device-resident Krylov loop around gmg_apply; PyTorch / AMDGPU.jl arrays) passes ITS stream: the library's work is then
 * ordered with the caller's without any device synchronisation on either side.  stream = NULL returns to the handle's own
 * stream -- it does NOT name HIP's null stream.  The device's default ("null", legacy-synchronising) stream, whose hipStream_t
 * is 0 -- what `torch.cuda.current_stream().cuda_stream` and AMDGPU.jl's default stream report -- is named by
 * GMG_STREAM_LEGACY (= hipStreamLegacy), the per-thread default stream by GMG_STREAM_PER_THREAD (= hipStreamPerThread).
 * The call waits for the work already issued on the stream it leaves.  No reference counterpart (the reference runs on
 * the host); `gmg_get_stream` returns the current one (e.g. to record an event on it). */
#define GMG_STREAM_LEGACY ((void *)1)
#define GMG_STREAM_PER_THREAD ((void *)2)
GMG_API int gmg_set_stream(gmg_handle_t h, void *stream);
GMG_API int gmg_get_stream(gmg_handle_t h, void **stream);
GMG_API int gmg_set_verbose(gmg_handle_t h, int verbose);
/* ns.solver.log of the GMG after the last solve!/ldiv! (also when it ran as a preconditioner inside a Krylov call). */
GMG_API int gmg_get_log(gmg_handle_t h, gmg_result *res, double *hist, int hist_cap);

/* numerical_setup(ss,A): GMGLinearSolvers.jl:183-210 -- uploads operators, builds
 * D^-1, R = P^T, patch factors, work vectors and the coarse solver
 * (default coarsest_solver = LUSolver(), :54,423-434 -> dense inverse applied as one GEMV per cycle;
 * factorised on the host up to 1500 dofs, inverted on the device above; see gmg_set_coarse_solver). */
GMG_API int gmg_setup(gmg_handle_t h);

/* ---- hot path ---------------------------------------------------------------- */
/* solve!(x,ns::GMGNumericalSetup,b) / ldiv!: GMGLinearSolvers.jl:612-649.
 * hist (may be NULL) receives niters+1 residual norms; hist_cap = its capacity. */
GMG_API int gmg_apply(gmg_handle_t h, const double *b, double *x, int memspace,
                      gmg_result *res, double *hist, int hist_cap);
/* solve!(x,ns::CGNumericalSetup,b) with Pl = this GMG: Krylov/CGSolvers.jl:73-120.
 * use_precond: 0 = Pl nothing, 1 = this GMG, 2 = JacobiLinearSolver() on the finest
 * matrix (the reference's CGSolver(JacobiLinearSolver())), 3 = LinearSolverFromSmoother(finest
 * pre-smoother) (LinearSolverFromSmoothers.jl:44-50, test/LinearSolvers/SmoothersTests.jl).
 * x = initial guess on entry. */
GMG_API int gmg_cg_solve(gmg_handle_t h, const double *b, double *x, int memspace,
                         int maxiter, double atol, double rtol, int flexible, int use_precond,
                         gmg_result *res, double *hist, int hist_cap);
/* The `diagnostic` of CGSolver (Krylov/CGSolvers.jl:19,87,114-115; KrylovUtils.jl:58-90): the scalars of the Lanczos tridiagonal.
 * capacity > 0: the outermost CG of gmg_cg_solve records alpha_k, beta_k of every iteration (device buffer of 2*capacity doubles,
 * allocated here, counted by gmg_device_bytes, kept across gmg_setup); capacity == 0: off, buffer released.  Off by default.
 * Iteration k (0-based) stores, bit for bit, the alpha_k = gamma_k / dot(p, w) its update kernel used and the beta_k its p = z + beta p
 * used ((gamma - delta)/gamma_old with `flexible`; beta_0 = gamma_0 / 1).  A CG nested below (coarsest solver, block diagonal) and
 * gmg_block_cg_solve record nothing.  One lane of the kernels that form the scalars stores them through a pointer that is null while
 * tracing is off: the launches, x and the history do not depend on tracing.  With tracing on, gmg_cg_solve with maxiter > capacity
 * returns GMG_ERR_INVALID before any work.
 * gmg_cg_get_trace: count = iterations recorded by the last gmg_cg_solve; alpha / beta (either may be NULL) receive count values.
 * GMG_ERR_STATE while tracing is off; GMG_ERR_INVALID when cap < count. */
GMG_API int gmg_cg_set_trace(gmg_handle_t h, int capacity);
GMG_API int gmg_cg_get_trace(gmg_handle_t h, int *count, double *alpha, double *beta, int cap);
/* solve!(x,ns::FGMRESNumericalSetup,b) with Pr = this GMG, Pl = nothing:
 * Krylov/FGMRESSolvers.jl:130-199, KrylovUtils.jl:17-54. */
GMG_API int gmg_fgmres_solve(gmg_handle_t h, const double *b, double *x, int memspace,
                             int m, int restart, int m_add, int maxiter, double atol, double rtol,
                             int use_precond, gmg_result *res, double *hist, int hist_cap);
/* The same with a LEFT preconditioner as well (FGMRESSolver(m,Pr;Pl=...), FGMRESSolvers.jl:26-30; krylov_mul! / krylov_residual!
 * with Pl, KrylovUtils.jl:14-18,46-50): use_precond_left takes the values of use_precond; the handle's GMG can serve on one
 * side only. */
GMG_API int gmg_fgmres_solve_pl(gmg_handle_t h, const double *b, double *x, int memspace,
                                int m, int restart, int m_add, int maxiter, double atol, double rtol,
                                int use_precond, int use_precond_left, gmg_result *res, double *hist, int hist_cap);
/* solve!(x,ns::MINRESNumericalSetup,b): Krylov/MINRESSolvers.jl:75-148 (MINRESSolver(;Pl,maxiter,atol,rtol), :16).
 * use_precond as in gmg_cg_solve (Pl = nothing / this GMG / Jacobi / the finest pre-smoother).  The preconditioner must be
 * symmetric positive definite (the reference's docstring, :8-9): dot(Pl(r), r) <= 0 at start-up (:97) or < 0 inside the loop
 * (sqrt, :116) returns GMG_ERR_INVALID.  x = initial guess on entry; the history holds the 2-norm of the preconditioned
 * residual.  Nine work vectors are allocated on the handle by the first call. */
GMG_API int gmg_minres_solve(gmg_handle_t h, const double *b, double *x, int memspace, int maxiter, double atol, double rtol,
                             int use_precond, gmg_result *res, double *hist, int hist_cap);
/* solve!(x,ns::GMRESNumericalSetup,b): Krylov/GMRESSolvers.jl:132-210; krylov_mul!/krylov_residual!, KrylovUtils.jl:17-54
 * (GMRESSolver(m;Pr,Pl,restart,m_add,maxiter,atol,rtol), :25).  use_precond_right (Pr) and use_precond_left (Pl) each take the
 * values of use_precond in gmg_cg_solve: 0 nothing, 1 this GMG, 2 Jacobi on the finest matrix, 3 the finest pre-smoother.  The
 * handle's GMG serves on one side only: both equal to 1 returns GMG_ERR_INVALID.  restart != 0: the basis holds m vectors and is
 * restarted every m iterations (:31-37); otherwise it grows by m_add vectors when full (:154-157).  x = initial guess on entry;
 * the history holds the 2-norm of the left-preconditioned residual estimate, one entry per iteration.  The first call allocates
 * m + 1 basis vectors and zl on the handle, and zr once a Pr is selected (m + 3 vectors where FGMRES(m) keeps 2 m + 1); later
 * calls reuse them, gmg_device_bytes counts them.  Option gmres_fused chooses the kernels of the Arnoldi column, same bits. */
GMG_API int gmg_gmres_solve(gmg_handle_t h, const double *b, double *x, int memspace, int m, int restart, int m_add,
                            int maxiter, double atol, double rtol, int use_precond_right, int use_precond_left,
                            gmg_result *res, double *hist, int hist_cap);
/* solve!(x,ns::RichardsonLinearNumericalSetup,b): RichardsonLinearSolvers.jl:79-106, scalar omega;
 * use_precond as in gmg_cg_solve (Pl = nothing / this GMG / Jacobi / the finest pre-smoother). */
GMG_API int gmg_richardson_solve(gmg_handle_t h, const double *b, double *x, int memspace, double omega,
                                 int maxiter, double atol, double rtol, int use_precond,
                                 gmg_result *res, double *hist, int hist_cap);

/* ---- operator-level entry points (duck-typed `mul!` / smoother `solve!`) ------ */
/* mul!(y,op,x) for op in {A_lev, P_lev, R_lev}: RichardsonSmoothers.jl:94,
 * GMGLinearSolvers.jl:484,491,495. */
GMG_API int gmg_op_apply(gmg_handle_t h, int lev, int op, const double *x, double *y, int memspace);
/* solve!(x,ns::RichardsonSmootherNumericalSetup,r): updates x AND r in place
 * (RichardsonSmoothers.jl:84-98). which = GMG_PRE or GMG_POST. */
GMG_API int gmg_smooth(gmg_handle_t h, int lev, int which, double *x, double *r, int memspace);
/* solve!(dx,Mns,r) of the smoother's inner solver (Jacobi / patch), no relaxation:
 * JacobiLinearSolvers.jl:43-47, PatchSolvers.jl:238-241, BlockJacobiSolvers.jl:119-123. */
GMG_API int gmg_precond_apply(gmg_handle_t h, int lev, int which, const double *r, double *dx, int memspace);
/* coarsest solve!(xh,coarsest_solver_cache,rh): GMGLinearSolvers.jl:474. */
GMG_API int gmg_coarse_solve(gmg_handle_t h, const double *r, double *x, int memspace);
/* dot / norm as used by the Krylov solvers (CGSolvers.jl:85,95,105). */
GMG_API int gmg_dot(gmg_handle_t h, int64_t n, const double *a, const double *b, int memspace, double *out);

/* ---- null space of the handle's operator: SolverInterfaces/NullSpaces.jl, LinearSolvers/NullspaceSolvers.jl ------------------
 * For singular systems (pure-Neumann Poisson, enclosed-flow pressure, floating sub-problems).  A null space lives on a set-up
 * handle: k vectors of the length of its Krylov vectors, copied into storage of the library's own that stays across later
 * gmg_setup calls (numerical_setup!) and is counted by gmg_device_bytes.  Single rank only: a communicator of more than one rank
 * (real or loopback) returns GMG_ERR_UNSUPPORTED.  Every operation except _set and _size returns GMG_ERR_STATE while no null
 * space is set.  v / p / V follow `memspace`; alpha, G and the k-vectors of results are always host arrays.
 * Option nullspace_fused chooses the kernels, same bits (see gmg_set_option).
 *   _set             V: k vectors, vector q at V + q*ld (ld >= n).  n must be the handle's vector length (GMG_ERR_INVALID
 *                    otherwise, as for k < 0 or a null V with k > 0).  Replaces -- and frees -- a null space set before; k = 0 clears it.
 *   _get / _size     the vectors as they are now (after _orthonormalize: orthonormal) / k and n (0, 0: none set)
 *   _orthonormalize  make_orthonormal!(N; method), NullSpaces.jl:67-100, on the device: method 0 = :gram_schmidt, 1 =
 *                    :modified_gram_schmidt, the reference's loops in their order.  A vector whose norm is exactly 0 when it is to
 *                    be normalised: GMG_ERR_SINGULAR.
 *   _project         project!(p,N,v), :107-116: alpha_k = dot(v, w_k), p = sum_k alpha_k w_k (from 0.0, in the order k = 1..K).  p and
 *                    alpha_out may be NULL.  subtract != 0: also v = v - p in the same pass (NullspaceSolvers.jl:116).
 *   _make_orthogonal make_orthogonal!(N,v), :118-126: sequential, alpha_k from the already updated v
 *   _reconstruct     reconstruct!(N,v,alpha), :134-139
 *   _gram            G_out[i*k + j] = dot(w_i, w_j): the host evaluates is_orthonormal / is_orthogonal(N) (:33-47) from it
 *   _dots            out_k[q] = dot(v, w_q): is_orthogonal(N, v), :49-55
 *   _image_norms     out_k[q] = norm(A w_q) through the handle's finest (Krylov) operator: is_orthogonal(N, A), :57-65
 *   _project_guess   on != 0: every Krylov entry of this handle (gmg_cg_solve, gmg_fgmres_solve[_pl], gmg_minres_solve,
 *                    gmg_gmres_solve, gmg_richardson_solve) projects the initial guess, x -= sum_k dot(x, w_k) w_k, once, on the
 *                    device copy of x before the iteration starts: solve!(::NullspaceSolverNS{:projected}), NullspaceSolvers.jl:109-120
 *                    (with an orthonormal basis this removes the kernel component; the returned solution is not projected, as
 *                    in the reference).  Skipped under option x0_zero.  Off by default; off costs no launch. */
GMG_API int gmg_nullspace_set(gmg_handle_t h, int64_t n, int k, const double *V, int64_t ld, int memspace);
GMG_API int gmg_nullspace_get(gmg_handle_t h, double *V_out, int64_t ld, int memspace);
GMG_API int gmg_nullspace_size(gmg_handle_t h, int *k, int64_t *n);
GMG_API int gmg_nullspace_orthonormalize(gmg_handle_t h, int method);
GMG_API int gmg_nullspace_project(gmg_handle_t h, double *v, double *p, double *alpha_out, int memspace, int subtract);
GMG_API int gmg_nullspace_make_orthogonal(gmg_handle_t h, double *v, double *alpha_out, int memspace);
GMG_API int gmg_nullspace_reconstruct(gmg_handle_t h, double *v, const double *alpha, int memspace);
GMG_API int gmg_nullspace_gram(gmg_handle_t h, double *G_out);
GMG_API int gmg_nullspace_dots(gmg_handle_t h, const double *v, double *out_k, int memspace);
GMG_API int gmg_nullspace_image_norms(gmg_handle_t h, double *out_k);
GMG_API int gmg_nullspace_project_guess(gmg_handle_t h, int on);
/* NullspaceSolver(LUSolver(), N; constrain_matrix = true) as the coarsest solver (NullspaceSolvers.jl:59-107): Kc holds k kernel
 * vectors of the coarsest matrix (vector q at Kc + q*ld, host memory; the coarsest matrix must have been set).  With the
 * dense-inverse coarse solver gmg_setup then inverts [A_L Kc; Kc' 0] on the host (LU with partial pivoting) and keeps its leading
 * n_L x n_L block: the per-cycle solve is the same GEMV, its result is orthogonal to Kc.  n_L + k > coarse_host_max, or another
 * coarse solver kind: GMG_ERR_UNSUPPORTED at gmg_setup.  gmg_update_values + gmg_setup rebuild it (numerical_setup!, :77-90).
 * k = 0 removes the constraint. */
GMG_API int gmg_set_coarse_nullspace(gmg_handle_t h, int k, const double *Kc, int64_t ld);

/* ---- multi-GPU: one handle per rank/GPU ---------------------------------
 * The reference row-partitions every level with PartitionedArrays (own-then-ghost local
 * numbering, JacobiLinearSolvers.jl:29-56) and communicates through `consistent!`
 * (owner->ghost, PatchSolvers.jl:231,256 and inside mul!(::PVector,::PSparseMatrix,::PVector))
 * and the reductions inside dot/norm.  Call order: gmg_create, gmg_comm_init_*,
 * gmg_set_partition + gmg_set_matrix/prolongation/restriction with LOCAL operators
 * (rows = owned dofs, columns = [own | ghost]), gmg_set_replication, gmg_setup.
 * Vectors passed to the solve calls hold the OWNED entries only. */
typedef void (*gmg_host_exchange_fn)(void *ctx, int nnbr, const int32_t *nbr_rank, const double *sendbuf,
                                     const int64_t *snd_ptr, double *recvbuf, const int64_t *rcv_ptr);
typedef void (*gmg_host_allreduce_fn)(void *ctx, double *vals, int n);
/* ncclGetUniqueId through the RCCL library at rccl_path (NULL: librccl.so.1); 128 bytes out.
 * Rank 0 calls it and the host language broadcasts the blob (MPI.bcast / torch.distributed). */
GMG_API int gmg_comm_unique_id(const char *rccl_path, char *id_out128);
/* RCCL over xGMI: grouped ncclSend/ncclRecv halos + ncclAllReduce on the handle's stream. */
GMG_API int gmg_comm_init_rccl(gmg_handle_t h, const char *rccl_path, const char *unique_id128, int rank, int nranks);
/* Diagnostic: all-reduce of 1.5 (-> out2[0] = 1.5*nranks) and a grouped self send/recv of
 * 42.0 (-> out2[1]) through the RCCL binding; valid on a 1-rank communicator. */
GMG_API int gmg_comm_selftest(gmg_handle_t h, double *out2);
/* Latency of the communication primitives exactly as the solver issues them (no reference counterpart: PartitionedArrays'
 * consistent! / dot over MPI, PatchSolvers.jl:231, CGSolvers.jl:85): out6[0] stream time in us of one halo exchange (event
 * hand-off to the communication stream, grouped ncclSend/ncclRecv of nmsg messages of `count` doubles, event hand-off back),
 * out6[1] host time to enqueue it, out6[2] / out6[3] the same for a 1-double ncclAllReduce + square root, out6[4] the
 * exchange issued in-stream, out6[5] an empty kernel.  Peers are the ring neighbours (the rank itself on one rank). */
GMG_API int gmg_comm_latency_probe(gmg_handle_t h, int nmsg, int64_t count, int reps, double *out6);
/* Loopback (testing / bring-up on one GPU; no reference counterpart -- the reference's analogue is running its MPI tests with one
 * process, test/LinearSolvers/mpi/GMGTests.jl:5-8): after gmg_comm_init_rccl(.., rank 0, nranks 1) or gmg_comm_init_host(.., 0, 1, ..)
 * declare that the partition handed over next was written for `virtual_nranks` ranks and FOLDED onto this one: every rank's owned rows
 * stacked, every rank's ghosts stacked behind them, every neighbour entry naming a rank other than 0 -- which then means "this rank".
 * Message k of a level's plan is sent to and received from this rank itself (RCCL matches the k-th send of a group with the k-th
 * receive), so pack -> ncclGroupStart/Send/Recv/GroupEnd on the communication stream -> event -> boundary fix-up -> ncclAllReduce
 * run exactly as on `virtual_nranks` GPUs, on the one that exists.  partition.fold_ranks() builds such a partition. */
GMG_API int gmg_comm_set_loopback(gmg_handle_t h, int virtual_nranks);
/* Optional, after gmg_comm_set_loopback: own_rows[q] = owned rows of virtual rank q on the Krylov level (their sum = the folded
 * level's owned rows).  Without it a dot product or norm of the folded handle is ONE reduction over the stacked rows, which differs
 * in the last bits from the sum of the ranks' reductions that `virtual_nranks` true ranks all-reduce.  With it the reductions of
 * gmg_dot / gmg_norm, of gmg_apply's history and of gmg_cg_solve (every dot, and the update with its partial ||r||^2) run per virtual
 * rank -- the same kernels on the same row counts; every rank but the last must own an even number of rows (GMG_ERR_UNSUPPORTED
 * otherwise: its successor's part of a folded vector would lose the 16-byte alignment a rank's own vector has) -- and the
 * sums are added in rank order before the all-reduce and the square root: the folded CG run then reproduces the scalars, and so x and
 * the history, of the true-rank run bit for bit (tested with two ranks).  The other Krylov drivers reduce their first stages in
 * kernels of their own and keep the single reduction.  own_rows = NULL switches it off.  Takes effect at once (no gmg_setup). */
GMG_API int gmg_comm_set_loopback_rows(gmg_handle_t h, const int64_t *own_rows, int virtual_nranks);
/* Host-staged transport through callbacks of the host language (MPI in Julia, gloo in the
 * Python tests); lets several ranks share one GPU.  Functional, not fast. */
GMG_API int gmg_comm_init_host(gmg_handle_t h, int rank, int nranks, gmg_host_exchange_fn exchange,
                               gmg_host_allreduce_fn allreduce, void *ctx);
/* Exchange plan of level lev: neighbours, local ids of owned entries to send (0-based),
 * and the ghost sub-ranges received from each neighbour (ghosts ordered by owner). */
GMG_API int gmg_set_partition(gmg_handle_t h, int lev, int64_t n_own, int64_t n_ghost, int nnbr,
                              const int32_t *nbr_rank, const int64_t *snd_ptr, const int64_t *snd_idx,
                              const int64_t *rcv_ptr);
/* The same for a level in the OVERLAPPING layout: owned and ghost entries share ONE local numbering of n_local entries chosen by the
 * caller (a structured box partition: the box extended by `depth` node layers, lexicographic), the local matrix is square over all of
 * them (rows of ghost entries are the true global rows restricted to the local columns -- exact except on the outermost layer), and
 * one exchange makes `depth` layers consistent.  A smoothing pass of Richardson(Jacobi) then communicates once per `depth`
 * sweeps instead of once per sweep: ghost layer j is recomputed redundantly and stays exact for depth - j sweeps, owned rows are
 * exact throughout and are summed in the order of a single-GPU run.  Transfers: P_lev has a row per local entry of level lev, R_lev's
 * rows of non-owned coarse entries are empty.  Levels >= 1; the finest level too when the Krylov operator is given separately (below).
 * snd_idx / rcv_idx: local ids (0-based) sent to / received from each neighbour, both sides enumerating in the same (global) order.
 * Reference analogue: consistent!(::PVector) once per mul! (RichardsonSmoothers.jl:94 through PartitionedArrays) -- here once per
 * `depth` applications.
 * Patch smoothers (round 4): gmg_set_smoother_patch with EVERY patch whose dofs all lie in the local box (local numbering), blocks
 * A[p,p] from the local matrix -- exact there --, patch_cols = patch_rows; `depth` then counts sweeps of Richardson(PatchSolver),
 * each of which consumes 3 order - 2 node layers on vertex stars (partition._OverlapGeom).  No assemble! and no consistent!(dx)
 * inside a block: ceil(niter / depth) exchanges per pass instead of 2 niter + niter reverse exchanges (PatchSolvers.jl:227-258). */
GMG_API int gmg_set_partition_overlap(gmg_handle_t h, int lev, int64_t n_local, int64_t n_ghost, int depth, int nnbr,
                                      const int32_t *nbr_rank, const int64_t *snd_ptr, const int64_t *snd_idx,
                                      const int64_t *rcv_ptr, const int64_t *rcv_idx);
/* Two of the exchanges a V-cycle makes on an overlapping level besides the smoothing blocks can be dropped when the halo geometry allows.
 * The caller states the GEOMETRY (it knows the halo in node layers; the library only knows `depth` in sweeps), the library decides:
 *   exact_node_layers, layers_per_sweep, restriction_reach -- the halo holds `exact_node_layers` node layers around the owned box, one
 *     sweep of this level's smoother makes `layers_per_sweep` more of them inexact (Richardson-Jacobi: `order`; vertex-star patches:
 *     3 order - 2), and the restriction of an owned coarse row reads fine nodes up to `restriction_reach` away (1 for Q1, 3 for Q2).
 *     After a smoothing pass of niter sweeps in blocks of `depth` the last block has niter - depth * ((niter - 1) / depth) sweeps;
 *     when exact_node_layers - that * layers_per_sweep >= restriction_reach, consistent!(r) before `rH = R rh`
 *     (GMGLinearSolvers.jl:484) is skipped -- evaluated per pass with the niter of the smoother that just ran (pre-smoother; the
 *     post-smoother on the second leg of a W / F cycle), so pre != post niter and later gmg_set_smoother_* calls cannot make it stale;
 *   correction_exact_near_owned -- P's local rows are complete (the coarse level is replicated, or overlapping with >= 1 layer) on every
 *     fine entry that `rh_own -= (A dxh)_own` reads: consistent!(dxh) before `rh -= A dxh` (:495) is skipped -- the ghost rows of r it
 *     leaves inexact are refreshed by the consistent!(r) that opens the post-smoothing pass.
 * Call AFTER gmg_set_partition_overlap and gmg_set_smoother_* of the level: both clear the hints (they were stated for the halo / the
 * smoother that was there before); zeros = no shortcut.  partition.overlap_hints() is the structured-grid rule; results on owned rows
 * are bit-identical with and without the hints. */
GMG_API int gmg_set_partition_overlap_hints(gmg_handle_t h, int lev, int exact_node_layers, int layers_per_sweep, int restriction_reach,
                                            int correction_exact_near_owned);
/* FINEST level in the overlapping layout (round 5).  The Krylov solver's vectors are the caller's -- own | ghost numbering, its dot
 * products run over owned entries -- so the solver then holds TWO finest operators: the preconditioner's level 0 in the overlapping
 * layout (gmg_set_partition_overlap(h, 0, ...), gmg_set_matrix(h, 0, square local matrix), P_0 / R_0 in that numbering) and the
 * Krylov operator in the own | ghost layout, passed through the same entry points with lev = GMG_LEVEL_KRYLOV:
 *   gmg_set_partition(h, GMG_LEVEL_KRYLOV, n_own, n_ghost, ...) ; gmg_set_matrix(h, GMG_LEVEL_KRYLOV, n_own x (n_own + n_ghost), ...)
 *   gmg_set_krylov_map(h, own_to_local, n_own)   -- local id, in level 0's overlapping numbering, of every owned entry.
 * gmg_cg_solve / gmg_fgmres_solve / gmg_apply take vectors of n_own entries; applying the preconditioner scatters r into level 0's
 * numbering (the first smoothing block's exchange fills the ghost layers), runs the cycle, and gathers the owned entries of the
 * correction: the finest smoothing passes then communicate once per `depth` sweeps like every other overlapping level, at the price
 * of (n_local - n_own) redundant rows and 32 bytes per owned row for the two index passes.  Worth it when the finest sweep is
 * shorter than a halo exchange (multigpu.plan_partition decides; at BASELINE config 4's 288^3 cells per GPU it is not).
 * The GMG runs as a preconditioner with maxiter = 1 in this form (its own residual norms would count ghost entries).
 * Reference analogue: none -- PartitionedArrays exchanges once per mul! (RichardsonSmoothers.jl:94). */
#define GMG_LEVEL_KRYLOV (-1)
GMG_API int gmg_set_krylov_map(gmg_handle_t h, const int64_t *own_to_local, int64_t n_own);
/* Halo exchanges and all-reduces this handle has issued since gmg_create (either may be NULL). */
GMG_API int gmg_get_comm_stats(gmg_handle_t h, int64_t *n_exchanges, int64_t *n_allreduces);
/* What the handle communicates through: *transport = 0 none / 1 RCCL / 2 host callbacks, its rank and rank count, what RCCL itself
 * reports for the communicator (ncclCommCount; -1 when not RCCL) and the HIP device it sits on (ncclCommCuDevice / the handle's
 * device).  Any pointer may be NULL.  bench.py prints these so that a multi-GPU line shows how many ranks RCCL really saw. */
GMG_API int gmg_get_comm_info(gmg_handle_t h, int *transport, int *rank, int *nranks, int *comm_count, int *comm_device);
/* What the last gmg_setup decided for the own | ghost split of partitioned level `lev` (read-only: it records decisions and changes
 * none; no reference counterpart -- PartitionedArrays has one form).  boundary_rows: owned rows with at least one ghost column, the rows
 * the fix-up after the exchange finishes; send_slots: entries of the level's send lists; ghost_entries: stored entries in ghost
 * columns.  fix_form: how the fix-up holds them, see below (halo_fix_sell, halo_fix_dict); dict_values: distinct doubles among the
 * slots of the sliced form when it carries a dictionary -- the 0.0 of padded slots counts as one, so at most 256 -- else 0.
 * pack_fused: 1 when every sent row is a boundary row and the fix-up of a sweep writes the next sweep's send buffer (halo_fuse_pack),
 * 0 when a pack kernel runs before every exchange.  r_split: 1 when the level's restriction is split the same way (halo_split_r);
 * r_boundary_rows / r_ghost_entries / r_form / r_dict_values: the same for the coarse rows of R that read ghost columns (zeros, and
 * GMG_HALO_FIX_NONE, without the split).  Any output may be NULL.  GMG_ERR_STATE before a setup, and on a level that is not
 * partitioned in the own | ghost layout (single rank, replicated, overlapping layout). */
enum gmg_halo_fix_form {
  GMG_HALO_FIX_NONE = 0,                /* no row reads a ghost column: no fix-up runs */
  GMG_HALO_FIX_CSR = 1,                 /* one thread walks each boundary row (ghost_fix_kernel) */
  GMG_HALO_FIX_SLICED = 2,              /* slices of 64 boundary rows, column-major, values as doubles (ghost_fix_sell_kernel) */
  GMG_HALO_FIX_SLICED_DICT = 3          /* the same with one-byte codes into a dictionary of <= 256 doubles */
};
GMG_API int gmg_get_halo_info(gmg_handle_t h, int lev, int64_t *boundary_rows, int64_t *send_slots, int64_t *ghost_entries,
                              int *fix_form, int *dict_values, int *pack_fused, int *r_split, int64_t *r_boundary_rows,
                              int64_t *r_ghost_entries, int *r_form, int *r_dict_values);
/* Levels >= lev are REPLICATED: every rank passes the GLOBAL operators of those levels
 * (gmg_set_matrix / _prolongation / _restriction, no gmg_set_partition) and computes them
 * redundantly -- no halo traffic where the level is tiny.  Across the boundary, P_{lev-1} has
 * this rank's fine rows and GLOBAL coarse columns; R_{lev-1} yields the rows listed in
 * own_global_ids (global numbering of level lev), which are summed into the replicated
 * residual with one all-reduce.  At least the coarsest level must be replicated.
 * Reference analogue: coarse levels living on fewer ranks (np_per_level, ModelHierarchies.jl:80-148)
 * with redistribute! at the boundary (GridTransferOperators.jl:447-532). */
GMG_API int gmg_set_replication(gmg_handle_t h, int lev, const int64_t *own_global_ids, int64_t n_own);
/* Levels lev .. (first replicated level - 1) live on a RANK SUBSET (round 5; the reference's np_per_level with redistribute! at the
 * boundary, ModelHierarchies.jl:80-148, GridTransferOperators.jl:447-532 -- redistribute_cell_dofs! there, two p2p plans here).
 * Level lev then exists in two partitions: the GLUED one of all ranks (its dofs with the owners of the fine dofs they coincide with;
 * own | ghost numbering of n_glue_own + n_glue_ghost entries: P_{lev-1} has those columns, R_{lev-1} yields the n_glue_own owned rows)
 * and the subset's (gmg_set_partition / _overlap + operators on the member ranks only; the other ranks pass nothing for the levels
 * lev .. rep-1 and member = 0).  to_sub carries the restricted residual from the glued owners to the subset owners; from_sub carries
 * the correction from the subset owners to the glued own AND ghost entries (so P needs no consistent! of its own).  A plan lists
 * per neighbour the local ids sent (in the source space) and the local ids received (in the destination space), both sides in the
 * same order, plus the entries that stay on the rank.  Ranks outside the subset take part in the collectives below (the all-reduce
 * that assembles the replicated residual) with a zero contribution.  Every rank calls this, with its own plans, before gmg_setup. */
typedef struct {
  int nnbr;
  const int32_t *nbr_rank;
  const int64_t *snd_ptr, *snd_idx, *rcv_ptr, *rcv_idx;
  int64_t nself;
  const int64_t *self_src, *self_dst;
} gmg_redist_plan;
GMG_API int gmg_set_redistribution(gmg_handle_t h, int lev, int member, int64_t n_glue_own, int64_t n_glue_ghost,
                                   const gmg_redist_plan *to_sub, const gmg_redist_plan *from_sub);

/* ---- measurement --------------------------------------------------------------- */
/* Bracket launches of the fused Richardson-Jacobi sweep on `lev` with HIP events on the handle's
 * stream: every GMG_PROF_STRIDE-th launch (default 7 -- odd on purpose: sweeps alternate between the variant that leaves x
 * alone and the one that adds two increments to it, `x = (x + s_{k-1}) + s_k`, and an even stride would time one of them only;
 * a sampled launch costs ~11 us of stream time -- two ~5.7 us bubbles, one per event (profiles/r05_tuning.md section 7: at stride 7 that
 * was 5 % of a 128^3 solve) -- so a caller that times whole solves at the same time sets the option prof_stride (read at this call;
 * odd and coprime with the number of sweeps per solve, e.g. 61) to keep the samples rare); enable=0 stops.  Read with gmg_get_kernel_stats (launch-weighted totals) and
 * gmg_get_kernel_stats_by_variant (index 0: sweeps that update x every time -- the generic layouts' first sweep, one-launch
 * passes, patch sweeps; 1: x untouched; 2: x updated with two increments; layout_bytes[v] = the bytes ONE launch of form v moves with the
 * stored layout, every operand once -- gmg_kernel_stats.layout_bytes is their launch-weighted mean). */
GMG_API int gmg_profile_enable(gmg_handle_t h, int lev, int enable);
GMG_API int gmg_get_kernel_stats(gmg_handle_t h, gmg_kernel_stats *out);
GMG_API int gmg_get_kernel_stats_by_variant(gmg_handle_t h, double total_ms[3], int64_t launches[3], double layout_bytes[3]);
/* Algorithmic bytes (SURVEY 8d byte model) of one V-cycle / one CG iteration. */
GMG_API int gmg_model_bytes(gmg_handle_t h, double *vcycle_bytes, double *cg_iter_bytes);
/* Storage chosen for A_lev at setup: *sell = 0 CSR-stream, 1 SELL-64 / SELL-C, 2 SELL-P (row-pattern
 * dictionary), 3 SELL-O (SELL-64 value stream, column offsets from an offset-pattern table); 8-bit value dictionary, 16-bit column offsets, bytes of matrix stream per stored nonzero,
 * padding factor. */
GMG_API int gmg_level_format(gmg_handle_t h, int lev, int *sell, int *vdict, int *idx16,
                             double *stream_bytes_per_nnz, double *padding);
/* cycle_values = "float32" (no counterpart in the reference, whose level matrices are the caller's SparseMatrixCSC{Float64};
 * GMGLinearSolvers.jl:468-500 is the cycle it applies to).  Option values_f32 = 1: inside the cycle of a preconditioner-mode handle
 * every level but the coarsest that gmg_setup lays out as SELL-64 or SELL-O with an explicit value stream is streamed from a float
 * copy of that stream.  The preconditioner is then exactly the fp64 cycle on the matrices whose stored values were rounded to float32
 * (nearest even) and read back as fp64: vectors, transfers, the coarsest solve and all arithmetic stay fp64, 1/diag of such a level
 * is that of the rounded matrix, and nothing outside the cycle reads the rounded values -- the Krylov drivers and gmg_op_apply stream
 * the fp64 ones.  Level 0 holds both streams; levels >= 1 release their fp64 values (gmg_op_apply(GMG_OP_A) is GMG_ERR_STATE there).
 * Levels on SELL-P / SELL-C / CSR-stream tiles and the coarsest level are untouched.  gmg_update_values[_csc] + gmg_setup refill both
 * streams in place.  gmg_setup refuses with GMG_ERR_INVALID: mode = solver, a partitioned handle, a Galerkin level, a patch-corrected
 * prolongation, a smoother other than Richardson-Jacobi on a level that would be float32, and a nonzero stored value outside
 * float32's normal range (magnitude below 2^-126 or rounding to infinity; the message names level and row, nothing is scaled).
 * gmg_level_values: *is_f32 = 1 on a float32 level, whose cycle stream is 8.0 (SELL-64: 4 B column + 4 B value) or 4.0 (SELL-O)
 * bytes per stored nonzero; elsewhere 0 and the figure of gmg_level_format, which itself is unchanged. */
GMG_API int gmg_level_values(gmg_handle_t h, int lev, int *is_f32, double *cycle_stream_bytes_per_nnz);
/* Kernel + template arguments + launch geometry of the fused sweep last launched on level lev ("" before the first sweep):
 * committed counter measurements (profiles/traffic_latest.json) are only attached to a bench line whose sweep has this signature.
 * A level that has run no row sweep (patch-smoothed wide-row levels) reports the wide-row operator kernel its matrix first ran
 * (sellw_zwalk_kernel<...>), or "" if none. */
GMG_API int gmg_sweep_signature(gmg_handle_t h, int lev, char *buf, int cap);
/* Measured streaming ceiling: a 16 B/lane copy kernel over nbytes (read) + nbytes (write), reps launches timed with HIP
 * events on the handle's stream; *gbytes_per_s = moved bytes / time.  Reported by bench.py beside the 8 TB/s spec. */
GMG_API int gmg_stream_probe(gmg_handle_t h, int64_t nbytes, int reps, double *gbytes_per_s);
/* The same for a READ-ONLY stream of nbytes (the sweeps read ~9x more than they write, so their ceiling lies between the two). */
GMG_API int gmg_stream_probe_read(gmg_handle_t h, int64_t nbytes, int reps, double *gbytes_per_s);
/* Device memory held by the handle, bytes. */
GMG_API int gmg_device_bytes(gmg_handle_t h, int64_t *bytes);

/* ---- block preconditioners --------------------------------------------------
 * The glue that calls the GMG hot path once per outer FGMRES iteration in the reference's block
 * applications (test/Applications/StokesGMG.jl:142-153): BlockDiagonalSolver
 * (BlockSolvers/BlockDiagonalSolvers.jl:165-177) and BlockTriangularSolver
 * (BlockSolvers/BlockTriangularSolvers.jl:186-242) with the outer CG / FGMRES on the block system,
 * all on the device.  Block vectors are contiguous: block i occupies [off_i, off_i + size_i).
 * A gmg handle given to gmg_block_set_diag_gmg stays owned by the caller, must be set up
 * first, must outlive the block handle's use of it and issues its work on the block handle's stream
 * from gmg_block_setup until gmg_block_destroy. */
typedef struct gmg_block_solver *gmg_block_handle_t;
enum gmg_block_kind {
  GMG_BLOCK_DIAGONAL = 0, GMG_BLOCK_LOWER = 1, GMG_BLOCK_UPPER = 2,
  GMG_BLOCK_SCHUR = 3       /* SchurComplementSolver(A,B,C,S), LinearSolvers/SchurComplementSolvers.jl:11-74 */
};
enum gmg_block_diag_kind {
  GMG_BLOCK_GMG = 1,        /* a GMGLinearSolver numerical setup (gmg handle) */
  GMG_BLOCK_CG_JACOBI = 2,  /* CGSolver(JacobiLinearSolver();maxiter,atol,rtol), CGSolvers.jl:73-120 */
  GMG_BLOCK_LU = 3,         /* LUSolver() on a small block: dense inverse on the device */
  GMG_BLOCK_JACOBI = 4,     /* JacobiLinearSolver(), JacobiLinearSolvers.jl:43-47 */
  GMG_BLOCK_KRYLOV_GMG = 5  /* FGMRESSolver(m,gmg) / GMRESSolver(m;Pr|Pl=gmg) / CGSolver(gmg): gmg_block_set_diag_krylov_gmg */
};
enum gmg_krylov_kind { GMG_KRYLOV_CG = 1, GMG_KRYLOV_FGMRES = 2, GMG_KRYLOV_GMRES = 3 };
/* BlockDiagonalSolver(solvers) / BlockTriangularSolver(blocks,solvers,coeffs,half): BlockTriangularSolvers.jl:55-85.
 * kind = GMG_BLOCK_SCHUR (exactly 2 blocks, GMG_ERR_INVALID otherwise): the block factorisation of [A B; C D] with S ~ D - C A^-1 B,
 *   solve!(x_u,A,y_u); bp = y_p - C x_u; solve!(x_p,S,bp); bu = B x_p; solve!(du,A,bu); x_u .-= du     (SchurComplementSolvers.jl:65-71)
 * The solver of block 0 is A's and that of block 1 is S's (gmg_block_set_diag_*; S brings its own matrix when the system has no
 * (1,1) block); B = block (0,1) and C = block (1,0), from gmg_block_set_precond_block or else the system; gmg_block_setup gives
 * GMG_ERR_STATE when one is absent.  The two first solves write into the caller's x: its content on entry is the initial guess of
 * an iterative block solver (CG-Jacobi, a GMG in solver mode), and du is kept between applications -- the triangular kinds solve
 * into an internal vector instead.  Coefficients are not consulted.  Single-GPU: GMG_ERR_UNSUPPORTED at gmg_block_setup on a
 * handle with a communicator of more than one rank. */
GMG_API int gmg_block_create(gmg_block_handle_t *h, int nblocks, const int64_t *block_sizes, int kind, int device_id);
GMG_API int gmg_block_destroy(gmg_block_handle_t h);
GMG_API const char *gmg_block_last_error(gmg_block_handle_t h);
/* Distributed block systems (one handle per rank, like the GMG handles): the communicator of the block solver, and per block
 * the exchange plan of its vector space (same meaning as gmg_set_partition; blocks without ghost columns need none).  Call
 * before the blocks are set: block (i,j) then has bsize(i) rows and bsize(j) + n_ghost(j) columns ([own | ghost] numbering
 * of block j), block vectors hold the owned entries of every block, a GMG handle given to gmg_block_set_diag_gmg is itself
 * distributed over the same ranks.  Reference: BlockTriangularSolvers.jl:216-242 on BlockPVector / BlockPMatrix
 * (test/Applications/mpi/StokesGMG.jl).  LUSolver() diagonal blocks stay single-GPU. */
GMG_API int gmg_block_comm_init_rccl(gmg_block_handle_t h, const char *rccl_path, const char *unique_id128, int rank, int nranks);
GMG_API int gmg_block_comm_init_host(gmg_block_handle_t h, int rank, int nranks, gmg_host_exchange_fn exchange,
                                     gmg_host_allreduce_fn allreduce, void *ctx);
/* gmg_comm_set_loopback for a block handle: its own communicator of one rank serves a folded partition (see there). */
GMG_API int gmg_block_comm_set_loopback(gmg_block_handle_t h, int virtual_nranks);
GMG_API int gmg_block_set_partition(gmg_block_handle_t h, int j, int64_t n_own, int64_t n_ghost, int nnbr,
                                    const int32_t *nbr_rank, const int64_t *snd_ptr, const int64_t *snd_idx,
                                    const int64_t *rcv_ptr);
/* blocks(mat)[i,j] of the system matrix (numerical_setup(ss,mat::AbstractBlockMatrix), BlockTriangularSolvers.jl:132-152);
 * absent blocks are zero. */
GMG_API int gmg_block_set_system_block(gmg_block_handle_t h, int i, int j, int64_t nrows, int64_t ncols, int64_t nnz,
                                       const void *ptr, const void *idx, const double *val,
                                       int layout, int index_base, int index_bytes);
/* Off-diagonal block of the PRECONDITIONER when it is not the system's (MatrixBlock / BiformBlock,
 * BlockSolverInterfaces.jl); default = the system block (LinearSystemBlock). */
GMG_API int gmg_block_set_precond_block(gmg_block_handle_t h, int i, int j, int64_t nrows, int64_t ncols, int64_t nnz,
                                        const void *ptr, const void *idx, const double *val,
                                        int layout, int index_base, int index_bytes);
/* coeffs[i,j] (default 1.0; a zero coefficient drops the block, BlockTriangularSolvers.jl:194,223) */
GMG_API int gmg_block_set_coeff(gmg_block_handle_t h, int i, int j, double c);
/* solvers[i] */
GMG_API int gmg_block_set_diag_gmg(gmg_block_handle_t h, int i, gmg_handle_t g);
/* solvers[i] = a Krylov solver around a GMG (test/Applications/NavierStokesGMG.jl:159-169: solver_u = FGMRESSolver(20,gmg;...)):
 * solve A y_i = w_i with A the GMG handle's own finest matrix -- the operator of gmg_fgmres_solve -- by FGMRES (FGMRESSolvers.jl:130-199,
 * the GMG as Pr), GMRES (GMRESSolvers.jl:132-210, side 0 = Pr, 1 = Pl) or CG (CGSolvers.jl:73-120, the GMG as Pl; flexible as there),
 * preconditioned by that GMG.  m, restart, m_add: FGMRES / GMRES; flexible: CG.  The content of y_i on entry is the initial guess: for
 * the diagonal and triangular kinds y_i is the handle's internal vector, which persists between applications (the reference's
 * ns.work_caches; zero after the first setup); for GMG_BLOCK_SCHUR it is the caller's x, then du (SchurComplementSolvers.jl:65-70).
 * The nested solve runs on the GMG handle's scalar slots, host mailbox, basis caches (allocated at the first application, kept across
 * gmg_setup refreshes of the GMG handle and counted by its gmg_device_bytes) on the block handle's stream, so it never collides with
 * the outer solve on the block handle.  numerical_setup!: as for a GMG block -- the caller refreshes the GMG handle,
 * gmg_block_refresh_diag_solver only checks it; an in-place gmg_block_setup stays in place.  The wrapper keeps a ConvergenceLog of
 * its own (gmg_block_diag_log: the last nested solve, not the GMG's).  Option fgmres_fused of the GMG handle chooses the kernels of
 * a nested FGMRES column (default: fused), same bits.
 * GMG_ERR_INVALID: bad krylov / side (FGMRES: 0, CG: 1), m < 1 or m_add < 1 (FGMRES / GMRES), a GMG handle that is not set up or whose
 * finest size is not bsize(i).  GMG_ERR_UNSUPPORTED at gmg_block_setup, naming the block, when the block handle or the GMG handle has
 * a communicator of more than one rank. */
GMG_API int gmg_block_set_diag_krylov_gmg(gmg_block_handle_t h, int i, gmg_handle_t g, int krylov, int m, int restart, int m_add,
                                          int flexible, int side, int maxiter, double atol, double rtol);
GMG_API int gmg_block_set_diag_solver(gmg_block_handle_t h, int i, int kind, int maxiter, double atol, double rtol);
/* matrix the solver of block i is set up on when it is not the system block (i,i) (e.g. the -1/alpha
 * pressure mass matrix, StokesGMG.jl:145) */
GMG_API int gmg_block_set_diag_matrix(gmg_block_handle_t h, int i, int64_t n, int64_t nnz, const void *ptr,
                                      const void *idx, const double *val, int layout, int index_base, int index_bytes);
/* numerical_setup; after gmg_block_update_values* / gmg_block_refresh_diag_solver: numerical_setup! (see below) */
GMG_API int gmg_block_setup(gmg_block_handle_t h);
/* ---- numerical_setup!(ns,A,x) of a block solver: new values on the same patterns, once per Newton step
 * (NonlinearSolvers/NewtonRaphsonSolver.jl:45,73 -> FGMRESSolvers.jl:112-128 -> BlockTriangularSolvers.jl:156-186 /
 * BlockDiagonalSolvers.jl:153-163 -> BlockSolverInterfaces.jl:104-118,232-236 -> GMGLinearSolvers.jl:260-297).
 * The update calls record the values on the handle's host copy of the block and mark it; gmg_block_setup must be called again.
 * GMG_ERR_STATE before the first gmg_block_setup; GMG_ERR_INVALID, with nothing changed, for an absent block, a wrong slot or a CSC
 * pattern whose size disagrees with the stored block.  When nothing but values changed since the last setup (no block set again, no
 * solver, partition or communicator changed, no coefficient changed from or to zero), the communicator has one rank, GMG_REFRESH
 * is not 0 and every changed block is stored with explicit values (CSR-stream or SELL-64: the rule of gmg_update_values), that
 * gmg_block_setup works IN PLACE: nothing is freed or allocated -- work vectors, Krylov bases, attachments stay -- and each changed
 * block costs one host-to-device copy of its values and a refill on the device.  Otherwise it is a full setup.  Both give the
 * same bits and keep the same state: the internal solution vector (the initial guesses of CG-Jacobi block solvers, the Schur
 * solver's du: the reference keeps its work caches across numerical_setup!) and a null space set on the handle survive either.
 * Which solvers are set up again follows the reference:
 *  - a diagonal block marked with gmg_block_refresh_diag_solver (NonlinearSystemBlock, BlockSolverInterfaces.jl:206-214,232-236):
 *    Jacobi / CG-Jacobi recompute D^-1 from the current values of their matrix (a zero diagonal: GMG_ERR_SINGULAR naming the block), LU
 *    rebuilds its dense inverse; for a GMG block the caller has refreshed the GMG handle itself (gmg_update_values* + gmg_setup on
 *    it, which leave it attached and on the block handle's stream) and the block handle only checks that it is set up;
 *  - a block that is not marked (LinearSystemBlock, MatrixBlock, :104-109) keeps its D^-1 / inverse EVEN WHEN system block (i,i) was
 *    updated: a Jacobi / CG-Jacobi block that streams the system's own (i,i) block then iterates on the new operator with the
 *    old D^-1 -- what the reference's aliasing gives when jacobian! updates A in place;
 *  - an off-diagonal preconditioner block without a gmg_block_set_precond_block entry IS the system block's storage and follows it.
 * Marks hold for one gmg_block_setup. */
enum gmg_block_slot { GMG_BLOCK_SLOT_SYSTEM = 0, GMG_BLOCK_SLOT_PRECOND = 1, GMG_BLOCK_SLOT_DIAG_MATRIX = 2 };
/* same pattern, new values, in the order of the arrays handed to gmg_block_set_system_block / _precond_block /
 * _diag_matrix (slot DIAG_MATRIX: j is ignored).  CSR-set blocks: values in CSR order. */
GMG_API int gmg_block_update_values(gmg_block_handle_t h, int slot, int i, int j, const double *val);
/* blocks that were set in GMG_CSC layout (GMG_ERR_STATE otherwise): nzval in CSC order; the first call per block also takes the
 * unchanged colptr / rowidx and records the transposition, later calls may pass NULL for both (as gmg_update_values_csc) */
GMG_API int gmg_block_update_values_csc(gmg_block_handle_t h, int slot, int i, int j, const void *colptr, const void *rowidx,
                                        const double *val, int index_base, int index_bytes);
/* block_numerical_setup!(NonlinearSystemBlock, ...), BlockSolverInterfaces.jl:232-236: the solver of diagonal block i is set up
 * again at the next gmg_block_setup from the current values of its matrix */
GMG_API int gmg_block_refresh_diag_solver(gmg_block_handle_t h, int i);
/* what the last gmg_block_setup did: kind 1 = full, 2 = in place; blocks whose values were (re)written; bytes of
 * values sent to the device; device bytes the handle holds now.  NULL pointers are skipped. */
GMG_API int gmg_block_get_setup_info(gmg_block_handle_t h, int *kind, int64_t *blocks_refreshed, int64_t *value_bytes,
                                     int64_t *device_bytes);
/* solve!(x,ns::BlockDiagonalSolverNS|BlockTriangularSolverNS,b) */
GMG_API int gmg_block_precond_apply(gmg_block_handle_t h, const double *b, double *x, int memspace);
/* mul!(y,A,x) on the block system */
GMG_API int gmg_block_apply_system(gmg_block_handle_t h, const double *x, double *y, int memspace);
/* FGMRESSolver(m,P) / CGSolver(P) on the block system with P = this block preconditioner (use_precond=1)
 * or nothing (0): FGMRESSolvers.jl:130-199, CGSolvers.jl:73-120 */
GMG_API int gmg_block_fgmres_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int m, int restart,
                                   int m_add, int maxiter, double atol, double rtol, int use_precond,
                                   gmg_result *res, double *hist, int hist_cap);
GMG_API int gmg_block_cg_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int maxiter, double atol,
                               double rtol, int flexible, int use_precond, gmg_result *res, double *hist, int hist_cap);
/* MINRESSolver(;Pl=P) on the block system with P = this block preconditioner (use_precond=1) or nothing (0):
 * MINRESSolvers.jl:75-148.  MINRES assumes a symmetric positive definite P (BlockDiagonalSolver with SPD blocks); a
 * block-triangular P is not rejected -- the reference does not reject it -- but lies outside those assumptions. */
GMG_API int gmg_block_minres_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int maxiter, double atol,
                                   double rtol, int use_precond, gmg_result *res, double *hist, int hist_cap);
/* GMRESSolver(m;Pr,Pl) on the block system (GMRESSolvers.jl:132-210): use_precond_right / use_precond_left are 0 (nothing) or 1
 * (this block preconditioner); at most one side may be 1 (GMG_ERR_INVALID otherwise).  Other arguments as gmg_gmres_solve. */
GMG_API int gmg_block_gmres_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int m, int restart, int m_add,
                                  int maxiter, double atol, double rtol, int use_precond_right, int use_precond_left,
                                  gmg_result *res, double *hist, int hist_cap);
/* ConvergenceLog of the last solve of diagonal block i (GMG / CG blocks; GMG_BLOCK_KRYLOV_GMG: the wrapper's own log) */
GMG_API int gmg_block_diag_log(gmg_block_handle_t h, int i, gmg_result *res);
/* applications of the solver of diagonal block i and the iterations they took in all, since the last gmg_block_setup (GMG, CG-Jacobi
 * and GMG_BLOCK_KRYLOV_GMG blocks; GMG_ERR_STATE for a direct one).  NULL pointers are skipped. */
GMG_API int gmg_block_diag_stats(gmg_block_handle_t h, int i, int64_t *napplies, int64_t *total_iters);
/* The null space of the block system (vectors of the total length, blocks concatenated): the twins of gmg_nullspace_* above, same
 * arguments and status codes; _project_guess covers gmg_block_cg_solve, _fgmres_solve, _minres_solve and _gmres_solve; _image_norms
 * applies the system blocks.  The handle must be set up; the null space stays across later gmg_block_setup calls. */
GMG_API int gmg_block_nullspace_set(gmg_block_handle_t h, int64_t n, int k, const double *V, int64_t ld, int memspace);
GMG_API int gmg_block_nullspace_get(gmg_block_handle_t h, double *V_out, int64_t ld, int memspace);
GMG_API int gmg_block_nullspace_size(gmg_block_handle_t h, int *k, int64_t *n);
GMG_API int gmg_block_nullspace_orthonormalize(gmg_block_handle_t h, int method);
GMG_API int gmg_block_nullspace_project(gmg_block_handle_t h, double *v, double *p, double *alpha_out, int memspace, int subtract);
GMG_API int gmg_block_nullspace_make_orthogonal(gmg_block_handle_t h, double *v, double *alpha_out, int memspace);
GMG_API int gmg_block_nullspace_reconstruct(gmg_block_handle_t h, double *v, const double *alpha, int memspace);
GMG_API int gmg_block_nullspace_gram(gmg_block_handle_t h, double *G_out);
GMG_API int gmg_block_nullspace_dots(gmg_block_handle_t h, const double *v, double *out_k, int memspace);
GMG_API int gmg_block_nullspace_image_norms(gmg_block_handle_t h, double *out_k);
GMG_API int gmg_block_nullspace_project_guess(gmg_block_handle_t h, int on);

#ifdef __cplusplus
}
#endif
#endif /* GMG_AMD_H */
