// gs.inc.hpp -- GaussSeidelSmoother / SymGaussSeidelSmoother (reference src/LinearSolvers/SymGaussSeidelSmoothers.jl) on the device
// (included at the end of gmg_amd.hip).
//
// solve!(x, ns, r), :175-208, repeats niter times: forward pass (types :forward, :symmetric) dx = L \ r ; dx .= w dx ; x .+= dx ;
// r .-= A dx, then the same backward pass with U (types :backward, :symmetric).  L / U: lower / upper triangle WITH the diagonal.
//
// The triangular solves run over the LEVEL SETS of the dependency graph: set(i) = 1 + max set(j) over the stored j < i (forward;
// j > i backward), 0 without any.  Rows of one set are independent, so one lane solves one row.  Seen from row i the reference's
// column-oriented loops (forward_sub! :55-69, backward_sub! :77-91) subtract a_ij * x_j in ascending j (forward) / descending j
// (backward), one rounded product and one rounded subtraction each, and divide by a_ii at the end: the tables hold the strict
// triangle of every row in exactly that order, and the library is built with -ffp-contract=off, so the results are bit for bit
// the reference's.  w scales AFTER the whole solve (rows read their dependencies unscaled).
//
// Tables per direction: rows permuted by set (stable in the row index); the strict triangle in slices of at most 64 permuted rows,
// column-major (int32 column, double value; lane q of a slice of `rows` rows reads entry j at off + j * rows + q), padded to the
// slice's longest row with column -1; a slice never straddles a set boundary.  The diagonal per permuted row.
//
// ONE kernel, gs_sets_kernel(sets [s0, s1)), two launch shapes fixed at setup from the set sizes:
//   chain  one workgroup of 1024 threads walks consecutive sets of at most 1024 rows each, __syncthreads() between sets;
//   wide   exactly one set of more than 1024 rows, ceil(rows / 256) workgroups of 256 threads.
// No launch waits on another workgroup: ordering across workgroups comes from launch boundaries only.
//
// VISITING ORDER (gmg_set_gs_ordering).  A level may be swept in another order than the natural one: order[k] is the row the forward
// sweep visits k-th, pos its inverse.  The solves are then forward_sub! / backward_sub! on B = A[order, order] applied to r[order]
// and scattered back: row i = order[k] subtracts a_ij dx_j over the stored j with pos(j) < k in ascending pos(j) (forward; pos(j) > k
// descending backward).  Schedule and tables are gs_schedule / gs_fill on B with rows and columns translated back to the level's
// numbering ("stable in the row index" reads "stable in the position").  MULTICOLOR is greedy first-fit on the symmetrised STORED
// pattern (explicit zeros count: rows of one colour then share no stored entry, and the level sets of B are the colours), rows sorted
// stably by colour.  The sets of such an order are few and large, and their launches go through a kernel of their own:
//   gs_wide_kernel  one wave per slice of 64 permuted rows, the slice header read once per wave, the entries in groups of four whose
//                   col / val loads issue back to back before their dx gathers (clamped index + select: no branch around a load).
//                   Same subtractions in the same order as gs_sets_kernel: the same bits.  Where w == 1 and EVERY launch of the
//                   direction's plan is wide, each lane also updates x and the gs_update_kernel launch of that direction is dropped.
// The natural order keeps gs_sets_kernel for both shapes.
//
// SEVERAL RANKS (the reference's distributed form, :155-165 with :71-75 / :93-97): every rank builds DiagonalIndices of its local matrix
// over own_to_local(indices) and runs forward_sub! / backward_sub! on own_values(x), so the triangles are those of the OWN x OWN BLOCK
// of each rank -- rank-block Gauss-Seidel, no communication inside a triangular solve -- and mul!(Adx, A, dx) is the distributed
// product with its halo exchange.  On an own | ghost level (gmg_set_partition) schedule, colouring, given order and tables are those
// of rows [0, n_own) and the stored columns < n_own of the level matrix; ghost columns enter nothing here, they are applied by
// r -= A dx (apply_A_sub: begin_exchange(dx), own columns, boundary fix-up).  A replicated level sweeps its global matrix (the
// reference with one part at that level); the overlapping layout is refused at gmg_setup.
//   gs_update_pack_kernel  dx .= w dx ; x .+= dx AND the pack of dx's send entries in one launch (option gs_pack_fused, default 1), on
//                   levels whose pack can fuse (can_fuse_pack: every sent row is a boundary row).  THE CHOICE: a row -> boundary-row
//                   index table of the level (Level::bidx, -1 off the boundary) leads the lane that updates row i to the row's
//                   send slots (the level's d_pk_ptr / d_pk_slot), and that lane stores the value it has just written to dx[i]:
//                   nobody reads dx[i] while another lane scales it.  Same roundings as gs_update_kernel.  Where the x update folds
//                   into gs_wide_kernel there is no update launch and the pack stays halo_pack_kernel.

namespace {

constexpr int kGsChainThreads = 1024;   // a set of at most this many rows is one pass of the chain workgroup
constexpr int kGsWideThreads = 256;

struct GsDir {
  bool built = false;
  int64_t nsets = 0, max_set_rows = 0, nslices = 0, nent = 0, nwide = 0;
  bool ordered = false;   // the level has a visiting order of its own: wide launches run gs_wide_kernel
  bool all_wide = false;  // every launch of the plan is wide (with `ordered` and w == 1 the x update folds into them)
  struct Launch { int32_t s0, s1; bool wide; };
  std::vector<Launch> plan;
  // host copy of the schedule: a value refresh refills val / diag through it (h_perm in the numbering of the ordered matrix)
  std::vector<int32_t> h_perm, h_slice0;
  std::vector<int64_t> h_setptr, h_soff;
  // device
  int32_t *perm = nullptr, *slice0 = nullptr, *col = nullptr;
  int64_t *setptr = nullptr, *soff = nullptr;
  double *val = nullptr, *diag = nullptr;
};

struct GsLevel {
  GsDir dir[2];          // 0 forward (L), 1 backward (U)
  // the visiting order this setup used (gmg_get_gs_ordering); `order` empty = natural.  A value refresh keeps it.
  int order_kind = GMG_GS_ORDER_NATURAL;
  int64_t ncolors = 0;
  std::vector<int32_t> order;
};

// rows of sets [s0, s1): dx[i] = (r[i] - sum_j a_ij dx[j]) / a_ii over the strict triangle in table order
__global__ void __launch_bounds__(kGsChainThreads)
gs_sets_kernel(int s0, int s1, const int64_t *__restrict__ setptr, const int32_t *__restrict__ slice0, const int64_t *__restrict__ soff,
               const int32_t *__restrict__ perm, const int32_t *__restrict__ col, const double *__restrict__ val,
               const double *__restrict__ diag, const double *r, double *dx)
{
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  for (int s = s0; s < s1; ++s) {
    const int64_t p0 = setptr[s], p1 = setptr[s + 1];
    for (int64_t q = tid; q < p1 - p0; q += nthr) {
      const int64_t sl = q >> 6;
      const int lane = (int)(q & 63);
      const int64_t rows = min((int64_t)64, p1 - p0 - (sl << 6));
      const int64_t k = (int64_t)slice0[s] + sl;
      const int64_t off = soff[k];
      const int w = (int)((soff[k + 1] - off) / rows);
      const int32_t i = perm[p0 + q];
      double acc = r[i];
      for (int j = 0; j < w; ++j) {
        const int64_t e = off + (int64_t)j * rows + lane;
        const int32_t c = col[e];
        if (c >= 0) acc = __dsub_rn(acc, __dmul_rn(val[e], dx[c]));
      }
      dx[i] = acc / diag[p0 + q];
    }
    if (s + 1 < s1) __syncthreads();                       // (chain shape only: one workgroup, the next set reads this one's rows)
  }
}

constexpr int kGsGroup = 4;             // entries of a row whose loads are in flight together (gs_wide_kernel)

__device__ __forceinline__ int64_t gs_uniform64(int64_t v)
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ONE set of an ordered sweep: permuted rows [p0, p0 + prows), slices [k0, k0 + nsl).  One wave per slice; the slice header is
// wave-uniform.  Entry j of lane q sits at off + j * rows + q, so the slice is walked by adding `rows` until its end: no division.
// xmode 0: dx only ; 1: also x_i += dx_i ; 2: also x_i = dx_i (x known to be zero) -- the rounding of gs_update_kernel at w == 1.
// A padded slot (column -1) gathers dx[0] and is dropped by the select, whatever that value is.
__global__ void __launch_bounds__(kGsWideThreads)
gs_wide_kernel(int64_t p0, int64_t prows, int64_t k0, int64_t nsl, const int64_t *__restrict__ soff, const int32_t *__restrict__ perm,
               const int32_t *__restrict__ col, const double *__restrict__ val, const double *__restrict__ diag, const double *r, double *dx,
               int xmode, double *x)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t sl = gs_uniform64((int64_t)blockIdx.x * (kGsWideThreads / 64) + (threadIdx.x >> 6));
  if (sl >= nsl) return;
  const int64_t off = gs_uniform64(soff[k0 + sl]), end = gs_uniform64(soff[k0 + sl + 1]);
  const int64_t left = prows - (sl << 6);
  const int rows = (int)(left < 64 ? left : 64);
  if (lane >= rows) return;                                  // (the ragged last slice of the set)
  const int64_t p = p0 + (sl << 6) + lane;
  const int32_t i = perm[p];
  const double d = diag[p];
  double acc = r[i];
  int64_t e = off;
  for (; e + (int64_t)(kGsGroup - 1) * rows < end; e += (int64_t)kGsGroup * rows) {
    int32_t c[kGsGroup];
    double v[kGsGroup], g[kGsGroup];
#pragma unroll
    for (int t = 0; t < kGsGroup; ++t) { c[t] = col[e + (int64_t)t * rows + lane]; v[t] = val[e + (int64_t)t * rows + lane]; }
#pragma unroll
    for (int t = 0; t < kGsGroup; ++t) g[t] = dx[c[t] < 0 ? 0 : c[t]];
#pragma unroll
    for (int t = 0; t < kGsGroup; ++t) {
      const double s = __dsub_rn(acc, __dmul_rn(v[t], g[t]));
      acc = c[t] >= 0 ? s : acc;
    }
  }
  for (; e < end; e += rows) {
    const int32_t c = col[e + lane];
    const double s = __dsub_rn(acc, __dmul_rn(val[e + lane], dx[c < 0 ? 0 : c]));
    acc = c >= 0 ? s : acc;
  }
  const double out = acc / d;
  dx[i] = out;
  if (xmode == 1) x[i] = __dadd_rn(x[i], out);
  else if (xmode == 2) x[i] = out;
}

// dx .= w .* dx (skipped at w == 1) ; x .= x .+ dx, or x = dx where x is known to be zero
__global__ void gs_update_kernel(int64_t n, double omega, int scale, int x_zero, double *__restrict__ dx, double *__restrict__ x)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {   // (grid_for caps the grid)
    double d = dx[i];
    if (scale) { d = __dmul_rn(omega, d); dx[i] = d; }
    x[i] = x_zero ? d : __dadd_rn(x[i], d);
  }
}

// gs_update_kernel on an own | ghost level + the pack of dx's send entries: the lane of row i stores the value it wrote to dx[i] into
// the row's send slots pk_slot[pk_ptr[q] .. pk_ptr[q + 1]), q = bidx[i] (every slot is below the length of sendbuf: gmg_setup)
__global__ void gs_update_pack_kernel(int64_t n, double omega, int scale, int x_zero, double *__restrict__ dx, double *__restrict__ x,
                                      const int32_t *__restrict__ bidx, const int64_t *__restrict__ pk_ptr, const int32_t *__restrict__ pk_slot,
                                      double *__restrict__ sendbuf)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {   // (grid_for caps the grid)
    const int32_t q = bidx[i];
    double d = dx[i];
    if (scale) { d = __dmul_rn(omega, d); dx[i] = d; }
    x[i] = x_zero ? d : __dadd_rn(x[i], d);
    if (q >= 0)
      for (int64_t k = pk_ptr[q]; k < pk_ptr[q + 1]; ++k) sendbuf[pk_slot[k]] = d;
  }
}

// the own x own block of an own | ghost level matrix: rows as they are, the stored columns below n_own in storage order
void gs_own_block(const HostCSR &A, int64_t n_own, HostCSR &B)
{
  B.nrows = B.ncols = n_own;
  B.ptr.assign((size_t)n_own + 1, 0);
  for (int64_t i = 0; i < n_own; ++i) {
    int64_t cnt = 0;
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k) cnt += A.col[(size_t)k] < n_own ? 1 : 0;
    B.ptr[(size_t)i + 1] = B.ptr[(size_t)i] + cnt;
  }
  B.col.resize((size_t)B.ptr[(size_t)n_own]); B.val.resize((size_t)B.ptr[(size_t)n_own]);
  parallel_for(n_own, [&](int64_t i) {
    int64_t at = B.ptr[(size_t)i];
    for (int64_t k = A.ptr[(size_t)i]; k < A.ptr[(size_t)i + 1]; ++k)
      if (A.col[(size_t)k] < n_own) { B.col[(size_t)at] = A.col[(size_t)k]; B.val[(size_t)at] = A.val[(size_t)k]; ++at; }
  });
}

// columns ascending inside every row: A itself when they are, a sorted copy in `tmp` otherwise
const HostCSR &gs_sorted_rows(const HostCSR &A, HostCSR &tmp)
{
  std::atomic<int> unsorted(0);
  parallel_for(A.nrows, [&](int64_t i) {
    for (int64_t k = A.ptr[(size_t)i] + 1; k < A.ptr[(size_t)i + 1]; ++k)
      if (A.col[(size_t)k] < A.col[(size_t)k - 1]) { unsorted.store(1); return; }
  });
  if (!unsorted.load()) return A;
  tmp = A;
  parallel_for(A.nrows, [&](int64_t i) {
    const int64_t a = A.ptr[(size_t)i], b = A.ptr[(size_t)i + 1];
    std::vector<int64_t> ord((size_t)(b - a));
    for (int64_t k = a; k < b; ++k) ord[(size_t)(k - a)] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t p, int64_t q) { return A.col[(size_t)p] < A.col[(size_t)q]; });
    for (int64_t k = a; k < b; ++k) { tmp.col[(size_t)k] = A.col[(size_t)ord[(size_t)(k - a)]]; tmp.val[(size_t)k] = A.val[(size_t)ord[(size_t)(k - a)]]; }
  });
  return tmp;
}

// position of the diagonal entry of every row (sorted rows); -1 where it is not stored
std::vector<int64_t> gs_diag_positions(const HostCSR &A)
{
  std::vector<int64_t> dpos((size_t)A.nrows, -1);
  parallel_for(A.nrows, [&](int64_t i) {
    const int32_t *c0 = A.col.data() + A.ptr[(size_t)i], *c1 = A.col.data() + A.ptr[(size_t)i + 1];
    const int32_t *it = std::lower_bound(c0, c1, (int32_t)i);
    if (it != c1 && *it == (int32_t)i) dpos[(size_t)i] = (int64_t)(it - A.col.data());
  });
  return dpos;
}

// B = A[order, order] with sorted rows: row k holds the entries of row order[k], columns renamed to their positions
void gs_permuted(const HostCSR &A, const std::vector<int32_t> &order, HostCSR &B)
{
  const int64_t n = A.nrows;
  std::vector<int32_t> pos((size_t)n);
  for (int64_t k = 0; k < n; ++k) pos[(size_t)order[(size_t)k]] = (int32_t)k;
  B.nrows = B.ncols = n;
  B.ptr.assign((size_t)n + 1, 0);
  for (int64_t k = 0; k < n; ++k) { const int64_t i = order[(size_t)k]; B.ptr[(size_t)k + 1] = B.ptr[(size_t)k] + A.ptr[(size_t)i + 1] - A.ptr[(size_t)i]; }
  B.col.resize(A.col.size()); B.val.resize(A.val.size());
  parallel_for(n, [&](int64_t k) {
    const int64_t i = order[(size_t)k], a = A.ptr[(size_t)i], cnt = A.ptr[(size_t)i + 1] - a, b = B.ptr[(size_t)k];
    std::vector<int64_t> ord((size_t)cnt);
    for (int64_t t = 0; t < cnt; ++t) ord[(size_t)t] = a + t;
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t p, int64_t q) { return pos[(size_t)A.col[(size_t)p]] < pos[(size_t)A.col[(size_t)q]]; });
    for (int64_t t = 0; t < cnt; ++t) { B.col[(size_t)(b + t)] = pos[(size_t)A.col[(size_t)ord[(size_t)t]]]; B.val[(size_t)(b + t)] = A.val[(size_t)ord[(size_t)t]]; }
  });
}

// first position of `order` that keeps it from being a permutation of [0, n); -1 if it is one
int64_t gs_bad_position(const int32_t *order, int64_t n)
{
  std::vector<uint8_t> seen((size_t)n, 0);
  for (int64_t k = 0; k < n; ++k) {
    if (order[k] < 0 || order[k] >= n || seen[(size_t)order[k]]) return k;
    seen[(size_t)order[k]] = 1;
  }
  return -1;
}

// level sets, permutation, slices and launch plan of one direction
void gs_schedule(const HostCSR &A, const std::vector<int64_t> &dpos, bool forward, GsDir &D)
{
  const int64_t n = A.nrows;
  std::vector<int32_t> set((size_t)n, 0);
  int32_t top = -1;
  for (int64_t t = 0; t < n; ++t) {
    const int64_t i = forward ? t : n - 1 - t;
    int32_t s = 0;
    if (forward) for (int64_t k = A.ptr[(size_t)i]; k < dpos[(size_t)i]; ++k) s = std::max(s, set[(size_t)A.col[(size_t)k]] + 1);
    else for (int64_t k = dpos[(size_t)i] + 1; k < A.ptr[(size_t)i + 1]; ++k) s = std::max(s, set[(size_t)A.col[(size_t)k]] + 1);
    set[(size_t)i] = s;
    top = std::max(top, s);
  }
  D.nsets = (int64_t)top + 1;
  D.h_setptr.assign((size_t)D.nsets + 1, 0);
  for (int64_t i = 0; i < n; ++i) D.h_setptr[(size_t)set[(size_t)i] + 1]++;
  D.max_set_rows = 0;
  for (int64_t s = 0; s < D.nsets; ++s) { D.max_set_rows = std::max(D.max_set_rows, D.h_setptr[(size_t)s + 1]); D.h_setptr[(size_t)s + 1] += D.h_setptr[(size_t)s]; }
  D.h_perm.resize((size_t)n);
  {
    std::vector<int64_t> fill(D.h_setptr.begin(), D.h_setptr.end() - 1);
    for (int64_t i = 0; i < n; ++i) D.h_perm[(size_t)fill[(size_t)set[(size_t)i]]++] = (int32_t)i;   // stable in the row index
  }
  // slices of at most 64 permuted rows inside a set, each padded to its longest row
  D.h_slice0.assign((size_t)D.nsets + 1, 0);
  for (int64_t s = 0; s < D.nsets; ++s)
    D.h_slice0[(size_t)s + 1] = D.h_slice0[(size_t)s] + (int32_t)((D.h_setptr[(size_t)s + 1] - D.h_setptr[(size_t)s] + 63) / 64);
  D.nslices = D.h_slice0[(size_t)D.nsets];
  D.h_soff.assign((size_t)D.nslices + 1, 0);
  for (int64_t s = 0; s < D.nsets; ++s) {
    const int64_t p0 = D.h_setptr[(size_t)s], p1 = D.h_setptr[(size_t)s + 1];
    for (int64_t b = p0; b < p1; b += 64) {
      const int64_t rows = std::min<int64_t>(64, p1 - b);
      int64_t w = 0;
      for (int64_t p = b; p < b + rows; ++p) {
        const int64_t i = D.h_perm[(size_t)p];
        w = std::max(w, forward ? dpos[(size_t)i] - A.ptr[(size_t)i] : A.ptr[(size_t)i + 1] - 1 - dpos[(size_t)i]);
      }
      D.h_soff[(size_t)(D.h_slice0[(size_t)s] + (b - p0) / 64) + 1] = rows * w;
    }
  }
  for (int64_t k = 0; k < D.nslices; ++k) D.h_soff[(size_t)k + 1] += D.h_soff[(size_t)k];
  D.nent = D.h_soff[(size_t)D.nslices];
  // launch plan: consecutive sets of at most kGsChainThreads rows share one chain launch, a larger set gets a wide launch of its own
  D.plan.clear();
  D.nwide = 0;
  for (int64_t s = 0; s < D.nsets;) {
    auto rows_of = [&](int64_t q) { return D.h_setptr[(size_t)q + 1] - D.h_setptr[(size_t)q]; };
    if (rows_of(s) > kGsChainThreads) { D.plan.push_back({(int32_t)s, (int32_t)(s + 1), true}); ++D.nwide; ++s; continue; }
    int64_t e = s;
    while (e < D.nsets && rows_of(e) <= kGsChainThreads) ++e;
    D.plan.push_back({(int32_t)s, (int32_t)e, false});
    s = e;
  }
  D.all_wide = D.nwide == (int64_t)D.plan.size();
}

// the tables of one direction in the schedule's layout: entries in the contract's order (forward: ascending column below the
// diagonal; backward: descending column above it).  col may be null (value refresh).
void gs_fill(const HostCSR &A, const std::vector<int64_t> &dpos, bool forward, const GsDir &D, int32_t *col, double *val, double *diag)
{
  parallel_for(D.nsets, [&](int64_t s) {
    const int64_t p0 = D.h_setptr[(size_t)s], p1 = D.h_setptr[(size_t)s + 1];
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t q = p - p0, sl = q >> 6, lane = q & 63;
      const int64_t rows = std::min<int64_t>(64, p1 - p0 - (sl << 6));
      const int64_t k = D.h_slice0[(size_t)s] + sl, off = D.h_soff[(size_t)k];
      const int64_t w = (D.h_soff[(size_t)k + 1] - off) / rows;
      const int64_t i = D.h_perm[(size_t)p], d = dpos[(size_t)i];
      diag[p] = A.val[(size_t)d];
      const int64_t cnt = forward ? d - A.ptr[(size_t)i] : A.ptr[(size_t)i + 1] - 1 - d;
      for (int64_t j = 0; j < w; ++j) {
        const int64_t e = off + j * rows + lane;
        const int64_t src = forward ? A.ptr[(size_t)i] + j : A.ptr[(size_t)i + 1] - 1 - j;
        if (col) col[e] = j < cnt ? A.col[(size_t)src] : -1;
        val[e] = j < cnt ? A.val[(size_t)src] : 0.0;
      }
    }
  });
}

void gs_directions(const Level &L, bool use[2])
{
  use[0] = use[1] = false;
  for (const Smoother *sp : {&L.pre, &L.post})
    if (sp->kind == SM_GAUSS_SEIDEL) {
      use[0] = use[0] || sp->gs_type != GMG_GS_BACKWARD;
      use[1] = use[1] || sp->gs_type != GMG_GS_FORWARD;
    }
}

const char *gs_tag(const Level &L)
{
  const bool f = L.gs && L.gs->dir[0].built, b = L.gs && L.gs->dir[1].built;
  return f && b ? "F+B" : f ? "F" : b ? "B" : "none";
}

} // namespace

// numerical_setup of the level's Gauss-Seidel smoother(s), :167-171: one copy of the tables per level, a direction only if a
// smoother of the level uses it.  values_only: same pattern, new values (the schedule and the column tables stay).
void gmg_solver::build_gs(int l, bool values_only)
{
  Level &L = lev[l];
  bool use[2];
  gs_directions(L, use);
  HostCSR expanded, sorted;
  const HostCSR *A0 = &L.hA;
  if (L.sA) { expanded = expand_stream(*L.sA); A0 = &expanded; }
  // own | ghost level (several ranks): the rank's block of rank-block Gauss-Seidel, rows [0, n_own) x stored columns < n_own
  const bool own_ghost = comm.nranks > 1 && L.halo.present && !L.halo.ovl;
  HostCSR block;
  if (own_ghost) {
    REQUIRE(A0->nrows == L.n && A0->ncols == L.nvec, GMG_ERR_INVALID, "Gauss-Seidel smoother: the local matrix must be n_own x (n_own + n_ghost) on level " + std::to_string(l));
    gs_own_block(*A0, L.n, block);
    A0 = &block;
  }
  REQUIRE(A0->nrows == A0->ncols && A0->nrows == L.n, GMG_ERR_INVALID, "Gauss-Seidel smoother: the level matrix must be square");
  const HostCSR &An = gs_sorted_rows(*A0, sorted);
  std::vector<int64_t> dpos = gs_diag_positions(An);
  for (int64_t i = 0; i < An.nrows; ++i)                    // SingularException(col), :31-33
    REQUIRE(dpos[(size_t)i] >= 0 && An.val[(size_t)dpos[(size_t)i]] != 0.0, GMG_ERR_SINGULAR,
            "Gauss-Seidel smoother: missing or zero diagonal entry in row " + std::to_string(i) + " on level " + std::to_string(l));
  if (!values_only) {
    L.gs = std::make_shared<GsLevel>();
    GsLevel &G = *L.gs;
    G.order_kind = L.gs_order_kind;
    if (G.order_kind == GMG_GS_ORDER_MULTICOLOR) {          // the pattern only: a value refresh keeps the order
      G.order.resize((size_t)An.nrows);
      std::vector<int32_t> color((size_t)An.nrows);
      const int st = gmg_gs_multicolor_order(An.nrows, An.ptr.data(), An.col.data(), G.order.data(), color.data(), &G.ncolors);
      REQUIRE(st == GMG_OK, st, "Gauss-Seidel smoother: colouring failed on level " + std::to_string(l) + ": " + g_last_error);
    } else if (G.order_kind == GMG_GS_ORDER_GIVEN) {
      REQUIRE((int64_t)L.gs_order.size() == An.nrows, GMG_ERR_INVALID, "Gauss-Seidel ordering of level " + std::to_string(l) + ": the order has " +
              std::to_string(L.gs_order.size()) + " entries, the level has " + std::to_string(An.nrows) + " rows (position " +
              std::to_string(std::min<int64_t>((int64_t)L.gs_order.size(), An.nrows)) + ")");
      G.order = L.gs_order;
    }
    // (the row -> boundary-row index table of gs_update_pack_kernel is the level's: Level::bidx, built with the halo split by gmg_setup)
    REQUIRE(!(own_ghost && L.halo.d_pk_ptr) || L.bidx != nullptr, GMG_ERR_STATE, "Gauss-Seidel smoother: no boundary-row index table on level " + std::to_string(l));
  }
  REQUIRE(L.gs != nullptr, GMG_ERR_STATE, "Gauss-Seidel smoother: value refresh without a schedule");
  const std::vector<int32_t> &order = L.gs->order;
  REQUIRE(order.empty() || (int64_t)order.size() == An.nrows, GMG_ERR_STATE, "Gauss-Seidel smoother: value refresh without a schedule");
  HostCSR ordered;
  if (!order.empty()) { gs_permuted(An, order, ordered); dpos = gs_diag_positions(ordered); }
  const HostCSR &A = order.empty() ? An : ordered;          // the matrix whose natural sweeps are this level's ordered ones
  for (int d = 0; d < 2; ++d) {
    GsDir &D = L.gs->dir[d];
    if (!use[d]) continue;
    if (!values_only) {
      gs_schedule(A, dpos, d == 0, D);
      D.ordered = !order.empty();
      if (D.ordered) {                                       // positions -> rows of the level
        std::vector<int32_t> rows((size_t)A.nrows);
        for (int64_t p = 0; p < A.nrows; ++p) rows[(size_t)p] = order[(size_t)D.h_perm[(size_t)p]];
        D.perm = upload(rows);
      } else D.perm = upload(D.h_perm);
      D.setptr = upload(D.h_setptr); D.slice0 = upload(D.h_slice0); D.soff = upload(D.h_soff);
      D.col = dalloc<int32_t>((size_t)D.nent); D.val = dalloc<double>((size_t)D.nent); D.diag = dalloc<double>((size_t)A.nrows);
    }
    REQUIRE(D.val != nullptr && (int64_t)D.h_perm.size() == A.nrows, GMG_ERR_STATE, "Gauss-Seidel smoother: value refresh without a schedule");
    std::vector<int32_t> hcol(values_only ? 0 : (size_t)D.nent);
    std::vector<double> hval((size_t)D.nent), hdiag((size_t)A.nrows);
    gs_fill(A, dpos, d == 0, D, values_only ? nullptr : hcol.data(), hval.data(), hdiag.data());
    if (D.ordered) parallel_for((int64_t)hcol.size(), [&](int64_t e) { if (hcol[(size_t)e] >= 0) hcol[(size_t)e] = order[(size_t)hcol[(size_t)e]]; });
    if (!values_only && D.nent > 0) HIP_CHECK(hipMemcpy(D.col, hcol.data(), sizeof(int32_t) * (size_t)D.nent, hipMemcpyHostToDevice));
    if (D.nent > 0) HIP_CHECK(hipMemcpy(D.val, hval.data(), sizeof(double) * (size_t)D.nent, hipMemcpyHostToDevice));
    if (A.nrows > 0) HIP_CHECK(hipMemcpy(D.diag, hdiag.data(), sizeof(double) * (size_t)A.nrows, hipMemcpyHostToDevice));
    D.built = true;
  }
}

// dx = T \ r, T = L (dir 0) or U (dir 1): the plan's launches, in order, on the handle's stream
// xmode != 0 (the caller's fold rule holds): the wide launches also update x, 1: x += dx, 2: x = dx
void gmg_solver::gs_solve(Level &L, int dir, const double *r, double *dx, int xmode, double *x)
{
  REQUIRE(L.gs && L.gs->dir[dir].built, GMG_ERR_STATE, "Gauss-Seidel smoother: no tables for this direction (gmg_setup missing)");
  const GsDir &D = L.gs->dir[dir];
  const bool own_kernel = D.ordered && opt_int("GMG_GS_WIDE", 1) != 0;
  REQUIRE(xmode == 0 || (own_kernel && D.all_wide && x), GMG_ERR_STATE, "Gauss-Seidel smoother: the x update cannot fold into this plan");
  for (const GsDir::Launch &q : D.plan) {
    const int64_t rows = D.h_setptr[(size_t)q.s1] - D.h_setptr[(size_t)q.s0];
    if (q.wide && own_kernel) {
      const int64_t nsl = (int64_t)D.h_slice0[(size_t)q.s1] - D.h_slice0[(size_t)q.s0];
      constexpr int wpb = kGsWideThreads / 64;
      hipLaunchKernelGGL(gs_wide_kernel, dim3((unsigned)((nsl + wpb - 1) / wpb)), dim3(kGsWideThreads), 0, stream, D.h_setptr[(size_t)q.s0], rows,
                         (int64_t)D.h_slice0[(size_t)q.s0], nsl, D.soff, D.perm, D.col, D.val, D.diag, r, dx, xmode, x);
    } else if (q.wide)
      hipLaunchKernelGGL(gs_sets_kernel, dim3((unsigned)((rows + kGsWideThreads - 1) / kGsWideThreads)), dim3(kGsWideThreads), 0, stream, q.s0, q.s1,
                         D.setptr, D.slice0, D.soff, D.perm, D.col, D.val, D.diag, r, dx);
    else
      hipLaunchKernelGGL(gs_sets_kernel, dim3(1), dim3(kGsChainThreads), 0, stream, q.s0, q.s1, D.setptr, D.slice0, D.soff, D.perm, D.col, D.val,
                         D.diag, r, dx);
    HIP_CHECK(hipGetLastError());
  }
}

// solve!(x, ns::GaussSeidelNumericalSetup, r), :175-208; r (one of the level's buffers) is updated in place
void gmg_solver::gs_pass(int l, Smoother &S, double *x, double *r, bool x_zero)
{
  Level &L = lev[l];
  const int64_t n = L.n;
  bool xz = x_zero;
  for (int it = 0; it < S.niter; ++it)
    for (int dir = 0; dir < 2; ++dir) {
      if (dir == 0 ? S.gs_type == GMG_GS_BACKWARD : S.gs_type == GMG_GS_FORWARD) continue;
      REQUIRE(L.gs && L.gs->dir[dir].built, GMG_ERR_STATE, "Gauss-Seidel smoother: no tables for this direction (gmg_setup missing)");
      const GsDir &D = L.gs->dir[dir];
      // the x update folds into the solve's launches under one rule: w == 1 and every launch of the plan is a gs_wide_kernel launch
      const bool fold = S.omega == 1.0 && D.ordered && D.all_wide && opt_int("GMG_GS_WIDE", 1) != 0;
      // profiled level: HIP events around the solve and the update of every direction, weighted with their launches
      const bool prof = (l == prof_level) && prof_used + 2 <= prof_ev.size();
      if (prof) HIP_CHECK(hipEventRecord(prof_ev[prof_used], stream));
      // own | ghost level whose pack can fuse: the update launch also fills the send buffer of dx's exchange (gs_update_pack_kernel)
      const bool pack = !fold && can_fuse_pack(l) && L.bidx != nullptr && opt_int("GMG_GS_PACK_FUSED", 1) != 0;
      gs_solve(L, dir, r, L.dx, fold ? (xz ? 2 : 1) : 0, x);   // :187-188 / :196-197
      if (pack) {
        hipLaunchKernelGGL(gs_update_pack_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, S.omega, S.omega != 1.0 ? 1 : 0, xz ? 1 : 0, L.dx, x,
                           L.bidx, L.halo.d_pk_ptr, L.halo.d_pk_slot, L.halo.d_sendbuf);
        HIP_CHECK(hipGetLastError());
      } else if (!fold) {
        hipLaunchKernelGGL(gs_update_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, S.omega, S.omega != 1.0 ? 1 : 0, xz ? 1 : 0, L.dx, x);   // :189-190
        HIP_CHECK(hipGetLastError());
      }
      if (prof) {
        HIP_CHECK(hipEventRecord(prof_ev[prof_used + 1], stream));
        prof_w[prof_used / 2] = (int)D.plan.size() + (fold ? 0 : 1);
        prof_xm[prof_used / 2] = -1;
        prof_used += 2;
      }
      xz = false;
      apply_A_sub(l, L.dx, r, nullptr, pack);               // :191-192 (the distributed product: exchanges dx)
    }
}

extern "C" {

int gmg_set_smoother_gauss_seidel(gmg_handle_t h, int lev, int which, int niter, double omega, int type)
{
  return guarded(h, [&] {
    check_level(h, lev, true);
    REQUIRE(type == GMG_GS_SYMMETRIC || type == GMG_GS_FORWARD || type == GMG_GS_BACKWARD, GMG_ERR_INVALID,
            "The type must be :symmetric, :forward or :backward.");
    REQUIRE(niter > 0, GMG_ERR_INVALID, "The number of iterations must be a positive integer.");
    REQUIRE(omega > 0.0, GMG_ERR_INVALID, "The relaxation parameter must be a positive real number.");
    Smoother S;
    S.kind = SM_GAUSS_SEIDEL; S.niter = niter; S.omega = omega; S.gs_type = type;
    assign_smoother(h, lev, which, S);
  });
}

int gmg_get_gs_schedule(gmg_handle_t h, int lev, int dir, int64_t *nsets, int64_t *max_set_rows, int64_t *nlaunches, int64_t *nwide)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, true);
    REQUIRE(dir == 0 || dir == 1, GMG_ERR_INVALID, "dir must be 0 (forward) or 1 (backward)");
    const Level &L = h->lev[lev];
    REQUIRE(L.gs && L.gs->dir[dir].built, GMG_ERR_STATE, "no Gauss-Seidel smoother of this level uses that direction");
    const GsDir &D = L.gs->dir[dir];
    if (nsets) *nsets = D.nsets;
    if (max_set_rows) *max_set_rows = D.max_set_rows;
    if (nlaunches) *nlaunches = (int64_t)D.plan.size();
    if (nwide) *nwide = D.nwide;
  });
}

int gmg_set_gs_ordering(gmg_handle_t h, int lev, int kind, const int32_t *order, int64_t n)
{
  return guarded(h, [&] {
    check_level(h, lev, true);
    const std::string where = "Gauss-Seidel ordering of level " + std::to_string(lev) + ": ";
    REQUIRE(kind == GMG_GS_ORDER_NATURAL || kind == GMG_GS_ORDER_MULTICOLOR || kind == GMG_GS_ORDER_GIVEN, GMG_ERR_INVALID,
            where + "the kind must be GMG_GS_ORDER_NATURAL, GMG_GS_ORDER_MULTICOLOR or GMG_GS_ORDER_GIVEN");
    REQUIRE(kind == GMG_GS_ORDER_GIVEN || order == nullptr, GMG_ERR_INVALID, where + "an order may only be passed with GMG_GS_ORDER_GIVEN");
    Level &L = h->lev[lev];
    std::vector<int32_t> given;
    if (kind == GMG_GS_ORDER_GIVEN) {
      REQUIRE(n >= 0 && (order != nullptr || n == 0), GMG_ERR_INVALID, where + "null order");
      if (L.hasA) REQUIRE(n == L.hA.nrows, GMG_ERR_INVALID, where + "the order has " + std::to_string(n) + " entries, the level has " +
                          std::to_string(L.hA.nrows) + " rows (position " + std::to_string(std::min(n, L.hA.nrows)) + ")");
      const int64_t bad = gs_bad_position(order, n);
      REQUIRE(bad < 0, GMG_ERR_INVALID, where + "not a permutation: position " + std::to_string(bad) + " holds row " +
              std::to_string(bad >= 0 ? order[bad] : 0) + ", which is out of range or already visited");
      given.assign(order, order + n);
    }
    L.gs_order_kind = kind;
    L.gs_order = std::move(given);
    h->touch();
  });
}

int gmg_get_gs_ordering(gmg_handle_t h, int lev, int *kind, int64_t *ncolors, int32_t *order, int64_t cap)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, true);
    const Level &L = h->lev[lev];
    REQUIRE(L.gs != nullptr, GMG_ERR_STATE, "no smoother of this level is Gauss-Seidel");
    if (kind) *kind = L.gs->order_kind;
    if (ncolors) *ncolors = L.gs->ncolors;
    if (order) {
      REQUIRE(cap >= L.n, GMG_ERR_INVALID, "gmg_get_gs_ordering: room for " + std::to_string(cap) + " entries, the order of level " +
              std::to_string(lev) + " has " + std::to_string(L.n));
      for (int64_t k = 0; k < L.n; ++k) order[k] = L.gs->order.empty() ? (int32_t)k : L.gs->order[(size_t)k];
    }
  });
}

int gmg_gs_multicolor_order(int64_t nrows, const int64_t *ptr, const int32_t *col, int32_t *order, int32_t *color, int64_t *ncolors)
{
  return guarded(nullptr, [&] {
    REQUIRE(nrows >= 0 && ptr && (col || ptr[nrows] == 0), GMG_ERR_INVALID, "gmg_gs_multicolor_order: null pattern");
    const int64_t n = nrows;
    REQUIRE(ptr[0] == 0, GMG_ERR_INVALID, "gmg_gs_multicolor_order: ptr must start at 0");
    for (int64_t i = 0; i < n; ++i) REQUIRE(ptr[i] <= ptr[i + 1], GMG_ERR_INVALID, "gmg_gs_multicolor_order: ptr not monotone at row " + std::to_string(i));
    // the transposed pattern: row i's neighbours are its own stored columns and the rows that store column i
    std::vector<int64_t> tptr((size_t)n + 1, 0);
    for (int64_t k = 0; k < ptr[n]; ++k) {
      REQUIRE(col[k] >= 0 && col[k] < n, GMG_ERR_INVALID, "gmg_gs_multicolor_order: column out of range at entry " + std::to_string(k));
      tptr[(size_t)col[k] + 1]++;
    }
    for (int64_t i = 0; i < n; ++i) tptr[(size_t)i + 1] += tptr[(size_t)i];
    std::vector<int32_t> trow((size_t)ptr[n]);
    {
      std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
      for (int64_t i = 0; i < n; ++i)
        for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) trow[(size_t)fill[(size_t)col[k]]++] = (int32_t)i;
    }
    // greedy first-fit in natural order: only rows below i are coloured when i is visited
    std::vector<int32_t> c((size_t)n, -1);
    std::vector<int64_t> taken;                              // taken[q] == i: colour q is held by a neighbour of row i
    int64_t nc = 0;
    for (int64_t i = 0; i < n; ++i) {
      auto mark = [&](int32_t j) { if (j < i) taken[(size_t)c[(size_t)j]] = i; };
      for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) mark(col[k]);
      for (int64_t k = tptr[(size_t)i]; k < tptr[(size_t)i + 1]; ++k) mark(trow[(size_t)k]);
      int64_t q = 0;
      while (q < nc && taken[(size_t)q] == i) ++q;
      if (q == nc) { taken.push_back(-1); ++nc; }
      c[(size_t)i] = (int32_t)q;
    }
    if (ncolors) *ncolors = nc;
    if (color) std::copy(c.begin(), c.end(), color);
    if (order) {                                             // rows sorted stably by colour
      std::vector<int64_t> start((size_t)nc + 1, 0);
      for (int64_t i = 0; i < n; ++i) start[(size_t)c[(size_t)i] + 1]++;
      for (int64_t q = 0; q < nc; ++q) start[(size_t)q + 1] += start[(size_t)q];
      for (int64_t i = 0; i < n; ++i) order[start[(size_t)c[(size_t)i]]++] = (int32_t)i;
    }
  });
}

} // extern "C"
