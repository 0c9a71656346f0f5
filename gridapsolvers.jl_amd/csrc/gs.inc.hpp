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

namespace {

constexpr int kGsChainThreads = 1024;   // a set of at most this many rows is one pass of the chain workgroup
constexpr int kGsWideThreads = 256;

struct GsDir {
  bool built = false;
  int64_t nsets = 0, max_set_rows = 0, nslices = 0, nent = 0, nwide = 0;
  struct Launch { int32_t s0, s1; bool wide; };
  std::vector<Launch> plan;
  // host copy of the schedule: a value refresh refills val / diag through it
  std::vector<int32_t> h_perm, h_slice0;
  std::vector<int64_t> h_setptr, h_soff;
  // device
  int32_t *perm = nullptr, *slice0 = nullptr, *col = nullptr;
  int64_t *setptr = nullptr, *soff = nullptr;
  double *val = nullptr, *diag = nullptr;
};

struct GsLevel {
  GsDir dir[2];          // 0 forward (L), 1 backward (U)
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

// dx .= w .* dx (skipped at w == 1) ; x .= x .+ dx, or x = dx where x is known to be zero
__global__ void gs_update_kernel(int64_t n, double omega, int scale, int x_zero, double *__restrict__ dx, double *__restrict__ x)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {   // (grid_for caps the grid)
    double d = dx[i];
    if (scale) { d = __dmul_rn(omega, d); dx[i] = d; }
    x[i] = x_zero ? d : __dadd_rn(x[i], d);
  }
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
  REQUIRE(A0->nrows == A0->ncols && A0->nrows == L.n, GMG_ERR_INVALID, "Gauss-Seidel smoother: the level matrix must be square");
  const HostCSR &A = gs_sorted_rows(*A0, sorted);
  const std::vector<int64_t> dpos = gs_diag_positions(A);
  for (int64_t i = 0; i < A.nrows; ++i)                     // SingularException(col), :31-33
    REQUIRE(dpos[(size_t)i] >= 0 && A.val[(size_t)dpos[(size_t)i]] != 0.0, GMG_ERR_SINGULAR,
            "Gauss-Seidel smoother: missing or zero diagonal entry in row " + std::to_string(i) + " on level " + std::to_string(l));
  if (!values_only) L.gs = std::make_shared<GsLevel>();
  REQUIRE(L.gs != nullptr, GMG_ERR_STATE, "Gauss-Seidel smoother: value refresh without a schedule");
  for (int d = 0; d < 2; ++d) {
    GsDir &D = L.gs->dir[d];
    if (!use[d]) continue;
    if (!values_only) {
      gs_schedule(A, dpos, d == 0, D);
      D.perm = upload(D.h_perm); D.setptr = upload(D.h_setptr); D.slice0 = upload(D.h_slice0); D.soff = upload(D.h_soff);
      D.col = dalloc<int32_t>((size_t)D.nent); D.val = dalloc<double>((size_t)D.nent); D.diag = dalloc<double>((size_t)A.nrows);
    }
    REQUIRE(D.val != nullptr && (int64_t)D.h_perm.size() == A.nrows, GMG_ERR_STATE, "Gauss-Seidel smoother: value refresh without a schedule");
    std::vector<int32_t> hcol(values_only ? 0 : (size_t)D.nent);
    std::vector<double> hval((size_t)D.nent), hdiag((size_t)A.nrows);
    gs_fill(A, dpos, d == 0, D, values_only ? nullptr : hcol.data(), hval.data(), hdiag.data());
    if (!values_only && D.nent > 0) HIP_CHECK(hipMemcpy(D.col, hcol.data(), sizeof(int32_t) * (size_t)D.nent, hipMemcpyHostToDevice));
    if (D.nent > 0) HIP_CHECK(hipMemcpy(D.val, hval.data(), sizeof(double) * (size_t)D.nent, hipMemcpyHostToDevice));
    if (A.nrows > 0) HIP_CHECK(hipMemcpy(D.diag, hdiag.data(), sizeof(double) * (size_t)A.nrows, hipMemcpyHostToDevice));
    D.built = true;
  }
}

// dx = T \ r, T = L (dir 0) or U (dir 1): the plan's launches, in order, on the handle's stream
void gmg_solver::gs_solve(Level &L, int dir, const double *r, double *dx)
{
  REQUIRE(L.gs && L.gs->dir[dir].built, GMG_ERR_STATE, "Gauss-Seidel smoother: no tables for this direction (gmg_setup missing)");
  const GsDir &D = L.gs->dir[dir];
  for (const GsDir::Launch &q : D.plan) {
    const int64_t rows = D.h_setptr[(size_t)q.s1] - D.h_setptr[(size_t)q.s0];
    if (q.wide)
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
      gs_solve(L, dir, r, L.dx);                            // :187-188 / :196-197
      hipLaunchKernelGGL(gs_update_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, S.omega, S.omega != 1.0 ? 1 : 0, xz ? 1 : 0, L.dx, x);   // :189-190
      HIP_CHECK(hipGetLastError());
      xz = false;
      apply_A_sub(l, L.dx, r);                              // :191-192
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

} // extern "C"
