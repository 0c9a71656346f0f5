// aggregation.inc.hpp -- smoothed-aggregation prolongations P_l built from A_l, included after galerkin.inc.hpp.  The reference takes
// every prolongation from a nested mesh hierarchy (GridTransferOperators.jl) and leaves for PETSc GAMG where there is none; this is the
// other half of the algebraic hierarchy of hypre / AMGX / PETSc PCMG next to the Galerkin products: the caller marks a level with
// gmg_set_aggregation and the level below it with gmg_set_galerkin.
//
// SEMANTICS (fixed: the tests compare bits with tests/aggregation_reference.py).  A: n x n, rows ascending, a stored nonzero diagonal,
// a structurally symmetric pattern; explicit zeros are legal and never strong.
//   strength    m_i = max over stored k != i of |a_ik|; (i, j), j != i, a_ij != 0, is row-strong iff |a_ij| >= theta * m_i; {i, j} is an
//               edge iff (i, j) or (j, i) is row-strong; w_ij = max(|a_ij|, |a_ji|)
//   priorities  key_i = mix(i + 0x9E3779B97F4A7C15 (seed + 1)), mix = the splitmix64 finaliser, wrapping; nodes order by (key_i, i)
//   MIS-2       synchronous rounds until no node is undecided: v = priority of an undecided node, else none; t1 = max of v over the
//               closed neighbourhood, t2 = max of t1 over it; an undecided i with t2_i = its own priority becomes a root; f1 = a root
//               in the closed neighbourhood, f2 = an f1 in it; an undecided non-root with f2 becomes covered
//   aggregates  roots numbered in ascending row index; pass 1: a non-root with a root neighbour joins it; pass 2: the others join the
//               aggregate of the pass-1 neighbour with the largest w_ij, ties to the smallest j
//   P           smooth = 0: T, one 1.0 per row at column agg(i).  smooth = 1: (I - omega D^-1 A) T without a sparse product: the
//               pattern of row i is {agg(k) : (i, k) stored} ascending, P(i, J) = t - w_i s_J, t = [J == agg(i)], s_J = the sum over
//               stored k ascending with agg(k) = J of a_ik from 0.0, w_i = omega (1 / a_ii); every operation rounded separately
//   omega       the caller's, or (4/3) / rho, rho = max_i (sum_k |a_ik| in stored order from 0.0) / |a_ii| -- the infinity-norm bound of
//               D^-1 A: a maximum does not depend on the order of the reduction, so omega is the same bits on every run (a power
//               iteration is not); it under-smooths against the true lambda_max
// The near-null space is the constant vector.  Not built: vector-valued candidates (rigid-body modes), filtered matrices, partitioned
// handles.
//
// gmg_setup calls aggregation_prepare(l) from galerkin_prepare before the product of level l + 1 is formed: the rows of A_l (the
// caller's matrix or the Galerkin product just formed) go to the device as temporaries, the kernels of kernels.hpp (agg_*) run -- one
// host round trip per MIS round, for the integer count of undecided nodes -- P comes back and is installed exactly as
// gmg_set_prolongation installs a caller's matrix; the temporaries are freed (never part of gmg_device_bytes).  New VALUES of A_l
// (gmg_update_values + gmg_setup): aggregates and the pattern of P are kept, rho, omega and the values of P are formed again -- the
// strength of connection is NOT evaluated again.  A new structure (gmg_set_matrix) aggregates afresh.

namespace {

struct AggLevel {
  double theta = 0.25, omega_in = 0.0;
  int smooth = 1;
  uint64_t seed = 0;
  bool have_agg = false;      // agg holds the aggregates of the structure the level has now (also where the level was then refused)
  bool built = false;         // so does the pattern of P
  bool computed = false;      // P.val belongs to the current values
  std::vector<int32_t> agg;
  int64_t nagg = 0;
  HostCSR P;
  int rounds = 0;
  double omega = 0.0, rho = 0.0;
  int64_t strong_edges = 0;
  float ms[4] = {0.f, 0.f, 0.f, 0.f};   // strength, MIS, assignment, P of the last build (a value refresh: strength = rho pass, P)
};

inline dim3 agg_grid(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 1 << 20))); }
inline dim3 agg_grid_rows(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + kBlock - 1) / kBlock)); }

// out[0 .. n] = exclusive prefix sums of in[0 .. n-1]
void agg_exscan(hipStream_t stream, GalerkinScratch &S, int64_t n, const int32_t *in, int64_t *out)
{
  const int64_t nb = std::max<int64_t>(1, (n + kAggScanTile - 1) / kAggScanTile);
  int64_t *bsum = S.alloc<int64_t>((size_t)nb);
  hipLaunchKernelGGL(agg_scan_local_kernel, dim3((unsigned)nb), dim3(kBlock), 0, stream, n, in, out, bsum);
  hipLaunchKernelGGL(agg_scan_top_kernel, dim3(1), dim3(kBlock), 0, stream, nb, bsum, out + n);
  hipLaunchKernelGGL(agg_scan_add_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, out, (const int64_t *)bsum);
  HIP_CHECK(hipGetLastError());
}

// the whole build (fresh) or the values of P on kept aggregates and a kept pattern (!fresh)
void aggregation_build(hipStream_t stream, const HostCSR &A, AggLevel &G, bool fresh, const std::string &where)
{
  const int64_t n = A.nrows, nnz = A.nnz();
  GalerkinScratch S;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int q = 0; q < 5; ++q) if (e[q]) (void)hipEventDestroy(e[q]); } } guard{ev};
  for (auto &e : ev) HIP_CHECK(hipEventCreate(&e));
  int64_t *ptr = S.upload(A.ptr);
  int32_t *col = S.upload(A.col);
  double *val = S.upload(A.val);
  double *diag = S.alloc<double>((size_t)n), *rmax = fresh ? S.alloc<double>((size_t)n) : nullptr;
  // integer words the kernels post to: 0 rho bits, 1 first bad row, 2 first bad pair, 3 flagged entries, 4 undecided, 5 unassigned
  unsigned long long h_w[6] = {0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
  unsigned long long *d_w = S.alloc<unsigned long long>(6);
  HIP_CHECK(hipMemcpyAsync(d_w, h_w, sizeof(h_w), hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipEventRecord(ev[0], stream));
  hipLaunchKernelGGL(agg_rowstat_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)col,
                     (const double *)val, diag, rmax, d_w + 0, d_w + 1);
  HIP_CHECK(hipGetLastError());
  int32_t *ecol = nullptr;
  double *w = nullptr;
  if (fresh) {
    ecol = S.alloc<int32_t>((size_t)nnz);
    w = S.alloc<double>((size_t)nnz);
    hipLaunchKernelGGL(agg_strong_kernel, agg_grid(nnz), dim3(kBlock), 0, stream, n, nnz, (const int64_t *)ptr, (const int32_t *)col,
                       (const double *)val, (const double *)rmax, G.theta, ecol, w, d_w + 2, d_w + 3);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipMemcpyAsync(h_w, d_w, sizeof(h_w), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipEventRecord(ev[1], stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  REQUIRE(h_w[1] == ~0ull, GMG_ERR_SINGULAR, where + "row " + std::to_string(h_w[1]) + " has no stored nonzero diagonal entry");
  REQUIRE(h_w[2] == ~0ull, GMG_ERR_INVALID, where + "the stored pattern is not structurally symmetric: (" + std::to_string(h_w[2] >> 32) + ", " +
          std::to_string(h_w[2] & 0xffffffffull) + ") is stored, its transposed entry is not");
  double rho;
  std::memcpy(&rho, &h_w[0], sizeof(double));
  G.rho = rho;
  G.omega = G.omega_in > 0.0 ? G.omega_in : (4.0 / 3.0) / rho;
  int32_t *agg = nullptr;
  if (fresh) {
    G.strong_edges = (int64_t)(h_w[3] / 2);
    // ---- distance-2 independent set
    uint8_t *state = S.alloc<uint8_t>((size_t)n), *root = S.alloc<uint8_t>((size_t)n), *f1 = S.alloc<uint8_t>((size_t)n);
    uint64_t *tk = S.alloc<uint64_t>((size_t)n);
    int32_t *ti = S.alloc<int32_t>((size_t)n);
    HIP_CHECK(hipMemsetAsync(state, 0, (size_t)std::max<int64_t>(n, 1), stream));
    const uint64_t salt = 0x9E3779B97F4A7C15ull * (G.seed + 1ull);
    G.rounds = 0;
    for (unsigned long long left = (unsigned long long)n; left > 0;) {
      REQUIRE(G.rounds < 4096, GMG_ERR_STATE, where + "the independent set did not finish in 4096 rounds");
      HIP_CHECK(hipMemsetAsync(d_w + 4, 0, sizeof(unsigned long long), stream));
      hipLaunchKernelGGL(agg_mis_t1_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ecol,
                         (const uint8_t *)state, salt, tk, ti);
      hipLaunchKernelGGL(agg_mis_t2_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ecol,
                         (const uint8_t *)state, (const uint64_t *)tk, (const int32_t *)ti, root);
      hipLaunchKernelGGL(agg_mis_f1_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ecol,
                         (const uint8_t *)root, f1);
      hipLaunchKernelGGL(agg_mis_f2_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ecol,
                         (const uint8_t *)root, (const uint8_t *)f1, state, d_w + 4);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(&left, d_w + 4, sizeof(left), hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      ++G.rounds;
    }
    HIP_CHECK(hipEventRecord(ev[2], stream));
    // ---- aggregates
    int32_t *flag = S.alloc<int32_t>((size_t)n), *agg1 = S.alloc<int32_t>((size_t)n);
    int64_t *rootid = S.alloc<int64_t>((size_t)n + 1);
    agg = S.alloc<int32_t>((size_t)n);
    hipLaunchKernelGGL(agg_rootflag_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const uint8_t *)state, flag);
    agg_exscan(stream, S, n, flag, rootid);
    hipLaunchKernelGGL(agg_pass1_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ecol,
                       (const uint8_t *)state, (const int64_t *)rootid, agg1);
    hipLaunchKernelGGL(agg_pass2_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ecol,
                       (const double *)w, (const int32_t *)agg1, agg, d_w + 5);
    HIP_CHECK(hipGetLastError());
    G.agg.assign((size_t)n, 0);
    HIP_CHECK(hipMemcpyAsync(G.agg.data(), agg, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(&G.nagg, rootid + n, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(h_w, d_w, sizeof(h_w), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipEventRecord(ev[3], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    REQUIRE(h_w[5] == 0, GMG_ERR_STATE, where + "a covered node found no assigned neighbour");
    G.have_agg = true;                                        // (the aggregates can be read even where the level is refused below)
    G.P = HostCSR();
    REQUIRE(G.nagg > 0 && G.nagg < n, GMG_ERR_UNSUPPORTED, where + "the level does not coarsen: " + std::to_string(n) + " rows, " +
            std::to_string(G.nagg) + " aggregates");
  } else {
    agg = S.upload(G.agg);
    HIP_CHECK(hipEventRecord(ev[2], stream));
    HIP_CHECK(hipEventRecord(ev[3], stream));
  }
  // ---- P
  int64_t *pptr = nullptr;
  int32_t *pcol = nullptr;
  double *pval = nullptr;
  int64_t pnnz = n;
  if (!G.smooth) {
    pptr = S.alloc<int64_t>((size_t)n + 1); pcol = S.alloc<int32_t>((size_t)n); pval = S.alloc<double>((size_t)n);
    hipLaunchKernelGGL(agg_tentative_kernel, agg_grid_rows(n + 1), dim3(kBlock), 0, stream, n, (const int32_t *)agg, pptr, pcol, pval);
    HIP_CHECK(hipGetLastError());
  } else {
    int32_t *ac = S.alloc<int32_t>((size_t)nnz);
    hipLaunchKernelGGL(agg_entry_kernel, agg_grid(nnz), dim3(kBlock), 0, stream, nnz, (const int32_t *)col, (const int32_t *)agg, ac);
    if (fresh) {
      int32_t *cnt = S.alloc<int32_t>((size_t)n);
      pptr = S.alloc<int64_t>((size_t)n + 1);
      hipLaunchKernelGGL(agg_prow_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ac, cnt,
                         (const int64_t *)nullptr, (int32_t *)nullptr);
      agg_exscan(stream, S, n, cnt, pptr);
      HIP_CHECK(hipMemcpyAsync(&pnnz, pptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      pcol = S.alloc<int32_t>((size_t)pnnz);
      hipLaunchKernelGGL(agg_prow_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const int32_t *)ac,
                         (int32_t *)nullptr, (const int64_t *)pptr, pcol);
    } else {
      pnnz = G.P.nnz();
      pptr = S.upload(G.P.ptr);
      pcol = S.upload(G.P.col);
    }
    pval = S.alloc<double>((size_t)pnnz);
    hipLaunchKernelGGL(agg_pval_kernel, agg_grid_rows(n), dim3(kBlock), 0, stream, n, (const int64_t *)ptr, (const double *)val,
                       (const int32_t *)ac, (const int32_t *)agg, (const double *)diag, G.omega, (const int64_t *)pptr,
                       (const int32_t *)pcol, pval);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipEventRecord(ev[4], stream));
  if (fresh) {
    G.P.nrows = n; G.P.ncols = G.nagg;
    G.P.ptr.assign((size_t)n + 1, 0);
    G.P.col.assign((size_t)pnnz, 0);
    HIP_CHECK(hipMemcpyAsync(G.P.ptr.data(), pptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, stream));
    if (pnnz > 0) HIP_CHECK(hipMemcpyAsync(G.P.col.data(), pcol, sizeof(int32_t) * (size_t)pnnz, hipMemcpyDeviceToHost, stream));
  }
  G.P.val.assign((size_t)pnnz, 0.0);
  G.built = true;
  if (pnnz > 0) HIP_CHECK(hipMemcpyAsync(G.P.val.data(), pval, sizeof(double) * (size_t)pnnz, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  for (int q = 0; q < 4; ++q) HIP_CHECK(hipEventElapsedTime(&G.ms[q], ev[q], ev[q + 1]));
  G.computed = true;
}

} // namespace

void gmg_solver::aggregation_invalidate(int l)
{
  if (l < 0 || l >= nlev || !lev[l].agg) return;
  lev[l].agg->have_agg = lev[l].agg->built = lev[l].agg->computed = false;
}

// what gmg_setup refuses on a handle with aggregated levels, before anything is built
void gmg_solver::aggregation_check() const
{
  for (int l = 0; l < nlev - 1; ++l) {
    const Level &L = lev[l];
    if (!L.agg) continue;
    const std::string where = "aggregated prolongation of level " + std::to_string(l) + ": ";
    REQUIRE(comm.nranks == 1, GMG_ERR_UNSUPPORTED, where + "the handle has a communicator of more than one rank; aggregates do not cross ranks");
    REQUIRE(!L.halo.present, GMG_ERR_UNSUPPORTED, where + "the level is partitioned (gmg_set_partition)");
    REQUIRE(!L.has_pcorr, GMG_ERR_UNSUPPORTED, where + "the level has a patch-corrected prolongation (gmg_set_prolongation_patch_correction)");
    REQUIRE(!L.hasR && !L.sR, GMG_ERR_UNSUPPORTED, where + "the level has an explicit restriction (gmg_set_restriction); the restriction is P^T");
    REQUIRE(lev[l + 1].gal != nullptr, GMG_ERR_INVALID, where + "level " + std::to_string(l + 1) + " is not marked with gmg_set_galerkin; a matrix "
            "of the caller's cannot match the aggregates");
    if (l + 1 < nlev - 1) {
      const Level &Cl = lev[l + 1];
      const Smoother &post = Cl.post_shares_pre ? Cl.pre : Cl.post;
      REQUIRE(Cl.pre.kind != SM_PATCH && post.kind != SM_PATCH && !Cl.has_pcorr, GMG_ERR_UNSUPPORTED,
              "level " + std::to_string(l + 1) + " takes its size from the aggregation of level " + std::to_string(l) +
              ": a patch-based smoother or prolongation there is refused, its tables cannot match");
    }
  }
}

// P_l of an aggregated level that is out of date, from the rows of A_l; called by galerkin_prepare before the product of level l + 1
void gmg_solver::aggregation_prepare(int l)
{
  Level &L = lev[l];
  if (!L.agg) return;
  AggLevel &G = *L.agg;
  if (G.built && G.computed) return;
  const std::string where = "aggregated prolongation of level " + std::to_string(l) + ": ";
  REQUIRE(L.hasA, GMG_ERR_STATE, "gmg_set_matrix missing for level " + std::to_string(l));
  HIP_CHECK(hipSetDevice(device));
  HostCSR ta;
  const HostCSR &A = *(L.gal ? &L.gal->C : &galerkin_rows(L.hA, L.sA, ta, where, ("the matrix of level " + std::to_string(l)).c_str()));
  REQUIRE(A.nrows == A.ncols, GMG_ERR_INVALID, where + "the level matrix is not square");
  const bool fresh = !G.built;
  if (!fresh && !G.smooth) { G.computed = true; return; }    // T does not depend on the values
  aggregation_build(stream, A, G, fresh, where);
  if (!fresh && !L.sP && L.hasP && L.hP.nnz() == G.P.nnz()) {
    L.hP.val = G.P.val;                                      // same pattern, new values: the value refresh takes them (refresh_values)
    L.p_dirty = true;
    setup_done = false;
    return;
  }
  const int64_t nnz = G.P.nnz();
  L.sP.reset();
  bool eager = false;
  if (nnz < (int64_t)INT32_MAX) {
    std::vector<int32_t> p32(G.P.ptr.begin(), G.P.ptr.end());
    eager = try_eager_pattern(L.sP, 1, G.P.nrows, G.P.ncols, nnz, p32.data(), G.P.col.data(), G.P.val.data(), GMG_CSR, 0, 4);
  }
  if (eager) { L.hP = HostCSR(); L.hP.nrows = G.P.nrows; L.hP.ncols = G.P.ncols; }   // shape only, as gmg_set_prolongation leaves it
  else L.hP = G.P;
  L.hasP = true;
  L.p_dirty = false;
  if (fresh) galerkin_invalidate(l + 1);
  touch();
}

void gmg_solver::aggregation_values_changed(int l)
{
  if (l >= 0 && l < nlev && lev[l].agg) lev[l].agg->computed = false;
}

extern "C" {

int gmg_set_aggregation(gmg_handle_t h, int lev, double theta, int smooth, double omega, int64_t seed)
{
  return guarded(h, [&] {
    check_level(h, lev, true);
    REQUIRE(theta >= 0.0 && theta <= 1.0, GMG_ERR_INVALID, "gmg_set_aggregation: theta must lie in [0, 1]");
    REQUIRE(seed >= 0, GMG_ERR_INVALID, "gmg_set_aggregation: seed < 0");
    REQUIRE(std::isfinite(omega), GMG_ERR_INVALID, "gmg_set_aggregation: omega is not finite");
    Level &L = h->lev[lev];
    L.agg = std::make_shared<AggLevel>();
    L.agg->theta = theta; L.agg->smooth = smooth ? 1 : 0; L.agg->omega_in = omega > 0.0 ? omega : 0.0; L.agg->seed = (uint64_t)seed;
    L.sP.reset();
    L.hP = HostCSR();
    L.hasP = false;
    L.p_dirty = false;
    h->galerkin_invalidate(lev + 1);
    h->touch();
  });
}

static const AggLevel &aggregation_of(gmg_handle_t h, int lev)
{
  check_level(h, lev, true);
  const Level &L = h->lev[lev];
  REQUIRE(L.agg && L.agg->have_agg, GMG_ERR_STATE, "level " + std::to_string(lev) + " has no aggregates (gmg_set_aggregation, then gmg_setup)");
  return *L.agg;
}

int gmg_get_aggregates(gmg_handle_t h, int lev, int64_t *nagg, int32_t *agg, int64_t cap)
{
  return guarded(h, [&] {
    REQUIRE(h, GMG_ERR_INVALID, "null handle");
    const AggLevel &G = aggregation_of(h, lev);
    if (nagg) *nagg = G.nagg;
    if (!agg) return;                                        // size query
    REQUIRE(cap >= (int64_t)G.agg.size(), GMG_ERR_INVALID, "gmg_get_aggregates: cap is smaller than the number of rows");
    std::copy(G.agg.begin(), G.agg.end(), agg);
  });
}

int gmg_get_prolongation(gmg_handle_t h, int lev, int64_t *nrows, int64_t *ncols, int64_t *nnz, int64_t *ptr, int32_t *col, double *val,
                         int64_t ptr_cap, int64_t nnz_cap)
{
  return guarded(h, [&] {
    check_ready(h);
    const AggLevel &G = aggregation_of(h, lev);
    REQUIRE(G.built && G.computed, GMG_ERR_STATE, "level " + std::to_string(lev) + ": the aggregated prolongation is out of date (gmg_setup)");
    const HostCSR &M = G.P;
    if (nrows) *nrows = M.nrows;
    if (ncols) *ncols = M.ncols;
    if (nnz) *nnz = M.nnz();
    if (!ptr && !col && !val) return;                        // size query
    REQUIRE((!ptr || ptr_cap >= M.nrows + 1) && ((!col && !val) || nnz_cap >= M.nnz()), GMG_ERR_INVALID,
            "gmg_get_prolongation: an output array is smaller than the matrix");
    if (ptr) std::copy(M.ptr.begin(), M.ptr.end(), ptr);
    if (col) std::copy(M.col.begin(), M.col.end(), col);
    if (val) std::copy(M.val.begin(), M.val.end(), val);
  });
}

int gmg_get_aggregation_info(gmg_handle_t h, int lev, int *rounds, double *omega, double *rho, int64_t *strong_edges, double *ms)
{
  return guarded(h, [&] {
    REQUIRE(h, GMG_ERR_INVALID, "null handle");
    const AggLevel &G = aggregation_of(h, lev);
    if (rounds) *rounds = G.rounds;
    if (omega) *omega = G.omega;
    if (rho) *rho = G.rho;
    if (strong_edges) *strong_edges = G.strong_edges;
    if (ms) for (int q = 0; q < 4; ++q) ms[q] = (double)G.ms[q];
  });
}

int gmg_get_level_size(gmg_handle_t h, int lev, int64_t *n)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, false);
    REQUIRE(n, GMG_ERR_INVALID, "null n");
    *n = h->lev[lev].n;
  });
}

} // extern "C"
