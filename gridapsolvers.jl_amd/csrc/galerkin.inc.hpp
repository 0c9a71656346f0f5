// galerkin.inc.hpp -- Galerkin coarse matrices A_{l+1} = R_l (A_l P_l), included at the end of gmg_amd.hip.  The reference takes the
// matrix of every level from the caller (GMGLinearSolverFromMatrices, GMGLinearSolvers.jl:336-340); this is the algebraic alternative
// of hypre / AMGX / PETSc PCMG: the caller marks a level with gmg_set_galerkin and hands over the finest matrix and the transfers.
//
// SEMANTICS (fixed: the tests compare bits with tests/galerkin_reference.py)
//   T = A P        T(i, J) = sum over k ascending of A(i, k) * P(k, J)
//   A_c = R T    A_c(I, J) = sum over i ascending of R(I, i) * T(i, J)
// every sum from 0.0, every product and every sum rounded separately; only stored entries contribute; the patterns are the structural
// products pattern(A) pattern(P) and pattern(R) pattern(T), so explicit zeros of the inputs count and an entry whose terms cancel stays
// stored; columns ascend in every row.  R is the level's restriction if one was set, else P^T (the rule of gmg_solver::setup).  Inputs
// with unsorted rows are sorted in the temporary copies only.
//
// SYMBOLIC PHASE (host, once per structure, kept across value refreshes): galerkin_symbolic, row chunks in parallel, a stamp per
// column.  NUMERIC PHASE (device): two launches of galerkin_gather_kernel (kernels.hpp), one lane per stored output entry, no atomics.
//
// gmg_setup calls galerkin_prepare first.  For every Galerkin level that is out of date, finest first: the rows of A, P, R of the finer
// level (a matrix gmg_set_matrix turned into a row stream gives its rows back into a temporary; the level's own layout is not touched),
// upload, the two launches, the values into the level's host CSR, free -- and the level is then set exactly as gmg_set_matrix sets a
// caller's matrix (first time or new structure) or refreshed exactly as gmg_update_values refreshes one (new values of a finer level).

namespace {

struct GalerkinLevel {
  bool sym_ok = false;        // T and C hold the patterns of the operators the handle has now
  bool computed = false;      // C.val is R (A P) of the current values
  bool installed = false;     // the level has been set from C with this structure
  HostCSR T;                  // pattern of A P (no values kept)
  HostCSR C;                  // the level matrix
  double symbolic_ms = 0.0;   // host time of the last symbolic phase (0 when it was kept)
  float ap_ms = 0.f, rt_ms = 0.f;   // HIP-event times of the two launches of the last numeric phase
};

// pattern(C) = pattern(A) pattern(B): rows of A in any order, duplicates allowed; the columns of every row of C ascend
void galerkin_symbolic(int64_t nrows, const int64_t *aptr, const int32_t *acol, const int64_t *bptr, const int32_t *bcol, int64_t ncols_b,
                       std::vector<int64_t> &cptr, std::vector<int32_t> &ccol)
{
  cptr.assign((size_t)nrows + 1, 0);
  const int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>(64, nrows / 2048));
  const int64_t per = (nrows + nchunk - 1) / nchunk;
  std::vector<std::vector<int32_t>> part((size_t)nchunk);
  parallel_chunks(nchunk, [&](int64_t t) {
    std::vector<int32_t> stamp((size_t)ncols_b, -1);
    std::vector<int32_t> &out = part[(size_t)t];
    for (int64_t i = t * per; i < std::min(nrows, (t + 1) * per); ++i) {
      const size_t first = out.size();
      for (int64_t k = aptr[i]; k < aptr[i + 1]; ++k)
        for (int64_t q = bptr[acol[k]]; q < bptr[acol[k] + 1]; ++q)
          if (stamp[(size_t)bcol[q]] != (int32_t)i) { stamp[(size_t)bcol[q]] = (int32_t)i; out.push_back(bcol[q]); }
      std::sort(out.begin() + (std::ptrdiff_t)first, out.end());
      cptr[(size_t)i + 1] = (int64_t)(out.size() - first);
    }
  });
  for (int64_t i = 0; i < nrows; ++i) cptr[(size_t)i + 1] += cptr[(size_t)i];
  ccol.resize((size_t)cptr[(size_t)nrows]);
  parallel_chunks(nchunk, [&](int64_t t) {
    const int64_t r0 = std::min(nrows, t * per);
    std::copy(part[(size_t)t].begin(), part[(size_t)t].end(), ccol.begin() + (std::ptrdiff_t)cptr[(size_t)r0]);
  });
}

void galerkin_check_pattern(int64_t nrows, int64_t ncols, const int64_t *ptr, const int32_t *col, const char *what)
{
  REQUIRE(nrows >= 0 && ncols >= 0 && ncols < (int64_t)INT32_MAX && nrows < (int64_t)INT32_MAX, GMG_ERR_INVALID, std::string(what) + ": bad shape");
  REQUIRE(ptr && ptr[0] == 0, GMG_ERR_INVALID, std::string(what) + ": the row pointers start at 0");
  for (int64_t i = 0; i < nrows; ++i) REQUIRE(ptr[i] <= ptr[i + 1], GMG_ERR_INVALID, std::string(what) + ": row pointers not monotone");
  REQUIRE(ptr[nrows] == 0 || col, GMG_ERR_INVALID, std::string(what) + ": null column array");
  for (int64_t k = 0; k < ptr[nrows]; ++k) REQUIRE(col[k] >= 0 && col[k] < ncols, GMG_ERR_INVALID, std::string(what) + ": column index out of range");
}

// The rows of an operator of the handle with ascending columns: H itself where it holds sorted rows, else `tmp` (the rows a stream
// gives back, or a sorted copy).  A stream the caller made has no rows to take.
const HostCSR &galerkin_rows(const HostCSR &H, const std::shared_ptr<PatStream> &S, HostCSR &tmp, const std::string &where, const char *what)
{
  const HostCSR *src = &H;
  if (S) {
    REQUIRE(S->complete(), GMG_ERR_STATE, where + what + ": row stream incomplete");
    REQUIRE(S->eager, GMG_ERR_UNSUPPORTED, where + what + " was streamed with gmg_set_operator_rows: the product needs its rows, pass it whole");
    tmp = gmg_solver::expand_stream(*S);
    src = &tmp;
  }
  std::atomic<int> unsorted(0);
  parallel_for(src->nrows, [&](int64_t i) {
    for (int64_t k = src->ptr[(size_t)i] + 1; k < src->ptr[(size_t)i + 1]; ++k)
      if (src->col[(size_t)k - 1] >= src->col[(size_t)k]) { unsorted.store(1); return; }
  });
  if (!unsorted.load()) return *src;
  if (src != &tmp) tmp = H;
  std::atomic<int> dup(0);
  parallel_for(tmp.nrows, [&](int64_t i) {
    const int64_t k0 = tmp.ptr[(size_t)i], len = tmp.ptr[(size_t)i + 1] - k0;
    std::vector<std::pair<int32_t, double>> row((size_t)len);
    for (int64_t j = 0; j < len; ++j) row[(size_t)j] = {tmp.col[(size_t)(k0 + j)], tmp.val[(size_t)(k0 + j)]};
    std::sort(row.begin(), row.end(), [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &b) { return a.first < b.first; });
    for (int64_t j = 0; j < len; ++j) {
      tmp.col[(size_t)(k0 + j)] = row[(size_t)j].first;
      tmp.val[(size_t)(k0 + j)] = row[(size_t)j].second;
      if (j > 0 && row[(size_t)j].first == row[(size_t)j - 1].first) dup.store(1);
    }
  });
  REQUIRE(!dup.load(), GMG_ERR_INVALID, where + what + " stores a column twice in one row");
  return tmp;
}

// device temporaries of one product: freed when the scope is left, never part of gmg_device_bytes
struct GalerkinScratch {
  std::vector<void *> mem;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~GalerkinScratch()
  {
    for (void *p : mem) (void)hipFree(p);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
  template <typename T>
  T *alloc(size_t n)
  {
    void *p = nullptr;
    HIP_CHECK(hipMalloc(&p, sizeof(T) * std::max<size_t>(n, 1)));
    mem.push_back(p);
    return (T *)p;
  }
  template <typename T>
  T *upload(const std::vector<T> &v)
  {
    T *p = alloc<T>(v.size());
    if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return p;
  }
  template <typename PtrT>
  PtrT *upload_ptr(const std::vector<int64_t> &v)
  {
    std::vector<PtrT> w(v.begin(), v.end());
    return upload(w);
  }
};

template <typename PtrT>
void galerkin_numeric(hipStream_t stream, const HostCSR &R, const HostCSR &A, const HostCSR &P, GalerkinLevel &G)
{
  GalerkinScratch S;
  for (auto &e : S.ev) HIP_CHECK(hipEventCreate(&e));
  const int64_t nnz_t = G.T.nnz(), nnz_c = G.C.nnz();
  PtrT *aptr = S.upload_ptr<PtrT>(A.ptr), *pptr = S.upload_ptr<PtrT>(P.ptr), *rptr = S.upload_ptr<PtrT>(R.ptr);
  PtrT *tptr = S.upload_ptr<PtrT>(G.T.ptr), *cptr = S.upload_ptr<PtrT>(G.C.ptr);
  int32_t *acol = S.upload(A.col), *pcol = S.upload(P.col), *rcol = S.upload(R.col), *tcol = S.upload(G.T.col), *ccol = S.upload(G.C.col);
  double *aval = S.upload(A.val), *pval = S.upload(P.val), *rval = S.upload(R.val);
  double *tval = S.alloc<double>((size_t)nnz_t), *cval = S.alloc<double>((size_t)nnz_c);
  auto grid = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 1 << 20))); };
  HIP_CHECK(hipEventRecord(S.ev[0], stream));
  if (nnz_t > 0)
    hipLaunchKernelGGL((galerkin_gather_kernel<PtrT>), grid(nnz_t), dim3(kBlock), 0, stream, A.nrows, nnz_t, (const PtrT *)tptr, (const int32_t *)tcol,
                       (const PtrT *)aptr, (const int32_t *)acol, (const double *)aval, (const PtrT *)pptr, (const int32_t *)pcol, (const double *)pval, tval);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(S.ev[1], stream));
  if (nnz_c > 0)
    hipLaunchKernelGGL((galerkin_gather_kernel<PtrT>), grid(nnz_c), dim3(kBlock), 0, stream, R.nrows, nnz_c, (const PtrT *)cptr, (const int32_t *)ccol,
                       (const PtrT *)rptr, (const int32_t *)rcol, (const double *)rval, (const PtrT *)tptr, (const int32_t *)tcol, (const double *)tval, cval);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(S.ev[2], stream));
  G.C.val.assign((size_t)nnz_c, 0.0);
  if (nnz_c > 0) HIP_CHECK(hipMemcpyAsync(G.C.val.data(), cval, sizeof(double) * (size_t)nnz_c, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  HIP_CHECK(hipEventElapsedTime(&G.ap_ms, S.ev[0], S.ev[1]));
  HIP_CHECK(hipEventElapsedTime(&G.rt_ms, S.ev[1], S.ev[2]));
}

} // namespace

void gmg_solver::galerkin_invalidate(int l)
{
  if (l < 1 || l >= nlev || !lev[l].gal) return;
  lev[l].gal->sym_ok = lev[l].gal->computed = false;
}

// the level takes G.C as a level takes a caller's matrix: gmg_set_matrix (fresh: first time, or the structure changed) or gmg_update_values
void gmg_solver::galerkin_install(int l, bool fresh)
{
  Level &L = lev[l];
  GalerkinLevel &G = *L.gal;
  if (!fresh) {
    update_values_impl(this, l, G.C.val.data());
    return;
  }
  const int64_t n = G.C.nrows, nnz = G.C.nnz();
  L.sA.reset();
  L.clear_split();
  L.input_layout = GMG_CSR;
  L.csc_perm.clear(); L.csc_perm.shrink_to_fit();
  bool eager = false;
  if (l < nlev - 1 && nnz < (int64_t)INT32_MAX) {
    std::vector<int32_t> p32(G.C.ptr.begin(), G.C.ptr.end());
    eager = try_eager_pattern(L.sA, 0, n, n, nnz, p32.data(), G.C.col.data(), G.C.val.data(), GMG_CSR, 0, 4);
  }
  if (eager) { L.hA = HostCSR(); L.hA.nrows = n; L.hA.ncols = n; }     // shape only, as gmg_set_matrix leaves it
  else L.hA = G.C;
  L.hasA = true;
  galerkin_invalidate(l + 1);
  aggregation_invalidate(l);
  touch();
  G.installed = true;
}

void gmg_solver::galerkin_prepare()
{
  aggregation_check();
  for (int l = 1; l < nlev; ++l) {
    Level &L = lev[l];
    if (!L.gal) continue;
    aggregation_prepare(l - 1);                              // an aggregated finer level: its prolongation first (aggregation.inc.hpp)
    GalerkinLevel &G = *L.gal;
    const std::string where = "Galerkin matrix of level " + std::to_string(l) + ": ";
    REQUIRE(comm.nranks == 1, GMG_ERR_UNSUPPORTED, where + "the handle has a communicator of more than one rank; the local rows of R, A and P "
            "do not hold the off-rank terms of the product");
    if (G.sym_ok && G.computed && G.installed) continue;
    Level &F = lev[l - 1];
    REQUIRE(F.hasA, GMG_ERR_STATE, "gmg_set_matrix missing for level " + std::to_string(l - 1));
    REQUIRE(F.hasP || (F.sP && !F.sP->eager), GMG_ERR_STATE, where + "gmg_set_prolongation missing on level " + std::to_string(l - 1));
    HIP_CHECK(hipSetDevice(device));
    HostCSR ta, tp, tr;
    const std::string lf = " of level " + std::to_string(l - 1);
    const HostCSR &A = *(F.gal ? &F.gal->C : &galerkin_rows(F.hA, F.sA, ta, where, ("the matrix" + lf).c_str()));
    const HostCSR &P = galerkin_rows(F.hP, F.sP, tp, where, ("the prolongation" + lf).c_str());
    if (!F.hasR && !F.sR) tr = transpose(P);                 // R = P^T (GridTransferOperators.jl:536-547); its rows ascend as P's do
    const HostCSR &R = *((F.hasR || F.sR) ? &galerkin_rows(F.hR, F.sR, tr, where, ("the restriction" + lf).c_str()) : &tr);
    REQUIRE(A.nrows == A.ncols && P.nrows == A.ncols && R.ncols == A.nrows && R.nrows == P.ncols, GMG_ERR_INVALID,
            where + "the shapes of R, A and P of level " + std::to_string(l - 1) + " do not chain to a square matrix");
    const bool fresh = !G.sym_ok || !G.installed;
    G.symbolic_ms = 0.0;
    if (!G.sym_ok) {
      const auto t0 = std::chrono::steady_clock::now();
      G.T = HostCSR(); G.C = HostCSR();
      G.T.nrows = A.nrows; G.T.ncols = P.ncols;
      G.C.nrows = R.nrows; G.C.ncols = P.ncols;
      galerkin_symbolic(A.nrows, A.ptr.data(), A.col.data(), P.ptr.data(), P.col.data(), P.ncols, G.T.ptr, G.T.col);
      galerkin_symbolic(R.nrows, R.ptr.data(), R.col.data(), G.T.ptr.data(), G.T.col.data(), P.ncols, G.C.ptr, G.C.col);
      G.symbolic_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      G.sym_ok = true;
      G.installed = false;
    }
    const int64_t big = std::max({A.nnz(), P.nnz(), R.nnz(), G.T.nnz(), G.C.nnz()});
    if (big >= (int64_t)INT32_MAX || opt_int("GMG_FORCE_PTR64", 0) != 0) galerkin_numeric<int64_t>(stream, R, A, P, G);
    else galerkin_numeric<int32_t>(stream, R, A, P, G);
    G.computed = true;
    galerkin_install(l, fresh);
  }
}

extern "C" {

static void galerkin_values_changed(gmg_handle_t h, int lev)
{
  if (lev + 1 < h->nlev && h->lev[lev + 1].gal) h->lev[lev + 1].gal->computed = false;
  h->aggregation_values_changed(lev);
}

static void galerkin_refuse_update(gmg_handle_t h, int lev)
{
  REQUIRE(!h->lev[lev].gal, GMG_ERR_STATE, "level " + std::to_string(lev) + " is a Galerkin level (gmg_set_galerkin): its values follow those of "
          "the finer levels, update those");
}

int gmg_set_galerkin(gmg_handle_t h, int lev)
{
  return guarded(h, [&] {
    check_level(h, lev, false);
    REQUIRE(lev >= 1, GMG_ERR_INVALID, "gmg_set_galerkin: level 0 has no finer level to form the product from");
    Level &L = h->lev[lev];
    L.sA.reset();
    L.clear_split();
    L.hA = HostCSR();
    L.hasA = false;
    L.input_layout = GMG_CSR;
    L.csc_perm.clear(); L.csc_perm.shrink_to_fit();
    L.gal = std::make_shared<GalerkinLevel>();
    h->galerkin_invalidate(lev + 1);
    h->aggregation_invalidate(lev);
    h->touch();
  });
}

int gmg_get_galerkin_matrix(gmg_handle_t h, int lev, int64_t *nrows, int64_t *nnz, int64_t *ptr, int32_t *col, double *val, int64_t cap_nnz)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, false);
    const Level &L = h->lev[lev];
    REQUIRE(L.gal && L.gal->computed, GMG_ERR_STATE, "level " + std::to_string(lev) + " is not a Galerkin level (gmg_set_galerkin)");
    const HostCSR &M = L.gal->C;
    if (nrows) *nrows = M.nrows;
    if (nnz) *nnz = M.nnz();
    if (!ptr && !col && !val) return;                        // size query
    REQUIRE(cap_nnz >= M.nnz(), GMG_ERR_INVALID, "gmg_get_galerkin_matrix: cap_nnz is smaller than the number of stored entries");
    if (ptr) std::copy(M.ptr.begin(), M.ptr.end(), ptr);
    if (col) std::copy(M.col.begin(), M.col.end(), col);
    if (val) std::copy(M.val.begin(), M.val.end(), val);
  });
}

int gmg_get_galerkin_timing(gmg_handle_t h, int lev, double *symbolic_ms, double *ap_ms, double *rt_ms)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, false);
    const Level &L = h->lev[lev];
    REQUIRE(L.gal && L.gal->computed, GMG_ERR_STATE, "level " + std::to_string(lev) + " is not a Galerkin level (gmg_set_galerkin)");
    if (symbolic_ms) *symbolic_ms = L.gal->symbolic_ms;
    if (ap_ms) *ap_ms = (double)L.gal->ap_ms;
    if (rt_ms) *rt_ms = (double)L.gal->rt_ms;
  });
}

int gmg_galerkin_pattern(int64_t nc, int64_t nf, const int64_t *rptr, const int32_t *rcol, const int64_t *aptr, const int32_t *acol,
                         const int64_t *pptr, const int32_t *pcol, int64_t *tptr, int32_t *tcol, int64_t tcap, int64_t *tnnz,
                         int64_t *cptr, int32_t *ccol, int64_t ccap, int64_t *cnnz)
{
  return guarded(nullptr, [&] {
    galerkin_check_pattern(nc, nf, rptr, rcol, "gmg_galerkin_pattern: R");
    galerkin_check_pattern(nf, nf, aptr, acol, "gmg_galerkin_pattern: A");
    galerkin_check_pattern(nf, nc, pptr, pcol, "gmg_galerkin_pattern: P");
    std::vector<int64_t> tp, cp;
    std::vector<int32_t> tc, cc;
    galerkin_symbolic(nf, aptr, acol, pptr, pcol, nc, tp, tc);
    galerkin_symbolic(nc, rptr, rcol, tp.data(), tc.data(), nc, cp, cc);
    if (tnnz) *tnnz = (int64_t)tc.size();
    if (cnnz) *cnnz = (int64_t)cc.size();
    if (!tptr && !tcol && !cptr && !ccol) return;           // size query
    REQUIRE((!tcol || tcap >= (int64_t)tc.size()) && (!ccol || ccap >= (int64_t)cc.size()), GMG_ERR_INVALID,
            "gmg_galerkin_pattern: an output array is smaller than the pattern");
    if (tptr) std::copy(tp.begin(), tp.end(), tptr);
    if (tcol) std::copy(tc.begin(), tc.end(), tcol);
    if (cptr) std::copy(cp.begin(), cp.end(), cptr);
    if (ccol) std::copy(cc.begin(), cc.end(), ccol);
  });
}

} // extern "C"
