// pmult.inc.hpp -- MultiplicativePatchSmoother: coloured block Gauss-Seidel over the patches of a patch smoother slot (multiplicative
// Schwarz / Vanka), included at the end of gmg_amd.hip.  The reference has the additive patch solver only and names this form as a
// TODO (SchwarzLinearSolvers.jl:3,13 "Implement the multiplicative case").
//
// One pass on (x, r), niter sweeps in the directions of the type:
//   dx = 0 ; r0 = r
//   for every colour c (ascending forward, descending backward), for every patch p of colour c:
//     t_i = r0[rows_p[i]] - sum_k a(rows_p[i], k) dx[k]   the stored row, summed from 0.0, product and sum rounded separately
//     d_i = sum_j inv(A_pp)[i, j] t_j                     as patch_apply_kernel sums
//     dx[rows_p[i]] += omega d_i
//   x = x + dx ; r = r - A dx                             (apply_A_sub: the level's "r -= A dx")
// inv(A_pp): the blocks build_patch makes (S.pmult keeps it from building the operator M and the incidence lists).
//
// COLOURING (host, at gmg_setup): patches p and q conflict when they share a dof or a stored entry a_ij / a_ji has i in p and j in q
// (explicit zeros count).  The neighbours of p are found through a dof -> patch incidence: every dof the rows and columns of p's dofs
// touch is visited once (a stamp per dof) and hands over the patches it sits in; the patch x patch graph is never formed.  Greedy
// first-fit in patch order, or the caller's colours -- which are validated by the same walk, always: the launches are race-free
// because of that check and nothing else.
//
// KERNELS (kernels.hpp): patch_mult_kernel / patch_mult_big_kernel, one launch per non-empty colour and direction (two where a colour
// holds patches on both sides of 64 dofs), or patch_mult_pass_kernel, the whole pass as one launch of one workgroup on small levels
// (option pmult_one_launch).  Rows of A come from the level's CSR, which gmg_setup keeps for such a level (drop_csr_stream).

namespace {

constexpr int kPmultMaxNp = 4096;        // t_p of patch_mult_big_kernel / patch_mult_pass_kernel in LDS: 32 KB
constexpr int kPmultOneLaunchMax = 32;   // default of pmult_one_launch_max (patches of the level): measured, profiles/patch_mult_timing.md --
                                         // one launch wins at 25 patches (0.085 ms against 0.091 ms), loses at 81 (0.146 against 0.100)

struct PmultTables {
  int64_t npatch = 0, ncolors = 0;       // ncolors = 1 + the largest colour in use
  int color_kind = 0;
  std::vector<int32_t> color;            // colour of every patch
  // the non-empty patches grouped by colour (ascending colour; inside a colour the patches of at most 64 dofs first, each part in
  // patch order); group g = the g-th colour that holds a non-empty patch
  struct Group { int64_t first, nsmall, nbig; int32_t color; };
  std::vector<Group> groups;
  int max_big = 0;                       // largest patch of more than 64 dofs (0: none)
  int32_t *d_order = nullptr;
  int64_t *d_cptr = nullptr, *d_csmall = nullptr;
};

// colour the patches (given == nullptr: greedy first-fit in patch order) or validate `given`; on a conflict of a given colouring
// conflict[0] < conflict[1] are the two patches, else both are -1
void pmult_color(int64_t n, const int64_t *ptr, const int32_t *col, int64_t npatch, const int64_t *pptr, const int32_t *pdofs,
                 const int32_t *given, int32_t *color, int64_t *ncolors, int64_t conflict[2])
{
  conflict[0] = conflict[1] = -1;
  // the transposed pattern: the rows that store column j
  std::vector<int64_t> tptr((size_t)n + 1, 0);
  for (int64_t k = 0; k < ptr[n]; ++k) tptr[(size_t)col[k] + 1]++;
  for (int64_t i = 0; i < n; ++i) tptr[(size_t)i + 1] += tptr[(size_t)i];
  std::vector<int32_t> trow((size_t)ptr[n]);
  {
    std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) trow[(size_t)fill[(size_t)col[k]]++] = (int32_t)i;
  }
  // dof -> patches, ascending patch index
  const int64_t ne = pptr[npatch];
  std::vector<int64_t> iptr((size_t)n + 1, 0);
  for (int64_t q = 0; q < ne; ++q) iptr[(size_t)pdofs[q] + 1]++;
  for (int64_t i = 0; i < n; ++i) iptr[(size_t)i + 1] += iptr[(size_t)i];
  std::vector<int32_t> inc((size_t)ne);
  {
    std::vector<int64_t> fill(iptr.begin(), iptr.end() - 1);
    for (int64_t p = 0; p < npatch; ++p)
      for (int64_t q = pptr[p]; q < pptr[p + 1]; ++q) inc[(size_t)fill[(size_t)pdofs[q]]++] = (int32_t)p;
  }
  std::vector<int64_t> stamp((size_t)n, -1);                 // stamp[j] == p: dof j has handed its patches to p already
  std::vector<int64_t> taken;                                // taken[c] == p: colour c is held by a neighbour of p
  int64_t nc = 0;
  if (given)
    for (int64_t p = 0; p < npatch; ++p) { color[p] = given[p]; nc = std::max<int64_t>(nc, (int64_t)given[p] + 1); }
  for (int64_t p = 0; p < npatch; ++p) {
    auto touch = [&](int32_t j) {
      if (stamp[(size_t)j] == p) return;
      stamp[(size_t)j] = p;
      for (int64_t k = iptr[(size_t)j]; k < iptr[(size_t)j + 1]; ++k) {
        const int64_t q = inc[(size_t)k];
        if (q >= p) break;                                   // (ascending: only the patches below p matter to either walk)
        if (!given) taken[(size_t)color[q]] = p;
        else if (color[q] == color[p] && (conflict[0] < 0 || p < conflict[1] || (p == conflict[1] && q < conflict[0]))) { conflict[0] = q; conflict[1] = p; }
      }
    };
    for (int64_t t = pptr[p]; t < pptr[p + 1]; ++t) {
      const int32_t i = pdofs[t];
      touch(i);
      for (int64_t k = ptr[i]; k < ptr[i + 1]; ++k) touch(col[k]);
      for (int64_t k = tptr[(size_t)i]; k < tptr[(size_t)i + 1]; ++k) touch(trow[(size_t)k]);
    }
    if (given) { if (conflict[0] >= 0) return; continue; }
    int64_t c = 0;
    while (c < nc && taken[(size_t)c] == p) ++c;
    if (c == nc) { taken.push_back(-1); ++nc; }
    color[p] = (int32_t)c;
  }
  if (ncolors) *ncolors = npatch > 0 ? nc : 0;
}

void pmult_check_tables(const char *who, int64_t nrows, const int64_t *ptr, const int32_t *col, int64_t npatch, const int64_t *pptr,
                        const int32_t *pdofs)
{
  const std::string w(who);
  REQUIRE(nrows >= 0 && ptr && (col || ptr[nrows] == 0), GMG_ERR_INVALID, w + ": null pattern");
  REQUIRE(ptr[0] == 0, GMG_ERR_INVALID, w + ": ptr must start at 0");
  for (int64_t i = 0; i < nrows; ++i) REQUIRE(ptr[i] <= ptr[i + 1], GMG_ERR_INVALID, w + ": ptr not monotone at row " + std::to_string(i));
  for (int64_t k = 0; k < ptr[nrows]; ++k)
    REQUIRE(col[k] >= 0 && col[k] < nrows, GMG_ERR_INVALID, w + ": column out of range at entry " + std::to_string(k));
  REQUIRE(npatch >= 0 && pptr && (pdofs || pptr[npatch] == 0), GMG_ERR_INVALID, w + ": null patch table");
  REQUIRE(pptr[0] == 0, GMG_ERR_INVALID, w + ": patch_ptr must start at 0");
  for (int64_t p = 0; p < npatch; ++p) REQUIRE(pptr[p] <= pptr[p + 1], GMG_ERR_INVALID, w + ": patch_ptr not monotone at patch " + std::to_string(p));
  for (int64_t q = 0; q < pptr[npatch]; ++q)
    REQUIRE(pdofs[q] >= 0 && pdofs[q] < nrows, GMG_ERR_INVALID, w + ": patch dof out of range at entry " + std::to_string(q));
}

// the slots of a level as gmg_setup sees them (a post-smoother that shares the pre-smoother is the pre-smoother's slot)
const Smoother &pmult_post_slot(const Level &L) { return L.post_shares_pre ? L.pre : L.post; }

std::string pmult_tag(const Level &L)
{
  bool f = false, b = false;
  int64_t nc = -1;
  for (const Smoother *sp : {&L.pre, &L.post}) {
    if (!sp->pmult) continue;
    f = f || sp->pmult_type != GMG_PMULT_BACKWARD;
    b = b || sp->pmult_type != GMG_PMULT_FORWARD;
    if (nc < 0 && sp->pm) nc = sp->pm->ncolors;
  }
  return std::string(f && b ? "F+B" : f ? "F" : "B") + "/" + std::to_string(std::max<int64_t>(nc, 0));
}

} // namespace

// what a level with a multiplicative patch slot cannot be: checked before gmg_setup builds anything
void gmg_solver::pmult_check(int l) const
{
  const Level &L = lev[l];
  for (const Smoother *sp : {&L.pre, &pmult_post_slot(L)}) {
    if (!sp->pmult) continue;
    const std::string where = "multiplicative patch smoother on level " + std::to_string(l) + ": ";
    REQUIRE(comm.nranks <= 1, GMG_ERR_UNSUPPORTED, where + "a communicator of more than one rank is not supported (the colours of a "
            "partitioned level would have to be agreed across the ranks)");
    REQUIRE(!(L.sA && !L.sA->eager), GMG_ERR_UNSUPPORTED, where + "the level operator was streamed (gmg_set_operator_rows) and has no CSR "
            "the sweeps could read rows from: hand the matrix over whole (gmg_set_matrix)");
    REQUIRE(sp->kind == SM_PATCH && sp->tab, GMG_ERR_STATE, where + "the slot holds no patch tables");
    REQUIRE(sp->tab->pcol.empty(), GMG_ERR_UNSUPPORTED, where + "patch_cols != patch_rows is not supported (the sweep needs one dof set per patch)");
    for (size_t p = 0; p + 1 < sp->tab->pptr.size(); ++p)
      REQUIRE(sp->tab->pptr[p + 1] - sp->tab->pptr[p] <= kPmultMaxNp, GMG_ERR_UNSUPPORTED, where + "patch " + std::to_string(p) + " has " +
              std::to_string(sp->tab->pptr[p + 1] - sp->tab->pptr[p]) + " dofs, the workgroup kernel stages at most " + std::to_string(kPmultMaxNp) + " in LDS");
  }
}

// colouring (or its validation) and the patches grouped by colour; after build_patch of the slot
void gmg_solver::pmult_setup(int l, Smoother &S)
{
  Level &L = lev[l];
  const std::string where = "multiplicative patch smoother on level " + std::to_string(l) + ": ";
  REQUIRE(S.tab && S.built, GMG_ERR_STATE, where + "the patch blocks are not built");
  REQUIRE(!L.sA && L.hA.nrows == L.n && L.hA.ncols == L.n && (int64_t)L.hA.ptr.size() == L.n + 1, GMG_ERR_STATE, where + "the level has no CSR rows");
  REQUIRE(L.A.rowptr && L.A.col && L.A.val, GMG_ERR_STATE, where + "the level's CSR is not on the device");
  const Smoother::Tables &T = *S.tab;
  const int64_t npatch = (int64_t)T.pptr.size() - 1;
  S.pm = std::make_shared<PmultTables>();
  PmultTables &M = *S.pm;
  M.npatch = npatch;
  M.color_kind = S.pmult_color_kind;
  M.color.assign((size_t)npatch, 0);
  const int32_t *given = nullptr;
  if (S.pmult_color_kind == 1) {
    REQUIRE((int64_t)S.pmult_color_in.size() == npatch, GMG_ERR_INVALID, where + "the given colouring has " + std::to_string(S.pmult_color_in.size()) +
            " entries, the slot has " + std::to_string(npatch) + " patches");
    given = S.pmult_color_in.data();
  }
  pmult_check_tables("multiplicative patch smoother", L.n, L.hA.ptr.data(), L.hA.col.data(), npatch, T.pptr.data(), T.prow.data());
  int64_t conflict[2];
  pmult_color(L.n, L.hA.ptr.data(), L.hA.col.data(), npatch, T.pptr.data(), T.prow.data(), given, M.color.data(), &M.ncolors, conflict);
  REQUIRE(conflict[0] < 0, GMG_ERR_INVALID, where + "patches " + std::to_string(conflict[0]) + " and " + std::to_string(conflict[1]) + " have the same colour " +
          std::to_string(conflict[0] >= 0 ? M.color[(size_t)conflict[0]] : 0) + " but share a dof or are coupled by a stored entry of the level matrix");
  if (!given) {                                              // the greedy colouring goes through the same check as a given one
    std::vector<int32_t> again(M.color);
    int64_t nc2 = 0;
    pmult_color(L.n, L.hA.ptr.data(), L.hA.col.data(), npatch, T.pptr.data(), T.prow.data(), M.color.data(), again.data(), &nc2, conflict);
    REQUIRE(conflict[0] < 0, GMG_ERR_STATE, where + "the greedy colouring left patches " + std::to_string(conflict[0]) + " and " + std::to_string(conflict[1]) + " in conflict");
  }
  // group the non-empty patches: sort stably by (colour, more than 64 dofs)
  std::vector<int32_t> order;
  order.reserve((size_t)npatch);
  for (int64_t p = 0; p < npatch; ++p)
    if (T.pptr[p + 1] > T.pptr[p]) order.push_back((int32_t)p);
  auto big = [&](int32_t p) { return T.pptr[(size_t)p + 1] - T.pptr[(size_t)p] > 64; };
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return M.color[(size_t)a] != M.color[(size_t)b] ? M.color[(size_t)a] < M.color[(size_t)b] : (!big(a) && big(b));
  });
  std::vector<int64_t> cptr(1, 0), csmall;
  for (size_t k = 0; k < order.size();) {
    size_t e = k;
    int64_t ns = 0;
    while (e < order.size() && M.color[(size_t)order[e]] == M.color[(size_t)order[k]]) {
      if (!big(order[e])) ++ns;
      else M.max_big = std::max<int>(M.max_big, (int)(T.pptr[(size_t)order[e] + 1] - T.pptr[(size_t)order[e]]));
      ++e;
    }
    M.groups.push_back({(int64_t)k, ns, (int64_t)(e - k) - ns, M.color[(size_t)order[k]]});
    cptr.push_back((int64_t)e);
    csmall.push_back(ns);
    k = e;
  }
  csmall.push_back(0);
  M.d_order = upload(order);
  M.d_cptr = upload(cptr);
  M.d_csmall = upload(csmall);
}

void gmg_solver::pmult_pass(int l, Smoother &S, double *x, double *r, bool x_zero)
{
  Level &L = lev[l];
  const int64_t n = L.n;
  REQUIRE(S.pmult && S.pm && S.built && S.pm->d_order && L.A.rowptr && L.A.col && L.A.val, GMG_ERR_STATE,
          "multiplicative patch smoother: no tables on level " + std::to_string(l) + " (gmg_setup missing)");
  const PmultTables &M = *S.pm;
  PmultArgs a;
  a.order = M.d_order; a.pptr = S.d_pptr; a.pdofs = S.d_pdofs;
  a.boff = S.dedup ? nullptr : S.d_boff; a.binv = S.dedup ? nullptr : S.d_binv;
  a.ublock = S.dedup ? S.d_ublock : nullptr; a.uboff = S.dedup ? S.d_uboff : nullptr; a.ubinv = S.dedup ? S.d_ubinv : nullptr;
  a.rowptr = L.A.rowptr; a.col = L.A.col; a.val = L.A.val; a.r0 = r; a.omega = S.omega;
  const int ngroups = (int)M.groups.size();
  REQUIRE(ngroups == 0 || (S.dedup ? (a.ublock && a.uboff && a.ubinv) : (a.boff && a.binv)), GMG_ERR_STATE,
          "multiplicative patch smoother: no inverse blocks on level " + std::to_string(l));
  const int nsweeps = S.pmult_type == GMG_PMULT_SYMMETRIC ? 2 * S.niter : S.niter;
  const int dir0 = S.pmult_type == GMG_PMULT_BACKWARD ? 1 : 0, dir1 = S.pmult_type == GMG_PMULT_FORWARD ? 0 : 1;
  const int mode = opt_int("GMG_PMULT_ONE_LAUNCH", 1);
  const bool one = ngroups > 0 && (mode == 2 || (mode == 1 && M.npatch <= (int64_t)opt_int("GMG_PMULT_ONE_LAUNCH_MAX", kPmultOneLaunchMax)));
  const size_t big_lds = sizeof(double) * (size_t)M.max_big;
  // profiled level: HIP events around the sweeps and the x update of the pass, weighted with their launches
  const bool prof = (l == prof_level) && prof_used + 2 <= prof_ev.size();
  int launches = 0;
  if (one) {
    if (prof) HIP_CHECK(hipEventRecord(prof_ev[prof_used], stream));
    if (L.A.ptr64)
      hipLaunchKernelGGL((patch_mult_pass_kernel<int64_t>), dim3(1), dim3(kBlock), big_lds, stream, a, n, ngroups, M.d_cptr, M.d_csmall, nsweeps, dir0, dir1, L.dx);
    else
      hipLaunchKernelGGL((patch_mult_pass_kernel<int32_t>), dim3(1), dim3(kBlock), big_lds, stream, a, n, ngroups, M.d_cptr, M.d_csmall, nsweeps, dir0, dir1, L.dx);
    HIP_CHECK(hipGetLastError());
    launches = 1;
  } else {
    zero(L.dx, n);
    if (prof) HIP_CHECK(hipEventRecord(prof_ev[prof_used], stream));
    for (int s = 0; s < nsweeps; ++s) {
      const bool backward = ((s & 1) ? dir1 : dir0) != 0;
      for (int gi = 0; gi < ngroups; ++gi) {
        const PmultTables::Group &G = M.groups[(size_t)(backward ? ngroups - 1 - gi : gi)];
        if (G.nsmall > 0) {
          const dim3 grid((unsigned)((G.nsmall + kBlock / 64 - 1) / (kBlock / 64)));
          if (L.A.ptr64) hipLaunchKernelGGL((patch_mult_kernel<int64_t>), grid, dim3(kBlock), 0, stream, a, G.first, G.nsmall, L.dx);
          else hipLaunchKernelGGL((patch_mult_kernel<int32_t>), grid, dim3(kBlock), 0, stream, a, G.first, G.nsmall, L.dx);
          HIP_CHECK(hipGetLastError());
          ++launches;
        }
        if (G.nbig > 0) {
          if (L.A.ptr64) hipLaunchKernelGGL((patch_mult_big_kernel<int64_t>), dim3((unsigned)G.nbig), dim3(kBlock), big_lds, stream, a, G.first + G.nsmall, L.dx);
          else hipLaunchKernelGGL((patch_mult_big_kernel<int32_t>), dim3((unsigned)G.nbig), dim3(kBlock), big_lds, stream, a, G.first + G.nsmall, L.dx);
          HIP_CHECK(hipGetLastError());
          ++launches;
        }
      }
    }
  }
  hipLaunchKernelGGL(gs_update_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, 1.0, 0, x_zero ? 1 : 0, L.dx, x);   // x = x + dx
  HIP_CHECK(hipGetLastError());
  if (prof) {
    HIP_CHECK(hipEventRecord(prof_ev[prof_used + 1], stream));
    prof_w[prof_used / 2] = launches + 1;
    prof_xm[prof_used / 2] = -1;
    prof_used += 2;
  }
  apply_A_sub(l, L.dx, r);                                   // r = r - A dx
}

extern "C" {

int gmg_set_smoother_patch_multiplicative(gmg_handle_t h, int lev, int which, int niter, double omega, int type)
{
  return guarded(h, [&] {
    check_level(h, lev, true);
    REQUIRE(which == GMG_PRE || which == GMG_POST || which == GMG_PRE_AND_POST, GMG_ERR_INVALID, "bad `which`");
    REQUIRE(type == GMG_PMULT_SYMMETRIC || type == GMG_PMULT_FORWARD || type == GMG_PMULT_BACKWARD, GMG_ERR_INVALID,
            "The type must be :symmetric, :forward or :backward.");
    REQUIRE(niter > 0, GMG_ERR_INVALID, "The number of iterations must be a positive integer.");
    REQUIRE(omega > 0.0, GMG_ERR_INVALID, "The relaxation parameter must be a positive real number.");
    Level &L = h->lev[lev];
    const bool on_pre = which != GMG_POST, on_post = which != GMG_PRE;
    for (const Smoother *sp : {on_pre ? static_cast<const Smoother *>(&L.pre) : nullptr, on_post ? &pmult_post_slot(L) : nullptr}) {
      if (!sp) continue;
      REQUIRE(sp->assigned && sp->kind == SM_PATCH && sp->tab, GMG_ERR_STATE,
              "gmg_set_smoother_patch_multiplicative: the slot holds no patch smoother (gmg_set_smoother_patch[_matrices] first)");
      REQUIRE(!sp->cheb, GMG_ERR_UNSUPPORTED, "gmg_set_smoother_patch_multiplicative: the slot holds a Chebyshev smoother (Chebyshev over the "
              "multiplicative sweep is not supported)");
    }
    // a slot of its own for the side that is changed alone
    if (which != GMG_PRE_AND_POST && L.post_shares_pre) { L.post = L.pre; L.post_shares_pre = false; }
    for (Smoother *sp : {on_pre ? &L.pre : nullptr, (on_post && !L.post_shares_pre) ? &L.post : nullptr}) {
      if (!sp) continue;
      sp->pmult = true;
      sp->niter = niter; sp->omega = omega; sp->pmult_type = type;
      sp->pmult_color_kind = 0; sp->pmult_color_in.clear();
      sp->pm.reset();
    }
    L.clear_overlap_hints();
    h->touch();
  });
}

int gmg_set_patch_coloring(gmg_handle_t h, int lev, int which, int kind, const int32_t *color, int64_t npatch)
{
  return guarded(h, [&] {
    check_level(h, lev, true);
    const std::string where = "patch colouring of level " + std::to_string(lev) + ": ";
    REQUIRE(which == GMG_PRE || which == GMG_POST || which == GMG_PRE_AND_POST, GMG_ERR_INVALID, "bad `which`");
    REQUIRE(kind == 0 || kind == 1, GMG_ERR_INVALID, where + "the kind must be 0 (greedy) or 1 (given)");
    REQUIRE(kind == 1 || color == nullptr, GMG_ERR_INVALID, where + "a colour array may only be passed with kind 1 (given)");
    Level &L = h->lev[lev];
    const bool on_pre = which != GMG_POST, on_post = which != GMG_PRE;
    for (const Smoother *sp : {on_pre ? static_cast<const Smoother *>(&L.pre) : nullptr, on_post ? &pmult_post_slot(L) : nullptr}) {
      if (!sp) continue;
      REQUIRE(sp->assigned && sp->kind == SM_PATCH && sp->tab, GMG_ERR_STATE, where + "the slot holds no patch smoother");
      if (kind == 1) {
        const int64_t have = (int64_t)sp->tab->pptr.size() - 1;
        REQUIRE(npatch == have, GMG_ERR_INVALID, where + "the colouring has " + std::to_string(npatch) + " entries, the slot has " + std::to_string(have) + " patches");
        REQUIRE(color != nullptr || npatch == 0, GMG_ERR_INVALID, where + "null colour array");
        for (int64_t p = 0; p < npatch; ++p) REQUIRE(color[p] >= 0, GMG_ERR_INVALID, where + "patch " + std::to_string(p) + " has the negative colour " + std::to_string(color[p]));
      }
    }
    if (which != GMG_PRE_AND_POST && L.post_shares_pre) { L.post = L.pre; L.post_shares_pre = false; }
    for (Smoother *sp : {on_pre ? &L.pre : nullptr, (on_post && !L.post_shares_pre) ? &L.post : nullptr}) {
      if (!sp) continue;
      sp->pmult_color_kind = kind;
      if (kind == 1) sp->pmult_color_in.assign(color, color + npatch);
      else sp->pmult_color_in.clear();
    }
    h->touch();
  });
}

int gmg_get_patch_coloring(gmg_handle_t h, int lev, int which, int64_t *ncolors, int32_t *color, int64_t cap)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, true);
    REQUIRE(which == GMG_PRE || which == GMG_POST, GMG_ERR_INVALID, "which must be GMG_PRE or GMG_POST");
    const Smoother &S = which == GMG_PRE ? h->lev[lev].pre : h->lev[lev].post;
    REQUIRE(S.pmult && S.pm, GMG_ERR_STATE, "this slot has no multiplicative patch smoother");
    if (ncolors) *ncolors = S.pm->ncolors;
    if (color) {
      REQUIRE(cap >= S.pm->npatch, GMG_ERR_INVALID, "gmg_get_patch_coloring: room for " + std::to_string(cap) + " entries, the slot has " +
              std::to_string(S.pm->npatch) + " patches");
      std::copy(S.pm->color.begin(), S.pm->color.end(), color);
    }
  });
}

int gmg_patch_multicolor(int64_t nrows, const int64_t *ptr, const int32_t *col, int64_t npatch, const int64_t *patch_ptr,
                         const int32_t *patch_dofs, int32_t *color, int64_t *ncolors)
{
  return guarded(nullptr, [&] {
    pmult_check_tables("gmg_patch_multicolor", nrows, ptr, col, npatch, patch_ptr, patch_dofs);
    std::vector<int32_t> c((size_t)npatch, 0);
    int64_t nc = 0, conflict[2];
    pmult_color(nrows, ptr, col, npatch, patch_ptr, patch_dofs, nullptr, c.data(), &nc, conflict);
    if (ncolors) *ncolors = nc;
    if (color) std::copy(c.begin(), c.end(), color);
  });
}

} // extern "C"
