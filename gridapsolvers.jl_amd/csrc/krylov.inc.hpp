// ----------------------------------------------------------------------------
// Krylov drivers (included by gmg_amd.hip after gmg_solver), written against callbacks (KrylovOps) so that the single-matrix
// solvers (gmg_cg_solve, gmg_fgmres_solve, ...) and the block solvers (gmg_block_*) share them.  `S` supplies the stream, the
// reductions and the vector kernels.  The small dense part of (F)GMRES is ArnoldiLSQ (krylov_small.hpp).
//
// Scalar slots (S.d_scalars / S.h_scalars, kScalarSlots doubles), shared by every driver that runs on one engine:
//   0                         the reduction helpers: norm, dot, and the residual norm cg_core posts
//   1 .. j + 1                the Arnoldi column of FGMRES / GMRES (H[1..j+1, j]); afterwards 1 .. j carry y to gmres_combine_kernel.
//                             The REQUIRE on the basis size keeps j + 3 below the MINRES block's end
//   16 ..                     MINRES: delta, beta_p, then the two halves of the state block (16 + 8 .. 16 + 8 + 2 kMinresState).  It
//                             sits in the Arnoldi range: MINRES never runs inside FGMRES / GMRES on one engine, nor they inside it
//   kScalarSlots - 8 * depth  cg_core: gamma (ping-pong), delta, dot(p, w) of nesting depth 1 .. 4 (a CG-Jacobi block or the coarsest
//                             solver under an outer CG is one depth further)
// ----------------------------------------------------------------------------

KrylovOps gmg_solver::level0_ops(int use_precond)
{
  KrylovOps ops;
  const int k = kl();
  ops.resid = [this, k](double *x, const double *b, double *r) { apply_A_resid(k, x, b, r); };
  ops.apply = [this, k](double *x, double *y) { apply_A_set(k, x, y); };
  if (comm.nranks == 1) ops.apply_dot = [this](double *x, double *y, double *parts) { return spmv_set_dot(lev[0].A, x, y, parts); };
  if (use_precond) ops.precond = [this, use_precond](double *z, const double *r, double known) { krylov_precond(use_precond, z, r, known); };
  return ops;
}

// solve!(x,ns::CGNumericalSetup,b), Krylov/CGSolvers.jl:73-120
static double cg_core(gmg_solver &S, int64_t n, const double *db, double *dx, double *w, double *p, double *z, double *r,
               const KrylovOps &ops, bool flexible, ConvLog &log, bool traced)
{
  // Scalars stay on the device: gamma (ping-pong), delta and dot(p,w) live in d_scalars and the vector
  // kernels form beta / alpha from them, so an iteration has ONE host round trip (the residual norm that
  // the stopping rule needs) instead of three.
  // A CG can run inside another Krylov solve (CG-Jacobi diagonal block or coarsest solver under an outer CG): every nesting
  // level owns its four slots.
  REQUIRE(S.krylov_depth < 4, GMG_ERR_UNSUPPORTED, "Krylov solvers nested deeper than 4");
  struct Depth { int &d; Depth(int &x) : d(x) { ++d; } ~Depth() { --d; } } depth_guard(S.krylov_depth);
  const int sbase = kScalarSlots - 8 * S.krylov_depth;
  const int kG0 = sbase, kG1 = sbase + 1, kDelta = sbase + 2, kPW = sbase + 3;
  int g_old = kG0, g_new = kG1;
  // traced (gmg_cg_solve with gmg_cg_set_trace on; never a nested CG): the kernels that form alpha_k and beta_k also store them.  The
  // count restarts here, so a re-run by with_persist_retry leaves one consistent trace.
  double *const tr_a = traced ? S.d_trace : nullptr, *const tr_b = traced ? S.d_trace + S.trace_cap : nullptr;
  int it = 0;
  if (traced) S.trace_count = 0;
  ops.resid(dx, db, r);                                  // CGSolvers.jl:79  w = A x ; r = b - w
  // :80 fill!(p,0): folded into the first p = z + beta*p ; :81 fill!(z,0): only the flexible variant reads z before writing it
  if (flexible) S.zero(z, n);
  hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, S.stream, S.d_scalars + g_old, 1.0);   // :82 gamma = 1
  HIP_CHECK(hipGetLastError());
  double resn = S.norm(n, r);                            // :85
  bool done = log.init(resn);                            // :86
  bool first = true;
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(kRedBlocks, (n + kBlock - 1) / kBlock));
  // fused second stages (sum_partials_all): gamma = dot(z,r) is summed by xpby_dev_kernel, dot(p,w) by cg_update_kernel, and
  // ||r|| is reduced and posted to the host by one launch -- 4 launches per iteration instead of 8 for the scalars
  const bool fuse = S.fuse_reductions();
  const bool split = fuse && S.opt_int("GMG_CG_SPLIT", 0) != 0;
  const unsigned xgrid = fuse ? (unsigned)nb : (unsigned)gmg_solver::grid_for(n);
  while (!done) {
    int ngp = 0;                                         // gamma still in partials?
    if (!ops.precond) {                                  // :90-92
      S.copy(z, r, n);
      if (fuse) ngp = S.dot_partials(n, r, r, S.d_partials); else S.dot_async(n, r, r, g_new, false);
    } else if (!flexible) {                              // :93-95
      ops.precond(z, r, resn);
      if (fuse) ngp = S.dot_partials(n, z, r, S.d_partials); else S.dot_async(n, z, r, g_new, false);
    } else {                                             // :96-99
      S.dot_async(n, z, r, kDelta, false);
      ops.precond(z, r, resn);
      if (fuse) ngp = S.dot_partials(n, z, r, S.d_partials); else S.dot_async(n, z, r, g_new, false);
    }
    hipLaunchKernelGGL(xpby_dev_kernel, dim3(xgrid), dim3(kBlock), 0, S.stream, n, z, S.d_scalars + g_new,
                       S.d_scalars + g_old, (ops.precond && flexible) ? S.d_scalars + kDelta : nullptr, p, first ? 1 : 0,
                       ngp ? S.d_partials : nullptr, ngp, tr_b ? tr_b + it : nullptr); // :101
    HIP_CHECK(hipGetLastError());
    int npw = 0;
    if (fuse && ops.apply_dot) npw = ops.apply_dot(p, w, S.d_partials);   // :104-105 in one kernel (> 0), or :104 alone (-1)
    if (npw <= 0) {
      if (npw == 0) ops.apply(p, w);                     // :104
      if (fuse) npw = S.dot_partials(n, p, w, S.d_partials); else { S.dot_async(n, p, w, kPW, false); npw = 0; }   // :105
    }
    double *nparts = fuse ? S.d_partials2 : S.d_partials;
    if (split) {
      // (option cg_split, default 0: measured equal to the single kernel, profiles/xnext_ab_128.md)
      // r -= alpha w and ||r|| first, x += alpha p behind the launch that posts the norm: it runs while the host decides
      hipLaunchKernelGGL(cg_update_r_kernel, dim3(nb), dim3(kBlock), 0, S.stream, n, S.d_scalars + g_new, S.d_scalars + kPW, w, r,
                         nparts, npw ? S.d_partials : nullptr, npw, tr_a ? tr_a + it : nullptr); // :109
      HIP_CHECK(hipGetLastError());
      S.finish_reduction(nb, 0, true, nparts, true);
      hipLaunchKernelGGL(cg_update_x_kernel, dim3(nb), dim3(kBlock), 0, S.stream, n, S.d_scalars + g_new, S.d_scalars + kPW, p, dx);   // :108
      HIP_CHECK(hipGetLastError());
    } else if (S.vr_split(n)) {
      // (gmg_comm_set_loopback_rows: the update and its partial ||r||^2 per virtual rank, as the W ranks launch them)
      double *sums = S.vr_sums();
      for (int q = 0; q < S.vr_count(); ++q) {
        const int64_t o = S.vr_off[(size_t)q], nq = S.vr_off[(size_t)q + 1] - o;
        const int nbq = (int)std::max<int64_t>(1, std::min<int64_t>(kRedBlocks, (nq + kBlock - 1) / kBlock));
        hipLaunchKernelGGL(cg_update_kernel, dim3(nbq), dim3(kBlock), 0, S.stream, nq, S.d_scalars + g_new, S.d_scalars + kPW, p + o, w + o,
                           dx + o, r + o, nparts, (const double *)nullptr, 0, tr_a ? tr_a + it : nullptr);   // (every launch stores the same alpha)
        hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kBlock), 0, S.stream, nbq, nparts, sums + q, 0);
        HIP_CHECK(hipGetLastError());
      }
      S.vr_finish(0, true);
    } else {
    hipLaunchKernelGGL(cg_update_kernel, dim3(nb), dim3(kBlock), 0, S.stream, n, S.d_scalars + g_new, S.d_scalars + kPW, p, w, dx, r,
                       nparts, npw ? S.d_partials : nullptr, npw, tr_a ? tr_a + it : nullptr); // :108-109
    HIP_CHECK(hipGetLastError());
    S.finish_reduction(nb, 0, true, nparts, true);
    }
    resn = S.fetch_scalar(0);                            // :111
    done = log.update(resn);                             // :112
    std::swap(g_old, g_new);
    first = false;
    ++it;
    if (traced) S.trace_count = it;
  }
  // the posted norm no longer implies that x is complete: the last x += alpha p was issued behind it.  The outermost solve hands x
  // to its caller (who may read it from another stream); a nested one is consumed in stream order.
  if (split && S.krylov_depth == 1) HIP_CHECK(hipStreamSynchronize(S.stream));
  return resn;
}

// Column j of the Arnoldi relation (FGMRESSolvers.jl:160-165, GMRESSolvers.jl:162-167): modified Gram-Schmidt of V[j] against
// V[0..j-1], the normalisation of V[j], and H[1..j+1, j] fetched into lsq.
// fuse: one dot_partial_kernel launch, j gmres_mgs_kernel launches and gmres_normalize_kernel, which posts the column to the host
// mailbox (post) -- the fused kernels take dot_partial_kernel's order for 16-byte aligned operands (the basis is dvec's, aligned by
// hipMalloc).  Otherwise dot_async (all-reduced), axmy_dev_kernel, div_dev_kernel and a copy of the scalar slots.  Both perform the
// same floating-point operations in the same order.
static void arnoldi_column(gmg_solver &S, int64_t n, const std::vector<double *> &V, int j, bool fuse, bool post, ArnoldiLSQ &lsq)
{
  const int grid = gmg_solver::grid_for(n);
  double *Vn = V[j];
  bool al = fuse;
  for (int i = 0; al && i <= j; ++i) al = gmg_solver::aligned16(V[i]);
  const double *col = S.h_scalars + 1;
  if (al) {
    double *pin = S.d_partials, *pout = S.d_partials2;
    int np = S.dot_partials(n, Vn, V[0], pin);             // first stage of H[1,j]
    const int nbd = gmg_solver::dot_grid(n);
    for (int i = 1; i <= j; ++i) {                         // the last launch leaves the partials of norm(V[j+1])^2
      hipLaunchKernelGGL(gmres_mgs_kernel, dim3(nbd), dim3(kBlock), 0, S.stream, n, Vn, V[i - 1],
                         i < j ? (const double *)V[i] : (const double *)nullptr, i < j ? 0 : 1, pin, np, S.d_scalars + i, pout);
      HIP_CHECK(hipGetLastError());
      std::swap(pin, pout);
      np = nbd;
    }
    unsigned long long want = 0;
    if (post) { S.need_mail_col(); want = ++S.mail_seq; }
    hipLaunchKernelGGL(gmres_normalize_kernel, dim3(grid), dim3(kBlock), 0, S.stream, n, Vn, pin, np, S.d_scalars + 1, j + 1,
                       S.d_mail_col, post ? &S.d_mail->value : nullptr, post ? &S.d_mail->seq : nullptr, want);
    HIP_CHECK(hipGetLastError());
    if (post) {
      S.posted = want;
      (void)S.fetch_scalar(j + 1);                         // waits for the number: the column is in the mailbox
      col = S.h_mail_col;
    }
  } else {
    for (int i = 1; i <= j; ++i) {                         // modified Gram-Schmidt
      S.dot_async(n, Vn, V[i - 1], i, false);
      hipLaunchKernelGGL(axmy_dev_kernel, dim3(grid), dim3(256), 0, S.stream, n, S.d_scalars + i, V[i - 1], Vn);
      HIP_CHECK(hipGetLastError());
    }
    S.dot_async(n, Vn, Vn, j + 1, true);
    hipLaunchKernelGGL(div_dev_kernel, dim3(grid), dim3(256), 0, S.stream, n, S.d_scalars + (j + 1), Vn);
    HIP_CHECK(hipGetLastError());
  }
  if (!(al && post)) {
    HIP_CHECK(hipMemcpyAsync(S.h_scalars + 1, S.d_scalars + 1, sizeof(double) * (size_t)(j + 1), hipMemcpyDeviceToHost, S.stream));
    HIP_CHECK(hipStreamSynchronize(S.stream));
  }
  for (int i = 1; i <= j + 1; ++i) lsq.H(i, j) = col[i - 1];
}

// y = y0 + sum_{i < j} g[i] vecs[i] (y0 = y, or nullptr for zero): the solution update of FGMRESSolvers.jl:191-193 and
// GMRESSolvers.jl:193-201.  fuse: one gmres_combine_kernel over `tab`, the device table of the pointers in vecs (y may be a sub-vector
// of a block vector, 8-byte aligned only: the kernel's scalar form then); otherwise j axpy_kernel launches.
static void krylov_combine(gmg_solver &S, int64_t n, double *y, const double *y0, const std::vector<double *> &vecs,
                           const double *const *tab, const double *g, int j, bool fuse)
{
  const int grid = gmg_solver::grid_for(n);
  if (fuse && j > 0) {
    bool vec = gmg_solver::aligned16(y);
    for (int i = 0; i < j; ++i) vec = vec && gmg_solver::aligned16(vecs[i]);
    for (int i = 1; i <= j; ++i) S.h_scalars[i] = g[i - 1];
    HIP_CHECK(hipMemcpyAsync(S.d_scalars + 1, S.h_scalars + 1, sizeof(double) * (size_t)j, hipMemcpyHostToDevice, S.stream));
    hipLaunchKernelGGL(gmres_combine_kernel, dim3(grid), dim3(kBlock), 0, S.stream, n, y, y0, tab, S.d_scalars + 1, j, vec ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (!y0) S.zero(y, n);
  for (int i = 1; i <= j; ++i) {
    hipLaunchKernelGGL(axpy_kernel, dim3(grid), dim3(256), 0, S.stream, n, g[i - 1], vecs[i - 1], y);
    HIP_CHECK(hipGetLastError());
  }
}

// solve!(x,ns::FGMRESNumericalSetup,b), Krylov/FGMRESSolvers.jl:130-199.  V/Z are the caller's basis
// caches (:58-70); they grow by m_add when the basis outgrows them (:151-154), and H, g, c, s with them (expand_krylov_caches!,
// :77-94; with restart=true j never exceeds m0).  nv = allocation length of a basis vector (n plus ghost space in distributed runs).
// Fused path (arnoldi_column, krylov_combine over the table of the Z pointers): option fgmres_fused, -1 = in solves nested in a
// block preconditioner (`nested`) only, 0 = never, 1 = always; one rank or rank-local reductions.
static double fgmres_core(gmg_solver &S, int64_t n, int64_t nv, const double *db, double *dx, std::vector<double *> &V,
                   std::vector<double *> &Z, const KrylovOps &ops, int m0, bool restart, int m_add, ConvLog &log, bool nested = false)
{
  int m = std::max<int>(m0, (int)Z.size());
  while ((int)V.size() < m + 1) V.push_back(S.dvec(nv));
  while ((int)Z.size() < m) Z.push_back(S.dvec(nv));
  m = (int)Z.size();
  ArnoldiLSQ lsq(m + 1);
  const int grid = gmg_solver::grid_for(n);
  const int fopt = S.opt_int("GMG_FGMRES_FUSED", -1);
  const bool fuse = (fopt > 0 || (fopt < 0 && nested)) && S.fuse_reductions();
  const bool post = fuse && S.opt_int("GMG_HOST_POLL", 1) != 0;

  // krylov_residual!(V[1],x,A,b,Pl,zl): KrylovUtils.jl:46-54 ; FGMRESSolvers.jl:136-140
  auto residual = [&](double *out) {
    if (ops.precond_left) { ops.resid(dx, db, ops.zl); ops.precond_left(out, ops.zl); }
    else ops.resid(dx, db, out);
  };
  residual(V[0]);
  double beta = S.norm(n, V[0]);                         // :141
  bool done = log.init(beta);                            // :142
  while (!done) {
    int j = 1;                                           // :145
    hipLaunchKernelGGL(div_kernel, dim3(grid), dim3(256), 0, S.stream, n, beta, V[0]); // :146
    HIP_CHECK(hipGetLastError());
    lsq.reset(beta);                                     // :147-148
    while (!done && !(restart && j > m0)) {              // :149
      if (j > m) {                                       // :151-154
        for (int q = 0; q < m_add; ++q) { V.push_back(S.dvec(nv)); Z.push_back(S.dvec(nv)); }
        m += m_add;
      }
      lsq.reserve(m + 1);
      REQUIRE(j + 3 < kScalarSlots - 40, GMG_ERR_UNSUPPORTED, "Krylov basis larger than the scalar buffer (use restart=true)");
      double *Vn = V[j], *Zj = Z[j - 1];
      // krylov_mul!(V[j+1],A,V[j],Pr,nothing,Z[j],zl): KrylovUtils.jl:22-25
      if (ops.precond) ops.precond(Zj, V[j - 1], -1.0);
      else S.copy(Zj, V[j - 1], n);
      if (ops.precond_left) { ops.apply(Zj, ops.zl); ops.precond_left(Vn, ops.zl); }   // krylov_mul! with Pl, KrylovUtils.jl:14-18
      else ops.apply(Zj, Vn);                            // :159
      arnoldi_column(S, n, V, j, fuse, post, lsq);       // :160-165
      beta = lsq.close_column(j);                        // :168-179
      j += 1;                                            // :180
      done = log.update(beta);                           // :181
    }
    j = j - 1;                                           // :183
    lsq.solve(j);                                        // :186-188
    krylov_combine(S, n, dx, dx, Z, fuse && j > 0 ? S.fgmres_table(Z, j) : nullptr, lsq.g.data(), j, fuse);   // :191-193
    residual(V[0]);                                      // :194
  }
  return beta;
}

// solve!(x,ns::GMRESNumericalSetup,b), Krylov/GMRESSolvers.jl:132-210.  ops.precond = Pr, ops.precond_left = Pl (either may be
// empty: the four krylov_mul! methods and the two krylov_residual! methods of KrylovUtils.jl:17-54).  The caches of :57-69 are the
// handle's (S.gm_V, S.gm_zl, S.gm_zr; nv = allocation length of a vector); V, H, g, c and s grow by m_add when the basis outgrows
// them (:76-92).  Fused path (arnoldi_column, krylov_combine over the table of the basis): option gmres_fused (default 1), one rank
// or rank-local reductions.
static double gmres_core(gmg_solver &S, int64_t n, int64_t nv, const double *db, double *dx, const KrylovOps &ops, int m0,
                         bool restart, int m_add, ConvLog &log)
{
  const bool has_pr = (bool)ops.precond, has_pl = (bool)ops.precond_left;
  S.gmres_work(nv, m0, has_pr);                          // :57-62 (an earlier solve may have left a larger basis)
  std::vector<double *> &V = S.gm_V;
  double *zl = S.gm_zl, *zr = S.gm_zr;
  int m = (int)V.size() - 1;                             // krylov_cache_length, :71-74
  ArnoldiLSQ lsq(m + 1);                                 // :64-67
  const int grid = gmg_solver::grid_for(n);
  const bool fuse = S.opt_int("GMG_GMRES_FUSED", 1) != 0 && S.fuse_reductions();
  const bool post = fuse && S.opt_int("GMG_HOST_POLL", 1) != 0;

  // krylov_residual!(V[1],x,A,b,Pl,zl): KrylovUtils.jl:46-54
  auto residual = [&](double *out) {
    if (has_pl) { ops.resid(dx, db, zl); ops.precond_left(out, zl); }
    else ops.resid(dx, db, out);
  };
  // krylov_mul!(y,A,x,Pr,Pl,zr,zl): KrylovUtils.jl:17-32
  auto kmul = [&](double *y, double *x) {
    if (has_pr) ops.precond(zr, x, -1.0);                // solve!(wr,Pr,x)
    double *ax = has_pr ? zr : x;
    if (has_pl) { ops.apply(ax, zl); ops.precond_left(y, zl); }   // mul!(wl,A,.) ; solve!(y,Pl,wl)
    else ops.apply(ax, y);                               // mul!(y,A,.)
  };
  residual(V[0]);                                        // :143
  double beta = S.norm(n, V[0]);                         // :144
  bool done = log.init(beta);                            // :145
  while (!done) {                                        // :146
    int j = 1;                                           // :148
    hipLaunchKernelGGL(div_kernel, dim3(grid), dim3(256), 0, S.stream, n, beta, V[0]); // :149
    HIP_CHECK(hipGetLastError());
    lsq.reset(beta);                                     // :150-151
    while (!done && !(restart && j > m0)) {              // :152 ; restart(solver,j), :31-37
      if (j > m) {                                       // :154-157
        for (int q = 0; q < m_add; ++q) V.push_back(S.dvec(nv));
        m += m_add;
      }
      lsq.reserve(m + 1);                                // expand_krylov_caches!, :86-89
      REQUIRE(j + 3 < kScalarSlots - 40, GMG_ERR_UNSUPPORTED, "Krylov basis larger than the scalar buffer (use restart=true)");
      kmul(V[j], V[j - 1]);                              // :160-161 (every entry of V[j+1] is written: no fill!)
      arnoldi_column(S, n, V, j, fuse, post, lsq);       // :162-167
      beta = lsq.close_column(j);                        // :170-181
      j += 1;                                            // :182
      done = log.update(beta);                           // :183
    }
    j = j - 1;                                           // :185
    lsq.solve(j);                                        // :188-190
    // :193-196 x .+= g[i] .* V[i] ; with Pr :198-201 the same into zl = 0
    krylov_combine(S, n, has_pr ? zl : dx, has_pr ? nullptr : dx, V, fuse && j > 0 ? S.gmres_table() : nullptr, lsq.g.data(), j, fuse);
    if (has_pr) {
      ops.precond(zr, zl, -1.0);                         // :202 solve!(zr,Pr,zl)
      hipLaunchKernelGGL(axpy_kernel, dim3(grid), dim3(256), 0, S.stream, n, 1.0, zr, dx);   // :203 x .+= zr
      HIP_CHECK(hipGetLastError());
    }
    residual(V[0]);                                      // :205
  }
  return beta;                                           // :208 finalize!(log,β)
}

// solve!(x,ns::MINRESNumericalSetup,b), Krylov/MINRESSolvers.jl:75-148.  vec = the caches of :39-44 in the order Vnew, V, Vold,
// Wnew, W, Wold, Znew, Z, Zold, nv entries each (A Z needs ghost space); parts = 2 kRedBlocks doubles that no preconditioner writes.
// The scalars stay on the device (state block, kernels.hpp: MinresState): an iteration is A Z (+ the first stage of delta), Pl,
// minres_lanczos_kernel and minres_update_kernel -- the Givens rotation is formed by every workgroup of the latter -- and ONE host
// round trip, for beta_r (the stopping rule).
static double minres_core(gmg_solver &S, int64_t n, int64_t nv, const double *db, double *dx, double *const vec[9], double *parts,
                          const KrylovOps &ops, ConvLog &log)
{
  double *Vnew = vec[0], *V = vec[1], *Vold = vec[2], *Wnew = vec[3], *W = vec[4], *Wold = vec[5], *Znew = vec[6], *Z = vec[7], *Zold = vec[8];
  (void)nv;
  // Scalar slots: FGMRES's basis range (MINRES never runs inside FGMRES, nor FGMRES inside MINRES).  A cg_core nested in the
  // preconditioner keeps kScalarSlots - 8*depth, the reduction helpers (norm / dot) slot 0.
  constexpr int kBase = 16;
  const int kDelta = kBase, kBetaP = kBase + 1, kSt = kBase + 8;
  static_assert(kBase + 8 + 2 * kMinresState < kScalarSlots - 8 * 4, "MINRES slots overlap the nested CG slots");
  double *st[2] = {S.d_scalars + kSt, S.d_scalars + kSt + kMinresState};   // state halves: read `cur`, minres_update_kernel writes the other
  int cur = 0;
  S.zero(W, n); S.zero(Wold, n); S.zero(Vold, n); S.zero(Zold, n);       // :85-88
  ops.resid(dx, db, Vnew);                                               // :90-91  Vnew = b - A x
  S.zero(Znew, n);                                                       // :92
  if (ops.precond) ops.precond(Znew, Vnew, -1.0); else S.copy(Znew, Vnew, n);   // :93
  double beta_r = S.norm(n, Znew);                                       // :95
  const double beta_p = S.dot(n, Znew, Vnew);                            // :96
  REQUIRE(beta_p > 0.0, GMG_ERR_INVALID, "MINRES: dot(Pl(r), r) <= 0 at start-up -- the preconditioner is not positive definite "
                                         "(MINRESSolvers.jl:97)");
  const double gamma = std::sqrt(beta_p);                                // :99
  const int grid = gmg_solver::grid_for(n);
  S.copy(V, Vnew, n); S.copy(Z, Znew, n);
  hipLaunchKernelGGL(div_kernel, dim3(grid), dim3(256), 0, S.stream, n, gamma, V);   // :103  V .= Vnew ./ gamma
  hipLaunchKernelGGL(div_kernel, dim3(grid), dim3(256), 0, S.stream, n, gamma, Z);   // :104
  hipLaunchKernelGGL(minres_init_kernel, dim3(1), dim3(1), 0, S.stream, st[cur], gamma, beta_r);   // :99-101,106
  HIP_CHECK(hipGetLastError());
  bool done = log.init(beta_r);                                          // :107
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(kRedBlocks, (n + kBlock - 1) / kBlock));
  const bool fuse = S.fuse_reductions();
  const bool dist = S.comm.nranks > 1 && !S.reduce_local;
  const bool post = !dist && S.red_fused && S.opt_int("GMG_HOST_POLL", 1);
  double *bparts = parts + kRedBlocks;
  while (!done) {
    int nd = 0;                                                          // delta still in partials?
    if (fuse && ops.apply_dot) nd = ops.apply_dot(Z, Vnew, parts);       // :110 + first stage of :112 in one kernel (> 0), or :110 alone (-1)
    if (nd <= 0) {
      if (nd == 0) ops.apply(Z, Vnew);                                   // :110
      if (fuse) nd = S.dot_partials(n, Vnew, Z, parts); else { S.dot_async(n, Vnew, Z, kDelta, false); nd = 0; }   // :112
    }
    // :111 (delta = dot(Vnew, Z) does not depend on Znew: its partials are taken before Pl runs).  The norm of Vnew is not formed
    // (the reference never needs it): the GMG preconditioner is told so with +Inf, see gmg_minres_solve.
    if (ops.precond) ops.precond(Znew, Vnew, HUGE_VAL); else S.copy(Znew, Vnew, n);
    hipLaunchKernelGGL(minres_lanczos_kernel, dim3(nb), dim3(kBlock), 0, S.stream, n, Vnew, V, Vold, Znew, Z, Zold, st[cur],
                       S.d_scalars + kDelta, nd ? parts : nullptr, nd, bparts);   // :112-115
    HIP_CHECK(hipGetLastError());
    if (!fuse) S.finish_reduction(nb, kBetaP, false, bparts);           // :115 (all-reduced)
    S.posted = 0;
    double *pv = nullptr;
    unsigned long long *ps = nullptr, want = 0;
    if (post) { S.need_mail(); want = ++S.mail_seq; pv = &S.d_mail->value; ps = &S.d_mail->seq; }
    hipLaunchKernelGGL(minres_update_kernel, dim3(nb), dim3(kBlock), 0, S.stream, n, Vnew, Znew, Z, W, Wold, Wnew, dx, st[cur],
                       st[cur ^ 1], S.d_scalars + kDelta, S.d_scalars + kBetaP, fuse ? bparts : nullptr, fuse ? nb : 0, pv, ps,
                       want);                                            // :116-133
    HIP_CHECK(hipGetLastError());
    S.posted = want;
    cur ^= 1;
    beta_r = S.fetch_scalar(kSt + cur * kMinresState + MR_BETA_R);
    REQUIRE(!(beta_r < 0.0), GMG_ERR_INVALID, "MINRES: sqrt of a negative dot(z, v) -- the preconditioner is not positive definite "
                                              "(MINRESSolvers.jl:116)");
    // :137-139 swap3: pointers only (the scalar triples were rotated by minres_update_kernel into the other state half)
    double *t;
    t = Vold; Vold = V; V = Vnew; Vnew = t;
    t = Wold; Wold = W; W = Wnew; Wnew = t;
    t = Zold; Zold = Z; Z = Znew; Znew = t;
    done = log.update(beta_r);                                           // :144
  }
  return beta_r;                                                         // :147
}

// solve!(x,ns::RichardsonLinearNumericalSetup,b), RichardsonLinearSolvers.jl:84-98, on the handle's level 0 (z and r are CG's)
static double richardson_core(gmg_solver &S, int64_t n, const double *db, double *dx, double omega, int use_precond, ConvLog &log)
{
  double *z = S.cg_z, *r = S.cg_r;
  const int grid = gmg_solver::grid_for(n);
  S.apply_A_resid(0, dx, db, r);                         // :84-85
  double resn = S.norm(n, r);
  bool done = log.init(resn);                            // :86
  while (!done) {
    const double *dir = r;
    if (use_precond) { S.krylov_precond(use_precond, z, r, resn); dir = z; }   // :89
    hipLaunchKernelGGL(axpy_kernel, dim3(grid), dim3(256), 0, S.stream, n, omega, dir, dx);   // :90,98 x .+= w .* z
    HIP_CHECK(hipGetLastError());
    S.apply_A_resid(0, dx, db, r);                       // :91-92
    resn = S.norm(n, r);
    done = log.update(resn);                             // :93
  }
  return resn;                                           // :95
}
