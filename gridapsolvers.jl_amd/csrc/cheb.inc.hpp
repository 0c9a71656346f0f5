// cheb.inc.hpp -- ChebyshevSmoother(M, degree) over the preconditioner M of a smoother slot, M in {JacobiLinearSolver, PatchSolver,
// BlockJacobiSolver} (included at the end of gmg_amd.hip).  The reference has no such smoother: like the Gauss-Seidel orderings it is an
// addition of the device library next to the reference's types, on one GPU and on partitioned handles (SEVERAL RANKS below).
//
// One pass of degree m on (x, r) is Saad, Iterative Methods, Alg. 12.1 in the residual form of the smoothers here, with
// z = M^-1 r the un-relaxed preconditioner of the slot (what gmg_precond_apply returns):
//
//   theta = (lmax + lmin)/2   delta = (lmax - lmin)/2   sigma = theta/delta   rho_0 = 1/sigma
//   sweep 0:            d = (1/theta) z                                  ; x += d ; r -= A d
//   sweep k = 1..m-1:   rho_k = 1/(2 sigma - rho_{k-1})
//                       d = (rho_k rho_{k-1}) d + (2 rho_k/delta) z      ; x += d ; r -= A d
//
// The 2m - 1 coefficients are computed on the host in double in exactly this order, once per setup (cheb_coefficients), and reach the
// kernels as arguments.  In the kernels every product is rounded, then the sum (__dmul_rn / __dadd_rn; the library is built with
// -ffp-contract=off anyway), so a*d + b*z in numpy is the same arithmetic.  Sweep 0 never reads d -- L.dx, which holds whatever the
// prolongation or the pass before left there -- and writes x = d where the pass starts from x = 0.
//
// SPECTRUM BOUNDS.  Given lambda_max: used as it is, with lambda_min (default lambda_max / eig_ratio).  Otherwise gmg_setup estimates
// lambda_max(M^-1 A) per smoothed level and slot (pre and post share the estimate when they share M) by eig_steps power steps from the
// start vector v_i = 1 + ((i * 2654435761) mod 1024)/1024 (0-based row i, unsigned 64-bit), normalised: w = M^-1 (A v) ;
// lambda_est = ||w||_2 ; v = w/lambda_est -- the level's mat-vec, the slot's preconditioner and the dot kernel, nothing new.  Then
// lambda_max = eig_safety lambda_est, lambda_min = lambda_max/eig_ratio (PETSc's interval convention).  KNOWN WEAKNESS: a few power
// steps under-estimate a clustered top of the spectrum (Jacobi on Q1 32^3: 1.336 after 10 steps against 1.494, so 1.1 lambda_est is
// still below lambda_max).  THE REMEDY is the Lanczos estimate below (gmg_set_chebyshev_eig_method: 1.455 after the same 10 steps, so
// 1.1 lambda_est covers lambda_max); a given lambda_max or more eig_steps do as well.  A value refresh (gmg_update_values + gmg_setup)
// estimates again, by the slot's method.
//
// LANCZOS ESTIMATE (GMG_CHEB_EIG_LANCZOS; POWER stays the default).  eig_steps steps of CG on A with preconditioner M from r = the same
// start vector, normalised; lambda_est is the largest eigenvalue of the Lanczos tridiagonal that CG builds:
//   r = v ; gamma_old = 1 ; k = 0
//   while k < eig_steps:
//     z = M^-1 r ; gamma = dot(z, r)    stop unless gamma is finite and > 0 ; for k > 0 also stop if gamma < 1e-24 * gamma_0
//     beta = gamma / gamma_old ; p = z + beta p   (k = 0: p = z)
//     w = A p ; pw = dot(p, w)          stop unless pw is finite and > 0
//     alpha = gamma / pw ; r -= alpha w ; record (alpha, beta) ; gamma_old = gamma ; k += 1
//   T (k x k): T[i,i] = 1/alpha_i + (i > 0 ? beta_i/alpha_{i-1} : 0) ; T[i,i+1] = T[i+1,i] = sqrt(beta_{i+1})/alpha_i   (textbook form)
// The 1e-24 stop is a condition, not a tolerance: the residual has dropped twelve digits in the M^-1 norm, the Krylov space is exhausted
// in double and further steps add rounding noise only (levels of 1, 9 and 27 rows stop after 1, 6 and 7 steps with the exact
// lambda_max).  A stop with no step recorded is GMG_ERR_SINGULAR.  Driven from the host like the power iteration -- the level's
// mat-vec, cheb_precond, the dot kernel, xpby_kernel and axpy_kernel, a fetch per dot; r, z, w in the level's work vectors, p in a vector
// that lives for the estimate only -- and the largest eigenvalue of T (at most eig_steps rows) by Sturm bisection on the host
// (cheb_tridiag_lambda_max).  Per step: one mat-vec, one M^-1 and two dots against one mat-vec, one M^-1 and one norm.  What it buys is
// a robust default interval, not a faster solve.  Pre and post share one estimate when they share M, eig_steps and the method.
//
// KERNELS (all HBM-bound streaming):
//   cheb_update_kernel<FIRST, DINV>   the pointwise update d = [a d +] b z ; x (+)= d with z = dinv .* r (Jacobi M, DINV) or z as it
//                                     is (patch M in operator form, after spmv_set(S.M, r, z)).  16-byte accesses where every pointer
//                                     is 16-byte aligned, a scalar tail for an odd n, scalar throughout otherwise.
//   patch_gather[_sell]_cheb_kernel   (kernels.hpp) patch M in the contribution-buffer forms: the update rides in the gather's epilogue.
// Each sweep is followed by the level's apply_A_sub (r -= A d).  d lives in L.dx, z of the operator form in the level's residual
// buffer the pass does not use: no new device buffer.
//
// SEVERAL RANKS.  A Chebyshev slot runs on the own | ghost levels (gmg_set_partition) and on the replicated levels of a handle with a
// communicator, real or loopback; a handle without one keeps its kernels, launches and bits.  On an own | ghost level recurrence,
// coefficients and roundings are those above on the n_own owned rows.  Jacobi M: the update is pointwise and rank-local.  Patch M, in
// the order RichardsonSmoother(PatchSolver) uses there: consistent!(r) (exchange), the patch solves, the gather over ALL local dofs
// into z, assemble!(z) (assemble_add), the pointwise update on the owned rows -- always the contribution-buffer form, which is what the
// Richardson pass takes on such a level; z lives in the residual buffer the pass does not use.  r -= A d is apply_A_sub: it exchanges d
// and fixes up the boundary rows.  r lives in a buffer of the level before anything is exchanged, never in a caller's vector.
//   cheb_update_pack_kernel<FIRST, DINV>   cheb_update_kernel AND the pack of d's send entries in one launch (option cheb_pack_fused,
//                                     default 1), on levels whose pack can fuse (can_fuse_pack: every sent row is a boundary row).  The
//                                     level's row -> boundary-row index table (Level::bidx, -1 off the boundary) leads the lane that
//                                     updates row i to the row's send slots (d_pk_ptr / d_pk_slot), and that lane stores the value it has
//                                     just written to d[i]: no lane reads a d another lane is writing.  Plain vector stores; apply_A_sub
//                                     then runs prepacked and the halo_pack_kernel launch of every sweep is gone.  Same bits either way;
//                                     where the pack cannot fuse the unfused form runs whatever the option says.
// The estimates are unchanged in form: the mat-vec is apply_A_set (with its exchange), M^-1 as in the pass, dot / norm all-reduced over
// the ranks, so the Lanczos stops and the GMG_ERR_SINGULAR decisions are taken on reduced scalars by all ranks together.  On replicated
// levels the reductions stay local and every rank gets the same estimate.  The start vector is the formula above with i the 0-based
// index of the row among THE HANDLE'S OWN ROWS, normalised in the global norm: on a folded (loopback) handle that is the stacked index
// and the estimate is the single-GPU estimate of the folded matrix; between true ranks the vector, and therefore lambda_est after a few
// steps, DEPENDS ON THE PARTITION (gmg_get_chebyshev_info reports the value).
//
// REFUSED: Gauss-Seidel slots (GMG_ERR_UNSUPPORTED at gmg_set_smoother_chebyshev).  At gmg_setup, GMG_ERR_UNSUPPORTED naming the level:
// the overlapping layout (gmg_set_partition_overlap), levels of a redistributed rank subset (gmg_set_redistribution), and a handle that has a
// communicator but no declared layout (gmg_set_replication never called).  The pass-level shortcuts of the Richardson-Jacobi passes
// (fold_level, emits_s0, smooth_persistent, r_dead) do not apply.

namespace {

typedef double cheb_d2 __attribute__((ext_vector_type(2)));

template <bool FIRST, bool DINV>
__device__ __forceinline__ double cheb_step(double a, double b, double dinv, double z, double d)
{
  if (DINV) z = __dmul_rn(dinv, z);
  const double t = __dmul_rn(b, z);
  return FIRST ? t : __dadd_rn(__dmul_rn(a, d), t);
}

// vec != 0: dinv, z, d, x are all 16-byte aligned -- pairs of rows per lane, then the odd last row
template <bool FIRST, bool DINV>
__global__ void cheb_update_kernel(int64_t n, double a, double b, const double *__restrict__ dinv, const double *__restrict__ z,
                                   double *__restrict__ d, double *__restrict__ x, int x_zero, int vec)
{
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if (vec) {
    const int64_t n2 = n >> 1;
    const cheb_d2 *z2 = reinterpret_cast<const cheb_d2 *>(z), *q2 = reinterpret_cast<const cheb_d2 *>(dinv);
    cheb_d2 *d2 = reinterpret_cast<cheb_d2 *>(d), *x2 = reinterpret_cast<cheb_d2 *>(x);
    for (int64_t i = tid; i < n2; i += nth) {
      const cheb_d2 zz = z2[i];
      cheb_d2 qq = {1.0, 1.0}, dd = {0.0, 0.0};
      if (DINV) qq = q2[i];
      if (!FIRST) dd = d2[i];
      cheb_d2 out;
      out.x = cheb_step<FIRST, DINV>(a, b, qq.x, zz.x, dd.x);
      out.y = cheb_step<FIRST, DINV>(a, b, qq.y, zz.y, dd.y);
      d2[i] = out;
      if (x_zero) x2[i] = out;
      else {
        cheb_d2 xx = x2[i];
        xx.x = __dadd_rn(xx.x, out.x);
        xx.y = __dadd_rn(xx.y, out.y);
        x2[i] = xx;
      }
    }
    done = n2 * 2;
  }
  for (int64_t i = done + tid; i < n; i += nth) {
    const double out = cheb_step<FIRST, DINV>(a, b, DINV ? dinv[i] : 1.0, z[i], FIRST ? 0.0 : d[i]);
    d[i] = out;
    x[i] = x_zero ? out : __dadd_rn(x[i], out);
  }
}

// the send slots pk_slot[pk_ptr[q] .. pk_ptr[q + 1]) of boundary row q take the value the lane has just written to d (every slot is
// below the length of sendbuf: gmg_setup)
__device__ __forceinline__ void cheb_pack_row(int32_t q, double v, const int64_t *__restrict__ pk_ptr, const int32_t *__restrict__ pk_slot,
                                              double *__restrict__ sendbuf)
{
  if (q >= 0)
    for (int64_t k = pk_ptr[q]; k < pk_ptr[q + 1]; ++k) sendbuf[pk_slot[k]] = v;
}

// cheb_update_kernel on an own | ghost level whose pack can fuse + the pack of d's send entries: the lane of row i stores the value it
// wrote to d[i] into the row's send slots, q = bidx[i].  Same body, same roundings; bidx (an allocation of its own) is read in pairs
// next to the 16-byte accesses.
template <bool FIRST, bool DINV>
__global__ void cheb_update_pack_kernel(int64_t n, double a, double b, const double *__restrict__ dinv, const double *__restrict__ z,
                                        double *__restrict__ d, double *__restrict__ x, int x_zero, int vec,
                                        const int32_t *__restrict__ bidx, const int64_t *__restrict__ pk_ptr,
                                        const int32_t *__restrict__ pk_slot, double *__restrict__ sendbuf)
{
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  int64_t done = 0;
  if (vec) {
    const int64_t n2 = n >> 1;
    const cheb_d2 *z2 = reinterpret_cast<const cheb_d2 *>(z), *q2 = reinterpret_cast<const cheb_d2 *>(dinv);
    cheb_d2 *d2 = reinterpret_cast<cheb_d2 *>(d), *x2 = reinterpret_cast<cheb_d2 *>(x);
    const int2 *b2 = reinterpret_cast<const int2 *>(bidx);
    for (int64_t i = tid; i < n2; i += nth) {
      const cheb_d2 zz = z2[i];
      const int2 bq = b2[i];
      cheb_d2 qq = {1.0, 1.0}, dd = {0.0, 0.0};
      if (DINV) qq = q2[i];
      if (!FIRST) dd = d2[i];
      cheb_d2 out;
      out.x = cheb_step<FIRST, DINV>(a, b, qq.x, zz.x, dd.x);
      out.y = cheb_step<FIRST, DINV>(a, b, qq.y, zz.y, dd.y);
      d2[i] = out;
      if (x_zero) x2[i] = out;
      else {
        cheb_d2 xx = x2[i];
        xx.x = __dadd_rn(xx.x, out.x);
        xx.y = __dadd_rn(xx.y, out.y);
        x2[i] = xx;
      }
      cheb_pack_row(bq.x, out.x, pk_ptr, pk_slot, sendbuf);
      cheb_pack_row(bq.y, out.y, pk_ptr, pk_slot, sendbuf);
    }
    done = n2 * 2;
  }
  for (int64_t i = done + tid; i < n; i += nth) {
    const double out = cheb_step<FIRST, DINV>(a, b, DINV ? dinv[i] : 1.0, z[i], FIRST ? 0.0 : d[i]);
    d[i] = out;
    x[i] = x_zero ? out : __dadd_rn(x[i], out);
    cheb_pack_row(bidx[i], out, pk_ptr, pk_slot, sendbuf);
  }
}

// start vector of the power iteration (not yet normalised)
__global__ void cheb_start_kernel(int64_t n, double *__restrict__ v)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    v[i] = 1.0 + (double)(((uint64_t)i * 2654435761ull) % 1024ull) / 1024.0;
}

// v = w / s (v may be w)
__global__ void cheb_div_kernel(int64_t n, const double *w, double s, double *v)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = w[i] / s;
}

// the 2m - 1 coefficients, in the order of the header comment: b[0] = 1/theta ; a[k] = rho_k rho_{k-1}, b[k] = 2 rho_k / delta
void cheb_coefficients(int m, double lmin, double lmax, std::vector<double> &a, std::vector<double> &b)
{
  a.assign((size_t)m, 0.0); b.assign((size_t)m, 0.0);
  const double theta = (lmax + lmin) / 2.0, delta = (lmax - lmin) / 2.0, sigma = theta / delta;
  double rho = 1.0 / sigma;
  b[0] = 1.0 / theta;
  for (int k = 1; k < m; ++k) {
    const double rho_k = 1.0 / (2.0 * sigma - rho);
    a[(size_t)k] = rho_k * rho;
    b[(size_t)k] = (2.0 * rho_k) / delta;
    rho = rho_k;
  }
}

// largest eigenvalue of the symmetric tridiagonal (diagonal d[0..k), off-diagonal e[0..k-1)) by Sturm bisection: the number of
// eigenvalues below x is the number of negative pivots of T - x I.  Bisected until the interval is two neighbouring doubles.
double cheb_tridiag_lambda_max(const std::vector<double> &d, const std::vector<double> &e)
{
  const int k = (int)d.size();
  if (k == 1) return d[0];
  double lo = d[0], hi = d[0];
  for (int i = 0; i < k; ++i) {                              // Gershgorin
    const double rad = (i > 0 ? std::fabs(e[(size_t)i - 1]) : 0.0) + (i + 1 < k ? std::fabs(e[(size_t)i]) : 0.0);
    lo = std::min(lo, d[(size_t)i] - rad); hi = std::max(hi, d[(size_t)i] + rad);
  }
  const double scale = std::max(std::fabs(lo), std::fabs(hi));
  const double eps = std::numeric_limits<double>::epsilon(), tiny = std::numeric_limits<double>::min();
  hi += 4.0 * eps * scale + tiny;                            // all k eigenvalues are below hi
  const auto below = [&](double x) {
    int c = 0;
    double q = d[0] - x;
    if (q < 0.0) ++c;
    for (int i = 1; i < k; ++i) {
      if (q == 0.0) q = eps * scale + tiny;
      q = d[(size_t)i] - x - e[(size_t)i - 1] * e[(size_t)i - 1] / q;
      if (q < 0.0) ++c;
    }
    return c;
  };
  for (int it = 0; it < 4096; ++it) {
    const double mid = lo + (hi - lo) / 2.0;
    if (!(mid > lo && mid < hi)) break;
    if (below(mid) == k) hi = mid; else lo = mid;
  }
  return lo + (hi - lo) / 2.0;
}

bool cheb_same_M(const Smoother &p, const Smoother &q)
{
  if (p.kind != q.kind) return false;
  if (p.kind == SM_JACOBI) return true;
  return p.kind == SM_PATCH && p.tab && p.tab == q.tab && p.patch_kind == q.patch_kind;
}

} // namespace

// z = M^-1 r, the un-relaxed preconditioner of the slot.  Patch M on an own | ghost level: consistent!(r) first (r and z are vectors of
// the level, with ghost room), then the local solves and assemble!(z) inside patch_precond
void gmg_solver::cheb_precond(int l, Smoother &S, double *r, double *z)
{
  Level &L = lev[l];
  if (S.kind == SM_JACOBI) {
    hipLaunchKernelGGL(jacobi_apply_kernel, dim3(grid_for(L.n)), dim3(256), 0, stream, L.n, L.dinv, r, z);
    HIP_CHECK(hipGetLastError());
  } else {
    if (comm.nranks > 1 && L.halo.present && !L.halo.ovl) exchange(l, r);
    patch_precond(L, S, r, 1.0, false, z, nullptr);
  }
}

// GMG_CHEB_EIG_LANCZOS: eig_steps steps of CG on A with preconditioner M from the normalised start vector, driven from the host (a fetch
// per dot: setup work); lambda_est = the largest eigenvalue of the textbook Lanczos tridiagonal of the recorded (alpha, beta).  r, z, w in
// the level's work vectors, p in a vector that lives for the estimate only.  Sets S.cheb_steps_done.
double gmg_solver::cheb_lanczos(int l, Smoother &S, const std::string &where)
{
  Level &L = lev[l];
  const int64_t n = L.n;
  double *r = L.rbuf[0], *z = L.rbuf[1], *w = L.dx, *p = dvec(L.nvec);
  struct Free { gmg_solver &G; double *&p; size_t n; ~Free() { (void)hipStreamSynchronize(G.stream); G.release(p, n); } } free_p{*this, p, (size_t)L.nvec};
  hipLaunchKernelGGL(cheb_start_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, r);
  HIP_CHECK(hipGetLastError());
  const double nv = norm(n, r);
  REQUIRE(std::isfinite(nv) && nv > 0.0, GMG_ERR_SINGULAR, where + "the start vector of the Lanczos estimate has norm " + std::to_string(nv));
  hipLaunchKernelGGL(cheb_div_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, r, nv, r);
  HIP_CHECK(hipGetLastError());
  std::vector<double> al, be;
  double gamma_old = 1.0, gamma0 = 0.0;
  for (int k = 0; k < S.cheb_eig_steps; ++k) {
    cheb_precond(l, S, r, z);
    const double gamma = dot(n, z, r);
    if (!(std::isfinite(gamma) && gamma > 0.0)) break;
    if (k == 0) gamma0 = gamma;
    else if (gamma < 1e-24 * gamma0) break;                  // the Krylov space is exhausted in double
    const double beta = gamma / gamma_old;
    if (k == 0) copy(p, z, n);
    else hipLaunchKernelGGL(xpby_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, z, beta, p);
    HIP_CHECK(hipGetLastError());
    apply_A_set(l, p, w);
    const double pw = dot(n, p, w);
    if (!(std::isfinite(pw) && pw > 0.0)) break;
    const double alpha = gamma / pw;
    hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, -alpha, w, r);
    HIP_CHECK(hipGetLastError());
    al.push_back(alpha); be.push_back(beta);
    gamma_old = gamma;
  }
  const int k = (int)al.size();
  REQUIRE(k > 0, GMG_ERR_SINGULAR, where + "the Lanczos estimate recorded no step: M^-1 A is not positive definite on level " +
          std::to_string(l) + " (use eig_method = power or pass lambda_max)");
  std::vector<double> d((size_t)k), e((size_t)k - 1);
  for (int i = 0; i < k; ++i) {
    d[(size_t)i] = 1.0 / al[(size_t)i] + (i > 0 ? be[(size_t)i] / al[(size_t)i - 1] : 0.0);
    if (i + 1 < k) e[(size_t)i] = std::sqrt(be[(size_t)i + 1]) / al[(size_t)i];
  }
  S.cheb_steps_done = k;
  return cheb_tridiag_lambda_max(d, e);
}

// spectrum bounds (given, or from the power iteration / the Lanczos estimate) and the coefficients of the slot.  same_M: the level's other
// slot, already set up
void gmg_solver::cheb_setup(int l, Smoother &S, const Smoother *same_M)
{
  Level &L = lev[l];
  const std::string where = "Chebyshev smoother on level " + std::to_string(l) + ": ";
  REQUIRE(S.kind == SM_JACOBI || S.kind == SM_PATCH, GMG_ERR_UNSUPPORTED, where + "M must be a Jacobi or a patch solver");
  if (S.cheb_lmax_in > 0.0) {
    S.cheb_lest = NAN;
    S.cheb_lmax = S.cheb_lmax_in;
    S.cheb_steps_done = 0;
  } else {
    // a replicated level of a handle with several ranks: every rank holds the whole vectors, the reductions of the estimate stay local
    struct Local { bool &flag; bool saved; ~Local() { flag = saved; } } local{reduce_local, reduce_local};
    if (comm.nranks > 1 && rep_from >= 0 && l >= rep_from) reduce_local = true;
    if (same_M && same_M->cheb && !(same_M->cheb_lmax_in > 0.0) && same_M->cheb_eig_steps == S.cheb_eig_steps &&
        same_M->cheb_eig_method == S.cheb_eig_method && cheb_same_M(*same_M, S)) {
      S.cheb_lest = same_M->cheb_lest;
      S.cheb_steps_done = same_M->cheb_steps_done;
    } else if (S.cheb_eig_method == GMG_CHEB_EIG_LANCZOS)
      S.cheb_lest = cheb_lanczos(l, S, where);
    else {
      // v, A v and M^-1 A v in the level's work vectors (nothing of a solve is alive during setup)
      const int64_t n = L.n;
      double *v = L.rbuf[0], *t = L.rbuf[1], *w = L.dx;
      hipLaunchKernelGGL(cheb_start_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, v);
      HIP_CHECK(hipGetLastError());
      double lam = norm(n, v);
      for (int s = 0; s <= S.cheb_eig_steps; ++s) {
        REQUIRE(std::isfinite(lam) && lam > 0.0, GMG_ERR_SINGULAR, where + "the power iteration on M^-1 A broke down (norm " + std::to_string(lam) + ")");
        if (s == S.cheb_eig_steps) break;
        hipLaunchKernelGGL(cheb_div_kernel, dim3(grid_for(n)), dim3(256), 0, stream, n, s == 0 ? v : w, lam, v);   // (s == 0: the start vector, normalised)
        HIP_CHECK(hipGetLastError());
        apply_A_set(l, v, t);
        cheb_precond(l, S, t, w);
        lam = norm(n, w);
      }
      S.cheb_lest = lam;
      S.cheb_steps_done = S.cheb_eig_steps;
    }
    S.cheb_lmax = S.cheb_eig_safety * S.cheb_lest;
  }
  S.cheb_lmin = S.cheb_lmin_in > 0.0 ? S.cheb_lmin_in : S.cheb_lmax / S.cheb_eig_ratio;
  REQUIRE(S.cheb_lmin > 0.0 && S.cheb_lmin < S.cheb_lmax, GMG_ERR_INVALID, where + "the bounds must satisfy 0 < lambda_min < lambda_max (" +
          std::to_string(S.cheb_lmin) + ", " + std::to_string(S.cheb_lmax) + ")");
  cheb_coefficients(S.cheb_degree, S.cheb_lmin, S.cheb_lmax, S.cheb_a, S.cheb_b);
}

// one pass of degree m on (x, r), r in place in one of the level's residual buffers (returned)
double *gmg_solver::cheb_pass(int l, Smoother &S, double *x, const double *r_in, bool x_zero)
{
  Level &L = lev[l];
  const int64_t n = L.n;
  REQUIRE((int)S.cheb_b.size() == S.cheb_degree && S.cheb_degree >= 1, GMG_ERR_STATE, "Chebyshev smoother: no coefficients (gmg_setup first)");
  double *r = nullptr;
  if (r_in == L.rbuf[0] || r_in == L.rbuf[1]) r = const_cast<double *>(r_in);
  else { r = L.rbuf[0]; copy(r, r_in, n); }
  double *d = L.dx;
  double *zbuf = (r == L.rbuf[0]) ? L.rbuf[1] : L.rbuf[0];   // z = M r of the operator form: the residual buffer this pass does not use
  // own | ghost level of several ranks: patch M is consistent!(r), local solves, gather over all local dofs, assemble!(z) -- then the
  // pointwise update on the owned rows; where the pack can fuse, the update also fills the send buffer of d's exchange
  const bool dist = comm.nranks > 1 && L.halo.present && !L.halo.ovl;
  const bool contrib_form = S.kind == SM_PATCH && !S.use_M && !dist;
  const bool pack = dist && can_fuse_pack(l) && L.bidx != nullptr && opt_int("GMG_CHEB_PACK_FUSED", 1) != 0;
  // launches of one sweep on such a level, for the profiled level's count (gmg_get_kernel_stats)
  int sweep_launches = 0;
  if (dist) {
    const HaloPlan &H = L.halo;
    const int pack_launch = H.nsend() > 0 && !H.nbr.empty() ? 1 : 0;
    sweep_launches = 1 + (pack ? 0 : pack_launch) + 1 + (L.split && L.nbnd > 0 ? 1 : 0);   // update, pack of d, own columns, boundary fix-up
    if (S.kind == SM_PATCH) {
      sweep_launches += pack_launch + (S.npatch > 0 ? 1 : 0) + 1;                          // pack of r, patch solves, gather
      for (size_t k = 0; k < H.nbr.size(); ++k) sweep_launches += H.snd_ptr[k + 1] > H.snd_ptr[k] ? 1 : 0;   // assemble!: one add per neighbour
    }
  }
  const auto aligned16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  for (int k = 0; k < S.cheb_degree; ++k) {
    const bool first = k == 0;
    const double a = S.cheb_a[(size_t)k], b = S.cheb_b[(size_t)k];
    const int xz = (x_zero && first) ? 1 : 0;
    const bool prof = dist && (l == prof_level) && prof_used + 2 <= prof_ev.size();
    if (prof) HIP_CHECK(hipEventRecord(prof_ev[prof_used], stream));
    if (dist) {
      const bool jac = S.kind == SM_JACOBI;
      const double *z = r;
      if (!jac) { cheb_precond(l, S, r, zbuf); z = zbuf; }
      const double *q = jac ? L.dinv : nullptr;
      const int vec = ((!jac || aligned16(q)) && aligned16(z) && aligned16(d) && aligned16(x)) ? 1 : 0;
      const int grid = grid_for(vec ? (n + 1) / 2 : n);
      if (pack) {
        const HaloPlan &H = L.halo;
        with_bools([&](auto F, auto D) { hipLaunchKernelGGL((cheb_update_pack_kernel<F(), D()>), dim3(grid), dim3(256), 0, stream, n, a, b, q, z, d, x, xz, vec,
                                                            L.bidx, H.d_pk_ptr, H.d_pk_slot, H.d_sendbuf); }, first, jac);
      } else {
        with_bools([&](auto F, auto D) { hipLaunchKernelGGL((cheb_update_kernel<F(), D()>), dim3(grid), dim3(256), 0, stream, n, a, b, q, z, d, x, xz, vec); }, first, jac);
      }
    } else if (contrib_form) {
      patch_contrib(S, r);
      const int grid = (int)std::max<int64_t>(1, (n + 255) / 256);
      if (S.d_isoff) {
        with_bool(first, [&](auto F) { hipLaunchKernelGGL((patch_gather_sell_cheb_kernel<F()>), dim3(grid), dim3(256), 0, stream, n, S.d_isoff, S.d_isinc, S.d_contrib, a, b, xz, d, x); });
      } else {
        with_bool(first, [&](auto F) { hipLaunchKernelGGL((patch_gather_cheb_kernel<F()>), dim3(grid), dim3(256), 0, stream, n, S.d_iptr, S.d_inc, S.d_contrib, a, b, xz, d, x); });
      }
    } else if (S.kind == SM_PATCH) {
      spmv_set(S.M, r, zbuf);
      const int vec = (aligned16(zbuf) && aligned16(d) && aligned16(x)) ? 1 : 0;
      const int grid = grid_for(vec ? (n + 1) / 2 : n);
      with_bool(first, [&](auto F) { hipLaunchKernelGGL((cheb_update_kernel<F(), false>), dim3(grid), dim3(256), 0, stream, n, a, b, (const double *)nullptr, zbuf, d, x, xz, vec); });
    } else {
      const int vec = (aligned16(L.dinv) && aligned16(r) && aligned16(d) && aligned16(x)) ? 1 : 0;
      const int grid = grid_for(vec ? (n + 1) / 2 : n);
      with_bool(first, [&](auto F) { hipLaunchKernelGGL((cheb_update_kernel<F(), true>), dim3(grid), dim3(256), 0, stream, n, a, b, L.dinv, r, d, x, xz, vec); });
    }
    HIP_CHECK(hipGetLastError());
    apply_A_sub(l, d, r, nullptr, pack);                     // (the distributed product: exchanges d, prepacked where the update packed it)
    if (prof) {
      HIP_CHECK(hipEventRecord(prof_ev[prof_used + 1], stream));
      prof_w[prof_used / 2] = sweep_launches;
      prof_xm[prof_used / 2] = -1;
      prof_used += 2;
    }
  }
  return r;
}

extern "C" {

int gmg_set_smoother_chebyshev(gmg_handle_t h, int lev, int which, int degree, double lambda_min, double lambda_max, int eig_steps,
                               double eig_ratio, double eig_safety)
{
  return guarded(h, [&] {
    check_level(h, lev, true);
    REQUIRE(which == GMG_PRE || which == GMG_POST || which == GMG_PRE_AND_POST, GMG_ERR_INVALID, "bad `which`");
    REQUIRE(degree >= 1, GMG_ERR_INVALID, "The degree must be a positive integer.");
    REQUIRE(!(lambda_min > 0.0 && lambda_max > 0.0) || lambda_min < lambda_max, GMG_ERR_INVALID, "lambda_min must be smaller than lambda_max.");
    REQUIRE(eig_ratio > 1.0, GMG_ERR_INVALID, "eig_ratio must be greater than 1.");
    REQUIRE(eig_safety >= 1.0, GMG_ERR_INVALID, "eig_safety must be at least 1.");
    REQUIRE(eig_steps >= 1, GMG_ERR_INVALID, "eig_steps must be a positive integer.");
    REQUIRE(!std::isnan(lambda_min) && !std::isnan(lambda_max), GMG_ERR_INVALID, "lambda_min / lambda_max must not be NaN.");
    Level &L = h->lev[lev];
    const bool on_pre = which != GMG_POST, on_post = which != GMG_PRE;
    // the slot as gmg_setup will see it: a post-smoother that shares the pre-smoother is the pre-smoother's slot
    const Smoother &P = L.pre, &Q = L.post_shares_pre ? L.pre : L.post;
    for (const Smoother *sp : {on_pre ? &P : nullptr, on_post ? &Q : nullptr}) {
      if (!sp) continue;
      REQUIRE(sp->assigned, GMG_ERR_STATE, "gmg_set_smoother_chebyshev: the slot has no smoother yet (gmg_set_smoother_jacobi / gmg_set_smoother_patch first)");
      REQUIRE(sp->kind != SM_GAUSS_SEIDEL, GMG_ERR_UNSUPPORTED, "gmg_set_smoother_chebyshev: M must be a Jacobi or a patch solver, the slot holds a Gauss-Seidel smoother");
      REQUIRE(!sp->pmult, GMG_ERR_UNSUPPORTED, "gmg_set_smoother_chebyshev: the slot holds a multiplicative patch smoother (Chebyshev over the "
              "multiplicative sweep is not supported)");
    }
    // a slot of its own for the side that is changed alone
    if (which != GMG_PRE_AND_POST && L.post_shares_pre) { L.post = L.pre; L.post_shares_pre = false; }
    for (Smoother *sp : {on_pre ? &L.pre : nullptr, (on_post && !L.post_shares_pre) ? &L.post : nullptr}) {
      if (!sp) continue;
      sp->cheb = true;
      sp->cheb_degree = degree; sp->cheb_eig_steps = eig_steps;
      sp->cheb_lmin_in = lambda_min > 0.0 ? lambda_min : 0.0;
      sp->cheb_lmax_in = lambda_max > 0.0 ? lambda_max : 0.0;
      sp->cheb_eig_ratio = eig_ratio; sp->cheb_eig_safety = eig_safety;
      sp->cheb_eig_method = GMG_CHEB_EIG_POWER; sp->cheb_steps_done = 0;
      sp->cheb_a.clear(); sp->cheb_b.clear();
    }
    L.clear_overlap_hints();
    h->touch();
  });
}

int gmg_set_chebyshev_eig_method(gmg_handle_t h, int lev, int which, int method)
{
  return guarded(h, [&] {
    check_level(h, lev, true);
    REQUIRE(which == GMG_PRE || which == GMG_POST || which == GMG_PRE_AND_POST, GMG_ERR_INVALID, "bad `which`");
    REQUIRE(method == GMG_CHEB_EIG_POWER || method == GMG_CHEB_EIG_LANCZOS, GMG_ERR_INVALID,
            "gmg_set_chebyshev_eig_method: the method must be GMG_CHEB_EIG_POWER or GMG_CHEB_EIG_LANCZOS");
    Level &L = h->lev[lev];
    const bool on_pre = which != GMG_POST, on_post = which != GMG_PRE;
    for (const Smoother *sp : {on_pre ? &L.pre : nullptr, on_post ? (L.post_shares_pre ? &L.pre : &L.post) : nullptr})
      REQUIRE(!sp || sp->cheb, GMG_ERR_STATE, "gmg_set_chebyshev_eig_method: the slot has no Chebyshev smoother (gmg_set_smoother_chebyshev first)");
    // a slot of its own for the side that is changed alone
    if (which != GMG_PRE_AND_POST && L.post_shares_pre) { L.post = L.pre; L.post_shares_pre = false; }
    for (Smoother *sp : {on_pre ? &L.pre : nullptr, (on_post && !L.post_shares_pre) ? &L.post : nullptr}) {
      if (!sp) continue;
      sp->cheb_eig_method = method; sp->cheb_steps_done = 0;
      sp->cheb_a.clear(); sp->cheb_b.clear();
    }
    h->touch();
  });
}

int gmg_get_chebyshev_eig(gmg_handle_t h, int lev, int which, int *method, int *steps_done)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, true);
    REQUIRE(which == GMG_PRE || which == GMG_POST, GMG_ERR_INVALID, "which must be GMG_PRE or GMG_POST");
    const Smoother &S = which == GMG_PRE ? h->lev[lev].pre : h->lev[lev].post;
    REQUIRE(S.cheb, GMG_ERR_STATE, "this slot has no Chebyshev smoother");
    if (method) *method = S.cheb_eig_method;
    if (steps_done) *steps_done = S.cheb_steps_done;
  });
}

int gmg_get_chebyshev_info(gmg_handle_t h, int lev, int which, int *degree, double *lambda_est, double *lambda_min, double *lambda_max,
                           int *eig_steps)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, true);
    REQUIRE(which == GMG_PRE || which == GMG_POST, GMG_ERR_INVALID, "which must be GMG_PRE or GMG_POST");
    const Smoother &S = which == GMG_PRE ? h->lev[lev].pre : h->lev[lev].post;
    REQUIRE(S.cheb, GMG_ERR_STATE, "this slot has no Chebyshev smoother");
    if (degree) *degree = S.cheb_degree;
    if (lambda_est) *lambda_est = S.cheb_lest;
    if (lambda_min) *lambda_min = S.cheb_lmin;
    if (lambda_max) *lambda_max = S.cheb_lmax;
    if (eig_steps) *eig_steps = S.cheb_eig_steps;
  });
}

} // extern "C"
