// f32.inc.hpp -- cycle_values = float32: level matrices streamed in single precision inside the multigrid cycle
// (included at the end of gmg_amd.hip).
//
// A preconditioner does not need fp64 matrix entries; the Krylov method around it does.  With option values_f32 the cycle of a
// preconditioner-mode handle is EXACTLY the fp64 cycle on matrices A~_l: A_l with every stored value rounded to float32 (nearest
// even) and read back as fp64.  Vectors, transfers, the coarsest solve and all arithmetic stay fp64; 1/diag of such a level is
// 1 / A~_ii.  Nothing outside the cycle reads A~: CG's w = A p, r = b - A x, gmg_op_apply stream the fp64 values.
//
// Which levels: the format selection runs unchanged on the fp64 values; every level but the coarsest that lands on SELL-64 or SELL-O
// with an explicit value stream gets a float twin of that stream in the same slice geometry (same soff, scol, rowlen, offset-pattern
// tables).  Level 0 keeps both streams, levels >= 1 release the fp64 one (gmg_op_apply(GMG_OP_A) is then refused there).  Levels on
// SELL-P / SELL-C / CSR-stream tiles are untouched.
//
// Kernels: sell_kernel / sello_kernel instantiated with VT = float (kernels.hpp) -- a value is widened to double in a register,
// which is exact, and enters the same v * g and s + pr in the same order: bit for bit the fp64 kernel on A~ (tested against a
// handle that is GIVEN the rounded matrices).  The cycle launches EPI_SWEEP (both gather forms, every x-update form) and EPI_SUB
// on a level matrix; those are the instantiations that exist.
//
// Refused (GMG_ERR_INVALID at gmg_setup): solver mode (the cycle's recurrence residual would converge to the solution of A~ x = b),
// a partitioned handle, a Galerkin level, a patch-corrected prolongation, any smoother but Richardson-Jacobi on a level that would
// be float32, and a nonzero value outside float32's normal range (no scaling is attempted).

bool gmg_solver::f32_stream(const DevCSR &M, bool cyc) const
{
  if (!M.sval32) return false;
  if (cyc) return true;
  REQUIRE(M.sval, GMG_ERR_STATE, "this level streams float32 values inside the cycle and has released its fp64 values (option values_f32): "
          "only level 0 keeps the fp64 operator");
  return false;
}

// what is refused before anything is built
void gmg_solver::f32_check() const
{
  if (!values_f32) return;
  const std::string why = "cycle_values = float32 (option values_f32): ";
  REQUIRE(mode == GMG_MODE_PRECONDITIONER, GMG_ERR_INVALID, why + "mode = solver is refused -- the cycle's recurrence residual would converge to the "
          "solution of the ROUNDED system; use the GMG as the preconditioner of a Krylov solver, which keeps A in fp64");
  bool part = comm.nranks > 1 || comm.kind != COMM_NONE;
  for (int l = 0; l < (int)lev.size(); ++l) part = part || lev[l].halo.present;
  REQUIRE(!part, GMG_ERR_INVALID, why + "a partitioned handle (communicator / gmg_set_partition) is refused");
  for (int l = 0; l < nlev; ++l) {
    REQUIRE(!lev[l].gal, GMG_ERR_INVALID, why + "level " + std::to_string(l) + " is a Galerkin level (gmg_set_galerkin), which is refused");
    if (l < nlev - 1) REQUIRE(!lev[l].has_pcorr, GMG_ERR_INVALID, why + "level " + std::to_string(l) + " has a patch-corrected prolongation "
                              "(PatchProlongationOperator), which is refused");
  }
}

static bool f32_jacobi_slot(const Smoother &S) { return S.kind == SM_JACOBI && !S.cheb && !S.pmult; }

// the float twin of A's value stream + 1/diag of the rounded matrix, from CSR-ordered fp64 values on the device (setup: A.val;
// numerical_setup!: the staged new values).  Allocates nothing.
void gmg_solver::f32_fill(DevCSR &A, const double *dval, double *dinv, int l, int &nzero)
{
  const int64_t n = A.nrows;
  HIP_CHECK(hipMemsetAsync(d_f32_flags, 0xff, sizeof(unsigned long long), stream));                 // bad row: none
  HIP_CHECK(hipMemsetAsync(d_f32_flags + 1, 0, sizeof(unsigned long long), stream));                // zero diagonals
  const int grid = (int)std::max<int64_t>(1, (n + 255) / 256);
  int *d_nzero = reinterpret_cast<int *>(d_f32_flags + 1);
  if (A.ptr64) hipLaunchKernelGGL((sell_fill_f32_kernel<int64_t>), dim3(grid), dim3(256), 0, stream, n, (const int64_t *)A.rowptr, A.soff, A.scol, dval, A.sval32, dinv, d_nzero, d_f32_flags);
  else hipLaunchKernelGGL((sell_fill_f32_kernel<int32_t>), dim3(grid), dim3(256), 0, stream, n, (const int32_t *)A.rowptr, A.soff, A.scol, dval, A.sval32, dinv, d_nzero, d_f32_flags);
  HIP_CHECK(hipGetLastError());
  unsigned long long flags[2] = {0, 0};
  HIP_CHECK(hipMemcpyAsync(flags, d_f32_flags, sizeof(flags), hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  REQUIRE(flags[0] == ~0ull, GMG_ERR_INVALID, "cycle_values = float32 (option values_f32): level " + std::to_string(l) + ", row " + std::to_string(flags[0]) +
          " stores a nonzero value outside float32's normal range (magnitude below 2^-126, or rounding to infinity); no scaling is attempted");
  int nz = 0;
  std::memcpy(&nz, &flags[1], sizeof(int));
  nzero = nz;
}

// setup, level l < nlev - 1, after the layout of L.A is chosen and L.dinv = 1 ./ diag(A) is built, before the CSR copy is dropped
void gmg_solver::f32_prepare(int l, int &nzero)
{
  Level &L = lev[l];
  DevCSR &A = L.A;
  if (!values_f32 || !A.sell || !(A.opat || A.explicit_values()) || !A.sval || !A.val || A.pat || A.vdict || A.comp_idx) return;
  const Smoother &post = L.post_shares_pre ? L.pre : L.post;
  REQUIRE(f32_jacobi_slot(L.pre) && f32_jacobi_slot(post), GMG_ERR_INVALID, "cycle_values = float32 (option values_f32): level " + std::to_string(l) +
          " would stream float32 values, where every smoother but RichardsonSmoother(JacobiLinearSolver(), ...) is refused");
  if (!d_f32_flags) d_f32_flags = dalloc<unsigned long long>(2);
  A.sval32 = dalloc<float>((size_t)A.zpad);
  HIP_CHECK(hipMemsetAsync(A.sval32, 0, sizeof(float) * (size_t)A.zpad, stream));                  // padding = 0.0f (masked by rowlen, never added)
  f32_fill(A, A.val, L.dinv, l, nzero);
  if (l > 0) release(A.sval, (size_t)A.zpad);                // nothing outside the cycle reads a coarser level's values
}

template <int EPI, bool ONEG>
void gmg_solver::launch_sell_f32(const DevCSR &M, const StreamArgs2 &a2)
{
  if constexpr (EPI == EPI_SWEEP || EPI == EPI_SUB) {
    SellArgs a;
    std::memset(&a, 0, sizeof(a));
    a.soff = M.soff; a.scol = M.scol; a.sval32 = M.sval32; a.rowlen = M.rowlen; a.nrows = M.nrows; a.nslices = M.nslices; a.xcd_remap = xcd_remap;
    take_stream_args(a, a2);
    const int wpb = sell_block > 0 ? sell_block / 64 : (M.nslices >= 256 * 32 ? 4 : 1);
    const dim3 g((M.nslices + wpb - 1) / wpb), b(64 * wpb);
    // non-temporal stream loads by the bytes of the float stream (8 B per padded entry), today's threshold; values_f32_nt overrides
    const bool huge = big_level(M);
    const int nt = f32_nt >= 0 ? f32_nt : ((nt_loads && (8.0 * (double)M.zpad > 192.0e6)) ? ((huge && nt_rowwise) ? 2 : 1) : 0);
    if (huge) a.xcd_remap = remap_for_big(M, 64 * wpb, (int)g.x);
    if constexpr (EPI == EPI_SWEEP && ONEG) {
      if (sell_un >= 6 && sell_un < 9 && (a2.xmode != 0 || nt == 2)) {
        M.note_sweep("sell_kernel<f32,EPI_SWEEP,ONEG,UN=6,NT=%d,XM=*> wpb=%d remap=%d", nt, wpb, a.xcd_remap);
        with_value<2, 1, 0>(nt, [&](auto NT) { with_value<1, 2, 0>(a2.xmode, [&](auto XM) {
          hipLaunchKernelGGL((sell_kernel<EPI_SWEEP, true, 6, NT(), XM(), float>), g, b, 0, stream, a); }); });
        HIP_CHECK(hipGetLastError());
        return;
      }
    }
    REQUIRE(a2.xmode == 0 || EPI != EPI_SWEEP, GMG_ERR_STATE, "deferred x update needs the default unroll of the SELL-64 sweep");
    const int un = sell_un >= 9 ? 9 : sell_un >= 6 ? 6 : 3;
    if (EPI == EPI_SWEEP) M.note_sweep("sell_kernel<f32,EPI_SWEEP,%s,UN=%d,NT=%d,XM=0> wpb=%d remap=%d", ONEG ? "ONEG" : "2G", un, nt ? 1 : 0, wpb, a.xcd_remap);
    with_value<9, 6, 3>(un, [&](auto UN) { with_value<1, 0>(nt ? 1 : 0, [&](auto NT) {
      hipLaunchKernelGGL((sell_kernel<EPI, ONEG, UN(), NT(), 0, float>), g, b, 0, stream, a); }); });
    HIP_CHECK(hipGetLastError());
  } else {
    (void)M; (void)a2;
    throw GmgError{GMG_ERR_STATE, "no float32 instantiation of this operator form: the cycle launches sweeps and r -= A dx on a level matrix"};
  }
}

template <int EPI, bool ONEG>
void gmg_solver::launch_sello_f32(const DevCSR &M, const StreamArgs2 &a2)
{
  if constexpr (EPI == EPI_SWEEP || EPI == EPI_SUB) {
    SellOArgs a;
    std::memset(&a, 0, sizeof(a));
    a.soff = M.soff; a.sval32 = M.sval32; a.rowlen = M.rowlen; a.rowpid = M.orowpid; a.rowbase = M.orowbase; a.poff = M.opoff;
    a.np = M.opat_np; a.W = M.opat_w; a.nrows = M.nrows; a.nslices = M.nslices; a.xcd_remap = xcd_remap;
    take_stream_args(a, a2);
    const int wpb = sell_block > 0 ? sell_block / 64 : (M.nslices >= 256 * 32 ? 4 : 1);
    const dim3 g((M.nslices + wpb - 1) / wpb), b(64 * wpb);
    const size_t lds = (size_t)M.opat_np * M.opat_w * 4;
    const bool huge = big_level(M);
    const int nt = f32_nt >= 0 ? f32_nt : ((nt_loads && (4.0 * (double)M.zpad > 128.0e6)) ? ((huge && nt_rowwise) ? 2 : 1) : 0);
    if (huge) a.xcd_remap = remap_for_big(M, 64 * wpb, (int)g.x);
    if constexpr (EPI == EPI_SWEEP && ONEG) {
      if (sell_un < 27 && (a2.xmode != 0 || nt == 2)) {
        M.note_sweep("sello_kernel<f32,EPI_SWEEP,ONEG,UN=9,NT=%d,XM=*> wpb=%d remap=%d", nt, wpb, a.xcd_remap);
        with_value<2, 1, 0>(nt, [&](auto NT) { with_value<1, 2, 0>(a2.xmode, [&](auto XM) {
          hipLaunchKernelGGL((sello_kernel<EPI_SWEEP, true, 9, NT(), XM(), float>), g, b, lds, stream, a); }); });
        HIP_CHECK(hipGetLastError());
        return;
      }
    }
    REQUIRE(a2.xmode == 0 || EPI != EPI_SWEEP, GMG_ERR_STATE, "deferred x update needs the default unroll of the SELL-O sweep");
    const int un = sell_un >= 9 ? 9 : 3;
    if (EPI == EPI_SWEEP) M.note_sweep("sello_kernel<f32,EPI_SWEEP,%s,UN=%d,NT=%d,XM=0> wpb=%d remap=%d", ONEG ? "ONEG" : "2G", un, nt ? 1 : 0, wpb, a.xcd_remap);
    with_value<9, 3>(un, [&](auto UN) { with_value<1, 0>(nt ? 1 : 0, [&](auto NT) {
      hipLaunchKernelGGL((sello_kernel<EPI, ONEG, UN(), NT(), 0, float>), g, b, lds, stream, a); }); });
    HIP_CHECK(hipGetLastError());
  } else {
    (void)M; (void)a2;
    throw GmgError{GMG_ERR_STATE, "no float32 instantiation of this operator form: the cycle launches sweeps and r -= A dx on a level matrix"};
  }
}

extern "C" int gmg_level_values(gmg_handle_t h, int lev, int *is_f32, double *cycle_stream_bytes_per_nnz)
{
  return guarded(h, [&] {
    check_ready(h);
    check_level(h, lev, false);
    REQUIRE(!h->inactive(lev), GMG_ERR_STATE, "this rank holds no part of that level (it lives on a rank subset, gmg_set_redistribution)");
    const DevCSR &A = h->lev[lev].A;
    const bool f32 = A.sval32 != nullptr;
    if (is_f32) *is_f32 = f32 ? 1 : 0;
    if (cycle_stream_bytes_per_nnz) {
      if (f32) *cycle_stream_bytes_per_nnz = A.opat ? 4.0 : 8.0;
      else *cycle_stream_bytes_per_nnz = (A.sell && (A.pat || A.vdict || A.comp_idx || A.opat)) ? A.stream_bytes_per_nnz : 12.0;
    }
  });
}
