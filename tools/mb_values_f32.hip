// tools/mb_values_f32.hip -- cycle_values = float32: how to keep bytes in flight when a lane's value load shrinks from 8 to 4 bytes.
// The fused one-gather sweep of the offset-pattern layout (sello_kernel<EPI_SWEEP, ONEG>) on a synthetic 27-point operator with
// distinct values, N^3 rows, in these forms:
//   f64 UN=9        the product's fp64 sweep (the reference time)
//   f32 UN=9        the same kernel with VT = float: the same number of loads in flight, half the bytes each
//   f32 UN=18 / 27  deeper unroll: 18 loads / the whole row in flight
//   f32 pair UN=9   a pair-interleaved slice layout -- entries (2k, 2k+1) of a row next to each other, one 8-byte load per pair,
//                   9 loads = 18 entries in flight (the slice width is rounded up to even; the summation order is unchanged)
// Every float form must give the bits of the fp64 kernel on the rounded values (checked on the first launch).
// Diagnostic only (not part of the product).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o mb_values_f32 tools/mb_values_f32.hip && ./mb_values_f32 [N=128] [reps=20] [nt=0]
#include "../gridapsolvers.jl_amd/csrc/kernels.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace gmg;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

// sello_kernel<EPI_SWEEP, true, UN, NT, 0, float> on the pair-interleaved stream: entry (j, lane) of a slice of (even) width w2 sits at
// 2 * soff[slice] ... base2 + (j / 2) * 128 + lane * 2 + (j % 2), so a lane fetches two consecutive entries with one 8-byte load
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int UN, int NT>
__global__ __launch_bounds__(kBlock) void sello_pair_kernel(SellOArgs a, const int64_t *__restrict__ soff2, const float2 *__restrict__ sval2_)
{
  const f32x2 *__restrict__ sval2 = reinterpret_cast<const f32x2 *>(sval2_);
  extern __shared__ double sp_smem[];
  int32_t *s_off = reinterpret_cast<int32_t *>(sp_smem);
  const int tot = a.np * a.W;
  for (int i = threadIdx.x; i < tot; i += blockDim.x) s_off[i] = a.poff[i];
  const int lane = threadIdx.x & 63;
  const int slice = __builtin_amdgcn_readfirstlane((int)(remap_block(blockIdx.x, gridDim.x, a.xcd_remap) * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const bool live = slice < a.nslices;
  const int sc = live ? slice : a.nslices - 1;
  const int64_t base = soff2[sc];                          // in float2 units
  const int wp = (int)((soff2[sc + 1] - base) >> 6);       // pairs per row
  const int64_t row = (int64_t)sc * 64 + lane;
  const bool valid = live && row < a.nrows;
  const int64_t rc = min(row, a.nrows - 1);
  const int len = valid ? a.rowlen[rc] : 0;
  const int pid = (int)a.rowpid[rc];
  const uint32_t base8 = 8u * (uint32_t)(a.rowbase ? a.rowbase[rc] : (int32_t)rc);
  const double *__restrict__ xg = a.x;
  const double omega = a.omega;
  const double e0 = a.b[rc], e1 = xg[rc], dinv_row = a.dinv[rc];
  const double xl = a.x2[rc], e2 = a.x_zero ? 0.0 : xl;
  __syncthreads();
  const f32x2 *vp = sval2 + base + lane;
  const int32_t *to = s_off + pid * a.W;
  double s = 0.0;
  int j = 0;
  auto batch = [&](auto K, int j0) {
    constexpr int M = decltype(K)::value;
    f32x2 vs[M];
    double g[2 * M];
#pragma unroll
    for (int u = 0; u < M; ++u) vs[u] = NT ? __builtin_nontemporal_load(vp + (int64_t)(j0 + u) * 64) : vp[(int64_t)(j0 + u) * 64];
#pragma unroll
    for (int u = 0; u < 2 * M; ++u) {
      const int jj = 2 * j0 + u;
      g[u] = ld_off(xg, base8 + (uint32_t)((jj < a.W) ? to[jj] : 0));
    }
#pragma unroll
    for (int u = 0; u < M; ++u) {
      const double p0 = (double)vs[u].x * g[2 * u], p1 = (double)vs[u].y * g[2 * u + 1];
      s = (2 * (j0 + u) < len) ? s + p0 : s;
      s = (2 * (j0 + u) + 1 < len) ? s + p1 : s;
    }
  };
  for (; j + UN <= wp; j += UN) batch(std::integral_constant<int, UN>{}, j);
  for (; j < wp; ++j) batch(std::integral_constant<int, 1>{}, j);
  if (valid) {
    const double rn = e0 - s;
    a.x2[row] = e2 + e1;
    a.y[row] = rn;
    a.s_out[row] = omega * (dinv_row * rn);
  }
}

static inline uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }
template <typename T> static T *up(const std::vector<T> &v)
{
  T *p = nullptr;
  CK(hipMalloc((void **)&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

int main(int argc, char **argv)
{
  const int N = argc > 1 ? atoi(argv[1]) : 128;
  const int reps = argc > 2 ? atoi(argv[2]) : 20;
  const int nt = argc > 3 ? atoi(argv[3]) : 0;
  const int64_t n = (int64_t)N * N * N, ns = (n + 63) / 64, W = 27, W2 = 14;
  const int64_t margin = (int64_t)N * N + N + 1;
  // one offset pattern (+ the empty one): the 27 neighbours, ascending; rows near the ends gather around a clamped base row
  std::vector<int32_t> poff((size_t)2 * W, 0), rowbase((size_t)n + 64), rowlen((size_t)n + 64, 27);
  {
    int q = 0;
    for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) poff[(size_t)q++] = 8 * (int32_t)(dz * N * N + dy * N + dx);
  }
  for (int64_t i = 0; i < n + 64; ++i) rowbase[(size_t)i] = (int32_t)std::min(std::max(i, margin), n - 1 - margin);
  std::vector<uint16_t> rowpid((size_t)n + 64, 0);
  std::vector<int64_t> soff((size_t)ns + 1), soff2((size_t)ns + 1);
  for (int64_t s = 0; s <= ns; ++s) { soff[(size_t)s] = s * 64 * W; soff2[(size_t)s] = s * 64 * W2; }
  std::vector<double> v64((size_t)(ns * 64 * W)), v64r(v64.size());
  std::vector<float> v32(v64.size());
  std::vector<float2> v32p((size_t)(ns * 64 * W2), make_float2(0.f, 0.f));
  for (int64_t s = 0; s < ns; ++s)
    for (int64_t j = 0; j < W; ++j)
      for (int l = 0; l < 64; ++l) {
        const int64_t q = s * 64 * W + j * 64 + l;
        const double v = (j == 13 ? 2.6 : -0.1) * (1.0 + 0.25 * (double)(mix((uint64_t)q + 99) >> 11) * 0x1.0p-53);
        v64[(size_t)q] = v; v32[(size_t)q] = (float)v; v64r[(size_t)q] = (double)(float)v;
        float2 &p = v32p[(size_t)(s * 64 * W2 + (j / 2) * 64 + l)];
        if (j & 1) p.y = (float)v; else p.x = (float)v;
      }
  std::vector<double> r0((size_t)n + 64), s0((size_t)n + 64), dinv((size_t)n + 64, 1.0 / 2.6);
  for (int64_t i = 0; i < n + 64; ++i) { r0[(size_t)i] = 1e-3 * ((double)(mix((uint64_t)i) >> 11) * 0x1.0p-53 - 0.5); s0[(size_t)i] = (2.0 / 3.0) * (dinv[(size_t)i] * r0[(size_t)i]); }
  int64_t *d_soff = up(soff), *d_soff2 = up(soff2);
  double *d_v64 = up(v64), *d_v64r = up(v64r);
  float *d_v32 = up(v32);
  float2 *d_v32p = up(v32p);
  int32_t *d_poff = up(poff), *d_rowbase = up(rowbase), *d_rowlen = up(rowlen);
  uint16_t *d_rowpid = up(rowpid);
  double *d_dinv = up(dinv), *d_s0 = up(s0), *d_r = up(r0), *d_x = up(r0), *d_s1 = up(r0);
  SellOArgs a;
  std::memset(&a, 0, sizeof(a));
  a.soff = d_soff; a.rowlen = d_rowlen; a.rowpid = d_rowpid; a.rowbase = d_rowbase; a.poff = d_poff; a.np = 2; a.W = (int)W;
  a.nrows = n; a.nslices = (int)ns; a.xcd_remap = 1; a.x = d_s0; a.dinv = d_dinv; a.omega = 2.0 / 3.0; a.y = d_r; a.b = d_r; a.x2 = d_x; a.s_out = d_s1;
  const int wpb = ns >= 256 * 32 ? 4 : 1;
  const dim3 g((unsigned)((ns + wpb - 1) / wpb)), b(64 * wpb);
  const size_t lds = (size_t)2 * W * 4;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<double> ref;
  printf("N = %d: %lld rows, %lld padded entries; value stream %.1f MB fp64, %.1f MB float, %.1f MB float pairs; row-wise vectors %.1f MB; NT = %d\n", N,
         (long long)n, (long long)(ns * 64 * W), 8e-6 * ns * 64 * W, 4e-6 * ns * 64 * W, 8e-6 * ns * 64 * W2, 1e-6 * 56.0 * n, nt);
  auto run = [&](const char *name, double stream_bytes, bool is_ref, auto &&launch) {
    std::vector<float> ms;
    for (int r = 0; r < reps + 1; ++r) {
      if (r == 0) { CK(hipMemcpy(d_r, r0.data(), sizeof(double) * r0.size(), hipMemcpyHostToDevice)); CK(hipMemset(d_x, 0, sizeof(double) * r0.size())); }
      CK(hipEventRecord(e0));
      launch();
      CK(hipGetLastError());
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float t = 0;
      CK(hipEventElapsedTime(&t, e0, e1));
      if (r > 0) ms.push_back(t);
      if (r == 0) {
        std::vector<double> out((size_t)n);
        CK(hipMemcpy(out.data(), d_r, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        if (is_ref) ref = out;
        else printf("  %-16s bits vs the fp64 kernel on the rounded values: %s\n", name, std::memcmp(out.data(), ref.data(), sizeof(double) * (size_t)n) == 0 ? "equal" : "DIFFER");
      }
    }
    std::sort(ms.begin(), ms.end());
    const double bytes = stream_bytes + 56.0 * (double)n + 6.0 * (double)n;
    printf("  %-16s median %8.1f us  min %8.1f  max %8.1f   %7.1f MB per launch, %6.0f GB/s at the median\n", name, 1e3 * ms[ms.size() / 2], 1e3 * ms.front(),
           1e3 * ms.back(), 1e-6 * bytes, bytes / (ms[ms.size() / 2] * 1e6));
  };
  const double z = (double)(ns * 64 * W);
#define LAUNCH(UN, VT) [&] { if (nt) hipLaunchKernelGGL((sello_kernel<EPI_SWEEP, true, UN, 1, 0, VT>), g, b, lds, 0, a); \
                             else hipLaunchKernelGGL((sello_kernel<EPI_SWEEP, true, UN, 0, 0, VT>), g, b, lds, 0, a); }
  a.sval = d_v64; run("f64 UN=9", 8.0 * z, true, LAUNCH(9, double));
  a.sval = d_v64r; run("f64 UN=9 rounded", 8.0 * z, true, LAUNCH(9, double));   // (the reference bits of the float forms)
  a.sval = nullptr; a.sval32 = d_v32;
  run("f32 UN=9", 4.0 * z, false, LAUNCH(9, float));
  run("f32 UN=18", 4.0 * z, false, LAUNCH(18, float));
  run("f32 UN=27", 4.0 * z, false, LAUNCH(27, float));
  run("f32 pair UN=9", 8.0 * (double)(ns * 64 * W2), false, [&] {
    if (nt) hipLaunchKernelGGL((sello_pair_kernel<9, 1>), g, b, lds, 0, a, d_soff2, d_v32p);
    else hipLaunchKernelGGL((sello_pair_kernel<9, 0>), g, b, lds, 0, a, d_soff2, d_v32p);
  });
  run("f32 pair UN=14", 8.0 * (double)(ns * 64 * W2), false, [&] {
    if (nt) hipLaunchKernelGGL((sello_pair_kernel<14, 1>), g, b, lds, 0, a, d_soff2, d_v32p);
    else hipLaunchKernelGGL((sello_pair_kernel<14, 0>), g, b, lds, 0, a, d_soff2, d_v32p);
  });
  run("f32 UN=9 again", 4.0 * z, false, LAUNCH(9, float));
  return 0;
}
