// tools/mb_refill.hip -- numerical_setup!'s device refill (new values into an existing SELL-64 layout + D^-1) taken apart:
// the product's sell_refill_kernel (one lane per row, the row walked serially) against two slice-cooperative forms,
//   slots  one wave per 64-row slice, the slice's columns walked wave-uniformly, UN independent loads per lane in flight,
//          the diagonal in a second pass over the (4-byte) columns;
//   lds    one wave per slice, the slice's contiguous CSR value range read with consecutive lanes on consecutive addresses
//          into LDS in chunks of CH entries, then written to the slots from LDS.
// Diagnostic only (not part of the product).  Every variant's sval and D^-1 are compared bit for bit with the product kernel's.
// Matrices (synthetic, built on the host; every value distinct, the diagonal present):
//   q2v    rows of 100..250 entries (a Q2 vector-valued velocity block), n rows
//   q1     27 entries per row (the Poisson levels the product kernel was written for)
//   rag    0..60 entries per row, about one row in seven empty, n not a multiple of 64 (no D^-1: rectangular blocks)
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o mb_refill tools/mb_refill.hip && ./mb_refill [case=q2v] [n=200000] [reps=5]
#include "../gridapsolvers.jl_amd/csrc/kernels.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace gmg;
__device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

template <typename PtrT, int UN>
__global__ __launch_bounds__(256) void refill_slots_kernel(int64_t nrows, int64_t nslices, const PtrT *__restrict__ rowptr,
                                                           const int64_t *__restrict__ soff, const int32_t *__restrict__ scol,
                                                           const double *__restrict__ val, double *__restrict__ sval,
                                                           double *__restrict__ dinv, int *__restrict__ nzero)
{
  const int lane = threadIdx.x & 63;
  const int64_t sl = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (sl >= nslices) return;
  const int64_t base = soff[sl] + lane;
  const int64_t w = (soff[sl + 1] - soff[sl]) >> 6;
  const int64_t i = sl * 64 + lane;
  int64_t k0 = 0, len = 0;
  if (i < nrows) { k0 = (int64_t)rowptr[i]; len = (int64_t)rowptr[i + 1] - k0; }
  for (int64_t j = 0; j < w; j += UN) {
    double v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) v[u] = (j + u < len) ? val[k0 + j + u] : 0.0;
#pragma unroll
    for (int u = 0; u < UN; ++u)
      if (j + u < len) sval[base + (j + u) * 64] = v[u];
  }
  if (dinv && i < nrows) {
    double d = 0.0;
    for (int64_t j = 0; j < len; ++j)
      if (scol[base + j * 64] == (int32_t)i) d += val[k0 + j];
    if (d == 0.0) atomicAdd(nzero, 1);
    dinv[i] = 1.0 / d;
  }
}

template <typename PtrT, int CH>
__global__ __launch_bounds__(64) void refill_lds_kernel(int64_t nrows, int64_t nslices, const PtrT *__restrict__ rowptr,
                                                        const int64_t *__restrict__ soff, const int32_t *__restrict__ scol,
                                                        const double *__restrict__ val, double *__restrict__ sval,
                                                        double *__restrict__ dinv, int *__restrict__ nzero)
{
  __shared__ double stage[CH];
  const int lane = threadIdx.x;
  const int64_t sl = blockIdx.x;
  const int64_t base = soff[sl] + lane;
  const int64_t i = sl * 64 + lane;
  const int64_t ilast = imin(sl * 64 + 64, nrows);
  const int64_t c_begin = (int64_t)rowptr[sl * 64], c_end = (int64_t)rowptr[ilast];
  int64_t k0 = c_end, len = 0;
  if (i < nrows) { k0 = (int64_t)rowptr[i]; len = (int64_t)rowptr[i + 1] - k0; }
  double d = 0.0;
  for (int64_t c0 = c_begin; c0 < c_end; c0 += CH) {
    const int64_t cn = imin((int64_t)CH, c_end - c0);
    for (int64_t t = lane; t < cn; t += 64) stage[t] = val[c0 + t];
    __syncthreads();
    // this lane's entries inside the chunk: j in [ja, jb)
    const int64_t ja = imax(k0, c0) - k0, jb = imin(k0 + len, c0 + cn) - k0;
    int64_t jlo = ja < jb ? ja : INT64_MAX, jhi = ja < jb ? jb : 0;
    for (int m = 32; m > 0; m >>= 1) {
      jlo = imin(jlo, (int64_t)__shfl_xor((long long)jlo, m));
      jhi = imax(jhi, (int64_t)__shfl_xor((long long)jhi, m));
    }
    for (int64_t j = jlo; j < jhi; ++j)
      if (j >= ja && j < jb) {
        const double v = stage[k0 + j - c0];
        sval[base + j * 64] = v;
        if (dinv && scol[base + j * 64] == (int32_t)i) d += v;
      }
    __syncthreads();
  }
  if (dinv && i < nrows) {
    if (d == 0.0) atomicAdd(nzero, 1);
    dinv[i] = 1.0 / d;
  }
}

struct Host {
  int64_t n = 0, ncols = 0;
  std::vector<int64_t> ptr, soff;
  std::vector<int32_t> col, scol;
  std::vector<double> val, sval0;
};

static inline uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }

static Host build(const std::string &cs, int64_t n)
{
  Host H;
  H.n = n; H.ncols = n;
  H.ptr.assign((size_t)n + 1, 0);
  std::vector<int64_t> len((size_t)n), start((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t l = cs == "q2v" ? 100 + (int64_t)(mix((uint64_t)i) % 151) : cs == "q1" ? 27 : (mix((uint64_t)i) % 7 == 0 ? 0 : (int64_t)(mix((uint64_t)i * 3 + 1) % 61));
    l = std::min(l, n);
    len[(size_t)i] = l;
    start[(size_t)i] = std::max<int64_t>(0, std::min(i - l / 2, n - l));
    H.ptr[(size_t)i + 1] = H.ptr[(size_t)i] + l;
  }
  const int64_t nnz = H.ptr[(size_t)n];
  H.col.resize((size_t)nnz); H.val.resize((size_t)nnz);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < len[(size_t)i]; ++j) {
      const int64_t k = H.ptr[(size_t)i] + j;
      H.col[(size_t)k] = (int32_t)(start[(size_t)i] + j);
      H.val[(size_t)k] = 1.0 + (double)(mix((uint64_t)k + 12345) >> 11) * 0x1.0p-53;
    }
  const int64_t ns = (n + 63) / 64;
  H.soff.assign((size_t)ns + 1, 0);
  for (int64_t s = 0; s < ns; ++s) {
    int64_t w = 0;
    for (int64_t i = s * 64; i < std::min(n, s * 64 + 64); ++i) w = std::max(w, len[(size_t)i]);
    H.soff[(size_t)s + 1] = H.soff[(size_t)s] + 64 * w;
  }
  // what set-up leaves in the slices: padded slots carry the row's first column and 0.0 (sell_build_kernel); the values are stale (-1)
  H.scol.assign((size_t)H.soff[(size_t)ns], 0); H.sval0.assign((size_t)H.soff[(size_t)ns], 0.0);
  for (int64_t s = 0; s < ns; ++s) {
    const int64_t w = (H.soff[(size_t)s + 1] - H.soff[(size_t)s]) / 64;
    for (int l = 0; l < 64; ++l) {
      const int64_t i = s * 64 + l;
      for (int64_t j = 0; j < w; ++j) {
        const int64_t q = H.soff[(size_t)s] + 64 * j + l;
        if (i < n && j < len[(size_t)i]) { H.scol[(size_t)q] = H.col[(size_t)(H.ptr[(size_t)i] + j)]; H.sval0[(size_t)q] = -1.0; }
        else H.scol[(size_t)q] = (i < n && len[(size_t)i] > 0) ? H.col[(size_t)H.ptr[(size_t)i]] : 0;
      }
    }
  }
  return H;
}

template <typename T> static T *up(const std::vector<T> &v, size_t pad = 0)
{
  T *p = nullptr;
  CK(hipMalloc((void **)&p, std::max<size_t>(v.size() + pad, 1) * sizeof(T)));
  if (!v.empty()) CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return p;
}

int main(int argc, char **argv)
{
  const std::string cs = argc > 1 ? argv[1] : "q2v";
  const int64_t n = argc > 2 ? atoll(argv[2]) : 200000;
  const int reps = argc > 3 ? atoi(argv[3]) : 5;
  Host H = build(cs, n);
  const int64_t nnz = H.ptr.back(), ns = (n + 63) / 64, zp = H.soff.back();
  const bool want_dinv = cs != "rag";
  printf("case %s: %lld rows, %lld nnz, %lld slices, %lld padded slots (%.2f x), D^-1 %s\n", cs.c_str(), (long long)n, (long long)nnz,
         (long long)ns, (long long)zp, (double)zp / (double)std::max<int64_t>(nnz, 1), want_dinv ? "yes" : "no");
  std::vector<int32_t> p32(H.ptr.begin(), H.ptr.end());
  int32_t *d_p32 = up(p32);
  int64_t *d_p64 = up(H.ptr), *d_soff = up(H.soff);
  int32_t *d_scol = up(H.scol);
  double *d_val = up(H.val), *d_sval = up(H.sval0), *d_dinv = nullptr;
  int *d_nzero = nullptr;
  CK(hipMalloc((void **)&d_dinv, sizeof(double) * (size_t)std::max<int64_t>(n, 1)));
  CK(hipMalloc((void **)&d_nzero, sizeof(int)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<double> ref_sval, ref_dinv;
  const double bytes = 8.0 * nnz * 2 + 4.0 * nnz + 16.0 * n;     // val in, sval out, scol in (the diagonal), row pointers + D^-1
  auto run = [&](const char *name, int ptr64, auto &&launch) {
    std::vector<float> ms;
    for (int r = 0; r < reps + 1; ++r) {                          // the first one warms up and is checked
      CK(hipMemcpy(d_sval, H.sval0.data(), sizeof(double) * H.sval0.size(), hipMemcpyHostToDevice));
      CK(hipMemset(d_dinv, 0, sizeof(double) * (size_t)n));
      CK(hipMemset(d_nzero, 0, sizeof(int)));
      CK(hipEventRecord(e0));
      launch(want_dinv ? d_dinv : nullptr);
      CK(hipGetLastError());
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float t = 0;
      CK(hipEventElapsedTime(&t, e0, e1));
      if (r > 0) ms.push_back(t);
      if (r == 0) {
        std::vector<double> sv(H.sval0.size()), dv((size_t)n);
        CK(hipMemcpy(sv.data(), d_sval, sizeof(double) * sv.size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(dv.data(), d_dinv, sizeof(double) * dv.size(), hipMemcpyDeviceToHost));
        int nz = 0;
        CK(hipMemcpy(&nz, d_nzero, sizeof(int), hipMemcpyDeviceToHost));
        if (ref_sval.empty() && ref_dinv.empty()) { ref_sval = sv; ref_dinv = dv; }
        const bool same = std::memcmp(sv.data(), ref_sval.data(), sizeof(double) * sv.size()) == 0 &&
                          std::memcmp(dv.data(), ref_dinv.data(), sizeof(double) * dv.size()) == 0;
        printf("  %-26s ptr%d  bits %s  nzero %d\n", name, ptr64 ? 64 : 32, same ? "equal" : "DIFFER", nz);
      }
    }
    std::sort(ms.begin(), ms.end());
    printf("  %-26s ptr%d  median %8.3f ms  min %8.3f  max %8.3f  (%6.1f GB/s at the median)\n", name, ptr64 ? 64 : 32, ms[ms.size() / 2],
           ms.front(), ms.back(), bytes / (ms[ms.size() / 2] * 1e6));
  };
  const int grid_rows = (int)std::max<int64_t>(1, (n + 255) / 256), grid_sl4 = (int)std::max<int64_t>(1, (ns + 3) / 4);
  for (int p64 = 0; p64 < 2; ++p64) {
#define ARGS(P) n, ns, (const P *)(p64 ? (void *)d_p64 : (void *)d_p32), d_soff, d_scol, d_val, d_sval, dinv, d_nzero
    run("product (lane per row)", p64, [&](double *dinv) {
      if (p64) hipLaunchKernelGGL((sell_refill_kernel<int64_t>), dim3(grid_rows), dim3(256), 0, 0, n, d_p64, d_soff, d_scol, d_val, d_sval, dinv, d_nzero);
      else hipLaunchKernelGGL((sell_refill_kernel<int32_t>), dim3(grid_rows), dim3(256), 0, 0, n, d_p32, d_soff, d_scol, d_val, d_sval, dinv, d_nzero);
    });
    run("slots UN=4", p64, [&](double *dinv) {
      if (p64) hipLaunchKernelGGL((refill_slots_kernel<int64_t, 4>), dim3(grid_sl4), dim3(256), 0, 0, ARGS(int64_t));
      else hipLaunchKernelGGL((refill_slots_kernel<int32_t, 4>), dim3(grid_sl4), dim3(256), 0, 0, ARGS(int32_t));
    });
    run("slots UN=8", p64, [&](double *dinv) {
      if (p64) hipLaunchKernelGGL((refill_slots_kernel<int64_t, 8>), dim3(grid_sl4), dim3(256), 0, 0, ARGS(int64_t));
      else hipLaunchKernelGGL((refill_slots_kernel<int32_t, 8>), dim3(grid_sl4), dim3(256), 0, 0, ARGS(int32_t));
    });
    run("lds CH=2048", p64, [&](double *dinv) {
      if (p64) hipLaunchKernelGGL((refill_lds_kernel<int64_t, 2048>), dim3((unsigned)ns), dim3(64), 0, 0, ARGS(int64_t));
      else hipLaunchKernelGGL((refill_lds_kernel<int32_t, 2048>), dim3((unsigned)ns), dim3(64), 0, 0, ARGS(int32_t));
    });
    run("lds CH=6144", p64, [&](double *dinv) {
      if (p64) hipLaunchKernelGGL((refill_lds_kernel<int64_t, 6144>), dim3((unsigned)ns), dim3(64), 0, 0, ARGS(int64_t));
      else hipLaunchKernelGGL((refill_lds_kernel<int32_t, 6144>), dim3((unsigned)ns), dim3(64), 0, 0, ARGS(int32_t));
    });
#undef ARGS
  }
  return 0;
}
