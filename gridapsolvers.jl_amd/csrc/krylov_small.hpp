// The small dense part of the Krylov solvers: the Givens rotation and the Hessenberg least-squares problem of (F)GMRES.
// Plain C++17 without HIP headers, so a host program can include and test it on its own (tests/host/arnoldi_small_main.cpp);
// under hipcc the two free functions are also device functions (minres_update_kernel forms its rotation with givens_lapack).
#pragma once

#include <math.h>
#include <algorithm>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__)
#define GMG_HOST_DEVICE __host__ __device__
#else
#define GMG_HOST_DEVICE
#endif

// LinearAlgebra.givensAlgorithm(f, g) -> (c, s, r): the LAPACK dlartg form Julia ships (safmn2 rescaling, r scaled back, the sign
// rule flipping c, s and r together).  jl_max is Julia's max (NaN if either is NaN), not fmax.
GMG_HOST_DEVICE inline double jl_max(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }
GMG_HOST_DEVICE inline void givens_lapack(double f, double g, double &cs, double &sn, double &r)
{
  const double safmn2 = 0x1p-485, safmx2 = 1.0 / safmn2;        // floatmin2(Float64) = reinterpret(Float64, 0x21a0000000000000)
  if (g == 0.0) { cs = 1.0; sn = 0.0; r = f; return; }
  if (f == 0.0) { cs = 0.0; sn = 1.0; r = g; return; }
  double f1 = f, g1 = g, scale = jl_max(fabs(f1), fabs(g1));
  if (scale >= safmx2) {
    int count = 0;
    do { ++count; f1 *= safmn2; g1 *= safmn2; scale = jl_max(fabs(f1), fabs(g1)); } while (!(scale < safmx2 || count >= 20));
    r = sqrt(f1 * f1 + g1 * g1); cs = f1 / r; sn = g1 / r;
    for (int i = 0; i < count; ++i) r *= safmx2;
  } else if (scale <= safmn2) {
    int count = 0;
    do { ++count; f1 *= safmx2; g1 *= safmx2; scale = jl_max(fabs(f1), fabs(g1)); } while (!(scale > safmn2));
    r = sqrt(f1 * f1 + g1 * g1); cs = f1 / r; sn = g1 / r;
    for (int i = 0; i < count; ++i) r *= safmn2;
  } else {
    r = sqrt(f1 * f1 + g1 * g1); cs = f1 / r; sn = g1 / r;
  }
  if (fabs(f) > fabs(g) && cs < 0.0) { cs = -cs; sn = -sn; r = -r; }
}

// H, g, c and s of FGMRESSolvers.jl:58-70 / GMRESSolvers.jl:57-69: H is (cap + 1) x cap like the reference's caches (column-major,
// 1-based accessor), rotated in place column by column, so that the least-squares problem min |beta e1 - H y| is a triangular solve.
struct ArnoldiLSQ {
  int hcap, ldh;                                           // rows of H = columns + 1 ; leading dimension
  std::vector<double> Hv, g, c, s;
  explicit ArnoldiLSQ(int cap)
    : hcap(cap), ldh(cap + 1), Hv((size_t)ldh * hcap, 0.0), g((size_t)hcap + 1, 0.0), c((size_t)hcap, 0.0), s((size_t)hcap, 0.0) {}
  double &H(int i, int j) { return Hv[(size_t)(i - 1) + (size_t)(j - 1) * ldh]; }
  // fill!(H,0) ; fill!(g,0) ; g[1] = beta (FGMRESSolvers.jl:147-148, GMRESSolvers.jl:150-151)
  void reset(double beta)
  {
    std::fill(Hv.begin(), Hv.end(), 0.0);
    std::fill(g.begin(), g.end(), 0.0); g[0] = beta;
  }
  // expand_krylov_caches! (FGMRESSolvers.jl:77-94, GMRESSolvers.jl:76-92): the old entries stay
  void reserve(int newcap)
  {
    if (newcap <= hcap) return;
    const int nld = newcap + 1;
    std::vector<double> H2((size_t)nld * newcap, 0.0);
    for (int jj = 0; jj < hcap; ++jj)
      for (int ii = 0; ii < ldh; ++ii) H2[(size_t)ii + (size_t)jj * nld] = Hv[(size_t)ii + (size_t)jj * ldh];
    Hv.swap(H2);
    g.resize((size_t)newcap + 1, 0.0); c.resize((size_t)newcap, 0.0); s.resize((size_t)newcap, 0.0);
    hcap = newcap; ldh = nld;
  }
  // Column j holds H[1..j+1, j]: apply rotations 1..j-1, form rotation j, update g; returns the new residual norm |g[j+1]|.
  // Line numbers: FGMRESSolvers.jl / GMRESSolvers.jl.
  double close_column(int j)
  {
    for (int i = 1; i <= j - 1; ++i) {                     // :168-172 / :170-174
      const double gm = c[i - 1] * H(i, j) + s[i - 1] * H(i + 1, j);
      H(i + 1, j) = -s[i - 1] * H(i, j) + c[i - 1] * H(i + 1, j);
      H(i, j) = gm;
    }
    double rr;
    givens_lapack(H(j, j), H(j + 1, j), c[j - 1], s[j - 1], rr);                 // :175 / :177 LinearAlgebra.givensAlgorithm
    H(j, j) = c[j - 1] * H(j, j) + s[j - 1] * H(j + 1, j); H(j + 1, j) = 0.0;     // :176 / :178
    g[j] = -s[j - 1] * g[j - 1]; g[j - 1] = c[j - 1] * g[j - 1];                  // :177 / :179
    return fabs(g[j]);                                     // :179 / :181
  }
  // back-substitution with the j closed columns: g[0..j-1] becomes y (:186-188 / :188-190)
  void solve(int j)
  {
    for (int i = j; i >= 1; --i) {
      double acc = 0.0;
      for (int k = i + 1; k <= j; ++k) acc += H(i, k) * g[k - 1];
      g[i - 1] = (g[i - 1] - acc) / H(i, i);
    }
  }
};
