// Stand-alone driver of ArnoldiLSQ (csrc/krylov_small.hpp) for tests/test_arnoldi_small_host.py: host C++ only, no HIP.
// stdin:  cap0 grow m beta, then for j = 1..m the j + 1 entries H[1..j+1, j] (anything strtod reads: hex floats, inf).
// The capacity follows the cores' rule: columns m_cap = cap0 - 1, m_cap += grow when j outgrows it, reserve(m_cap + 1).
// stdout: one "name index value" line per number, values as hex floats (%a):
//   beta j      what close_column(j) returned            c j, s j    rotation j
//   g i         g after the last column (i = 0..m)       r i j       the rotated H (upper triangle and the zeroed sub-diagonal)
//   y i         g[0..m-1] after solve(m)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../gridapsolvers.jl_amd/csrc/krylov_small.hpp"

static double next_number()
{
  char buf[128];
  if (std::scanf("%127s", buf) != 1) { std::fprintf(stderr, "arnoldi_small_main: input ended early\n"); std::exit(2); }
  char *end = nullptr;
  const double v = std::strtod(buf, &end);
  if (end == buf || *end) { std::fprintf(stderr, "arnoldi_small_main: not a number: %s\n", buf); std::exit(2); }
  return v;
}

int main()
{
  const int cap0 = (int)next_number(), grow = (int)next_number(), m = (int)next_number();
  const double beta = next_number();
  if (cap0 < 2 || grow < 1 || m < 1) { std::fprintf(stderr, "arnoldi_small_main: bad sizes\n"); return 2; }
  ArnoldiLSQ lsq(cap0);
  lsq.reset(beta);
  int mcap = cap0 - 1;
  for (int j = 1; j <= m; ++j) {
    if (j > mcap) mcap += grow;
    lsq.reserve(mcap + 1);
    for (int i = 1; i <= j + 1; ++i) lsq.H(i, j) = next_number();
    std::printf("beta %d %a\n", j, lsq.close_column(j));
  }
  for (int j = 1; j <= m; ++j) std::printf("c %d %a\ns %d %a\n", j, lsq.c[(size_t)j - 1], j, lsq.s[(size_t)j - 1]);
  for (int i = 0; i <= m; ++i) std::printf("g %d %a\n", i, lsq.g[(size_t)i]);
  for (int j = 1; j <= m; ++j)
    for (int i = 1; i <= j + 1; ++i) std::printf("r %d,%d %a\n", i, j, lsq.H(i, j));
  lsq.solve(m);
  for (int i = 0; i < m; ++i) std::printf("y %d %a\n", i, lsq.g[(size_t)i]);
  return 0;
}
