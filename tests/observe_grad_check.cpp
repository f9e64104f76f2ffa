// Host-side run of csrc/observe_grad.h (compiled with the host compiler alone by tests/test_observable_terms_cpu.py, once plainly
// and once with the address and undefined-behaviour sanitizers).  Reads cases from standard input, one per line:
//   d kind level smooth  c_0 .. c_d  dc_0 .. dc_d
// and prints, with 17 significant digits, one line per case:  b0  g_0 .. g_d  Hd_0 .. Hd_d  n_in  -- the fraction V_T / |T|, its
// gradient by the vertex values, its second derivative applied to dc (zeros for SHARP) and the in-count (-1 unless SHARP), for
// the comparison with tests/observable_terms_common.py.
#include <cstdio>

#include "observe_grad.h"

template <int D>
static int run(int kind, double level, double smooth) {
  double c[D + 1], dc[D + 1], g[D + 1], Hd[D + 1], b0 = 0.0;
  for (int i = 0; i < D + 1; ++i)
    if (std::scanf("%lf", &c[i]) != 1) return 1;
  for (int i = 0; i < D + 1; ++i)
    if (std::scanf("%lf", &dc[i]) != 1) return 1;
  const int n_in = glims_og_cell<D>(kind, level, smooth, c, &b0, g, dc, Hd);
  std::printf("%.17g", b0);
  for (int k = 0; k < D + 1; ++k) std::printf(" %.17g", g[k]);
  for (int k = 0; k < D + 1; ++k) std::printf(" %.17g", Hd[k]);
  std::printf(" %d\n", n_in);
  return 0;
}

int main() {
  int d, kind;
  double level, smooth;
  while (std::scanf("%d %d %lf %lf", &d, &kind, &level, &smooth) == 4) {
    if (d != 2 && d != 3) return 2;
    if (kind < GLIMS_OC_MASS || kind > GLIMS_OC_SMOOTH) return 4;
    if (d == 2 ? run<2>(kind, level, smooth) : run<3>(kind, level, smooth)) return 3;
  }
  return 0;
}
