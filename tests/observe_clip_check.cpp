// Host-side run of csrc/observe_clip.h (compiled with the host compiler alone by tests/test_observe_cpu.py).  Reads cases from
// standard input, one per line:  d kind level smooth  p_0 .. p_d (d numbers each)  c_0 .. c_d  -- and prints the 1 + d numbers
// (V, M_0 .. M_{d-1}) of glims_oc_observe with 17 significant digits, one line per case, for the comparison with
// tests/observe_common.py.
#include <cstdio>

#include "observe_clip.h"

template <int D>
static int run(int kind, double level, double smooth) {
  double p[D + 1][D], c[D + 1], out[D + 1];
  for (int i = 0; i < D + 1; ++i)
    for (int a = 0; a < D; ++a)
      if (std::scanf("%lf", &p[i][a]) != 1) return 1;
  for (int i = 0; i < D + 1; ++i)
    if (std::scanf("%lf", &c[i]) != 1) return 1;
  glims_oc_observe<D>(kind, level, smooth, p, c, out);
  for (int k = 0; k < D + 1; ++k) std::printf(k ? " %.17g" : "%.17g", out[k]);
  std::printf("\n");
  return 0;
}

int main() {
  int d, kind;
  double level, smooth;
  while (std::scanf("%d %d %lf %lf", &d, &kind, &level, &smooth) == 4) {
    if (d != 2 && d != 3) return 2;
    if (d == 2 ? run<2>(kind, level, smooth) : run<3>(kind, level, smooth)) return 3;
  }
  return 0;
}
