// Host-side run of the first-moment templates of csrc/observe_grad.h (compiled with the host compiler alone by
// tests/test_com_terms_cpu.py, once plainly and once with the address and undefined-behaviour sanitizers).  Reads cases from
// standard input, one per line:
//   d kind level smooth  c_0 .. c_d  psi_0 .. psi_d
// and prints, with 17 significant digits, one line per case:  b_0 .. b_{d+1}  g_0 .. g_d  n_in  o_0 .. o_{d+1}  -- the values
// b of glims_og_moment_*, the contraction g_i = sum_m psi_m d b_{1+m} / d c_i, the in-count (-1 unless SHARP) and the values o
// that observe_clip.h's glims_oc_* give for the same case (what b must equal, and what the test differences).
#include <cstdio>

#include "observe_grad.h"

template <int D>
static int run(int kind, double level, double smooth) {
  double c[D + 1], psi[D + 1], g[D + 1], b[D + 2], o[D + 2];
  for (int i = 0; i < D + 1; ++i)
    if (std::scanf("%lf", &c[i]) != 1) return 1;
  for (int i = 0; i < D + 1; ++i)
    if (std::scanf("%lf", &psi[i]) != 1) return 1;
  const int n_in = glims_og_moment_cell<D>(kind, level, smooth, c, psi, b, g);
  if (kind == GLIMS_OC_MASS) glims_oc_mass<D>(c, o);
  else if (kind == GLIMS_OC_SHARP) glims_oc_sharp<D>(level, c, o);
  else if constexpr (D == 2) glims_oc_smooth<2, GLIMS_DQ2_N>(level, smooth, c, glims_dq2_lam, glims_dq2_w, o);
  else glims_oc_smooth<3, GLIMS_DQ3_N>(level, smooth, c, glims_dq3_lam, glims_dq3_w, o);
  for (int k = 0; k < D + 2; ++k) std::printf("%s%.17g", k ? " " : "", b[k]);
  for (int k = 0; k < D + 1; ++k) std::printf(" %.17g", g[k]);
  std::printf(" %d", n_in);
  for (int k = 0; k < D + 2; ++k) std::printf(" %.17g", o[k]);
  std::printf("\n");
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
