// Host-side run of glims_og_volume_grad (csrc/observe_grad.h) for tests/test_deformed_volume_cpu.py.  Reads cases from stdin, one
// per line:
//   d h p[0][0] .. p[d][d-1]
// and prints per case: glims_oc_volume(p), the (d+1) d cofactors d vol / d p[a][k] (vertex-major), and the (d+1) d central
// differences (vol(p + h e_ak) - vol(p - h e_ak)) / (2 h) of glims_oc_volume itself.  Built with the host compiler alone, plain
// and with -fsanitize=address,undefined.
#include <cstdio>

#include "observe_grad.h"

template <int D>
static int run_case(double h, const double* v) {
  constexpr int NV = D + 1;
  double p[NV][D], dv[NV][D];
  for (int a = 0; a < NV; ++a)
    for (int k = 0; k < D; ++k) p[a][k] = v[a * D + k];
  glims_og_volume_grad<D>(p, dv);
  printf("%.17g", glims_oc_volume<D>(p));
  for (int a = 0; a < NV; ++a)
    for (int k = 0; k < D; ++k) printf(" %.17g", dv[a][k]);
  for (int a = 0; a < NV; ++a)
    for (int k = 0; k < D; ++k) {
      const double keep = p[a][k];
      p[a][k] = keep + h;
      const double vp = glims_oc_volume<D>(p);
      p[a][k] = keep - h;
      const double vm = glims_oc_volume<D>(p);
      p[a][k] = keep;
      printf(" %.17g", (vp - vm) / (2.0 * h));
    }
  printf("\n");
  return 0;
}

int main() {
  int d;
  double h, v[12];
  while (scanf("%d %lf", &d, &h) == 2) {
    if (d != 2 && d != 3) return 2;
    for (int i = 0; i < (d + 1) * d; ++i)
      if (scanf("%lf", &v[i]) != 1) return 3;
    if (d == 2) run_case<2>(h, v);
    else run_case<3>(h, v);
  }
  return 0;
}
