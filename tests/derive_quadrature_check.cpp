// Host-side check of csrc/derive_quadrature.h (compiled with the host compiler alone by tests/test_derive_cpu.py): the weights sum
// to 1 and the rule integrates every monomial lambda^alpha of degree <= 7 over the reference simplex to
// d! prod(alpha_i!) / (d + |alpha|)! (the integral with respect to the measure normalised to 1) within 1e-15.  Then it prints
// every point and weight with 17 significant digits, for the comparison with simplex_quadrature(d, 4).
#include <cmath>
#include <cstdio>

#include "derive_quadrature.h"

static double factorial(int n) {
  double f = 1.0;
  for (int k = 2; k <= n; ++k) f *= k;
  return f;
}

template <int NV, int NQ>
static int check(const double (&lam)[NQ][NV], const double (&w)[NQ]) {
  const int d = NV - 1;
  int bad = 0;
  double sw = 0.0;
  for (int q = 0; q < NQ; ++q) sw += w[q];
  if (std::fabs(sw - 1.0) > 1e-15) {
    std::fprintf(stderr, "d = %d: weights sum to 1 %+.3e\n", d, sw - 1.0);
    ++bad;
  }
  for (int q = 0; q < NQ; ++q) {
    double s = 0.0;
    for (int a = 0; a < NV; ++a) s += lam[q][a];
    if (std::fabs(s - 1.0) > 4e-16) {
      std::fprintf(stderr, "d = %d: point %d: coordinates sum to 1 %+.3e\n", d, q, s - 1.0);
      ++bad;
    }
  }
  int al[4] = {0, 0, 0, 0};
  for (al[0] = 0; al[0] <= 7; ++al[0])
    for (al[1] = 0; al[0] + al[1] <= 7; ++al[1])
      for (al[2] = 0; al[0] + al[1] + al[2] <= 7; ++al[2])
        for (al[3] = 0; al[0] + al[1] + al[2] + al[3] <= (NV == 4 ? 7 : al[0] + al[1] + al[2]); ++al[3]) {
          int deg = 0;
          double exact = factorial(d);
          for (int a = 0; a < NV; ++a) {
            deg += al[a];
            exact *= factorial(al[a]);
          }
          exact /= factorial(d + deg);
          double sum = 0.0;
          for (int q = 0; q < NQ; ++q) {
            double t = w[q];
            for (int a = 0; a < NV; ++a) t *= std::pow(lam[q][a], al[a]);
            sum += t;
          }
          if (std::fabs(sum - exact) > 1e-15) {
            std::fprintf(stderr, "d = %d: monomial (%d %d %d %d): %.17g, exact %.17g\n", d, al[0], al[1], al[2], al[3], sum,
                         exact);
            ++bad;
          }
        }
  for (int q = 0; q < NQ; ++q) {
    std::printf("%d %d", d, q);
    for (int a = 0; a < NV; ++a) std::printf(" %.17g", lam[q][a]);
    std::printf(" %.17g\n", w[q]);
  }
  return bad;
}

int main() {
  const int bad = check<3, GLIMS_DQ2_N>(glims_dq2_lam, glims_dq2_w) + check<4, GLIMS_DQ3_N>(glims_dq3_lam, glims_dq3_w);
  return bad ? 1 : 0;
}
