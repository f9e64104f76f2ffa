// Host check of glimslib_amd/csrc/lame_derivs.h (compiled and run by tests/test_lame_derivs_cpu.py, no GPU): central
// differences of the first derivatives of the Lame pair give the second derivatives to 1e-7 relative, the rows that the host
// combines from the per-label sums reduce to the first-order formula, and the first derivatives are printed for the Python
// side to compare with tests/adjoint_elastic_common.lame_derivatives.
#include <cmath>
#include <cstdio>

#include "lame_derivs.h"

static int failures = 0;

// |cd - d2| <= 1e-7 max(|d2|, scale): scale stands in where the second derivative is exactly 0 (m and l are linear in E)
static void close(const char* what, double E, double nu, double cd, double d2, double scale) {
  const double den = std::fabs(d2) > 0.0 ? std::fabs(d2) : scale;
  const double err = std::fabs(cd - d2) / den;
  if (!(err <= 1e-7)) {
    std::fprintf(stderr, "%s at E = %g, nu = %g: central difference %.17g, lame_derivs %.17g (rel %.3e)\n", what, E, nu, cd, d2,
                 err);
    ++failures;
  }
}

int main() {
  const double nus[] = {-0.3, 0.0, 0.1, 0.4, 0.49}, Es[] = {1e-3, 1.0, 1e7};
  for (double E : Es)
    for (double nu : nus) {
      const LameDerivs d = lame_derivs(E, nu);
      // steps: m, l are linear in E (any step is exact up to rounding); in nu the derivatives grow like 1 / (1 - 2 nu)^k, so
      // the truncation h^2 f''' / (6 f') stays below 1e-8 at nu = 0.49 with h = 3e-7
      const double hE = 1e-4 * E, hn = 3e-7;
      const LameDerivs Ep = lame_derivs(E + hE, nu), Em = lame_derivs(E - hE, nu);
      const LameDerivs Np = lame_derivs(E, nu + hn), Nm = lame_derivs(E, nu - hn);
      close("m_EE", E, nu, (Ep.m_E - Em.m_E) / (2 * hE), d.m_EE, std::fabs(d.m_E) / E);
      close("l_EE", E, nu, (Ep.l_E - Em.l_E) / (2 * hE), d.l_EE, std::fabs(d.m_E) / E);
      close("m_Enu (d/dE of m_nu)", E, nu, (Ep.m_nu - Em.m_nu) / (2 * hE), d.m_Enu, 1.0);
      close("l_Enu (d/dE of l_nu)", E, nu, (Ep.l_nu - Em.l_nu) / (2 * hE), d.l_Enu, 1.0);
      close("m_Enu (d/dnu of m_E)", E, nu, (Np.m_E - Nm.m_E) / (2 * hn), d.m_Enu, 1.0);
      close("l_Enu (d/dnu of l_E)", E, nu, (Np.l_E - Nm.l_E) / (2 * hn), d.l_Enu, 1.0);
      close("m_nunu", E, nu, (Np.m_nu - Nm.m_nu) / (2 * hn), d.m_nunu, E);
      close("l_nunu", E, nu, (Np.l_nu - Nm.l_nu) / (2 * hn), d.l_nunu, E);
      // the direction's Lame change and the rows: a zero direction leaves only the direction's sums, weighted as first order
      double dm, dl;
      lame_direction(d, 2.0, -3.0, &dm, &dl);
      if (dm != 2.0 * d.m_E + -3.0 * d.m_nu || dl != 2.0 * d.l_E + -3.0 * d.l_nu) {
        std::fprintf(stderr, "lame_direction at E = %g, nu = %g\n", E, nu);
        ++failures;
      }
      const ElasticSums tot = {0.3, -0.7, 1.1}, dir = {0.2, 0.5, -0.4}, zero = {0.0, 0.0, 0.0};
      for (int which = 0; which < 2; ++which) {
        const double mp = which ? d.m_nu : d.m_E, lp = which ? d.l_nu : d.l_E;
        for (int dim = 2; dim <= 3; ++dim) {
          const double first = elastic_gradient_row(dim, 0.25, mp, lp, dir);
          const double row = elastic_hessian_row(dim, which, d, 0.25, 0.0, 0.0, 0.0, tot, dir);
          if (std::fabs(row - first) > 1e-15 * (std::fabs(first) + 1e-300)) {
            std::fprintf(stderr, "elastic_hessian_row with a zero direction at E = %g, nu = %g: %.17g vs %.17g\n", E, nu, row,
                         first);
            ++failures;
          }
          if (elastic_hessian_row(dim, which, d, 0.25, 0.1, 1.0, 1.0, zero, zero) != 0.0) {
            std::fprintf(stderr, "elastic_hessian_row of zero sums is not 0 at E = %g, nu = %g\n", E, nu);
            ++failures;
          }
        }
      }
      std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", E, nu, d.m_E, d.l_E, d.m_nu, d.l_nu);
    }
  return failures ? 1 : 0;
}
