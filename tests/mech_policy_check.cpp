// Host-side check of the elasticity solve's policy (glimslib_amd/csrc/mech_policy.h): the ring of stored solves, the
// least-squares fit of the initial guess and the scalar rules, as their comments state them.  Built and run by
// tests/test_mech_policy_cpu.py; exit status 0 = every check held.
#include <cstdint>
#include <cstdio>
#include <limits>

#include "mech_policy.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static const int NV = 40;   // components of the vectors the Gram matrices are built from

// standard normal numbers from a fixed seed (64-bit LCG + Box-Muller: the same on every host)
struct Normal {
  uint64_t state = 0x9E3779B97F4A7C15ull;
  double uniform() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return ((state >> 11) + 0.5) / 9007199254740992.0;
  }
  double operator()() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }
};

static double dot(const double* a, const double* b) {
  double s = 0.0;
  for (int i = 0; i < NV; ++i) s += a[i] * b[i];
  return s;
}

static void diagonal_gram() {
  // a diagonal system is solved without a rounding error of the elimination: a_k = g_k / (G_kk + ridge)
  for (int m = 1; m <= GL_MHIST; ++m) {
    double G[GL_MHIST][GL_MHIST] = {{0.0}}, g[GL_MHIST] = {0.0}, a[GL_MHIST];
    double tr = 0.0, nb2 = 1.0;   // (a right-hand side with a part outside the span of the stored ones)
    for (int k = 0; k < m; ++k) {
      G[k][k] = 1.0 + k / 4.0;
      g[k] = 0.5 - k / 8.0;
      tr += G[k][k];
      nb2 += g[k] * g[k] / G[k][k];
    }
    CHECK(mech_history_fit(m, G, g, std::sqrt(nb2), m - 1, a));
    for (int k = 0; k < m; ++k) CHECK(a[k] == g[k] / (G[k][k] + GL_MECH_RIDGE * tr));
    for (int k = m; k < GL_MHIST; ++k) CHECK(a[k] == 0.0);
  }
  CHECK(GL_MECH_RIDGE == 1e-13);
}

static void gram_of_vectors() {
  Normal rnd;
  static double V[GL_MHIST][NV], b[NV];
  for (int k = 0; k < GL_MHIST; ++k)
    for (int i = 0; i < NV; ++i) V[k][i] = rnd();
  for (int i = 0; i < NV; ++i) b[i] = rnd();
  double G[GL_MHIST][GL_MHIST];
  for (int k = 0; k < GL_MHIST; ++k)
    for (int l = 0; l < GL_MHIST; ++l) G[k][l] = dot(V[k], V[l]);
  double worst = 0.0;
  for (int m = 1; m <= GL_MHIST; ++m) {
    // the right-hand side IS stored vector j: the coefficients are e_j, whichever branch returns them (with j the last
    // slot the warm start predicts exactly 0 and the fit a rounding error of either sign)
    for (int j = 0; j < m; ++j) {
      double g[GL_MHIST] = {0.0}, a[GL_MHIST];
      for (int k = 0; k < m; ++k) g[k] = G[k][j];
      mech_history_fit(m, G, g, std::sqrt(G[j][j]), m - 1, a);
      for (int k = 0; k < m; ++k) worst = std::max(worst, std::fabs(a[k] - (k == j ? 1.0 : 0.0)));
    }
    // a generic right-hand side: finite coefficients, and a TRUE residual (from the vectors, not from the function's own
    // prediction) no larger than that of the plain warm start, whichever slot is the last
    for (int last = 0; last < m; ++last) {
      double g[GL_MHIST] = {0.0}, a[GL_MHIST];
      for (int k = 0; k < m; ++k) g[k] = dot(V[k], b);
      mech_history_fit(m, G, g, std::sqrt(dot(b, b)), last, a);
      double r_fit[NV], r_warm[NV];
      for (int i = 0; i < NV; ++i) {
        r_fit[i] = b[i];
        for (int k = 0; k < m; ++k) r_fit[i] -= a[k] * V[k][i];
        r_warm[i] = b[i] - V[last][i];
      }
      for (int k = 0; k < m; ++k) CHECK(std::isfinite(a[k]));
      CHECK(dot(r_fit, r_fit) <= dot(r_warm, r_warm));
    }
  }
  std::printf("right-hand side = stored vector: max |a - e_j| = %.3e\n", worst);
  CHECK(worst <= 1e-10);
}

static void degenerate_inputs() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double a[GL_MHIST];
  {   // two identical stored right-hand sides: only the ridge makes the system regular
    double G[GL_MHIST][GL_MHIST] = {{0.0}}, g[GL_MHIST] = {1.0, 1.0};
    G[0][0] = G[0][1] = G[1][0] = G[1][1] = 1.0;
    mech_history_fit(2, G, g, 1.0, 1, a);
    CHECK(std::isfinite(a[0]) && std::isfinite(a[1]) && std::fabs(a[0] + a[1] - 1.0) <= 1e-9);
  }
  {   // an all-zero Gram matrix has no pivot: the plain warm start
    double G[GL_MHIST][GL_MHIST] = {{0.0}}, g[GL_MHIST] = {0.25, -1.0, 2.0};
    CHECK(!mech_history_fit(3, G, g, 3.0, 1, a));
    CHECK(a[0] == 0.0 && a[1] == 1.0 && a[2] == 0.0);
  }
  {   // a NaN among the products: the plain warm start
    double G[GL_MHIST][GL_MHIST] = {{0.0}}, g[GL_MHIST] = {0.5, nan, 0.5};
    for (int k = 0; k < 3; ++k) G[k][k] = 1.0;
    CHECK(!mech_history_fit(3, G, g, 1.0, 2, a));
    CHECK(a[0] == 0.0 && a[1] == 0.0 && a[2] == 1.0);
  }
}

static void ring() {
  CHECK(GL_MHIST == 16);
  CHECK(MechRing::depth_of(-3) == 0 && MechRing::depth_of(0) == 0 && MechRing::depth_of(8) == 8 &&
        MechRing::depth_of(16) == 16 && MechRing::depth_of(100) == GL_MHIST);
  MechRing r;
  CHECK(r.stored(8) == 0);
  for (int k = 0; k < 3; ++k) r.advance(3);
  CHECK(r.count == 3 && r.next == 0 && r.last(3) == 2);   // `last` wraps
  r.advance(3);
  CHECK(r.count == 3 && r.next == 1 && r.last(3) == 0);   // `count` saturates at the depth
  for (int k = 0; k < 10; ++k) r.advance(3);
  CHECK(r.count == 3 && r.next == 2 && r.last(3) == 1 && r.stored(3) == 3);
  CHECK(r.stored(0) == 0);   // depth 0: no history, whatever the ring holds
  // a ring whose next slot lies beyond a smaller depth restarts; one that fits stays
  MechRing big;
  for (int k = 0; k < 5; ++k) big.advance(8);
  MechRing kept = big;
  kept.fit_depth(8);
  CHECK(kept.count == 5 && kept.next == 5);
  kept.fit_depth(6);
  CHECK(kept.count == 5 && kept.next == 5);
  big.fit_depth(3);
  CHECK(big.count == 0 && big.next == 0 && big.stored(3) == 0);
  MechRing one;
  one.advance(8);
  one.fit_depth(0);   // (depth 0 keeps slot 0 as the only admissible `next`)
  CHECK(one.count == 0 && one.next == 0);
  r.restart();
  CHECK(r.count == 0 && r.next == 0);
}

static void scalar_rules() {
  // mech_mixed: 0 never, 2 always, 1 only with block-Jacobi and an operator beyond 256 MiB
  const size_t lim = (size_t)256 << 20;
  CHECK(GL_MECH_MIXED_BYTES == lim);
  for (int mode = 0; mode <= 2; ++mode)
    for (int big = 0; big <= 1; ++big)
      for (int mg = 0; mg <= 1; ++mg)
        CHECK(mech_mixed_wanted(mode, big ? lim + 1 : lim, mg != 0) == (mode == 2 || (mode == 1 && big && !mg)));
  // the verification loop ends within 4 x the tolerance, or after two extra rounds
  const double tol = 3e-7, above = std::nextafter(4.0 * tol, 1.0);
  CHECK(mech_verify_done(4.0 * tol, tol, 0) && mech_verify_done(0.0, tol, 0));
  CHECK(!mech_verify_done(above, tol, 0) && !mech_verify_done(above, tol, 1) && mech_verify_done(above, tol, 2));
  CHECK(mech_verify_done(1e300, tol, 3));
  // the mixed loop
  CHECK(GL_MECH_OUTER == 12);
  CHECK(mech_inner_tol(1e-9, 1.0) == 1e-6 && mech_inner_tol(1e-9, 1e-4) == 1e-9 && mech_inner_tol(2e-7, 0.1) == 2e-7);
  CHECK(!mech_fp32_exhausted(0.49, 1.0) && mech_fp32_exhausted(0.5, 1.0) && mech_fp32_exhausted(2.0, 1.0));
  CHECK(mech_fp32_exhausted(std::numeric_limits<double>::quiet_NaN(), 1.0));
}

int main() {
  diagonal_gram();
  gram_of_vectors();
  degenerate_inputs();
  ring();
  scalar_rules();
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  return failures ? 1 : 0;
}
