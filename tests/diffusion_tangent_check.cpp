// Host-side check of what the tangent fields take from glimslib_amd/csrc/diffusion_tensor.h (tests/test_tensor_controls_cpu.py
// compiles and runs it with the host compiler alone, -Wall -Werror, once plain and once with -fsanitize=address,undefined):
//   1. glims_dt_form with INDEFINITE symmetric tangents against a dense d x d product, and its symmetry a^T T b = b^T T a;
//   2. the zero tangent gives exactly 0, also for huge vectors;
//   3. linearity in the tangent: form(T1 + T2) = form(T1) + form(T2) to rounding, form(s T) = s form(T) for s a power of two
//      exactly;
//   4. the fibre tangent dT/dr = s' (I + (r - 1) e e^T) + s e e^T against the central difference of the tensor in r, and its
//      trace 0;
//   5. glims_dt_finite: finite fields (indefinite, zero, negative definite) pass, a NaN or an infinity in any slot does not;
//   6. a K-plane field [K][n_cells][NT] read at ((k n_cells + e) NT) as k_sens_tangent reads it: every entry once, none twice.
// Prints one summary line and returns 0, or the first failure and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "diffusion_tensor.h"

static uint64_t g_state = 0x2545f4914f6cdd1dull;
static double rnd() {   // xorshift64*, uniform in [-1, 1)
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

static int g_fail = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (!g_fail) {                          \
        fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);         \
        fprintf(stderr, "\n");                \
      }                                       \
      g_fail = 1;                             \
    }                                         \
  } while (0)

template <int D>
static double dense_form(const double* T, const double* a, const double* b) {
  double s = 0.0;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) s += a[i] * glims_dt_at<D>(T, i, j) * b[j];
  return s;
}

// trace-normalised fibre tensor of direction e (unit) and ratio r, packed
template <int D>
static void fibre(const double* e, double r, double* T) {
  const double s = D / (D + r - 1.0);
  for (int a = 0; a < D; ++a)
    for (int b = a; b < D; ++b) T[glims_dt_index<D>(a, b)] = s * ((a == b ? 1.0 : 0.0) + (r - 1.0) * e[a] * e[b]);
}
template <int D>
static void fibre_tangent(const double* e, double r, double* dT) {
  const double q = D + r - 1.0, s = D / q, sp = -D / (q * q);
  for (int a = 0; a < D; ++a)
    for (int b = a; b < D; ++b)
      dT[glims_dt_index<D>(a, b)] = sp * ((a == b ? 1.0 : 0.0) + (r - 1.0) * e[a] * e[b]) + s * e[a] * e[b];
}

template <int D>
static double check_dim(int* n_indefinite) {
  constexpr int NT = glims_dt_size<D>();
  double worst = 0.0;
  for (int it = 0; it < 2000; ++it) {
    double T1[NT], T2[NT], S[NT], a[D], b[D];
    for (int k = 0; k < NT; ++k) T1[k] = rnd(), T2[k] = rnd(), S[k] = T1[k] + T2[k];
    for (int k = 0; k < D; ++k) a[k] = rnd(), b[k] = rnd();
    if (!glims_dt_spd<D>(T1)) ++*n_indefinite;
    CHECK(glims_dt_finite<D>(T1), "a finite tangent is refused");
    // 1. against the dense product, symmetry
    const double f = glims_dt_form<D>(T1, a, b), d = dense_form<D>(T1, a, b), ft = glims_dt_form<D>(T1, b, a);
    CHECK(std::fabs(f - d) <= 1e-15 * D * D, "form against the dense product: %.3e", std::fabs(f - d));
    CHECK(std::fabs(f - ft) <= 1e-15 * D * D, "symmetry: %.3e", std::fabs(f - ft));
    worst = std::fmax(worst, std::fmax(std::fabs(f - d), std::fabs(f - ft)));
    // 3. linearity in the tangent
    const double fs = glims_dt_form<D>(S, a, b), f2 = glims_dt_form<D>(T2, a, b);
    CHECK(std::fabs(fs - (f + f2)) <= 4e-15 * D * D, "additivity: %.3e", std::fabs(fs - (f + f2)));
    double H[NT];
    for (int k = 0; k < NT; ++k) H[k] = -4.0 * T1[k];
    CHECK(glims_dt_form<D>(H, a, b) == -4.0 * f, "scaling by a power of two is not exact");
    // 2. the zero tangent
    double Z[NT] = {}, big[D];
    for (int k = 0; k < D; ++k) big[k] = 1e150 * (a[k] + 2.0);
    CHECK(glims_dt_form<D>(Z, a, b) == 0.0 && glims_dt_form<D>(Z, big, big) == 0.0, "the zero tangent does not give 0");
    CHECK(glims_dt_finite<D>(Z), "the zero tangent is refused");
    // 4. the fibre tangent
    double e[D], n = 0.0;
    for (int k = 0; k < D; ++k) e[k] = rnd(), n += e[k] * e[k];
    n = std::sqrt(n);
    if (n > 1e-3) {
      for (int k = 0; k < D; ++k) e[k] /= n;
      const double r = 1.0 + 9.5 * (rnd() + 1.0), h = 1e-5;
      double Tp[NT], Tm[NT], dT[NT], tr = 0.0;
      fibre<D>(e, r + h, Tp);
      fibre<D>(e, r - h, Tm);
      fibre_tangent<D>(e, r, dT);
      for (int k = 0; k < NT; ++k) {
        const double fd = (Tp[k] - Tm[k]) / (2.0 * h);
        CHECK(std::fabs(fd - dT[k]) <= 1e-9, "fibre tangent against the central difference: %.3e", std::fabs(fd - dT[k]));
      }
      for (int k = 0; k < D; ++k) tr += dT[glims_dt_index<D>(k, k)];
      CHECK(std::fabs(tr) <= 1e-14, "trace of the normalised fibre tangent: %.3e", tr);
      CHECK(!glims_dt_spd<D>(dT), "a trace-free tangent cannot be definite");
    }
    // 5. finiteness, slot by slot
    const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                           -std::numeric_limits<double>::infinity()};
    double B[NT];
    for (int k = 0; k < NT; ++k) B[k] = T1[k];
    B[it % NT] = bad[it % 3];
    CHECK(!glims_dt_finite<D>(B), "a tangent that is not finite is accepted (slot %d)", it % NT);
  }
  double neg[NT] = {};
  for (int k = 0; k < D; ++k) neg[glims_dt_index<D>(k, k)] = -1.0;
  CHECK(glims_dt_finite<D>(neg) && !glims_dt_spd<D>(neg), "a negative-definite tangent");
  // 6. the plane layout of k_sens_tangent: heap arrays of the exact size, so that the address sanitizer sees an index too far
  const int K = 4, n_cells = 37;
  std::vector<double> planes((size_t)K * n_cells * NT);
  std::vector<int> seen(planes.size(), 0);
  for (size_t i = 0; i < planes.size(); ++i) planes[i] = (double)i;
  for (int k = 0; k < K; ++k)
    for (int64_t e = 0; e < n_cells; ++e) {
      const double* T = planes.data() + ((int64_t)k * n_cells + e) * NT;
      double one[D];
      for (int j = 0; j < D; ++j) one[j] = 1.0;
      double want = 0.0;
      for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) want += glims_dt_at<D>(T, i, j);
      CHECK(std::fabs(glims_dt_form<D>(T, one, one) - want) <= 1e-12 * std::fabs(want) + 1e-12, "plane %d cell %d", k, (int)e);
      for (int j = 0; j < NT; ++j) seen[(size_t)(T - planes.data()) + j]++;
    }
  for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "entry %zu of the planes is read %d times", i, seen[i]);
  return worst;
}

int main() {
  int indefinite = 0;
  const double w2 = check_dim<2>(&indefinite), w3 = check_dim<3>(&indefinite);
  CHECK(indefinite > 3000, "the random tangents should be indefinite: only %d of 4000 are", indefinite);
  if (g_fail) return 1;
  printf("diffusion_tangent_check: ok (form against dense: %.1e in 2-D, %.1e in 3-D; %d of 4000 tangents not definite)\n", w2, w3,
         indefinite);
  return 0;
}
