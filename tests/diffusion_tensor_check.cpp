// Host-side check of glimslib_amd/csrc/diffusion_tensor.h (tests/test_anisotropic_cpu.py compiles and runs it with the host
// compiler alone, -Wall -Werror, once plain and once with -fsanitize=address,undefined):
//   1. glims_dt_form against a dense d x d product on random symmetric tensors, and glims_dt_apply against the dense rows;
//   2. symmetry of the form, a^T T b = b^T T a, to rounding;
//   3. the identity gives the dot product exactly (the same bits);
//   4. glims_dt_spd on SPD, indefinite, semi-definite, negative-definite, NaN and infinite inputs;
//   5. glims_dt_ratio on Q diag(l) Q^T with known l, coinciding eigenvalues (fibre tensors) and diagonal tensors included.
// Prints one summary line and returns 0, or the first failure and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "diffusion_tensor.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
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
static void unpack(const double* T, double M[D][D]) {
  int k = 0;
  for (int a = 0; a < D; ++a)
    for (int b = a; b < D; ++b) M[a][b] = M[b][a] = T[k++];
}
template <int D>
static void pack(const double M[D][D], double* T) {
  int k = 0;
  for (int a = 0; a < D; ++a)
    for (int b = a; b < D; ++b) T[k++] = M[a][b];
}

// Q diag(l) Q^T with Q a product of random plane rotations
template <int D>
static void from_eigen(const double* l, double* T) {
  double Q[D][D] = {};
  for (int a = 0; a < D; ++a) Q[a][a] = 1.0;
  for (int p = 0; p < D; ++p)
    for (int q = p + 1; q < D; ++q) {
      const double th = 3.14159265358979 * rnd(), c = std::cos(th), s = std::sin(th);
      for (int a = 0; a < D; ++a) {
        const double x = Q[a][p], y = Q[a][q];
        Q[a][p] = c * x - s * y;
        Q[a][q] = s * x + c * y;
      }
    }
  double M[D][D];
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) {
      double t = 0.0;
      for (int k = 0; k < D; ++k) t += Q[a][k] * l[k] * Q[b][k];
      M[a][b] = t;
    }
  for (int a = 0; a < D; ++a)
    for (int b = a + 1; b < D; ++b) M[a][b] = M[b][a] = 0.5 * (M[a][b] + M[b][a]);
  pack<D>(M, T);
}

template <int D>
static double check_dim() {
  constexpr int NT = D * (D + 1) / 2;
  static_assert(glims_dt_size<D>() == NT, "packed size");
  const double eps = std::numeric_limits<double>::epsilon();
  double worst = 0.0;
  // layout: entry (a, b) sits where the row-by-row upper triangle puts it
  {
    int k = 0;
    for (int a = 0; a < D; ++a)
      for (int b = a; b < D; ++b) CHECK(glims_dt_index<D>(a, b) == k++, "index (%d, %d) in %d-D", a, b, D);
  }
  for (int it = 0; it < 2000; ++it) {
    double T[NT], M[D][D], a[D], b[D], Tb[D];
    for (int k = 0; k < NT; ++k) T[k] = 3.0 * rnd();
    unpack<D>(T, M);
    for (int k = 0; k < D; ++k) a[k] = rnd(), b[k] = rnd();
    double dense = 0.0, mag = 0.0;
    for (int i = 0; i < D; ++i) {
      double row = 0.0;
      for (int j = 0; j < D; ++j) {
        row += M[i][j] * b[j];
        mag += std::fabs(a[i] * M[i][j] * b[j]);
      }
      dense += a[i] * row;
    }
    glims_dt_apply<D>(T, b, Tb);
    for (int i = 0; i < D; ++i) {
      double row = 0.0;
      for (int j = 0; j < D; ++j) row += M[i][j] * b[j];
      CHECK(Tb[i] == row, "apply row %d in %d-D: %.17g against %.17g", i, D, Tb[i], row);
    }
    const double f = glims_dt_form<D>(T, a, b), ft = glims_dt_form<D>(T, b, a);
    // d^2 products and d^2 - 1 additions of terms whose absolute sum is mag
    const double tol = 2.0 * D * D * eps * mag;
    CHECK(std::fabs(f - dense) <= tol, "form against dense in %d-D: %.17g against %.17g", D, f, dense);
    CHECK(std::fabs(f - ft) <= tol, "symmetry in %d-D: %.17g against %.17g", D, f, ft);
    if (mag > 0.0) worst = std::fmax(worst, std::fabs(f - ft) / (eps * mag));
    // identity: the dot product, bit for bit
    double I[NT];
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) I[glims_dt_index<D>(i, j)] = i == j ? 1.0 : 0.0;
    double dot = 0.0;
    for (int k = 0; k < D; ++k) dot += a[k] * b[k];
    CHECK(glims_dt_form<D>(I, a, b) == dot, "identity in %d-D: %.17g against %.17g", D, glims_dt_form<D>(I, a, b), dot);
    CHECK(glims_dt_spd<D>(I), "identity is SPD in %d-D", D);
    CHECK(glims_dt_ratio<D>(I) == 1.0, "ratio of the identity in %d-D", D);
  }
  // SPD test and ratio on tensors of known spectrum
  for (int it = 0; it < 2000; ++it) {
    double l[D], T[NT];
    double lmax = 0.0, lmin = 1e300;
    for (int k = 0; k < D; ++k) {
      l[k] = std::exp(1.5 * rnd());
      if (it % 4 == 1 && k > 0) l[k] = l[0];             // a multiple of the identity
      if (it % 4 == 2 && k > 0) l[k] = 1.0;              // a fibre tensor: one direction apart, the others coincide
      lmax = std::fmax(lmax, l[k]);
      lmin = std::fmin(lmin, l[k]);
    }
    from_eigen<D>(l, T);
    CHECK(glims_dt_spd<D>(T), "SPD tensor refused in %d-D (it %d)", D, it);
    const double want = lmax / lmin, got = glims_dt_ratio<D>(T);
    CHECK(std::fabs(got - want) <= 64.0 * eps * want * want, "ratio in %d-D (it %d): %.17g against %.17g", D, it, got, want);
    // one eigenvalue negative: indefinite; all negative: negative definite
    double li[D], Ti[NT];
    for (int k = 0; k < D; ++k) li[k] = l[k];
    li[it % D] = -l[it % D];
    from_eigen<D>(li, Ti);
    CHECK(!glims_dt_spd<D>(Ti), "indefinite tensor accepted in %d-D (it %d)", D, it);
    for (int k = 0; k < D; ++k) li[k] = -l[k];
    from_eigen<D>(li, Ti);
    CHECK(!glims_dt_spd<D>(Ti), "negative-definite tensor accepted in %d-D (it %d)", D, it);
    // non-finite entries, one at a time
    for (int k = 0; k < NT; ++k) {
      double Tn[NT];
      for (int j = 0; j < NT; ++j) Tn[j] = T[j];
      Tn[k] = std::numeric_limits<double>::quiet_NaN();
      CHECK(!glims_dt_spd<D>(Tn), "NaN entry %d accepted in %d-D", k, D);
      Tn[k] = std::numeric_limits<double>::infinity();
      CHECK(!glims_dt_spd<D>(Tn), "infinite entry %d accepted in %d-D", k, D);
    }
  }
  // exactly semi-definite: e e^T with small-integer e (every minor is computed exactly and one of them is 0), and zero
  for (int it = 0; it < 200; ++it) {
    double e[D], M[D][D], T[NT];
    for (int k = 0; k < D; ++k) e[k] = std::floor(4.0 * rnd());
    for (int a = 0; a < D; ++a)
      for (int b = 0; b < D; ++b) M[a][b] = e[a] * e[b];
    pack<D>(M, T);
    CHECK(!glims_dt_spd<D>(T), "semi-definite e e^T accepted in %d-D (it %d)", D, it);
    if (D == 3) {   // rank two: e e^T + f f^T
      double f[D];
      for (int k = 0; k < D; ++k) f[k] = std::floor(4.0 * rnd());
      for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) M[a][b] += f[a] * f[b];
      pack<D>(M, T);
      CHECK(!glims_dt_spd<D>(T), "semi-definite rank-2 tensor accepted in 3-D (it %d)", it);
    }
  }
  {
    double Z[NT] = {};
    CHECK(!glims_dt_spd<D>(Z), "zero tensor accepted in %d-D", D);
  }
  return worst;
}

int main() {
  const double w2 = check_dim<2>();
  const double w3 = check_dim<3>();
  if (g_fail) return 1;
  printf("diffusion_tensor_check: ok (asymmetry of the form at most %.2f / %.2f eps of the terms' absolute sum in 2-D / 3-D)\n",
         w2, w3);
  return 0;
}
