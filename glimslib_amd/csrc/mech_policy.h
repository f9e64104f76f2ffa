// The elasticity solve's memory and decisions (gl_solve_mechanics, solver.hip): the ring of stored solves, the least-squares
// fit that turns them into an initial guess, and every rule that is a function of scalars.  Plain C++17 -- no device types,
// no handle -- so that tests/mech_policy_check.cpp exercises them on the host.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

static const int GL_MHIST = 16;   // upper bound of glims_options.mech_history

// Ring of the last `depth` solves (depth: glims_options.mech_history, clamped): slots [0, count) hold solves, `next` is
// written next
struct MechRing {
  int count = 0, next = 0;
  void restart() { count = next = 0; }
  static int depth_of(int mech_history) { return std::max(0, std::min(GL_MHIST, mech_history)); }
  int stored(int depth) const { return (count > 0 && depth > 0) ? count : 0; }
  int last(int depth) const { return (next + depth - 1) % depth; }   // the most recent solve's slot (depth > 0)
  void advance(int depth) {
    next = (next + 1) % depth;
    count = std::min(count + 1, depth);
  }
  void fit_depth(int depth) { if (next >= std::max(1, depth)) restart(); }   // the depth option shrank
};

// Initial guess.  K_el is linear and does not change in time, so if rhs ~ sum_k a_k rhs_k for previously solved
// right-hand sides then x ~ sum_k a_k x_k with residual rhs - sum_k a_k rhs_k: least-squares fit over the stored
// solves; the concentration evolves smoothly, the fit removes several decades of the initial residual.
// Falls back to the previous displacement (the fit with a = e_last) when that is better.
// G: Gram matrix (rhs_k, rhs_l) of the m stored right-hand sides, g[k] = (rhs_k, rhs), nb = ||rhs||, last: slot of the most
// recent solve.  Returns whether the fit was used.
static const double GL_MECH_RIDGE = 1e-13;   // x trace(G): the right-hand sides of consecutive steps are nearly parallel
inline bool mech_history_fit(int m, const double (*G)[GL_MHIST], const double* g, double nb, int last, double* a /*[GL_MHIST]*/) {
  for (int k = 0; k < GL_MHIST; ++k) a[k] = 0.0;
  // normal equations with a small ridge
  double A[GL_MHIST][GL_MHIST + 1];
  double tr = 0.0;
  for (int k = 0; k < m; ++k) tr += G[k][k];
  for (int k = 0; k < m; ++k) {
    for (int l = 0; l < m; ++l) A[k][l] = G[k][l] + (k == l ? GL_MECH_RIDGE * tr : 0.0);
    A[k][m] = g[k];
  }
  bool ok = true;
  for (int c = 0; c < m && ok; ++c) {   // Gaussian elimination with partial pivoting on the m x m system
    int piv = c;
    for (int r = c + 1; r < m; ++r)
      if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
    if (!(std::fabs(A[piv][c]) > 0.0)) {
      ok = false;
      break;
    }
    for (int q = 0; q <= m; ++q) std::swap(A[c][q], A[piv][q]);
    for (int r = c + 1; r < m; ++r) {
      const double f = A[r][c] / A[c][c];
      for (int q = c; q <= m; ++q) A[r][q] -= f * A[c][q];
    }
  }
  if (ok)
    for (int c = m - 1; c >= 0; --c) {
      double v = A[c][m];
      for (int q = c + 1; q < m; ++q) v -= A[c][q] * a[q];
      a[c] = v / A[c][c];
    }
  // predicted squared residual of the fit against the plain warm start (most recent solution alone)
  auto res2 = [&](const double* coef) {
    double v = nb * nb;
    for (int k = 0; k < m; ++k) {
      v -= 2.0 * coef[k] * g[k];
      for (int l = 0; l < m; ++l) v += coef[k] * coef[l] * G[k][l];
    }
    return v;
  };
  double e_last[GL_MHIST] = {0.0};
  e_last[last] = 1.0;
  bool finite = ok;
  for (int k = 0; k < m; ++k) finite = finite && std::isfinite(a[k]);
  if (finite && res2(a) <= res2(e_last)) return true;
  for (int k = 0; k < m; ++k) a[k] = e_last[k];
  return false;
}

// Mixed precision (mech_mixed: 0 off, 1 auto, 2 always).  Auto = with the block-Jacobi preconditioner, where an
// iteration IS one operator pass, and only where the operator is streamed from HBM (below ~256 MB, the Infinity Cache,
// an iteration is latency bound and the restarts of the refinement loop only add iterations).  Never with the multigrid
// preconditioner: the operator pass is 7 % of an iteration there, and the restarts cost more than that -- C5 at 10 M
// nodes 102 vs 107 ms per solve, Delaunay 1 M points 99 vs 117 ms, and with a stiff inclusion (stiffness jump 1e4) the
// restarted iteration loses the superlinear phase of CG altogether: 11 iterations against 29-55.
static const size_t GL_MECH_MIXED_BYTES = (size_t)256 << 20;
inline bool mech_mixed_wanted(int mech_mixed, size_t operator_bytes, bool use_mg) {
  return mech_mixed == 2 || (mech_mixed == 1 && operator_bytes > GL_MECH_MIXED_BYTES && !use_mg);
}

// fp64 solve: the true residual after the Krylov iteration may miss the tolerance by the drift one expects of the recurrence
// (GL_MECH_DRIFT x); beyond that the iteration continues from it, GL_MECH_VERIFY_ROUNDS times at the most
static const double GL_MECH_DRIFT = 4.0;
static const int GL_MECH_VERIFY_ROUNDS = 2;
inline bool mech_verify_done(double res, double tol, int round) {
  return res <= GL_MECH_DRIFT * tol || round >= GL_MECH_VERIFY_ROUNDS;
}

// Mixed solve: inner reduction 1e-6 (round 1: 1e-3): the single-precision operator is good for that, and with the
// solve-history guess (initial residual ~1e-6 |rhs|) ONE inner solve then reaches the target -- the loop costs
// two fp64 operator passes (initial residual, verification) instead of four to five.  At most GL_MECH_OUTER rounds; a round
// that gains less than a factor 2 was single precision's last.
static const double GL_MECH_INNER_RED = 1e-6, GL_MECH_STAGNATION = 0.5;
static const int GL_MECH_OUTER = 12;
inline double mech_inner_tol(double tol, double nr) { return std::max(tol, GL_MECH_INNER_RED * nr); }
inline bool mech_fp32_exhausted(double nr_new, double nr) { return !(nr_new < GL_MECH_STAGNATION * nr); }
