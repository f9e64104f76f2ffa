// Host-side check of the RD time stepper's policy (glimslib_amd/csrc/step_policy.h): the rules as their comments state them,
// compared exactly.  Built and run by tests/test_step_policy_cpu.py; exit status 0 = every check held.
#include <cstdio>

#include "step_policy.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static RunMemory settled(int mode) {   // a run past the steps that do not count
  RunMemory m;
  m.nw_steps = GL_NW_SETTLE;
  m.nw_mode = mode;
  return m;
}

static void forcing_mode() {
  // mode 0: +4 for a step of three iterations, -1 otherwise, threshold 6
  RunMemory m = settled(0);
  forcing_mode_after_step(m, true, 3, false);
  CHECK(m.nw_mode == 0 && m.nw_hold == 4);
  forcing_mode_after_step(m, true, 2, false);
  CHECK(m.nw_mode == 0 && m.nw_hold == 3);
  forcing_mode_after_step(m, true, 3, false);
  CHECK(m.nw_mode == 1 && m.nw_hold == 0 && m.nw_since == 0);
  m = settled(0);   // one such step in ten does not switch
  for (int k = 0; k < 100; ++k) {
    forcing_mode_after_step(m, true, k % 10 == 0 ? 3 : 2, false);
    CHECK(m.nw_mode == 0);
  }
  // mode 1: a three-iteration step gives mode 2 for 16 steps, then mode 1 again
  m = settled(1);
  forcing_mode_after_step(m, true, 3, false);
  CHECK(m.nw_mode == 2 && m.nw_hold == 16);
  for (int k = 0; k < 15; ++k) forcing_mode_after_step(m, true, 4, false);
  CHECK(m.nw_mode == 2);
  forcing_mode_after_step(m, true, 4, false);
  CHECK(m.nw_mode == 1 && m.nw_since == 0);
  // the 64th step of two iterations returns to mode 0
  m = settled(1);
  for (int k = 0; k < 63; ++k) forcing_mode_after_step(m, true, 2, false);
  CHECK(m.nw_mode == 1 && m.nw_since == 63);
  forcing_mode_after_step(m, true, 2, false);
  CHECK(m.nw_mode == 0 && m.nw_hold == 0);
  // nothing counts during the first 8 steps of a run
  m = RunMemory();
  for (int k = 0; k < 8; ++k) forcing_mode_after_step(m, true, 3, false);
  CHECK(m.nw_mode == 0 && m.nw_hold == 0 && m.nw_steps == 8);
  forcing_mode_after_step(m, true, 3, false);
  CHECK(m.nw_hold == 4 && m.nw_steps == 9);
  // a third iteration flagged warm2_miss does not count; neither does a step of another mode of operation
  m = settled(1);
  forcing_mode_after_step(m, true, 3, true);
  CHECK(m.nw_mode == 1 && m.nw_since == 1);
  forcing_mode_after_step(m, false, 5, false);
  CHECK(m.nw_mode == 1 && m.nw_since == 1 && m.nw_steps == GL_NW_SETTLE + 2);
}

static void second_solve_guess() {
  RunMemory m;
  const int expect[] = {8, 16, 32, 64, 128, 256, 256, 256};
  for (int k = 0; k < 8; ++k) {
    m.d2_good = 5;
    d2_missed(m);
    CHECK(m.d2_off == expect[k] && m.d2_good == 0);
  }
  CHECK(m.d2_backoff == 256);
  for (int k = 0; k < 31; ++k) d2_hit(m);
  CHECK(m.d2_backoff == 256);
  d2_hit(m);
  CHECK(m.d2_backoff == 8);
  // continuity: same regime and |R_1| within 0.7 .. 1.43 of the last one
  m = RunMemory();
  m.have_d2 = true;
  m.d2_depth = 2;
  m.d2_regime = 103;
  m.d2_r1 = 2.0;
  CHECK(d2_continues(m, 103, 0.71 * 2.0) && d2_continues(m, 103, 1.42 * 2.0));
  CHECK(!d2_continues(m, 103, 0.69 * 2.0) && !d2_continues(m, 103, 1.44 * 2.0));
  CHECK(!d2_continues(m, 102, 2.0) && !d2_continues(m, 103 + GL_D2_REGIME_PCG, 2.0) && d2_continues(m, 103, 2.0));
}

static void forcing_and_evaluation() {
  glims_options o = {};
  o.cg_rtol = 1e-3;
  o.newton_rtol = 1e-10;
  const double r0 = 1.0, target = 1e-10 * r0;
  // a step's first solve, mode 0 (0.3 cg_rtol) and mode 2 (cg_rtol); the evaluation after it is a plain sweep
  Forcing f = forcing_term(o, 0, r0, r0, target, 0.3 * 1e-3, 1e-3, 1e-3);
  CHECK(!f.adaptive && f.tol_lin == 0.3 * 1e-3 && f.floor_pred == 1e-3 && f.pred_next == 1e-3);
  CHECK(!speculate_next(o, false, true, f.pred_next, target, r0, r0) && !cheap_next(true, false, false, 0));
  f = forcing_term(o, 0, r0, r0, target, 1e-3, 1e-3, 1e-3);
  CHECK(f.tol_lin == 1e-3 && !f.adaptive);
  // a second solve with nq_first_ratio = 5e-4: the tolerance follows 0.3 x the predicted remainder q nr^2 / r0
  f = forcing_term(o, 1, 1e-2, r0, target, 0.3 * 1e-3, 5e-4, 0.2);
  CHECK(f.adaptive && f.floor_pred == 5e-4 * 1e-2 * (1e-2 / 1.0) && f.tol_lin == 0.3 * f.floor_pred);
  CHECK(f.pred_next == f.tol_lin + f.floor_pred);
  bool spec = speculate_next(o, false, true, f.pred_next, target, 1e-2, r0);   // 6.5e-8 against 3e-10: the cheap residual
  CHECK(!spec && cheap_next(true, spec, false, 1) && !cheap_next(true, spec, true, 1) && !cheap_next(false, spec, false, 1));
  f = forcing_term(o, 1, 1e-4, r0, target, 0.3 * 1e-3, 5e-4, 0.2);   // the Newton target bounds the tolerance from below
  CHECK(f.floor_pred == 5e-4 * 1e-4 * (1e-4 / 1.0) && f.tol_lin == 0.5 * target && f.pred_next == 0.5 * target + f.floor_pred);
  spec = speculate_next(o, false, true, f.pred_next, target, 1e-4, r0);   // 5.5e-11 <= 3e-10: the sweep prepares the next step
  CHECK(spec && !cheap_next(true, spec, false, 1) && !speculate_next(o, true, true, f.pred_next, target, 1e-4, r0));
  // without the quadratic residuals: the sweep speculates from 1e-4 r0 (at newton_rtol = 1e-10)
  CHECK(speculate_next(o, false, false, 1.0, target, 1e-4, r0) && !speculate_next(o, false, false, 0.0, target, 1.1e-4, r0));
  // GLIMS_FLAG_FIXED_FORCING: cg_rtol for every solve, the prediction from the last contraction
  glims_options fixed = o;
  fixed.flags = GLIMS_FLAG_FIXED_FORCING;
  f = forcing_term(fixed, 1, 1e-2, r0, target, 1e-3, 5e-4, 0.25);
  CHECK(!f.adaptive && f.tol_lin == 1e-3 * 1e-2 && f.pred_next == 1e-2 * 0.25);
  // cg_atol above the residual: the tolerance is met before the solve starts
  glims_options loose = o;
  loose.cg_atol = 1e-3;
  f = forcing_term(loose, 1, 1e-4, r0, target, 0.3 * 1e-3, 5e-4, 0.2);
  CHECK(f.tol_lin == 1e-3 && f.tol_lin >= 1e-4);
  // (c): a residual above five times what the solve was sized for
  f = forcing_term(o, 1, 1e-2, r0, target, 0.3 * 1e-3, 5e-4, 0.2);
  CHECK(!needs_rebase(o, f, 5.0 * f.floor_pred, 1e-2) && needs_rebase(o, f, 5.01 * f.floor_pred, 1e-2));
  f = forcing_term(fixed, 1, 1e-2, r0, target, 1e-3, 5e-4, 0.25);
  CHECK(!needs_rebase(fixed, f, 5.0 * (1e-3 * 1e-2), 1e-2) && needs_rebase(fixed, f, 5.01 * (1e-3 * 1e-2), 1e-2));
}

static void dot_free_solves() {
  ChebState cb;
  CHECK(prefer_pcg(cb, true, 0, GL_CHEB_LONG + 1, 1.0, 1e-3) && !prefer_pcg(cb, true, 1, GL_CHEB_LONG, 1.0, 1e-3));
  // four decades at 2 PCG iterations per decade: 9 iterations against 0.95 x cost ratio x passes
  cb.cost_ratio = 1.0;
  cb.pcg_its_per_decade = 2.0;
  CHECK(prefer_pcg(cb, true, 1, 10, 1e4, 1.0) && !prefer_pcg(cb, true, 1, 9, 1e4, 1.0));
  CHECK(!prefer_pcg(cb, true, 0, 10, 1e4, 1.0) && !prefer_pcg(cb, false, 1, 10, 1e4, 1.0));
  // two weak solves in a row make the next step a learning step; one does not
  cb.age = 3;
  count_weak_solve(cb, 1e-3, 1e-10, 0.99e-4);
  CHECK(cb.weak == 1 && cb.age == 3);
  count_weak_solve(cb, 1e-3, 1e-10, 1.01e-4);
  CHECK(cb.weak == 0 && cb.age == 3);
  count_weak_solve(cb, 1e-3, 1e-10, 0.99e-4);
  count_weak_solve(cb, 1e-11, 1e-10, 1e-14);   // (below the target: not weak)
  CHECK(cb.weak == 0 && cb.age == 3);
  count_weak_solve(cb, 1e-3, 1e-10, 0.99e-4);
  count_weak_solve(cb, 1e-3, 1e-10, 0.99e-4);
  CHECK(cb.weak == 0 && cb.age >= GL_CHEB_RELEARN);
  // the loose interval serves reductions down to GL_CHEB_LOOSE, where there is one
  cb.lmin = 0.1;
  cb.lmax = 3.0;
  double a, b;
  cheb_interval(cb, 1.0, 1e-3, &a, &b);
  CHECK(a == 0.9 * 0.1 && b == 1.06 * 3.0 * 1.0);
  cb.lmin0 = 0.5;
  cb.lmax0 = 2.0;
  cheb_interval(cb, 1.0, 3e-5, &a, &b);
  CHECK(a == 0.9 * 0.5 && b == 1.06 * 2.0 * 1.0);
  cheb_interval(cb, 0.5, 2.9e-5, &a, &b);
  CHECK(a == 0.9 * 0.1 && b == 1.06 * 3.0 * 0.5);
}

int main() {
  forcing_mode();
  second_solve_guess();
  forcing_and_evaluation();
  dot_free_solves();
  CHECK(RunMemory().d2_backoff == GL_D2_BACKOFF_MIN && RunMemory().fg2_red == 0.0 && !PreparedStep().valid);
  PreparedStep p;
  p.valid = p.guess.valid = true;
  p.drop();
  CHECK(!p.valid && !p.guess.valid);
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  return failures ? 1 : 0;
}
