// The RD time stepper's memory and decisions (gl_step, solver.hip): what a run remembers from one step to the next, what one
// step knows about itself, and every decision that is a function of scalars.  Plain C++17 -- no device types, no handle -- so
// that tests/step_policy_check.cpp exercises the rules on the host.
#pragma once
#include <algorithm>
#include <cmath>
#include "../../include/glims_hip.h"   // (glims_options: plain C)

// Dot-free RD linear solves (Chebyshev semi-iteration, solver.hip): interval of the spectrum of Dinv A(c) the right-hand sides
// of this run excite, from the Lanczos coefficients of recorded PCG solves
struct ChebState {
  bool valid = false;                    // [lmin, lmax] usable
  // Two intervals: [1] from all PCG solves of the last learning step, [0] from its LOOSE ones only (reduction >= GL_CHEB_LOOSE):
  // what a tight solve has to resolve (components of relative size 1e-7 at the ends of the spectrum) a solve to 3e-4 may
  // ignore -- brain-like mesh at 1 M nodes: [0.70, 1.96] against [0.033, 3.63]
  double lmin = 0.0, lmax = 0.0;         // [1]
  double lmin0 = 0.0, lmax0 = 0.0;       // [0]; lmax0 = 0: none (then [1] serves)
  double acc_lmin = 0.0, acc_lmax = 0.0; // ... being accumulated by the current learning step
  double acc_lmin0 = 0.0, acc_lmax0 = 0.0;
  int learned = 0, learned0 = 0;         // PCG solves that contributed to acc_* / acc_*0
  int age = 0;                           // steps since the interval was measured
  int weak = 0;                          // consecutive dot-free solves that contracted far less than they were sized for
  int m_hint[2] = {0, 0};                // passes the device chose for the last warm-started solve (bounds the next one's launches):
                                         // [0] a step's first solve, [1] its second
  // Which iteration a solve AFTER a step's first one uses (the first, loose one always takes the dot-free iteration): PCG
  // needs fewer operator passes for a tight solve (superlinear convergence: 8 iterations where the Chebyshev bound asks for
  // 13-15 at config C4), the dot-free iteration cheaper ones.  cost_ratio = cost of a Chebyshev pass / cost of a PCG
  // iteration from a byte model of the two (solver.hip, cheb_cost_ratio: 0.74 at 10 M rows, 0.66 at 1.26 M -- measured 0.74 /
  // 0.6), pcg_its_per_decade from the tightest PCG solve of the last learning step.  Deterministic (no timings): the
  // iteration path of a run stays reproducible bit for bit.  0 = unknown (then: Chebyshev).
  double cost_ratio = 0.0, pcg_its_per_decade = 0.0;
  int pcg_best_its = 0;                  // iterations of the solve pcg_its_per_decade comes from
};

// Fused guess pass (gl_step): the first pass of a dot-free solve that the sweep before it has run (guess in cg_u, y_1 in cg_p)
struct FusedGuess {
  bool valid = false;
  int kind = 0;               // 1: from the guess, 2: from zero
  double ia = 0.0, ib = 0.0;  // the interval whose theta the sweep used
  int second_order = 0;       // how the guess was extrapolated
  double rr = 0.0;            // kind 1: |res - A u|^2 of the guess, from the sweep's mail (the solve's count follows from it)
};

// The next step as the sweep that confirmed this one prepared it: cg_r / b / vA hold its first assembly, r0 is its first residual
// norm, `guess` the first pass of its first solve where the sweep carried one.  Whatever touches the state, the operator or the
// Krylov work vectors drops all of it.
struct PreparedStep {
  bool valid = false;
  double r0 = 0.0;
  FusedGuess guess;
  void drop() { *this = PreparedStep(); }
};

// Everything the stepper remembers from one step to the next and that belongs to ONE run: glims_set_state starts from
// RunMemory(), so a restarted run takes the iteration path of a fresh handle.
struct RunMemory {
  // default forcing: how a step's FIRST solve is run (gl_step).  0: tolerance 0.3 cg_rtol; 1: the same + midpoint correction;
  // 2: cg_rtol, no correction (for nw_hold steps after a step that took three iterations even with the correction)
  int nw_mode = 0, nw_hold = 0, nw_since = 0, nw_steps = 0;   // nw_steps: steps since glims_set_state
  double nq_first_ratio = 1e-3;            // residual contraction of the last step's first Newton iteration
  int nq_skip_steps = 0;                   // steps left without cheap evaluations (after a poor contraction)
  int cg_hint[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // PCG iterations of the k-th Newton solve of the previous step
  bool have_d2 = false;                    // cheb_delta2 holds the previous step's second correction (same run, no jump in the state)
  int d2_depth = 0;                        // consecutive steps whose second correction was kept (2: d2_prev is a real one)
  int d2_regime = -1;                      // the step cheb_delta2 comes from: passes of its FIRST solve and the forcing mode (what that solve
                                           // left behind depends on them) ...
  double d2_r1 = 0.0;                      // ... and the Newton residual its second solve started from
  int d2_off = 0, d2_backoff = 8, d2_good = 0;   // steps for which the guess stays unused after one that missed the target; the length
                                           // doubles with every miss (8 .. 256) and returns to 8 after 32 guesses that did not
  int ws_depth = 0;                        // 1 once ws_du (the increment of the step before the last) holds a real increment
  bool have_c_old = false;                 // c_old holds the state at the start of the previous step
  double fg2_red = 0.0;                    // reduction the last second dot-free solve was asked for (0: none yet)
  ChebState cheb;
};

// What one step knows about itself: its modes, fixed when it starts, and what has happened in it so far
struct StepFacts {
  bool verbose = false, verbose_cheb = false, rd_mg = false;   // (from gl_step: the two environment flags, read once per call)
  bool extrapolate = false, warm_on = false, fixed_forcing = false, cheb_allowed = false, cheb_learning = false, fuse_on = false;
  bool quad = false, midpoint = false;     // cheap residuals possible; the first right-hand side gets the midpoint correction
  int nw_mode = 2, regime_now = -1;        // (regime_now: below)
  double first_rtol = 0.0, r0 = 0.0, target = 0.0, ratio_est = 0.0;   // ratio_est: contraction of the previous Newton iteration
                                                                      // (first one: of the last step's first)
  int64_t newton0 = 0, cg0 = 0;            // the handle's counters when the step began
  FusedGuess fg1, fg2;                     // guess passes that came with a sweep: of this step's first solve, of its second
  bool base_is_current = true, ck_is_c0 = false;   // see gl_step (copies of iterates)
  // What has happened in the step.  regime_now: passes of its first solve when it was a dot-free one, and the forcing mode;
  // r1_now: the Newton residual its second solve started from.  pcg_rest: a dot-free solve under-delivered, the remaining
  // solves run PCG; used_warm2: the second solve started from the previous step's second correction; warm2_miss: ... and left
  // the residual above the target (the third iteration is the guess's doing); d2_pcg: the second solve was a PCG one;
  // d2_written: it left its correction in cheb_delta2; rebase: (c) of the residual rules, the next evaluation is a sweep.
  double r1_now = 0.0;
  bool pcg_rest = false, used_warm2 = false, warm2_miss = false, d2_pcg = false, d2_written = false, rebase = false;
  void second_solve_ran(double nr, bool warm2, bool pcg) {   // (its correction is in cheb_delta2)
    d2_written = true;
    d2_pcg = pcg;
    r1_now = nr;
    used_warm2 = warm2;
  }
};

// ---- the dot-free solves' interval ---------------------------------------------------------------------------------------
// Safety factors on the chosen interval.  A lower end set too low only costs iterations (prototype: 0.5 x -> +50 %); an upper
// end set too low makes the iteration diverge on what lies above it, so that end gets more room.
// GL_CHEB_LOOSE: reductions down to this use the interval of the loose learning solves; GL_PCG_COST_MARGIN: see prefer_pcg.
// GL_CHEB_RELEARN: steps after which the interval is measured again; GL_CHEB_LONG: solves that would need more passes run PCG.
static const double GL_CHEB_LO = 0.9, GL_CHEB_HI = 1.06, GL_CHEB_LOOSE = 3e-5, GL_PCG_COST_MARGIN = 0.95;
static const int GL_CHEB_RELEARN = 32, GL_CHEB_LONG = 48;
// the interval a solve that wants the reduction `red` uses (scale_hi: the handle's test hook on the upper end, 1 otherwise)
inline void cheb_interval(const ChebState& cs, double scale_hi, double red, double* a, double* b) {
  const bool loose = red >= GL_CHEB_LOOSE && cs.lmax0 > 0.0;
  *a = GL_CHEB_LO * (loose ? cs.lmin0 : cs.lmin);
  *b = GL_CHEB_HI * (loose ? cs.lmax0 : cs.lmax) * scale_hi;
}
// PCG instead of the dot-free iteration for a solve from |R| = nr to tol_lin (< nr) that the Chebyshev bound sizes at `passes`
inline bool prefer_pcg(const ChebState& cb, bool auto_linear, int it, int passes, double nr, double tol_lin) {
  // an ill-conditioned system (stiff step with the Jacobi preconditioner forced): the Chebyshev bound grows like
  // sqrt(kappa) per decade, PCG converges superlinearly there -- and a count cut off at GL_CHEB_MAX would be a weak solve
  if (passes > GL_CHEB_LONG) return true;
  if (it >= 1 && auto_linear && cb.cost_ratio > 0.0 && cb.pcg_its_per_decade > 0.0) {
    // a tight solve: PCG's iterations (from its rate in the last learning step) against the passes the Chebyshev bound
    // asks for, weighted by what each costs
    const double its_pcg = std::ceil(cb.pcg_its_per_decade * std::log10(nr / tol_lin)) + 1.0;
    return its_pcg < GL_PCG_COST_MARGIN * cb.cost_ratio * passes;
  }
  return false;
}
// A dot-free solve that contracts, but far less than it was sized for (10 x its tolerance plus the quadratic remainder),
// has an interval that no longer fits what the right-hand sides excite: not a take-back -- the Newton iteration copes --
// but two of them in a row make the next step a learning step instead of waiting for the 32nd.
static const double GL_WEAK_FACTOR = 10.0;
inline void count_weak_solve(ChebState& cb, double nr, double target, double sized_for) {
  const bool weak = nr > target && nr > GL_WEAK_FACTOR * sized_for;
  cb.weak = weak ? cb.weak + 1 : 0;
  if (cb.weak >= 2) {
    cb.age = 1 << 20;
    cb.weak = 0;
  }
}

// ---- forcing -------------------------------------------------------------------------------------------------------------
// GL_FIRST_RTOL: a first solve in modes 0 and 1 runs at this x cg_rtol; GL_FLOOR_SAFETY: safety factor on the predicted
// quadratic remainder; GL_RATIO_MIN / MAX: bounds of an observed contraction used as a prediction; GL_TARGET_SHARE: no solve
// is asked for less than this x the Newton target; GL_REBASE_FACTOR: see needs_rebase; GL_REBASE_SKIP: decremented at the
// start of a step, so the next eight run with sweeps only.
static const double GL_FIRST_RTOL = 0.3, GL_FLOOR_SAFETY = 0.3, GL_RATIO_MIN = 1e-6, GL_RATIO_MAX = 0.5, GL_TARGET_SHARE = 0.5;
// (margin 3: with 1 the cheap pass reported convergence unpredicted -- pass + confirming sweep -- in 14-28 % of the steps
//  of C4 / C3, with 3 in 2 %; with 10 the failed confirmations are back)
static const double GL_SPEC_MARGIN = 3.0, GL_REBASE_FACTOR = 5.0;
static const int GL_REBASE_SKIP = 9;
// Forcing term.  The first solve of a step gets cg_rtol (1e-3): the quadratic term dt N(delta) delta that the step
// leaves behind is of that size anyway.  From the second solve on the Jacobian is the one of c_1 and Newton converges
// quadratically: the remainder after a solve from residual nr is ~ q nr^2 / r0, with q = the contraction the step's first
// iteration was observed to achieve (R_1 / r_0: what the quadratic term alone leaves).  Solving to cg_rtol x nr again
// would stop three decades short of that floor and spend a whole Newton iteration (evaluation, start-up of a solve) on
// them: the linear tolerance follows the floor instead (Eisenstat & Walker's "eta_k = O(|R_k|)").  Where Jacobi-PCG
// needs few iterations per decade (lattice configs: 3.1 Newton iterations per step either way) nothing changes; on the
// unstructured brain-like mesh a step takes 2.25 Newton iterations instead of 4 and 30 PCG iterations instead of 39
// (fewer restarts of the Krylov space): 3.86 -> 2.86 ms per step; C3 1.79 -> 1.65; C4 unchanged (10.7 vs 10.7-10.9).
// Safety factor on the predicted remainder: 0.3 (with 1.0 more steps need a third iteration: 2.95 / 1.68 ms).
// GLIMS_FLAG_FIXED_FORCING: cg_rtol always.
struct Forcing {
  bool adaptive = false;
  // the quadratic remainder the iteration is expected to leave; the linear solve's absolute tolerance; what the iteration is
  // expected to leave: the linear residual plus the quadratic remainder
  double floor_pred = 0.0, tol_lin = 0.0, pred_next = 0.0;
};
inline Forcing forcing_term(const glims_options& o, int it, double nr, double r0, double target, double first_rtol,
                            double first_ratio, double ratio_est) {
  Forcing f;
  f.adaptive = (o.flags & GLIMS_FLAG_FIXED_FORCING) == 0 && it >= 1;
  f.floor_pred = std::min(GL_RATIO_MAX, std::max(GL_RATIO_MIN, first_ratio)) * nr * (nr / std::max(r0, 1e-300));
  f.tol_lin = std::max(std::max(o.cg_atol, GL_TARGET_SHARE * target),
                       f.adaptive ? std::min(o.cg_rtol * nr, GL_FLOOR_SAFETY * f.floor_pred)
                                  : (it == 0 ? first_rtol : o.cg_rtol) * nr);
  f.pred_next = f.adaptive ? f.tol_lin + f.floor_pred : nr * std::min(GL_RATIO_MAX, std::max(GL_RATIO_MIN, ratio_est));
  return f;
}
// Newton converges quadratically here (the nonlinearity is exactly quadratic): once the residual before the
// solve was below ~sqrt(rtol) of the initial one, the next sweep will almost surely only confirm convergence,
// so let it also assemble the next step (costs one extra mass SpMV, saves a whole sweep per step).
// Otherwise the evaluation after this solve is the cheap one -- both known before the solve.
// With cheap evaluations a sweep that FAILS to confirm convergence is the expensive mistake (C4, steps 60-160 of the
// 500: four iterations per step, the third evaluation a sweep that did not converge), so the prediction there is
// "this iteration contracts like the previous one did": residual x last observed contraction <= target.
inline bool speculate_next(const glims_options& o, bool extrapolate, bool quad, double pred_next, double target, double nr,
                           double r0) {
  return !extrapolate && (quad ? pred_next <= GL_SPEC_MARGIN * target : nr <= 1e-4 * std::sqrt(o.newton_rtol / 1e-10) * r0);
}
// (not after the step's FIRST solve, which takes the big step: its sweep moves A_0 to c_1, within ~1e-3 |delta_0| of
//  the step's solution -- with A(c^n) kept instead every later iteration contracts by dt rho |c - c^n| ~ 3e-3 only,
//  and the count per step rose from 3.35 to 3.65 at config C4)
inline bool cheap_next(bool quad, bool speculate, bool rebase, int it) { return quad && !speculate && !rebase && it >= 1; }
// (c): the solve was asked for cg_rtol (cheap evaluations only happen where that bound, not the Newton target,
// set its tolerance); a residual five times larger is the Jacobian's age showing
inline bool needs_rebase(const glims_options& o, const Forcing& f, double nr, double nr_before) {
  return nr > GL_REBASE_FACTOR * (f.adaptive ? std::max(f.tol_lin, f.floor_pred) : o.cg_rtol * nr_before);
}

// ---- the second solve's guess ----------------------------------------------------------------------------------------------
// (what the first solve leaves behind is a fixed polynomial of the operator applied to the extrapolation error: a first solve
//  of another degree leaves something else -- config C4 / 8, step 24: 3 -> 2 passes, |R_1| 1.8e-5 -> 2.8e-5 -- and the
//  second corrections before and after such a change do not continue each other)
// The same for the forcing mode (a midpoint-corrected first right-hand side leaves a residual twenty times smaller), and
// the check that needs no model: the correction is proportional to the residual it removes, so |R_1| has to continue too.
static const double GL_D2_R1_LO = 0.7, GL_D2_R1_HI = 1.43;
static const int GL_D2_REGIME_PCG = 500;      // added to the regime of a step whose second solve was a PCG one
inline bool d2_continues(const RunMemory& m, int regime, double nr) {
  return regime == m.d2_regime && nr > GL_D2_R1_LO * m.d2_r1 && nr < GL_D2_R1_HI * m.d2_r1;
}
// A second solve that started from the guess and left the residual above the target (by any margin): what it left is more
// likely the guess's doing (components that the previous steps' solves amplified instead of damping come back with it) than
// the quadratic remainder -- the guess stays unused for a while (the solves from zero in between start clean): 8 steps,
// doubling with every miss up to 256; 32 guesses in a row that did not miss return the length to 8.
static const int GL_D2_BACKOFF_MIN = 8, GL_D2_BACKOFF_MAX = 256, GL_D2_GOOD_RUN = 32;
inline void d2_missed(RunMemory& m) {
  m.d2_off = m.d2_backoff;
  m.d2_backoff = std::min(GL_D2_BACKOFF_MAX, 2 * m.d2_backoff);
  m.d2_good = 0;
}
inline void d2_hit(RunMemory& m) { if (++m.d2_good >= GL_D2_GOOD_RUN) m.d2_backoff = GL_D2_BACKOFF_MIN; }

// ---- the forcing mode after a step -----------------------------------------------------------------------------------------
// The mode follows the outcome: 0 until two steps within a few take three iterations (one step in ten doing so is cheaper
// than the correction's pass on every step: +4 for such a step, -1 otherwise, threshold 6), then 1; a step that takes three
// WITH the correction sends the next 16 back to cg_rtol without it (mode 2); every 64th step in mode 1 tries mode 0 again.
// (the first steps of a run have no increments to extrapolate from and take three iterations whatever the mode: they do
//  not speak for it; a third iteration that the second solve's guess caused says nothing about the forcing mode either)
static const int GL_NW_SETTLE = 8, GL_NW_MANY = 3, GL_NW_HOLD_UP = 4, GL_NW_HOLD_SWITCH = 6, GL_NW_MODE2_STEPS = 16,
                 GL_NW_RETRY = 64;
inline void forcing_mode_after_step(RunMemory& m, bool counts, int64_t iterations, bool warm2_miss) {
  ++m.nw_steps;
  if (!counts || m.nw_steps <= GL_NW_SETTLE) return;
  const int64_t count = iterations - (warm2_miss ? 1 : 0);
  if (m.nw_mode == 0) {
    m.nw_hold = count >= GL_NW_MANY ? m.nw_hold + GL_NW_HOLD_UP : std::max(0, m.nw_hold - 1);
    if (m.nw_hold >= GL_NW_HOLD_SWITCH) {
      m.nw_mode = 1;
      m.nw_since = m.nw_hold = 0;
    }
  } else if (m.nw_mode == 1) {
    if (count >= GL_NW_MANY) {
      m.nw_mode = 2;
      m.nw_hold = GL_NW_MODE2_STEPS;
    } else if (++m.nw_since % GL_NW_RETRY == 0) {
      m.nw_mode = 0;
      m.nw_hold = 0;
    }
  } else if (--m.nw_hold <= 0) {
    m.nw_mode = 1;
    m.nw_since = 0;
  }
}
