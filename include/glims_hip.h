/*
 * glims_hip.h -- C-ABI of libglimship.so, the MI355X (gfx950) backend of the forward time-stepping
 * path of GlimSLib's TumorGrowth / TumorGrowthBrain models.
 *
 * The reference has no FFI of its own: its seam is the Python protocol of FenicsSimulation
 * (glimslib/simulation/simulation_base.py:36-158), where run() (:236-317) only touches
 * `self.solver.solve()` (:285/:302), `self.solution` and `u_previous.assign(self.solution)` (:312).
 * This library replaces what sits behind `self.solver.solve()` -- DOLFIN assemble + PETSc SNES/LU,
 * set up in glimslib/simulation/simulation_tumor_growth.py:78-140 and
 * glimslib/simulation/simulation_tumor_growth_brain.py:24-125 -- and the surrounding n-step loop.
 * Each entry point below names the reference interface it stands in for.
 *
 * Conventions
 *   - plain C, opaque handle, caller-owned host buffers (row-major, contiguous), no global state;
 *   - every function returns a status: GLIMS_OK (0), GLIMS_NOT_CONVERGED (1), GLIMS_NAN (2),
 *     or a negative GLIMS_E_* code; glims_last_error() gives the message of the last failure;
 *   - one handle = one device + its own HIP streams; a handle is not thread-safe, distinct handles are;
 *   - node/cell indices are 0-based and local to the handle (rank-local in a partitioned run);
 *   - displacement dofs are node-major interleaved: dof = node*dim + component
 *     (the reference's mixed space W = [P1^dim, P1], simulation_tumor_growth.py:67-72);
 *   - all floating point is IEEE fp64.
 *
 * Environment variables read by the library (everything else is a glims_options field):
 *   GLIMS_VERBOSE        any value: timing lines of the set-up phases and the solver's one-off decisions (preconditioner,
 *                        spectral interval of the dot-free solves, solves taken back) on stderr
 *   GLIMS_VERBOSE_CHEB   any value: one line per dot-free RD solve (residual before / after, tolerance, passes)
 *   GLIMS_DERIVE_TIMING  any value: glims_derive puts a HIP event pair around its cell pass and around its gather and prints one
 *                        line per projection with both times on stderr (tools/derive_cost.py; a synchronisation per pass)
 *   GLIMS_OBSERVE_TIMING any value: glims_observe puts a HIP event pair around each source's pass and prints one line per source
 *                        with the time on stderr (a synchronisation per source)
 *   GLIMS_OBSERVABLE_TIMING any value: the stored volume misfit terms put a HIP event pair around their cell pass and around their
 *                        gather and print one line per pass with both times on stderr (tools/observable_term_cost.py); a pass
 *                        with a deformed term adds a line with the times of its load kernel and of the load's gather
 *   GLIMS_HOST_THREADS   OpenMP team of the host-side symbolic phase (default: the CPUs this process may use,
 *                        divided by the ranks on the host)
 *   GLIMS_HOST_SYMBOLIC  TEST HOOK: glims_create runs the host (OpenMP) implementation of the symbolic phase instead of
 *                        the device one -- same structures, array by array (tests/test_gpu_symbolic.py)
 *   GLIMS_WIN_LIMIT      TEST HOOK: at most this many (<= 32) column windows per 64-row slice before a slice falls back
 *                        to 4-byte column indices -- lets tests/ exercise the mixed 16-bit / 32-bit index path on
 *                        meshes whose slices would all be compressible
 *   GLIMS_CHEB_TEST_SCALE_HI  TEST HOOK (read once by glims_create, per handle): factor on the measured upper end of the
 *                        spectral interval of the dot-free RD solves -- 0.5 makes their polynomial diverge on part of the
 *                        right-hand side, so that tests/ can exercise the take-back / PCG fallback path
 *   GLIMS_MG_BOX_MIN_NODES  TEST HOOK: smallest replicated first grid (nodes, at least 6 001) on which a partitioned run
 *                        limits each rank's smoothing to its work box (see GLIMS_FLAG_MG_WHOLE_GRID), instead of the
 *                        library's estimate of what that saves -- lets tests/ exercise the path on small meshes
 */
#ifndef GLIMS_HIP_H
#define GLIMS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLIMS_ABI_VERSION 6

enum {
  GLIMS_OK = 0,
  GLIMS_NOT_CONVERGED = 1,   /* Newton or Krylov hit its iteration cap (reference: exception from solver.solve(),
                                swallowed at simulation_base.py:303-305 -> "warn, stop, return last solution") */
  GLIMS_NAN = 2,             /* non-finite residual */
  GLIMS_E_USAGE = -1,        /* bad argument / wrong call order */
  GLIMS_E_HIP = -2,          /* HIP runtime error */
  GLIMS_E_RCCL = -3,         /* RCCL error */
  GLIMS_E_NO_DEVICE = -4     /* no usable gfx950 device: the library has no CPU fallback */
};

typedef struct glims_ctx glims_ctx;

/* Solver options.  The reference hard-codes 'snes' with DOLFIN defaults (simulation_tumor_growth.py:126-130:
 * SNES rtol 1e-9, atol 1e-10, max_it 50, linear_solver 'default' = sparse LU); this backend replaces LU by
 * Jacobi-preconditioned CG and therefore converges *tighter* than those defaults. */
typedef struct glims_options {
  double dt;              /* params.sim_time_step (simulation_tumor_growth.py:108) */
  double newton_rtol;     /* ||R_k||_2 <= max(newton_atol, newton_rtol*||R_0||_2);            default 1e-10 */
  double newton_atol;     /*                                                               default 1e-13 */
  int    newton_maxit;    /*                                                               default 50    */
  double cg_rtol;         /* RD linear solve: ||r||_2 <= max(cg_atol, cg_rtol*||R_k||_2,
                             0.5*newton target)   (inexact Newton forcing term)            default 1e-3  */
  double cg_atol;         /*                                                               default 0     */
  int    cg_maxit;        /*                                                               default 5000  */
  double mech_rtol;       /* mechanics PCG: ||r||_2 <= max(mech_atol, mech_rtol*||b||_2)    default 1e-10 */
  double mech_atol;       /*                                                               default 0     */
  int    mech_maxit;      /*                                                               default 200000*/
  int    check_every;     /* Krylov iterations enqueued between host convergence polls when the
                             iteration count cannot be predicted from the previous solve    default 8     */
  int    flags;           /* GLIMS_FLAG_*                                                   default WARM_START */
  /* ---- ABI 2: elasticity solver.  The reference gets its robustness for nu -> 0.5 from a sparse LU of the monolithic
   * system (simulation_tumor_growth.py:126-130) and names AMG as the alternative
   * (simulation_tumor_growth_brain_quad.py:116-119); here: PCG preconditioned by one multigrid V-cycle. */
  int    mech_precond;    /* GLIMS_PRECOND_BLOCK_JACOBI | GLIMS_PRECOND_MULTIGRID                default MULTIGRID */
  int    mech_mixed;      /* inner PCG streams a single-precision copy of K_el under an fp64 iterative-refinement
                             loop: 0 off, 1 auto (block-Jacobi preconditioner and K_el larger than the Infinity
                             Cache; never with the multigrid preconditioner), 2 always              default 1     */
  int    mech_history;    /* right-hand sides / solutions of the last k solves kept for the least-squares initial
                             guess (K_el is linear and time independent), 0..16                     default 8     */
  int    mg_smooth;       /* Chebyshev degree of the pre- and of the post-smoother on every level
                             (1 = damped block-Jacobi)                                             default 3     */
  int    mg_coarse_nodes; /* coarsen until a grid has at most this many nodes; that level is solved with a dense
                             inverse computed once (Gauss-Jordan on the device)                     default 216   */
  double mg_h_factor;     /* spacing of the first auxiliary Cartesian grid in units of the mesh width (lattice meshes:
                             of the lattice constant per axis); 0 = 2 on one GPU, and in partitioned runs with a global
                             frame (glims_set_mg_frame), whose Cartesian levels are replicated on every rank, 2 / 3 / 4
                             for <= 2 / <= 6 / more ranks                                          default 0     */
  double mg_cheb_ratio;   /* the Chebyshev smoothers act on [lambda_max / ratio, lambda_max] of Dinv A;
                             0 = by mesh class: 30 on lattice meshes and on general meshes of bounded node spacing,
                             10 on meshes with long edges / slivers (measured)                       default 0     */
  int    time_kernels;    /* HIP-event pairs on the handle's stream around hot kernels of glims_step: 1 = the Krylov
                             SpMV, 2 = also the assembly sweep and the PCG vector update; 3 = instead the level-0
                             multigrid pass and the block SpMV of glims_solve_mechanics; results in glims_stats.*_steps / *_mech /
                             us_*_median (bench.py's roofline figures)                                default 0     */
  /* ---- ABI 3: preconditioner of the RD linear solves.  The reference's LU does not care how stiff a step is
   * (simulation_tumor_growth.py:126-130); Jacobi-PCG needs ~sqrt(2 dt D / h^2 ...) iterations per Newton solve, e.g.
   * 66 / 129 on the unit cube with D = 0.1, dt = 1 at n = 32 / 64 (BASELINE config C2 is such a case), 4-5 on the
   * mass-dominated brain-extent configs C3 / C4. */
  int    rd_precond;      /* GLIMS_RD_PRECOND_AUTO | _JACOBI | _MULTIGRID.  MULTIGRID: one V-cycle of the same auxiliary-grid
                             hierarchy as the elasticity solver's, with 1 x 1 blocks, built once per glims_setup on the
                             static part S = (1 - dt rho) M + dt K_D of the Jacobian (S^-1 A(c) has its spectrum in
                             [1, 1 + 2 dt rho c / (1 - dt rho)]).  AUTO decides at the first glims_step after glims_setup
                             from q = mean_i S_ii / M_ii: multigrid when the predicted Jacobi count sqrt(2 q) exceeds the
                             break-even (20 for >= 400 k rows, 45 for >= 50 k, 90 below); the choice and q are in
                             glims_stats.rd_precond_used / rd_stiffness_ratio.  General (non-lattice) meshes: four
                             times those break-even counts (the cycle is weaker and dearer there), and because the
                             prediction is poor on such meshes, AUTO also switches to the hierarchy after any step
                             whose OBSERVED Jacobi count per solve exceeds the break-even                 default AUTO  */
  int    rd_mg_smooth;    /* Chebyshev degree of the RD hierarchy's smoothers (1 = damped Jacobi); 0 = by mesh class: 1 on
                             lattice meshes, 3 on general ones.  Measured on the unit cube with D = 0.1, dt = 1 at 0.1 / 1 /
                             10 M rows: degree 1 on [lambda/10, lambda] 1.9 / 4.3 / 26.3 ms per step, degree 3 on
                             [lambda/30, lambda] 2.9 / 7.4 / 46.2 (Jacobi-PCG: 4.4 / 26.5 / 486); on a Delaunay mesh of
                             200 k random points degree 1 / 3: 77 / 40 iterations per solve.  mg_cheb_ratio = 0 means 10
                             for this hierarchy                                                           default 0     */
  /* ---- ABI 6: the Krylov iteration of the Jacobi-preconditioned RD solves, and how its operator streams are cached.  PETSc's
   * counterpart is the KSP type (-ksp_type cg | chebyshev) behind solver.parameters (simulation_tumor_growth.py:126-130). */
  int    rd_linear;       /* GLIMS_RD_LINEAR_AUTO | _PCG | _CHEBYSHEV.  CHEBYSHEV: the dot-free iteration -- ONE kernel per
                             iteration (operator pass with the Chebyshev recurrence in its epilogue; a step's first solve takes the
                             warm-start guess as its first iterate, so the product A u is that solve's first pass), no dot
                             product, no reduction kernel, no all-reduce in partitioned runs.  The iteration count follows from
                             the wanted reduction and an interval [lmin, lmax] of Dinv A(c) chosen from the spectral measure of the
                             run's own right-hand sides (Lanczos coefficients of PCG solves: all solves of the first step after
                             glims_set_state and of every 32nd step run PCG and (re)measure it; loose and tight solves keep
                             intervals of their own).  Every solve is followed by a Newton residual evaluation anyway: one that
                             did not contract is taken back, the interval dropped and the iteration repeated with PCG
                             (glims_stats.cheb_fallbacks); two that contract far less than sized for bring the next learning step
                             forward; a solve whose bound exceeds 48 passes runs PCG.  AUTO = CHEBYSHEV wherever the RD solves
                             are Jacobi-preconditioned, except that a tight solve goes to PCG when a byte model of the two
                             iterations and PCG's measured rate say it is cheaper; solves with the multigrid preconditioner
                             always use PCG.  The choice never depends on timings: runs are bitwise reproducible
                                                                                                          default AUTO  */
  int    stream_policy;   /* GLIMS_STREAM_AUTO | _NONTEMPORAL | _CACHED: cache policy of the operator's value / column-code
                             streams in the Krylov operator pass.  Non-temporal keeps the gathered vector in L2 when the
                             operator is far larger than the 256 MiB Infinity Cache (config C4: +3 %); default-policy loads
                             let a small operator (a 1/8 share of C4 per GPU) stay resident between the passes of a solve.
                             AUTO picks by the working set at glims_setup              default AUTO  */
} glims_options;

#define GLIMS_PRECOND_BLOCK_JACOBI 0
#define GLIMS_PRECOND_MULTIGRID 1
#define GLIMS_RD_PRECOND_AUTO 0
#define GLIMS_RD_PRECOND_JACOBI 1
#define GLIMS_RD_PRECOND_MULTIGRID 2
#define GLIMS_RD_LINEAR_AUTO 0
#define GLIMS_RD_LINEAR_PCG 1
#define GLIMS_RD_LINEAR_CHEBYSHEV 2
#define GLIMS_STREAM_AUTO 0
#define GLIMS_STREAM_NONTEMPORAL 1
#define GLIMS_STREAM_CACHED 2

#define GLIMS_FLAG_EXTRAPOLATE_GUESS 1  /* Newton guess c^n + (c^n - c^{n-1}) instead of c^n (reference: c^n) */
#define GLIMS_FLAG_FP32_JACOBIAN 4       /* OFF by default.  The Newton Jacobian A(c) is stored and streamed in single
                                           precision inside the Krylov solves (products, sums, all vectors and the Newton
                                           residual stay fp64, so the iteration still converges to the fp64 tolerance of
                                           the same fixed point); takes effect at glims_setup */
#define GLIMS_FLAG_MG_FP32_SMOOTHER 8     /* OFF by default.  The level-0 smoother of the elasticity multigrid streams a
                                           single-precision copy of K_el instead of the (scaled) half-precision one, and
                                           the first Cartesian grid keeps its single-precision stencils */
#define GLIMS_FLAG_MG_FP64_VECTORS 32    /* OFF by default.  The level-0 cycle vectors of the elasticity multigrid (iterate,
                                           direction, scaled residual) are kept in double instead of single precision; the
                                           preconditioned residual handed to the Krylov solver is double either way */
#define GLIMS_FLAG_FULL_NEWTON 128       /* OFF by default.  Every Newton iteration of the RD block re-assembles Jacobian and
                                           residual in a sweep.  Default: in the middle of a time step (after its second,
                                           third ... solve, unless convergence is expected) the residual follows from the
                                           Krylov solver's final residual plus the exactly quadratic term dt N(a) delta -- one
                                           pass over the incidence lists, the Jacobian of the previous sweep stays in use; the
                                           sweep after the first solve and the one that confirms convergence (true residual,
                                           next step's Jacobian) still run, and an iteration whose residual exceeds 5 x the
                                           linear tolerance falls back to sweeps */
#define GLIMS_FLAG_MG_WHOLE_GRID 64      /* OFF by default.  Partitioned runs with glims_set_mg_frame: every rank smooths the
                                           WHOLE replicated first grid instead of its work box (its part plus the smoothers'
                                           dependency margin) -- the same preconditioner up to rounding, more work per rank */
#define GLIMS_FLAG_INT32_COLUMNS 16       /* OFF by default.  Stream the 4-byte column indices everywhere instead of the 16-bit
                                           (window, offset) codes (same bits in every result; takes effect at glims_setup) */
#define GLIMS_FLAG_FIXED_FORCING 256      /* OFF by default.  Every linear solve of the RD Newton iteration is asked for cg_rtol x
                                           its right-hand side and no right-hand side gets the midpoint correction (steps of
                                           three to four Newton iterations: the textbook inexact Newton the tests compare
                                           with).  Default: a step's FIRST solve runs at 0.3 cg_rtol, with that correction once
                                           steps start taking a third iteration; from the second solve on the tolerance follows
                                           the quadratic remainder the iteration is about to leave (q |R_k|^2 / |R_0|, q observed
                                           in the step's first iteration) -- two Newton iterations per step */
#define GLIMS_FLAG_MG_NO_LUMPING 512      /* OFF by default.  Mesh -> first-grid Galerkin product of the multigrid hierarchies: mesh
                                           edges whose end points' parents lie more than the stencil radius apart lose their
                                           cross terms only.  Default: a far POSITIVE coupling is lumped onto the two rows' own
                                           diagonals (the edge's term taken out whole: positive semi-definite, row sums kept) --
                                           sliver meshes 51 / 45 / 35 -> 48 / 39 / 32 iterations; lattices and quality-controlled
                                           meshes have no such edges and are not affected (rebuilds the hierarchies) */
#define GLIMS_FLAG_WARM_START 2         /* first linear solve of a step starts from the increment extrapolated from the previous two steps',
                                           its second solve from the second correction extrapolated likewise (round 5; only where the
                                           previous steps' continue each other); iteration counts change, what a
                                           step returns does not -- the Newton tolerance decides that
                                           (ignored when GLIMS_FLAG_EXTRAPOLATE_GUESS is set) */

#define GLIMS_FLAG_NO_FUSED_GUESS 1024    /* OFF by default.  Default: an assembly sweep that is followed by a dot-free solve also runs
                                           that solve's first pass -- the guess pass of a step's first and second solve, or the
                                           start of a second solve from zero -- on the row it has just formed, instead of a
                                           launch that streams the Jacobian again (single rank, fp64 Jacobian, rows of at most
                                           32 entries; same bits in every result, glims_stats.cheb_fused_passes counts them).
                                           Set: the separate launches (A/B in one build) */
#define GLIMS_FLAG_NO_FUSED_MASS 2048     /* OFF by default.  Default: a sweep of the stepping path that is about to use a new
                                           right-hand side b = M c + load (the speculative sweeps' b2, a step's first b) forms
                                           that product itself from the (row, cell) incidence records it walks anyway -- for
                                           every row whose cells share one rho > 0: (M c)_i = (d+3)/rho sum_T w_T (s_T + c_i)
                                           -- and the mass SpMV runs over the slices with other rows only (interfaces of two
                                           rho, tissues with rho = 0; glims_stats.rd_mass_fallback_rows) or not at all.  Single
                                           rank, fp64 Jacobian, rows of at most 32 entries; the right-hand side differs from
                                           the SpMV's in the last bits (another summation order), results agree to ~1e-15;
                                           glims_stats.rd_mass_in_sweep counts the sweeps.  A step whose first b is formed
                                           before new Dirichlet values or the extrapolated guess enter the iterate keeps the
                                           SpMV for that b.  Set: the mass SpMV everywhere (A/B in one build) */
#define GLIMS_FLAG_SLOT_WORDS32 4096       /* OFF by default.  Default: the straight-line assembly sweeps (rows of at most 32
                                           entries) read the slots of an incidence record from a 16-bit word -- the row's own
                                           slot dropped, 5 bits for each other vertex of the cell -- instead of the 32-bit word
                                           with a byte per vertex: 2 bytes less per (row, cell) incidence and sweep, the same
                                           slots and the same bits in every result.  Set: the 32-bit words (A/B in one build;
                                           the compact records below embed the 16-bit fields and are switched off as well) */
#define GLIMS_FLAG_RECORD_WORDS_FULL 8192  /* OFF by default.  Default: a straight-line sweep reads the records of a COMPACT slice
                                           from one 32-bit word each -- the 16-bit slot fields and, in the upper 17 bits, the
                                           offset of the fp64 reaction weight's bit pattern from a per-slice base -- instead
                                           of the weight (8 B) and the slot word (2 B): 6 bytes less per (row, cell) incidence
                                           and sweep, decoded to the same 64 bits, so the same bits in every result.  A slice
                                           is compact where its weights differ by rounding noise only (congruent cells of one
                                           rho: lattices, voxel meshes; glims_stats.rd_rec_compact_slices); the other (full)
                                           slices keep today's streams.  fp64 Jacobian with 16-bit column codes only.
                                           Set: weight + slot word for every slice (A/B in one build) */
#define GLIMS_FLAG_NO_VALUE_CODES 16384    /* OFF by default.  Default: a pass of the dot-free Krylov solve reads a slice of the
                                           Jacobian whose stored values ARE those of the static operator S, bit for bit (away
                                           from the tumour fl(S + 2 dt N(c)) = S; the assembly sweep flags such slices, per
                                           slice and per sweep), from one 32-bit word per entry -- the 16-bit column code, a
                                           5-bit index into the slice's dictionary of 32 bit patterns and an 11-bit offset --
                                           instead of the value (8 B) and the column code (2 B), decoded to the same 64 bits,
                                           so the same bits in every result.  The words are built by glims_setup (4 bytes per
                                           padded entry of extra device memory); a slice of S that needs more than 32
                                           dictionary entries keeps the 10-byte stream (glims_stats.rd_scode_slices).  fp64
                                           Jacobian with 16-bit column codes on one rank only; partitioned handles, the PCG,
                                           the multigrid and the adjoint read the stored values as before.
                                           Set: no words are built and every pass reads the values (A/B in one build) */
#define GLIMS_FLAG_STORE_LINEAR_SLICES 32768 /* OFF by default.  Default: a straight-line assembly sweep that finds a slice of 64
                                           rows exactly linear (every value of A = S + 2 dt N(c) it has formed has the bits of
                                           its entry of S) where the previous sweep found and left it so does not store the
                                           slice's values: the memory holds those very bits already (8 B per entry and sweep
                                           less; glims_stats.rd_lin_kept_slices).  Every incidence is still streamed, every row
                                           assembled and tested, and every residual, diagonal and flag written; the stored
                                           Jacobian keeps its bits for every reader.  On the handles that keep the per-slice
                                           flags only (those of GLIMS_FLAG_NO_VALUE_CODES's default); every other handle
                                           stores every slice as before.
                                           Set: every sweep stores every slice (A/B in one build) */

typedef struct glims_stats {
  int64_t steps;            /* implicit time steps taken */
  int64_t newton_its;       /* Newton linear solves (RD) */
  int64_t rd_assemblies;    /* Jacobian+residual assembly sweeps */
  int64_t cg_its;           /* RD Krylov iterations = SpMV applications of A(c) */
  int64_t mech_solves;
  int64_t mech_cg_its;
  double  last_newton_res;  /* ||R||_2 at exit of the last step */
  double  last_cg_res;
  double  last_mech_res;
  double  ms_steps;         /* device time of glims_step calls (HIP events on the handle's stream) */
  double  ms_spmv;          /* accumulated by glims_apply only */
  int64_t n_rows;           /* owned rows */
  int64_t nnz;              /* structural nonzeros of the scalar operator (unpadded) */
  int64_t nnz_padded;       /* stored SELL-64 entries */
  int64_t n_corners;        /* (row, cell) incidences */
  int64_t nnz_idx16;        /* stored entries whose column is streamed as a 16-bit (window, offset) code */
  double  ms_spmv_steps;    /* time_kernels = 1 only: HIP-event time of the Krylov SpMV launches inside glims_step */
  int64_t n_spmv_steps;     /*   ... and how many of them really ran (launches skipped behind the decision word excluded) */
  /* ---- ABI 2 */
  int64_t failed_steps;     /* time steps whose Newton / Krylov solve gave up (not counted in `steps`) */
  int64_t mg_levels;        /* levels of the elasticity multigrid hierarchy incl. the mesh itself (0 = not built) */
  int64_t mg_cycles;        /* V-cycles applied */
  double  mg_complexity;    /* stored operator entries of all levels / entries of K_el */
  double  ms_mg_setup;      /* wall time of the last hierarchy set-up (transfer lists, Galerkin products, eigenvalue
                               estimates, coarse inverse) */
  double  ms_mech;          /* wall time spent in elasticity solves */
  /* time_kernels = 1 only; launches skipped behind the decision word (a few microseconds) are left out */
  double  ms_sweep_steps;   /* assembly sweeps (k_rd_assemble) inside glims_step */
  int64_t n_sweep_steps;
  double  ms_update_steps;  /* PCG vector updates (k_cg_update) of the RD solves inside glims_step */
  int64_t n_update_steps;
  double  us_spmv_median;   /* medians over the last glims_step call */
  double  us_sweep_median;
  double  us_update_median;
  /* ---- ABI 3 */
  int64_t rd_precond_used;  /* GLIMS_RD_PRECOND_JACOBI | _MULTIGRID: what the RD solves really use (0 = not decided yet) */
  double  rd_stiffness_ratio; /* q = mean over the rows of S_ii / M_ii, the number `auto` decides on */
  int64_t rd_mg_levels;     /* levels of the RD hierarchy incl. the mesh (0 = not built) */
  int64_t rd_mg_cycles;     /* V-cycles applied inside glims_step */
  double  rd_mg_complexity; /* stored operator entries of all levels / entries of S */
  double  ms_rd_mg_setup;   /* wall time of the last set-up of the RD hierarchy */
  /* time_kernels = 3 only: the two dominant kernels of glims_solve_mechanics (HIP events, eager launches) */
  double  ms_mgfine_mech;   /* level-0 passes of the elasticity multigrid (k_mg_fine) */
  int64_t n_mgfine_mech;
  double  us_mgfine_median;
  double  ms_spmvb_mech;    /* block SpMV of the Krylov iteration (k_spmv_block2) */
  int64_t n_spmvb_mech;
  double  us_spmvb_median;
  /* ---- ABI 4: Newton residuals from the quadratic structure of the RD residual (see GLIMS_FLAG_FULL_NEWTON) */
  int64_t rd_quad_updates;  /* residual evaluations through the incidence lists only (no sweep, no Jacobian) */
  double  ms_quad_steps;    /* time_kernels = 2: those passes (k_rd_quad), HIP events */
  int64_t n_quad_steps;
  double  us_quad_median;
  /* ---- ABI 5: which paths of the Newton iteration ran (the re-entrancy / parity tests assert on these) */
  int64_t midpoint_steps;   /* time steps whose first right-hand side carried the midpoint correction -dt N(u) u */
  int64_t rebase_events;    /* Newton iterations after which a cheap residual exceeded 5 x the linear tolerance: fresh Jacobian,
                               sweeps only for the next steps */
  /* ---- ABI 5: partitioned runs, per rank (what the first multi-GPU run needs to say where its time went) */
  int64_t halo_exchanges;   /* neighbour exchanges started by glims_step / glims_solve_mechanics (mesh halos and first-grid boxes) */
  int64_t halo_bytes;       /* bytes this rank SENT in them */
  double  ms_exchange;      /* time_kernels != 0: duration of the exchanges on the communication stream (pack -> last receive),
                               HIP events; 0 with a host transport (glims_set_transport: the callback is synchronous) */
  double  ms_exchange_exposed; /* time_kernels != 0: part of it the compute stream really waited for (not hidden behind the
                               interior slices) */
  int64_t allreduces;       /* scalar all-reduces of the Krylov / Newton iterations */
  int64_t reduce_transport; /* how they travel: 0 single rank, 1 node mailbox (inside the reduction kernel), 2 ncclAllReduce,
                               3 host callback */
  int64_t mg_grid1_bytes;   /* elasticity multigrid: bytes of the first Cartesian grid's operator held by this rank */
  /* ---- ABI 6 */
  int64_t halo_exchanges_timed; /* exchanges that carried an event pair (ms_exchange / this = time per exchange; the event pools hold
                               4096 pairs per glims_step call, exchanges of the multigrid's first grid and of host transports
                               carry none) */
  int64_t cheb_solves;      /* RD linear solves by the dot-free Chebyshev iteration (glims_options.rd_linear) */
  int64_t cheb_its;         /* ... their operator passes (also counted in cg_its: "Krylov iterations") */
  int64_t cheb_fallbacks;   /* ... taken back because the Newton residual did not contract; repeated with PCG */
  int64_t cheb_learn_solves;/* PCG solves whose Lanczos coefficients (re)measured the interval */
  double  cheb_lmin;        /* the interval of Dinv A(c) in use (0 = none yet) */
  double  cheb_lmax;
  double  ms_cheb_steps;    /* time_kernels != 0: launches of the dot-free iteration's kernel (k_cheb) inside glims_step */
  int64_t n_cheb_steps;
  double  us_cheb_median;
  int64_t stream_nontemporal; /* what stream_policy resolved to: 1 non-temporal, 0 cached */
  int64_t krylov_working_set; /* bytes the operator pass + vector update of one Krylov iteration touch (what AUTO decides on) */
  double  mg_box_fraction;  /* elasticity multigrid, partitioned runs: this rank's work box / the replicated first grid (1 = the
                               whole grid: not box-limited); with parts that are boxes (recursive coordinate bisection) ~ 1 / ranks
                               + the smoothers' margin */
  /* ---- appended under ABI 6 (readers of the older layout are unaffected) */
  int64_t cheb_fused_passes;/* first passes of dot-free solves (guess pass, or start from zero) that an assembly sweep ran and
                               the solve took over; still counted in cheb_its and cg_its (see GLIMS_FLAG_NO_FUSED_GUESS) */
  int64_t rd_mass_in_sweep; /* assembly sweeps that formed the mass product M c + load of their new right-hand side themselves
                               (see GLIMS_FLAG_NO_FUSED_MASS) */
  int64_t rd_mass_fallback_rows; /* owned rows whose mass product stays with the SpMV: cells of different rho, or rho = 0
                               (set by glims_setup / glims_set_materials; kept by glims_reset_stats) */
  int64_t cheb_host_counts; /* warm-started dot-free solves whose pass count the host chose: the solve's first pass came with
                               an assembly sweep, and |b - A u|^2 with that sweep's norms (no second reduction, no plan
                               kernel, no launch that returns at once); the other warm-started solves choose it on the device */
  int64_t cheb_fused_zero_starts; /* the folded first passes (cheb_fused_passes) of solves that start from zero: a count the host
                               always knew; cheb_fused_passes = cheb_host_counts + cheb_fused_zero_starts */
  int64_t rd_slot16_sweeps; /* assembly sweeps (glims_apply hooks included) whose straight-line launches read the 16-bit slot
                               words (in cs16 or inside the compact records); 0 under GLIMS_FLAG_SLOT_WORDS32 and on a mesh
                               without a straight-line class */
  int64_t rd_rec_compact_slices; /* slices of straight-line classes whose records fit the compact 32-bit word ... */
  int64_t rd_rec_full_slices;    /* ... and those that do not (both set by glims_setup; kept by glims_reset_stats) */
  int64_t rd_rec32_sweeps;  /* assembly sweeps (glims_apply hooks included) that read compact records for at least one slice; 0
                               under GLIMS_FLAG_RECORD_WORDS_FULL, GLIMS_FLAG_SLOT_WORDS32, GLIMS_FLAG_INT32_COLUMNS and
                               GLIMS_FLAG_FP32_JACOBIAN */
  int64_t rd_scode_slices;  /* slices of S whose entries all have a 32-bit value code (at most 32 dictionary entries) ... */
  int64_t rd_scode_uncoded_slices; /* ... and those that have none (both set by glims_setup, kept by glims_reset_stats; both 0
                               where no codes are built: GLIMS_FLAG_NO_VALUE_CODES, GLIMS_FLAG_FP32_JACOBIAN,
                               GLIMS_FLAG_INT32_COLUMNS, partitioned handles) */
  int64_t rd_lin_slices;    /* slices the latest assembly sweep found exactly linear (their values of A are S's, bit for bit),
                               read from the device by glims_get_stats; not a running count */
  int64_t cheb_coded_passes; /* launches of the dot-free pass in which at least one slice -- exactly linear and coded -- was read
                               from the 4-byte words (counted on the device, collected by glims_get_stats) */
  int64_t rd_lin_kept_slices; /* those of rd_lin_slices whose values the latest assembly sweep did not store, because the memory
                               held S's bits already (read from the device like rd_lin_slices; not a running count; 0 under
                               GLIMS_FLAG_STORE_LINEAR_SLICES) */
} glims_stats;

/* ---- lifetime -------------------------------------------------------------------------------------- */

/* Builds the device-resident discretisation for one mesh (rank-local sub-mesh in a partitioned run):
 * renumbering, SELL-64 sparsity, (row, cell) incidence lists, per-cell geometry.
 * Stands in for FenicsSimulation.__init__ + _setup_functionspace (simulation_base.py:91-109,
 * simulation_tumor_growth.py:67-72) and the cell-subdomain MeshFunction (helper_classes.py:402-444).
 *   dim        2 (triangles) or 3 (tetrahedra);  cells are [n_cells][dim+1] vertex indices
 *   n_own      nodes [0, n_own) are owned rows; nodes [n_own, n_nodes) are ghosts (single GPU: n_own == n_nodes)
 *   cell_label tissue id per cell, 0 <= label < 256
 *   device     HIP device ordinal */
int glims_create(glims_ctx** out, int dim, int64_t n_nodes, int64_t n_own, int64_t n_cells,
                 const double* xyz, const int32_t* cells, const int32_t* cell_label, int device);
int glims_destroy(glims_ctx* h);
const char* glims_last_error(const glims_ctx* h);   /* h may be NULL: error of the last failed glims_create */
int glims_abi_version(void);

/* ---- model data ------------------------------------------------------------------------------------ */

/* Per-label coefficient tables (what DiscontinuousScalar.eval_cell looks up per cell, helper_classes.py:47-58,
 * or TumorGrowthBrain's per-tissue constants, simulation_tumor_growth_brain.py:29-39,82-104).
 * All arrays have n_labels entries; label l of glims_create indexes them. */
int glims_set_materials(glims_ctx* h, int n_labels, const double* D, const double* rho,
                        const double* gamma, const double* E, const double* nu);
int glims_options_default(glims_options* opt);
int glims_set_options(glims_ctx* h, const glims_options* opt);

/* Dirichlet data (fenics.DirichletBC lists built at helper_classes.py:632-723).  n == 0 clears. */
int glims_set_dirichlet_u(glims_ctx* h, int64_t n, const int64_t* dof_ids, const double* values);
/* Concentration: the listed nodes are held at `values` from the next glims_step on.  As with fenics.DirichletBC the
 * data constrain the UNKNOWN of a step: the state that enters the step's 'u_previous' term keeps the values it has
 * (simulation_tumor_growth.py:115-117), the new values are written into the Newton iterate.  Time-dependent data: call
 * again before the next glims_step, as BoundaryConditions.time_update_bcs does for every step
 * (helper_classes.py:839-859).  Partitioned runs: a COLLECTIVE call -- every rank makes it, with its own constrained nodes
 * (n = 0 where it owns none): the next glims_step exchanges the halo of the iterate on all ranks. */
int glims_set_dirichlet_c(glims_ctx* h, int64_t n, const int64_t* node_ids, const double* values);

/* Load vectors already integrated by the host (NULL clears):
 *   rd_load[n_nodes]        = dt*( int s phi_i dx + oint g D phi_i ds )   (simulation_tumor_growth.py:119-120)
 *   mech_load[n_nodes*dim]  = int f.v dx + oint g.v ds                    (simulation_tumor_growth.py:112-113) */
int glims_set_rd_load(glims_ctx* h, const double* rd_load);
int glims_set_mech_load(glims_ctx* h, const double* mech_load);

/* (Re)assembles the time-independent operators for the current materials and dt:
 * M, S = (1 - dt rho) M + dt K_D, the per-incidence reaction weights, and -- if with_mechanics --
 * K_el (dim x dim blocks) and the coupling operator G.  Stands in for _setup_problem
 * (simulation_tumor_growth.py:78-140); cheap enough to call again after a parameter change
 * (run_for_adjoint, :142-155). */
int glims_setup(glims_ctx* h, int with_mechanics);

/* ---- state + time stepping --------------------------------------------------------------------------- */

/* c[n_nodes], u[n_nodes*dim] (u may be NULL = zero).  create_initial_value_function (helper_classes.py:983-986). */
int glims_set_state(glims_ctx* h, const double* c, const double* u);
int glims_get_state(glims_ctx* h, double* c, double* u);   /* either may be NULL */

/* `steps` counts converged steps only; a step whose solve gave up is counted in `failed_steps`, ends the call with
 * GLIMS_NOT_CONVERGED / GLIMS_NAN and leaves the iterate where the solver stopped (reference: simulation_base.py:301-305).
 * n_steps backward-Euler steps of the concentration equation, entirely on the device
 * (the `while` loop body solver.solve() + u_previous.assign, simulation_base.py:297-312, for the F_rd block). */
int glims_step(glims_ctx* h, int n_steps);

/* Solves K_el u = G c + f for the current concentration (the F_m block; it is linear in u and does not
 * feed back into c, simulation_tumor_growth.py:110-120, so it is only needed at recorded steps).
 * After the Krylov iteration the residual is recomputed with the fp64 operator (one pass) and the iteration continues
 * from it should it miss the tolerance; glims_stats.last_mech_res is that true residual. */
int glims_solve_mechanics(glims_ctx* h);

/* A copy of the counters.  On a handle that streams value codes (GLIMS_FLAG_NO_VALUE_CODES not set, fp64 Jacobian, 16-bit column
 * codes, one rank) the call also waits for the handle's stream and reads one byte per slice plus 1 KB from the device (about
 * 160 KB at 10 M rows): rd_lin_slices and rd_lin_kept_slices are the device's flags as they are now, and cheb_coded_passes includes the launches the
 * device has counted since they were last collected.  Every other handle gets the plain copy, without synchronisation.  (The
 * solver itself collects those launches once in 1024 coded passes, with one synchronisation of its stream.) */
int glims_get_stats(const glims_ctx* h, glims_stats* st);
int glims_reset_stats(glims_ctx* h);

/* ---- operator hooks (tests, roofline) ---------------------------------------------------------------- */

/* y = Op x, repeated `reps` times on the handle's stream and timed with HIP events (ms_total out, may be NULL).
 * which: 0 = current RD Jacobian A(c), 1 = S, 2 = M (scalar, [n_nodes]);  3 = K_el, ([n_nodes*dim], unconstrained);
 *        4 = G (x [n_nodes] -> y [n_nodes*dim]);  5 = A(c) through the kernel variant with the Krylov iteration's
 *        fused dot product;  7 = the MATRIX-FREE product (S + 2 dt N(c)) x rebuilt from the (row, cell) incidence lists
 *        for the current state c (equals which = 0 once A(c) has been assembled for that state; not used by the solver:
 *        measured 4.2x slower than the assembled product at 10 M rows -- 1.38 ms and 5.15 GB against 0.33 ms and 1.77 GB --
 *        profiles/r02_matfree_ab.txt);  8 = the assembly sweep at c = x with a zero right-hand side, y = -1/2 (A(x) + S) x
 *        (timing hook, tools/ab_sweep.py; with a state set, A(c) and its diagonal are re-assembled before the call returns);
 *        9 = the quadratic-term pass (k_rd_quad / k_rd_quad_s) with a = delta = x rounded to single precision: y starts at 0
 *        and every repetition runs the pass on it, y <- y - dt N(x) x, so `reps` repetitions return -reps dt N(x) x up to the
 *        pass's single-precision rounding (timing hook and TEST HOOK).  N(a)_ij = sum_T rho_T int_T a_h phi_i phi_j.  Rows with
 *        a Dirichlet value of the concentration (glims_set_dirichlet_c) are returned as exactly 0, ghost rows as 0.  No state is
 *        needed and neither the state nor A(c) is touched; the slice sums the last repetition left (|y|^2 per slice) can be read
 *        with glims_peek_partials;
 *        10 = TEST HOOK: y = M x + rd_load as the stepping path forms a step's first right-hand side where the sweep carries
 *        the mass product (GLIMS_FLAG_NO_FUSED_MASS not set): the mass SpMV over the slices with fallback rows, then the
 *        single-right-hand-side sweep at c = x, and the b it wrote is returned.  GLIMS_E_USAGE where that mode is off for the
 *        handle.  Like glims_rd_residual it drops the system a previous step prepared (the next step re-assembles); with a
 *        state set, A(c) and its diagonal are re-assembled before the call returns, as for which = 8.
 *        11 = TEST HOOK: the quadratic-term pass with a != delta, prepared as the stepper prepares it after a solve.  Needs a
 *        state (GLIMS_E_USAGE without one).  Every repetition runs the stepper's preparation kernel with c_new = x, c_k = the
 *        state c as glims_get_state returns it (Dirichlet values set since the last step are not yet in it) and c_0 = 0, i.e.
 *        a = x + c and delta = x - c, both formed in double and then rounded to single precision, and then the pass on y, which
 *        starts at 0: y <- y - dt N(x + c) (x - c), so `reps` repetitions return -reps dt N(x + c) (x - c).  Rows returned as
 *        0 and the slice sums: as for which = 9.  Like which = 8 .. 10 it drops the system a previous step prepared; the state
 *        and A(c) are not touched.
 *        12 = TEST HOOK: y_i = dinv_i x_i with the inverse diagonal as the most recent assembly sweep left it (glims_apply
 *        8 | 10, glims_rd_residual, a step): 1 / A_ii of that sweep's iterate, and exactly 1 on rows with a Dirichlet value of
 *        the concentration.  It feeds Jacobi-PCG and the folded first iterate and is visible nowhere else.  Nothing but the
 *        product is launched; the state, A(c) and a prepared system are not touched.  GLIMS_E_USAGE before any sweep has run
 *        on the handle.
 *        Ghost rows of y are returned as 0. */
int glims_apply(glims_ctx* h, int which, const double* x, double* y, int reps, double* ms_total);

/* Assembles A(c) and the Newton residual R(c; c_prev) for host vectors (ghost rows 0):
 *   R = 1/2 (A(c) + S) c - M c_prev - rd_load.  R may be NULL. */
int glims_rd_residual(glims_ctx* h, const double* c, const double* c_prev, double* R);

/* TEST HOOK: what the last incidence-list kernel -- the assembly sweep (glims_apply 8 | 10, glims_rd_residual, a step) or the
 * quadratic-term pass (glims_apply 9 | 11) -- left in its per-slice partial sums [slices][2]: out[k] = the sum of column k over
 * the slices in slice order, in double.  Column 0 is the squared norm of the rows the kernel wrote (padding rows of the last
 * slice, ghost rows and Dirichlet rows add 0), column 1 the second right-hand side's (0 where the kernel has none).  Reads
 * only: no run memory, mailbox or reduce chain is touched.  GLIMS_E_USAGE before glims_setup. */
int glims_peek_partials(glims_ctx* h, double out[2]);

/* Diagnostics of the symbolic phase (node renumbering, SELL-64 sparsity, incidence lists, column codes -- built on the
 * device by glims_create; DOLFIN's counterpart is the dofmap + AIJ preallocation behind fenics.FunctionSpace,
 * helper_classes.py:271-282).
 *   glims_get_numbering     old2new[n_nodes]: internal index of the caller's node i (ghosts keep their index)
 *   glims_pattern_checksum  64-bit FNV-1a hashes of the device arrays, in this order: slice offsets, columns, 16-bit
 *                           column codes, window bases, window flags, diagonal slots, incidence offsets, incidence slots,
 *                           incidence cells, interior slice list, boundary slice list, numbering, row lengths (13 values).  Two handles
 *                           with equal checksums hold identical discretisation structures (tests compare the device-built
 *                           structures with the host implementation kept behind the test hook GLIMS_HOST_SYMBOLIC). */
int glims_get_numbering(glims_ctx* h, int32_t* old2new);
int glims_pattern_checksum(glims_ctx* h, uint64_t out[13]);

/* ---- device-resident time series ----------------------------------------------------------------------------------
 * Results.add_to_results deep-copies the mixed solution on the host at every recorded step
 * (helper_classes.py:1128-1144, called from simulation_base.py:306-309).  With 288 GB of HBM the recorded
 * concentration fields can stay on the device instead (80 MB per step at 10 M nodes), and -- because the displacement of
 * a step depends only on that step's concentration (simulation_tumor_growth.py:110-120) -- the elastic solve of a
 * recorded step can be deferred until somebody asks for its displacement.
 *   glims_snapshot_save       copies the current concentration into a new device buffer, returns its id (>= 0)
 *   glims_snapshot_load       concentration of snapshot `id` -> host c[n_nodes]
 *   glims_snapshot_mechanics  solves K_el u = G c_id + f for that snapshot -> host u[n_nodes*dim]; the time-stepping
 *                             state is not touched (status as glims_solve_mechanics)
 *   glims_snapshot_clear      releases all snapshots */
int glims_snapshot_save(glims_ctx* h, int64_t* id_out);
int glims_snapshot_load(glims_ctx* h, int64_t id, double* c);
int glims_snapshot_mechanics(glims_ctx* h, int64_t id, double* u);
int glims_snapshot_clear(glims_ctx* h);

/* ---- discrete adjoint ----------------------------------------------------------------------------------------------------
 * The reference fits the tissue parameters by L-BFGS-B on a misfit J of the simulated fields, with dJ/dm from dolfin-adjoint's
 * fenics.ReducedFunctional.derivative (optimization_workflow/image_based_optimization.py:660-767, controls and derivative at
 * :700-708; the forward runs it differentiates: run_for_adjoint*, simulation_tumor_growth*.py:142-170).  Here the gradient is
 * the exact discrete adjoint of the backward-Euler / Newton scheme glims_step runs, on the device:
 * one linear solve with the step's own Jacobian A(c_n) (symmetric: the forward preconditioner and PCG carry it) and one
 * parameter-sensitivity pass per recorded step, backwards.
 *
 * glims_adjoint_record(h, 1) clears the trajectory, stores the current concentration as c_0 and from then on keeps a device
 * copy of c_n after every CONVERGED step (8 B per node and step; not one bit of the forward run changes).  glims_set_state while
 * recording starts a new trajectory at the new state.  A failed step, glims_setup / glims_set_materials, or a new Dirichlet
 * node SET of the concentration invalidate it (new Dirichlet values do not: they carry no parameter sensitivity).  on = 0
 * stops recording and releases the trajectory.
 *
 * Partitioned handles (world > 1): recording is per rank (the local n_nodes per step, not collective).  glims_adjoint_gradient
 * is COLLECTIVE: every rank calls it, with the same term list (SPMD: same count, order, steps, kinds, weights, levels and
 * smooths; each rank's targets in its own local numbering).  A rank whose arguments or trajectory are refused makes every rank
 * return GLIMS_E_USAGE (one all-reduce of the verdicts comes before any other collective).  J and the three per-label arrays
 * are global and bitwise the same on every rank; dJ_dc0 is in the local numbering, meaningful on the owned nodes (ghost
 * entries 0).  glims_adjoint_stats is per rank. */
int glims_adjoint_record(glims_ctx* h, int on);

/* One term of J, observed after recorded step `step` (0 = c_0).  `target` has n_nodes values (n_nodes * dim for
 * GLIMS_MISFIT_U_L2, node-major), in the caller's node order; level / smooth are read by GLIMS_MISFIT_C_THRESH only.
 *   GLIMS_MISFIT_C_L2      1/2 w (c_k - t)^T M (c_k - t)
 *   GLIMS_MISFIT_C_THRESH  1/2 w (h(c_k) - t)^T M (h(c_k) - t),  h(c) = 1/2 (tanh((c - level) / smooth) + 1) NODEWISE
 *                          (the reference's thresh(), image_based_optimization.py:1404-1407, is L2-projected instead)
 *   GLIMS_MISFIT_U_L2      1/2 w (u_k - t)^T M_vec (u_k - t),  u_k = K_el^-1 (G c_k + f) (needs glims_setup(with_mechanics=1)) */
#define GLIMS_MISFIT_C_L2 0
#define GLIMS_MISFIT_C_THRESH 1
#define GLIMS_MISFIT_U_L2 2
typedef struct glims_misfit {
  int64_t step;
  int kind;
  double level, smooth, weight;
  const double* target;
} glims_misfit;

/* J of the recorded trajectory and its gradient: dJ_dD / dJ_drho / dJ_dgamma [n_labels of glims_set_materials] with respect
 * to the per-label tables, dJ_dc0 [n_nodes] (caller's node order; may be NULL) with respect to the initial concentration.
 * Any output pointer except J may be NULL.  The load vector of glims_set_rd_load is taken as parameter-independent (a
 * Neumann flux term in it scales with D: the caller must not ask for dJ_dD then).  RD adjoint solves: PCG with the
 * preconditioner the forward solves use, to ||r|| <= 1e-12 ||rhs||; elastic solves to 1e-12 ||rhs||.  The forward state
 * (iterate, displacement, warm-start / Chebyshev / solve histories, glims_stats) is left exactly as it was; the same
 * trajectory gives the same bits on every call.  Stands in for fenics.ReducedFunctional.__call__ + .derivative
 * (image_based_optimization.py:700-708). */
int glims_adjoint_gradient(glims_ctx* h, int n_terms, const glims_misfit* terms, double* J, double* dJ_dD,
                           double* dJ_drho, double* dJ_dgamma, double* dJ_dc0);

/* glims_adjoint_gradient plus dJ_dE / dJ_dnu [n_labels of glims_set_materials], the derivatives with respect to the per-label
 * Young's modulus and Poisson ratio (glims_adjoint_gradient is this call with both NULL; any output except J may be NULL).
 * K_el and G are linear in each cell's Lame pair (mu_t, lam_t), so with u_k = K_el^-1 (G c_k + f) (its Dirichlet values in
 * place) and mu_k = K_el^-1 dJ/du_k (0 on the constrained dofs) at every step k that a GLIMS_MISFIT_U_L2 term observes:
 *   dJ/dp_t = sum_k mu_k^T (dG/dp c_k - dK/dp u_k) = gamma_t (2 mu' + d lam') C_t - (2 mu' A_t + lam' B_t),
 *   A_t = sum_k int_t eps(mu_k):eps(u_k),  B_t = sum_k int_t div mu_k div u_k,  C_t = sum_k int_t 1/(d+1) div mu_k sum_a c_k,a
 * (C_t per cell |T|/(d+1) div mu_k times the sum of c_k over its vertices), with
 *   p = E_t:   mu' = 1 / (2 (1 + nu)),        lam' = nu / ((1 + nu)(1 - 2 nu))
 *   p = nu_t:  mu' = -E / (2 (1 + nu)^2),     lam' = E (1 + 2 nu^2) / ((1 + nu)^2 (1 - 2 nu)^2).
 * A term list without GLIMS_MISFIT_U_L2 gives dJ_dE = dJ_dnu = 0 exactly.  The E / nu pass (one per-cell pass per observed
 * displacement step) runs only when dJ_dE or dJ_dnu is non-NULL; it adds no elastic solve, and the other outputs keep their
 * bits.  Collective on partitioned handles like glims_adjoint_gradient: every rank passes NULL or non-NULL dJ_dE / dJ_dnu
 * alike (GLIMS_E_USAGE on every rank otherwise); dJ_dE and dJ_dnu are bitwise the same on every rank. */
int glims_adjoint_gradient_full(glims_ctx* h, int n_terms, const glims_misfit* terms, double* J, double* dJ_dD,
                                double* dJ_drho, double* dJ_dgamma, double* dJ_dc0, double* dJ_dE, double* dJ_dnu);

/* Second order: J, the gradient of glims_adjoint_gradient (bitwise the same: the lambda sweep issues gradient's kernels and
 * solves in the same order on the same set-up) and
 * n_dir (1..8) Hessian-vector products H dm of the recorded trajectory, dm = (dD, drho, dgamma [n_labels], dc0 [n_nodes]).
 * Directions and products are laid out [n_dir][n_labels] and [n_dir][n_nodes] (caller's node order); a NULL direction array
 * is 0, any output except J may be NULL.  Per direction, with A(c) the step Jacobian (symmetric) and K_t, G_t the label-t
 * parts of the stiffness and coupling operators ("Second order"):
 *   tangent-linear sweep  A(c_n) dc_n = M dc_{n-1} - dt sum_t dD_t K_t c_n - dt sum_t drho_t int_t (c_n^2 - c_n) phi,
 *                         dc_0 = dir_c0 (or 0), dc_n = 0 on the Dirichlet nodes;
 *   second-order adjoint  A(c_n) nu_n = M nu_{n+1} + dg_n - 2 dt sum_t rho_t int_t dc_n lam_n phi - dt sum_t dD_t K_t lam_n
 *                         - dt sum_t drho_t int_t (2 c_n - 1) lam_n phi,  nu_{N+1} = 0, nu_n = 0 on the Dirichlet nodes;
 *   dg_n = d(dJ/dc_n + G^T mu_n): C_L2 w M dc;  C_THRESH w (h' M(h' dc) + h'' M(h - t) dc) nodewise;  U_L2 G^T dmu_k +
 *          sum_t dgamma_t G_t^T mu_k with du_k = K_el^-1 (G dc_k + sum_t dgamma_t G_t c_k), dmu_k = K_el^-1 w M_vec du_k;
 *   hv_D_t = -dt sum_n int_t (grad nu_n . grad c_n + grad lam_n . grad dc_n),
 *   hv_rho_t = -dt sum_n int_t (nu_n (c_n^2 - c_n) + lam_n (2 c_n - 1) dc_n),
 *   hv_gamma_t = sum_k (dmu_k^T G_t c_k + mu_k^T G_t dc_k),   hv_c0 = M nu_1 + dg_0.
 * RD solves (tangent-linear and second-order, every direction at every step): one n_dir-column Jacobi-PCG that shares a
 * multi-right-hand-side SpMV per iteration, each column stopped at ||r|| <= 1e-12 ||rhs||; when the handle uses the RD
 * multigrid (stiff steps) the V-cycle PCG runs column by column instead.  Column j of an n_dir-direction call has the bits
 * of a one-direction call in direction j.  Elastic
 * solves to 1e-12 ||rhs||, 2 per direction at each step a U_L2 term observes.  E and nu are first order only (no direction,
 * no product; glims_adjoint_hessian_full below has both).  Device memory on top of the trajectory: 8 n_dir B per node and recorded state (the stored dc_n) plus
 * O(n_dir) vectors; a call that does not fit returns GLIMS_E_HIP before it allocates.  The forward state and glims_stats are
 * left as they were; glims_adjoint_stats does not count this call.  stats (may be NULL) [4]: tangent-linear PCG iterations,
 * second-order PCG iterations, extra elastic solves, wall ms.  Partitioned handles: GLIMS_E_USAGE on every rank (no
 * collective is entered; glims_adjoint_hessian_spmd below is the collective call).  Stands in
 * for fenics.ReducedFunctional.hessian (the H that minimize_custom hands its optimizer, image_based_optimization.py:646). */
int glims_adjoint_hessian(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                          const double* dir_rho, const double* dir_gamma, const double* dir_c0, double* J, double* dJ_dD,
                          double* dJ_drho, double* dJ_dgamma, double* dJ_dc0, double* hv_D, double* hv_rho,
                          double* hv_gamma, double* hv_c0, double* stats);

/* glims_adjoint_hessian, collective on partitioned handles.  world <= 1: the same function, the same bits in every output.
 * world > 1, with the contract of the partitioned glims_adjoint_gradient: every rank calls it with the same term list
 * (targets in its local numbering), the same n_dir, the same dir_D / dir_rho / dir_gamma tables and the same NULL pattern of
 * the four direction arrays.  dir_c0 and hv_c0 are [n_dir][n_nodes] in the local numbering: the owned entries of dir_c0 are
 * read (its ghost entries are not trusted: dc_0 exchanges its ghosts after the upload), the owned entries of hv_c0 are
 * written and its ghost entries are 0.  J, the gradient arrays, hv_D, hv_rho and hv_gamma are bitwise the same on every rank
 * and on every call; J and the gradient are bitwise those of glims_adjoint_gradient on the same handle.  Each cell enters
 * the per-label sums on the smallest rank that owns one of its vertices; the ranks' sums are added in rank order.  The
 * n_dir-column PCG exchanges the ghosts of its operand before every multi-right-hand-side SpMV and takes its scalar step
 * from sums over all ranks (two all-reduces per iteration), so every rank runs the same iterations; column j still has the
 * bits of a one-direction call.  Before any other collective the ranks' verdicts -- arguments and trajectory, n_dir, the
 * NULL pattern, the stored image terms (count and steps), device memory -- go through one all-reduce: if any rank refuses,
 * every rank returns the same status (GLIMS_E_USAGE, or GLIMS_E_HIP for memory) and the handle is left as it was.  stats is
 * per rank (the iteration counts are the same on all ranks).  Single node; E and nu stay first order (second order in them:
 * glims_adjoint_hessian_full, one GPU). */
int glims_adjoint_hessian_spmd(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                               const double* dir_rho, const double* dir_gamma, const double* dir_c0, double* J,
                               double* dJ_dD, double* dJ_drho, double* dJ_dgamma, double* dJ_dc0, double* hv_D,
                               double* hv_rho, double* hv_gamma, double* hv_c0, double* stats);

/* glims_adjoint_hessian with directions and products in the per-label Young's modulus and Poisson ratio too (appended under
 * ABI 6): dm = (dD, drho, dgamma, dE, dnu [n_labels], dc0 [n_nodes]).  Layouts and NULL rules of glims_adjoint_hessian: dir_E /
 * dir_nu / hv_E / hv_nu are [n_dir][n_labels], a NULL direction array is 0, any output except J may be NULL; J and the six
 * gradient arrays are bitwise those of glims_adjoint_gradient_full, and with dir_E = dir_nu = NULL hv_D / hv_rho / hv_gamma /
 * hv_c0 are bitwise those of glims_adjoint_hessian.  The concentration does not depend on E or nu; K_el and G are linear in
 * each cell's Lame pair (m, l), so with (dm_t, dl_t) = dE_t d_E(m, l)_t + dnu_t d_nu(m, l)_t, kappa(m, l) = 2 m + d l,
 * dK = sum_t the stiffness with the pair (dm_t, dl_t), dG = sum_t (dgamma_t kappa_t + gamma_t kappa(dm_t, dl_t)) G_t per unit
 * coefficient, at every step k that a U_L2 term observes (u_k with its Dirichlet values, du_k = dmu_k = 0 on the constrained
 * dofs):
 *   K du_k = G dc_k + dG c_k - dK u_k,     K dmu_k = w M_vec du_k - dK mu_k,     dg_k += G^T dmu_k + dG^T mu_k,
 *   hv_p_t = gamma_t kappa(m_p, l_p) [C_t(dmu, c) + C_t(mu, dc)] - 2 m_p [A_t(dmu, u) + A_t(mu, du)]
 *            - l_p [B_t(dmu, u) + B_t(mu, du)] + [dgamma_t kappa(m_p, l_p) + gamma_t kappa(dm_p, dl_p)] C_t(mu, c)
 *            - 2 dm_p A_t(mu, u) - dl_p B_t(mu, u)          summed over k, for p = E, nu,
 *   (m_p, l_p) = d_p(m, l)_t, (dm_p, dl_p) = dE_t d_pE(m, l)_t + dnu_t d_pnu(m, l)_t  (A_t, B_t, C_t as in
 *   glims_adjoint_gradient_full; the derivatives: csrc/lame_derivs.h),
 *   hv_gamma_t gains kappa(dm_t, dl_t) sum_k C_t(mu_k, c_k); hv_D, hv_rho and hv_c0 change through dmu_k and dG^T mu_k alone.
 * No elastic solve is added (stats[2] as glims_adjoint_hessian): a direction in E / nu costs two row-owned passes of dK per
 * observed step (all columns at once), one more cell and row pass of dG^T mu and the E / nu sum pass per direction.  A term
 * list without GLIMS_MISFIT_U_L2 gives hv_E = hv_nu = 0 exactly.  Column j of an n_dir-direction call has the bits of a
 * one-direction call; the same trajectory gives the same bits on every call.  Device memory: 2 n_dir more vectors of
 * dim x n_nodes when dir_E or dir_nu is given, inside the check that glims_adjoint_hessian makes before it allocates.
 * GLIMS_E_USAGE, the handle left as it was: a partitioned handle (on every rank, before any collective), stored deformed image
 * terms, n_dir outside 1..8, a non-NULL dir_E / dir_nu / hv_E / hv_nu on a handle set up without mechanics. */
int glims_adjoint_hessian_full(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                               const double* dir_rho, const double* dir_gamma, const double* dir_c0, const double* dir_E,
                               const double* dir_nu, double* J, double* dJ_dD, double* dJ_drho, double* dJ_dgamma,
                               double* dJ_dc0, double* dJ_dE, double* dJ_dnu, double* hv_D, double* hv_rho, double* hv_gamma,
                               double* hv_c0, double* hv_E, double* hv_nu, double* stats);

/* Counters of the adjoint (not in glims_stats, whose layout is fixed): out[0] gradient calls, [1] backward steps,
 * [2] RD adjoint PCG iterations, [3] elastic solves, [4] their PCG iterations, [5] recorded states held now;
 * ms[0] wall time of the backward sweeps (may be NULL). */
int glims_adjoint_stats(const glims_ctx* h, int64_t out[6], double* ms);

/* L2 projection onto the P1 space: solves M x = rhs for `ncomp` right-hand sides stored [n_nodes][ncomp]
 * (rhs_i = int f phi_i dx, integrated by the caller), Jacobi-PCG to ||r|| <= rtol*||rhs|| per component.
 * Stands in for fenics.project(expr, FunctionSpace(mesh, "Lagrange", 1)) as used by the PostProcess classes
 * (helper_classes.py:1566-1618, 1736-1786).  Ghost entries of rhs are ignored, ghosts of x are filled. */
int glims_project(glims_ctx* h, const double* rhs, double* x, int ncomp, double rtol);

/* ---- samplers: a P1 field evaluated at arbitrary points --------------------------------------------------------------------
 * The reference evaluates FE functions off their mesh point by point: create_image_from_fenics_function loops function(Point)
 * over every voxel (glimslib/utils/data_io.py:176-225), and fenics.LagrangeInterpolator moves fields between non-matching
 * meshes (optimization_workflow/image_based_optimization.py:1410-1412, used at :1092; image_based_optimization_atlas.py:57,
 * 103-104).  Both are "evaluate a P1 field at points".  A sampler is a fixed set of query points located ONCE in the handle's
 * mesh and kept on the device as cell[p] and barycentric weights w[p][dim+1]; it is then applied to as many fields as the
 * caller likes.  A sampler needs only glims_create (with GLIMS_FIELD_HOST a handle made from a bare mesh is an interpolator
 * for any nodal array); it owns its buffers and touches neither the solver state nor glims_stats.
 *
 * The operator P:
 *   - barycentric coordinates lambda_a(x) of x in cell T from the cell's vertex coordinates, fp64, lambda_0 = 1 - sum lambda_a;
 *   - T accepts x iff min_a lambda_a >= -GLIMS_SAMPLE_EPS;
 *   - among the accepting cells the one with the SMALLEST CALLER CELL INDEX wins (independent of the internal renumbering);
 *   - no accepting cell: cell = -1, weights 0, sampled value = fill; the transpose ignores such points.
 * Location is an integer atomic min per (cell, point) pair, the transpose uses no float atomics: both are bitwise reproducible.
 *
 * Partitioned handles (world > 1): creation is rank-local, NOT collective.  A rank locates in its local cells and reports its
 * local cell index; merging P f over the ranks is the host program's (smallest GLOBAL cell id wins).  The fields' ghost values
 * must be current (glims_step / glims_solve_mechanics leave them so).  Cells on the cut exist on several ranks and a point on a
 * face, edge or vertex is accepted by several cells, so the ranks' local winners differ: until glims_sampler_resolve (below)
 * has been called, glims_sampler_apply_t returns GLIMS_E_USAGE there. */
#define GLIMS_SAMPLE_EPS 1e-10   /* far above the rounding kappa(T) 2^-52 of lambda on every mesh class this library runs
                                    (kappa <= 7.6e4 measured on random-point Delaunay meshes), twelve orders below a voxel */
#define GLIMS_FIELD_C 0            /* the current concentration */
#define GLIMS_FIELD_U 1            /* the current displacement (ncomp = dim; needs glims_setup(with_mechanics=1)) */
#define GLIMS_FIELD_SNAPSHOT_C 2   /* the device snapshot `snapshot` of glims_snapshot_save: no host round trip */
#define GLIMS_FIELD_HOST 3         /* nodal[n_nodes][ncomp], caller's node order */
#define GLIMS_SAMPLE_MAX_COMP 8

/* Points xyz[n][dim] (n = 0 is valid) / the voxel centres origin + index * spacing of a grid of size[dim] points per axis, x
 * fastest (point p = (k * size[1] + j) * size[0] + i: the order of an image array [z][y][x]); no coordinates are uploaded for a
 * grid.  flags is reserved and must be 0.  The id (>= 0) is valid until glims_sampler_destroy / glims_destroy. */
int glims_sampler_create_points(glims_ctx* h, int64_t n, const double* xyz, int flags, int64_t* id);
int glims_sampler_create_grid(glims_ctx* h, const double* origin, const double* spacing, const int64_t* size, int flags,
                              int64_t* id);
int glims_sampler_info(glims_ctx* h, int64_t id, int64_t* n_points, int64_t* n_found);   /* outputs may be NULL */
/* cell[n]: the caller's cell index or -1;  w[n][dim+1]: the weights in the vertex order of the caller's `cells` row.  Either
 * may be NULL. */
int glims_sampler_get(glims_ctx* h, int64_t id, int32_t* cell, double* w);
/* out[n][ncomp] = P f (ncomp 1..8; GLIMS_FIELD_C / _SNAPSHOT_C: 1, GLIMS_FIELD_U: dim); points outside the mesh get `fill`
 * (NaN is what the reference's images hold there).  nodal is read for GLIMS_FIELD_HOST only, snapshot for _SNAPSHOT_C only.
 * GLIMS_FIELD_DERIVED (defined with glims_derive below): the result of the last glims_derive, ncomp = its component count (1, or
 * d(d+1)/2 for a tensor); GLIMS_E_USAGE with nothing derived or another ncomp.  GLIMS_FIELD_XYZ (defined with the deformed
 * samplers below): the mesh's reference coordinates, ncomp = dim. */
int glims_sampler_apply(glims_ctx* h, int64_t id, int field, int64_t snapshot, const double* nodal, int ncomp, double fill,
                        double* out);
/* g[n_nodes][ncomp] = P^T r, r[n][ncomp], caller's node order; values of r at points outside the mesh are not read into any
 * sum.  Per cell, the products w r are summed in point order (long lists in fixed chunks, added in chunk order), per node
 * the cells in the order of the row's incidence list: the same bits on every call and on every handle of the same mesh. */
int glims_sampler_apply_t(glims_ctx* h, int64_t id, const double* r, int ncomp, double* g);
/* Collective.  Every rank passes its rank-local sampler `id` of the SAME points and cell_gid[n_cells]: the global id of each
 * of the caller's cells, strictly increasing in the caller's cell order (partition_mesh's cell_ids).  Afterwards the sampler
 * is RESOLVED: a point whose local winner is not the smallest global cell id over all ranks is dropped on this rank (cell -1,
 * weights 0), the transpose's lists are built from the kept points, and a point is COUNTED on the smallest rank that keeps it.
 * world <= 1: GLIMS_OK, nothing changes (the sampler is already global).
 * On a resolved sampler glims_sampler_info's n_found is the number of KEPT points, glims_sampler_apply fills the dropped
 * points with `fill`, and glims_sampler_apply_t works: r[n][ncomp] is the same on every rank, g comes back in the caller's
 * (local) node order with the OWNED rows complete and the ghost rows 0 -- an owned node has all its cells local and every
 * rank that holds a cell keeps the same points in it, so no exchange is needed; the bits are the same on every call.
 * GLIMS_E_USAGE on EVERY rank, with the sampler left as it was, when any rank has an unknown id, a null or not strictly
 * increasing cell_gid, a sampler that a stored image term uses, or another n_points (the verdicts are all-reduced before any
 * other collective).  Resolving twice is a no-op.  The keys travel in chunks of points through a buffer of at most 64 MiB. */
int glims_sampler_resolve(glims_ctx* h, int64_t id, const int64_t* cell_gid);
/* counted[n_points] (0/1); world <= 1 or unresolved: 1 where found */
int glims_sampler_get_counted(glims_ctx* h, int64_t id, uint8_t* counted);
int glims_sampler_destroy(glims_ctx* h, int64_t id);   /* glims_destroy releases what is left */

/* ---- deformed-configuration samplers and image warping ----------------------------------------------------------------------
 * The samplers above live in the REFERENCE configuration X.  An MR image shows the DEFORMED configuration x = X + u(X); the
 * reference's optimisation workflow builds its targets there by warping the result mesh with vtk and pushing images through ANTs
 * (image_based_optimization.py:876-941 _create_deformed_image, :264-292).  A deformed sampler locates its points in the mesh
 * whose node a sits at
 *     y_a = fl(X_a + fl(scale * u_a))            (two roundings, never contracted: numpy's  X + scale * u),
 * with the rules of the samplers above applied to those coordinates: acceptance with GLIMS_SAMPLE_EPS, the smallest caller
 * cell index wins (also where a FOLDED mesh overlaps itself), the winner's barycentric weights.  With scale = 0 it equals the
 * undeformed sampler bit for bit.  Since it keeps only (cell, nodes, weights), glims_sampler_apply / _apply_t / _get / _info /
 * _destroy and GLIMS_FIELD_DERIVED work on it unchanged: P f is f at the material point that sits at x_p.
 * GLIMS_FIELD_XYZ (every sampler) applies P to the mesh's reference coordinates: on a deformed sampler the back map X(x_p), the
 * exact inverse of the P1 map X -> X + scale u_h(X) where that map is one-to-one; on the others x_p itself.
 *
 * u_source (the constants are defined with glims_derive below): an id of glims_snapshot_save -- its displacement is solved as
 * glims_snapshot_mechanics solves it (U is written, the solve enters the elastic solve history), unless U already belongs to that
 * snapshot: the same memory glims_derive uses, so a derive and a deformed sampler of one step solve once between them, in either
 * order (glims_derive_info's elastic solves count both) --; GLIMS_DERIVE_CURRENT: U as it stands; GLIMS_DERIVE_HOST:
 * u_host[n_nodes*dim], caller's node order (neither c nor U is touched).  CURRENT and HOST change nothing on the handle; in
 * every case the concentration steps that follow keep the bits of a handle that never made the call.
 * The sampler is FROZEN: later steps, solves or glims_snapshot_clear do not move it.
 * Returns the worst status of the elastic solve (GLIMS_OK / GLIMS_NOT_CONVERGED / GLIMS_NAN; the sampler exists for the first
 * two).  GLIMS_E_USAGE with a reason, before anything is allocated or changed: a partitioned handle (world > 1), a snapshot or
 * CURRENT source on a handle set up without mechanics, an unknown snapshot, CURRENT before glims_set_state, HOST with a NULL
 * u_host, a non-finite scale, flags != 0, and everything the undeformed creators refuse.
 * glims_adjoint_image_terms refuses a deformed sampler: its points depend on the state through u, and a frozen-location
 * gradient would be silently inexact.  glims_adjoint_deformed_image_terms (below) is the term that moves with the state. */
#define GLIMS_FIELD_XYZ 5   /* glims_sampler_apply: the mesh's REFERENCE coordinates (ncomp = dim) -> the back map X(x_p) */
int glims_sampler_create_grid_deformed(glims_ctx* h, const double* origin, const double* spacing, const int64_t* size,
                                       int64_t u_source, const double* u_host, double scale, int flags, int64_t* id);
int glims_sampler_create_points_deformed(glims_ctx* h, int64_t n, const double* xyz, int64_t u_source, const double* u_host,
                                         double scale, int flags, int64_t* id);
/* out[0] = 1 for a deformed sampler (0: the others, out[1] = 0, *min_ratio = 1); out[1] = number of cells whose ratio
 * det(E_deformed) / det(E_reference) is not > 0 (folded, flat or non-finite); *min_ratio = the smallest ratio
 * (= min_T det(I + scale grad u_h)).  Either output may be NULL. */
int glims_sampler_deformation_info(glims_ctx* h, int64_t id, int64_t out[2], double* min_ratio);
/* out[n][ncomp] = image(X(x_p)): the source image (array [z][y][x][ncomp], voxel centres origin + index * spacing, size points
 * per axis) evaluated at the back-mapped position X = sum_a w_a X_a of every found point.  Per axis t = (X - o) / s.
 *   order 1 (d-linear): the point is inside the source iff 0 <= t <= n - 1 on every axis; i0 = min(floor(t), n - 2) (n = 1:
 *           i0 = 0 and f = 0), f = t - i0; the value is the sum over the 2^d corners of the product of f or 1 - f, times the
 *           voxel -- plain IEEE arithmetic, so a NaN voxel of the stencil propagates.
 *   order 0 (nearest voxel): inside iff -0.5 <= t < n - 0.5, the index is floor(t + 0.5).
 * Points outside the mesh, and points whose X lies outside the source image, get `fill`.  ncomp is 1..8.  Works on every
 * sampler of a single-rank handle (on an undeformed one X(x_p) = x_p: plain resampling inside the mesh).  The image is
 * uploaded per call into the sampler's staging; the same arguments give the same bits.  GLIMS_E_USAGE: order outside {0, 1},
 * ncomp outside 1..8, a NULL image, a non-positive size or spacing, a partitioned handle. */
int glims_sampler_warp(glims_ctx* h, int64_t id, const double* image, const double* origin, const double* spacing,
                       const int64_t* size, int ncomp, int order, double fill, double* out);

/* ---- image-space misfit terms: a voxel image or point set as an observation of the recorded trajectory --------------------
 * The reference compares the simulated concentration with thresholded T1 / T2 segmentations
 * (optimization_workflow/image_based_optimization.py:660-708, thresh() at :1404).  Here the data stay where they were
 * measured: with P the sampler's operator (above) and p its points,
 *   J_img = 1/2 w sum_p q_p (h((P c_k)_p) - t_p)^2,
 *   dJ_img/dc_k = P^T r,            r_p = w q_p h'(v_p) (h(v_p) - t_p),   v = P c_k,
 *   d(dJ_img/dc_k) . dc = P^T r2,   r2_p = w q_p (h'(v_p)^2 + h''(v_p) (h(v_p) - t_p)) (P dc)_p.
 * A point is OBSERVED iff the sampler found it in the mesh, t_p is not NaN and q_p != 0; the others add nothing (a NaN target
 * enters no arithmetic).  The terms are STORED on the handle: glims_adjoint_image_terms copies target and pweight to the device
 * once, and every later glims_adjoint_gradient / _gradient_full / _hessian call adds the stored terms to the J of its nodal
 * list (n_terms = 0 there is fine): per step the nodal terms in list order, then the step's image terms in their list order.
 * They survive glims_setup, glims_set_materials, glims_set_state and a new recording (they depend on the sampler and the data
 * only); a term's `step` is checked against the trajectory by the gradient / Hessian call (GLIMS_E_USAGE).  Nothing passes
 * through the host between the trajectory and the adjoint's right-hand side; the sum over the points is taken in a fixed order
 * (per block, then the blocks in order) and P^T is the atomics-free transpose of glims_sampler_apply_t: J and every output
 * have the same bits on every call.  With no stored term every call issues exactly the work it issued before.
 *
 * glims_adjoint_image_terms REPLACES the handle's whole list (n = 0 clears it).  GLIMS_E_USAGE, with the old list left in
 * place: unknown sampler id or kind, a threshold term with smooth <= 0, a non-finite weight, a negative or non-finite q_p, a
 * null target.  GLIMS_E_HIP (with the figures) when hipMemGetInfo says the copies do not fit.  glims_sampler_destroy of a
 * sampler that a stored term uses returns GLIMS_E_USAGE and destroys nothing; glims_destroy releases the stored terms.
 * Neither call touches the forward state, glims_stats or glims_adjoint_stats.
 *
 * Partitioned handles (world > 1): n > 0 needs every term's sampler RESOLVED (glims_sampler_resolve), else GLIMS_E_USAGE;
 * every rank passes the same list (target and pweight in point order, the same on every rank) and n = 0 is always fine.  A
 * rank computes r at the points it KEEPS -- P^T r fills its owned rows of dJ/dc_k without an exchange -- and adds the squares
 * of the points it COUNTS; the ranks' sums of a term are gathered by one small all-reduce and added in rank order, so J and
 * every output have the same bits on every rank and on every call.  glims_adjoint_gradient checks, in its first all-reduce,
 * that the ranks agree on the stored list (count and steps) and refuses on all of them otherwise.  glims_adjoint_hessian
 * stays refused on partitioned handles. */
#define GLIMS_MISFIT_IMG_L2     0   /* h = identity */
#define GLIMS_MISFIT_IMG_THRESH 1   /* h(v) = 1/2 (tanh((v - level)/smooth) + 1), as GLIMS_MISFIT_C_THRESH */
typedef struct glims_image_misfit {
  int64_t step;            /* recorded step observed (0 = c_0) */
  int64_t sampler;         /* id from glims_sampler_create_grid / _points on this handle */
  int     kind;
  double  level, smooth, weight;
  const double* target;    /* [n_points], point order of the sampler; NaN = point not observed */
  const double* pweight;   /* [n_points] q_p (mask, voxel volume, ...), or NULL = 1 */
} glims_image_misfit;
int glims_adjoint_image_terms(glims_ctx* h, int n, const glims_image_misfit* terms);
/* out = (sampler id, number of points, number of observed points) of stored term k; on a partitioned handle out[2] is the
 * number of observed points THIS RANK counts (their sum over the ranks is the term's observed count) */
int glims_adjoint_image_info(glims_ctx* h, int k, int64_t out[3]);

/* ---- image terms in the deformed configuration: the gradient through the location ---------------------------------------------
 * The terms above observe the REFERENCE configuration X.  A scan shows x = X + u(X): a segmentation of a tumour with mass effect
 * is a target in the deformed configuration, and it is the only image data that carry information on the coupling, E and nu
 * (the reference gets a displacement target from an ANTs registration instead, image_based_optimization.py:264-292).  A deformed
 * term observing recorded step k locates its points x_p, at EVERY evaluation, in the mesh whose node a sits at
 *     y_a = fl(X_a + fl(scale * u_k,a)),   u_k = K_el^-1 (G c_k + f)   (the adjoint's own solve, to 1e-12 ||rhs||),
 * with the rules of the samplers (GLIMS_SAMPLE_EPS, the smallest caller cell index wins), and with the winner's weights w_p,a
 *     v_p = sum_a w_p,a c_k,a,    J_img = 1/2 w sum_p q_p (h(v_p) - t_p)^2,    r_p = w q_p h'(v_p) (h(v_p) - t_p),
 *     dJ_img/dc_k = P^T r                                   (the formula above with the deformed weights),
 *     dJ_img/du_k = P^T S,   S_p = -scale r_p grad_y c_k|T(p)   [n_points][dim],
 * since differentiating sum_a w_a y_a = x_p gives dv_p/dy_b = -w_p,b grad_y c_k|T(p), the constant gradient of c_k on the
 * deformed cell.  dJ/du_k is added to the right-hand side of the elastic adjoint, the vector a GLIMS_MISFIT_U_L2 term of the
 * same step writes to: u_k is solved ONCE per observed step and mu_k = K_el^-1 dJ/du_k once, whatever the number of terms;
 * G^T mu_k and the gamma, E and nu sums follow as for a displacement term (Dirichlet dofs as that solve handles them).
 * J is continuous and piecewise smooth in the parameters: it has a KINK where a point crosses a cell face and a JUMP where a
 * point enters or leaves the displaced mesh (possible only where the boundary is not clamped).  The gradient is that of the
 * smooth piece the evaluation sits on.  A winning cell whose det(E_deformed) / det(E_reference) is not > 0 (folded, flat or
 * non-finite) gets S_p = 0.
 *
 * A point is OBSERVED iff it is found in the displaced mesh AT THIS EVALUATION, t_p is not NaN and q_p != 0.  The sampler keeps
 * no coordinates, so a moving term carries its own point set: xyz[n_points][dim], or (xyz == NULL) the grid origin + index *
 * spacing of size[dim] points, x fastest; it is copied to the device once, with target and pweight.  The terms are a SECOND
 * stored list: glims_adjoint_deformed_image_terms replaces this list only (n = 0 clears it), and glims_adjoint_gradient /
 * _gradient_full evaluate, per step, the nodal terms in list order, then the fixed image terms, then the deformed terms in
 * list order.  With an empty deformed list every call issues exactly the work it issued before.  The forward state,
 * glims_stats, the forward path's elastic solve history and the derive cache of U are left as they were; no float atomics,
 * block sums in a fixed order: the same call gives the same bits every time.  With scale = 0, J and the c-derivatives have
 * the bits of the fixed term on the same points and dJ/du_k is 0.
 *
 * GLIMS_E_USAGE with a reason, the old list left in place: a partitioned handle (world > 1), a handle set up without
 * mechanics, an unknown kind, smooth <= 0 for a threshold term, a non-finite weight or scale, a negative or non-finite q_p, a
 * null target, and everything the sampler creators refuse of their points.  A step beyond the trajectory is refused by the
 * gradient call.  GLIMS_E_HIP (with the figures) when hipMemGetInfo says the copies or the scratch sampler do not fit.
 * Second order through the location is not built: glims_adjoint_hessian / _hessian_spmd return GLIMS_E_USAGE while the list
 * is non-empty. */
typedef struct glims_deformed_image_misfit {
  int64_t step; int kind;                 /* GLIMS_MISFIT_IMG_L2 / _IMG_THRESH */
  double level, smooth, weight, scale;
  int64_t n_points; const double* xyz;    /* point set [n_points][dim], or xyz == NULL: the grid below */
  double origin[3], spacing[3]; int64_t size[3];
  const double* target;                   /* [n_points] or grid order [z][y][x]; NaN = not observed */
  const double* pweight;                  /* q_p or NULL */
} glims_deformed_image_misfit;
int glims_adjoint_deformed_image_terms(glims_ctx* h, int n, const glims_deformed_image_misfit* terms);
/* out = n_points, found, observed, folded cells of the LAST evaluation of term k (-1 before the first); min_ratio likewise
 * (1 before the first).  folded cells / min_ratio: the figures of glims_sampler_deformation_info for the mesh at X + scale u_k
 * (cells of the mesh whose ratio is not > 0; the smallest ratio). */
int glims_adjoint_deformed_image_info(glims_ctx* h, int k, int64_t out[4], double* min_ratio);

/* ---- derived fields of a recorded step, on the device -----------------------------------------------------------------------
 * The reference's PostProcess classes project UFL expressions of a recorded step onto the P1 space (helper_classes.py:1521-1972:
 * get_strain_tensor :1566, get_pressure :1587, get_van_mises_stress :1595, get_displacement_norm :1612, get_stress_tensor :1736,
 * get_logistic_growth :1746, get_mech_expansion :1754, get_total_jacobian :1763, get_growth_induced_jacobian :1771,
 * get_concentration_deformed_configuration :1779; save_all :1922 writes them).  glims_derive computes one such field from data
 * that are already on the device: a per-cell pass evaluates the integrand -- cell-wise constants
 * exactly, the others with the 16 / 64-point conical-product Gauss-Jacobi rule of csrc/derive_quadrature.h (degree 7) --, an
 * atomics-free gather along each row's incidence list sums the right-hand sides, and glims_project's Jacobi-PCG solves the mass
 * systems component by component to ||r|| <= rtol ||rhs||.  The same arguments give the same bits on every call.
 *
 * Source of c and u:
 *   snapshot >= 0          an id of glims_snapshot_save; where the kind needs the displacement it is solved on the device as
 *                          glims_snapshot_mechanics solves it (same status codes), unless the handle's U already belongs to that
 *                          snapshot.  glims_snapshot_mechanics sets that memory; glims_step, glims_set_state,
 *                          glims_solve_mechanics, glims_set_materials, glims_setup, a new elastic Dirichlet set or load and
 *                          glims_snapshot_clear forget it.
 *   GLIMS_DERIVE_CURRENT   the handle's current c and U as they stand (the caller has solved the mechanics)
 *   GLIMS_DERIVE_HOST      c_host[n_nodes], u_host[n_nodes*dim] in the caller's node order (NULL where the kind needs none);
 *                          uploaded into scratch, neither c nor U is touched
 * Kinds (ncomp components; tensors are kept and sampled as their d(d+1)/2 symmetric components xx, yy, (zz,) xy, (xz, yz)):
 *   _STRAIN           projection of eps(u_h)                              cell-wise constant   tensor
 *   _STRESS           projection of 2 mu_T eps + lambda_T tr(eps) I       cell-wise constant   tensor
 *   _PRESSURE         1/3 tr of the P1 stress of _STRESS, nodewise (no further solve)          scalar
 *   _VON_MISES        projection of sqrt(3/2 dev:dev) of the P1 stress (dev = sigma - 1/3 tr I) scalar, second stage
 *   _DISP_NORM        projection of |u_h|                                                      scalar
 *   _LOG_GROWTH       projection of rho_T c_h (1 - c_h)                                        scalar
 *   _MECH_EXPANSION   gamma c nodewise when gamma is one value over all cells (the labels the cells carry), else the projection of
 *                     gamma_T c_h; the scalar s of the growth strain s I                       scalar
 *   _TOTAL_JACOBIAN   projection of det(I + grad u_h)                     cell-wise constant   scalar
 *   _GROWTH_JACOBIAN  projection of (1 + s_h)^d, s_h the P1 field of _MECH_EXPANSION           scalar, second stage
 *   _CONC_DEFORMED    projection of c_h (1 + gamma_T c_h)^d / det(I + grad u_h)                scalar
 * The projected P1 stress of (snapshot or CURRENT, displacement generation) is kept in a one-entry device cache: _PRESSURE and
 * _VON_MISES of one step project it once between them; a cached stress is reused only by calls whose rtol is not tighter than
 * the one it was solved to.  glims_derive_info makes that countable.
 *
 * The result stays on the device (planes [ncomp][n_nodes], internal numbering) until the next glims_derive or glims_destroy;
 * glims_sampler_apply(field = GLIMS_FIELD_DERIVED, ncomp = its component count) evaluates it at a sampler's points.  out (may be
 * NULL) receives [n_nodes] for a scalar and the full [n_nodes][d][d] for a tensor, caller's node order.
 *
 * Like glims_project the call shares the Jacobi diagonal and the PCG work vectors with the time stepper and drops the step the
 * last sweep prepared; the steps that follow have the bits of a run that never called it.
 * Returns the worst status of its solves (GLIMS_OK / GLIMS_NOT_CONVERGED / GLIMS_NAN).  GLIMS_E_USAGE, with a reason in
 * glims_last_error and nothing changed: unknown kind or snapshot, a call before glims_setup, a kind that needs u on a handle set
 * up without mechanics, GLIMS_DERIVE_CURRENT before glims_set_state, a required host pointer that is NULL, rtol <= 0, a
 * partitioned handle (world > 1: the host path of the Python layer stays there). */
#define GLIMS_DERIVE_STRAIN 0
#define GLIMS_DERIVE_STRESS 1
#define GLIMS_DERIVE_PRESSURE 2
#define GLIMS_DERIVE_VON_MISES 3
#define GLIMS_DERIVE_DISP_NORM 4
#define GLIMS_DERIVE_LOG_GROWTH 5
#define GLIMS_DERIVE_MECH_EXPANSION 6
#define GLIMS_DERIVE_TOTAL_JACOBIAN 7
#define GLIMS_DERIVE_GROWTH_JACOBIAN 8
#define GLIMS_DERIVE_CONC_DEFORMED 9
#define GLIMS_DERIVE_CURRENT (-1)
#define GLIMS_DERIVE_HOST (-2)
#define GLIMS_FIELD_DERIVED 4      /* glims_sampler_apply: the result of the last glims_derive, from its device buffer */
int glims_derive(glims_ctx* h, int kind, int64_t snapshot, const double* c_host, const double* u_host, double rtol,
                 double* out);
/* cumulative since glims_create: out[0] cell passes, [1] mass solves, [2] elastic solves, [3] hits of the stress cache */
int glims_derive_info(const glims_ctx* h, int64_t out[4]);

/* ---- tumour volumes and centres of mass per tissue, on the device ---------------------------------------------------------------
 * The first numbers the reference's workflow computes from a run: ImageBasedOptimizationBase.compute_from_conc_for_each_time_step
 * (optimization_workflow/image_based_optimization.py:1333-1397) takes q = conditional(c >= threshold, 1, 0) of every recording
 * step and integrates compute_volume / compute_com over dx and over dx(subdomain_id) of every tissue; compute_volume_thresholded /
 * compute_com_all (:1262-1301, :1416-1430, :1470-1472) do the same for the smooth thresh() fields, post_process (:1305) runs all
 * of it for T2 = 0.12 and T1 = 0.80.  glims_observe computes, for every source, query and label, the measure and the first
 * moments of q over the cells of that label (the per-cell mathematics is csrc/observe_clip.h):
 *   GLIMS_OBSERVE_MASS    q = c_h                                      exact
 *   GLIMS_OBSERVE_SHARP   q = 1 where c_h >= level (a tie is in)       exact: the simplex is clipped at the level set
 *   GLIMS_OBSERVE_SMOOTH  q = 1/2 (tanh((c_h - level) / smooth) + 1)   the degree-7 rule of csrc/derive_quadrature.h (the discrete
 *                                                                      statement of that rule, not a converged integral where
 *                                                                      smooth is far below the range of c over a cell)
 * src[i]: an id of glims_snapshot_save; with n_src == 1 also GLIMS_DERIVE_CURRENT (the handle's c, and U as it stands) or
 * GLIMS_DERIVE_HOST (c_host[n_nodes], u_host[n_nodes*dim] in the caller's node order, uploaded into scratch), as in glims_derive.
 * out[n_src][n_q][n_labels][1 + dim] = (V, M_0 .. M_{dim-1}) with n_labels that of glims_set_materials; a label that no cell
 * carries gets exact zeros; the whole-domain figures are the sums over the labels and the centre of mass is M / V (the caller's).
 *
 * deformed = 0: the reference configuration, V = int q dX.  deformed = 1: the configuration x = X + scale u, V = int q det(I +
 * scale grad u) dX and the moments of x; a folded cell counts negatively (as GLIMS_DERIVE_TOTAL_JACOBIAN).  It needs
 * glims_setup(with_mechanics=1); a snapshot's displacement is solved as glims_snapshot_mechanics solves it (same status codes; U
 * is written and the solve enters the elastic solve history) unless U already belongs to that snapshot -- the memory glims_derive
 * and the deformed samplers use; glims_observe_info and glims_derive_info count the solve.  Nothing else the time stepper owns
 * is touched: the steps that follow have the bits of a run that never called it.
 *
 * One pass over the cells per source serves all n_q queries (glims_observe_info counts the passes); there are no floating-point
 * atomics and the same handle and arguments give the same bits on every call.  With GLIMS_OBSERVE_TIMING set (any value) an
 * event pair around each source's pass prints one line per source on stderr.
 * Returns the worst status of its elastic solves (GLIMS_OK / GLIMS_NOT_CONVERGED / GLIMS_NAN).  GLIMS_E_USAGE, with a reason in
 * glims_last_error and nothing written: a call before glims_setup, an unknown kind or snapshot, n_q outside 1..8, n_src < 1,
 * CURRENT / HOST with n_src != 1, CURRENT before glims_set_state, a required pointer that is NULL, smooth <= 0 of a SMOOTH query,
 * deformed on a handle set up without mechanics, a scale or level that is not finite, a cell label >= n_labels, a partitioned
 * handle (world > 1: the numpy statement of the Python layer serves there). */
#define GLIMS_OBSERVE_MASS 0
#define GLIMS_OBSERVE_SHARP 1
#define GLIMS_OBSERVE_SMOOTH 2
#define GLIMS_OBSERVE_MAX_QUERIES 8
typedef struct glims_observable {
  int kind;               /* GLIMS_OBSERVE_* */
  double level, smooth;   /* smooth: SMOOTH only */
} glims_observable;
int glims_observe(glims_ctx* h, int n_src, const int64_t* src, const double* c_host, const double* u_host, int deformed,
                  double scale, int n_q, const glims_observable* q, double* out);
/* cumulative since glims_create: out[0] cell passes, [1] elastic solves, [2] sources observed, [3] 0 */
int glims_observe_info(const glims_ctx* h, int64_t out[4]);

/* ---- volume misfit terms: fits to tumour-volume series --------------------------------------------------------------------------
 * The clinical datum is often a volume series, not an image: the T2- / T1-like tumour volume (c above 0.12 / 0.80) at a few scan
 * dates, per tissue or over the whole domain -- the numbers glims_observe computes.  A stored volume term makes such a number a
 * misfit term of the adjoint calls (the per-cell mathematics is csrc/observe_grad.h).  For the term that
 * observes recorded step k,
 *     V = sum over the cells T of the counted labels of V_T(c_k),    J_obs = 1/2 weight (V - target)^2,
 * V the measure glims_observe returns for the query (kind, level, smooth) in the REFERENCE configuration (deformed = 0), summed
 * over the counted labels, and
 *     dJ_obs/dc_k = weight (V - target) g,    g_i = sum over the counted cells T that hold node i of dV_T/dc_i:
 *   MASS    dV_T/dc_i = |T| / (d+1)
 *   SMOOTH  dV_T/dc_i = |T| sum_q w_q h'(v_q) lam_qi      (the degree-7 rule of glims_observe, differentiated as it stands)
 *   SHARP   the derivative of the clipped fraction through the edge parameters t = (c_a - level) / (c_a - c_b) of the cut edges;
 *           a cell with 0 or d+1 vertices in contributes 0.  V is continuous and piecewise smooth in c: the gradient is that of
 *           the smooth piece the evaluation sits on (a tie c_i == level counts as in).
 * The terms are a THIRD stored list: glims_adjoint_observable_terms replaces this list only (n = 0 clears it), and every gradient /
 * Hessian call evaluates, per step, the nodal terms in list order, then the fixed image terms, the deformed image terms and the
 * volume terms, each in list order.  With an empty list every call issues exactly the work it issued before.  One pass over the
 * cells serves up to GLIMS_OBSERVE_MAX_QUERIES terms of a step (more terms: more passes, in list order); it writes the vertex
 * partials per cell, block sums in a fixed order give V, and a row-owned gather along the incidence lists adds them to the
 * sweep's right-hand side: no float atomics, the same call gives the same bits every time.  The scratch (8 (dim+1) n_cells bytes per
 * term of a pass, twice that in a Hessian call) is sized from the mesh; GLIMS_E_HIP with the figures when hipMemGetInfo says it
 * does not fit.  The terms survive glims_setup, glims_set_materials (same label count), glims_set_state and a new recording;
 * they touch neither the forward state nor glims_stats nor the bits of later steps.
 *
 * Second order (glims_adjoint_hessian, _hessian_spmd with world = 1, _hessian_full), MASS and SMOOTH: per direction j
 *     dg_j += weight (g (g^T dc_j) + (V - target) H dc_j),    H = sum_T |T| sum_q w_q h''(v_q) lam_q lam_q^T  (MASS: 0),
 * g^T dc_j summed cell by cell in the same fixed order.  SHARP is piecewise smooth with jumps in its second derivative where
 * the level set crosses a vertex: while a SHARP term is stored the Hessian entry points return GLIMS_E_USAGE.
 *
 * GLIMS_E_USAGE with a reason, the old list left in place: a partitioned handle (world > 1), a call before glims_setup, an unknown
 * kind, smooth <= 0 of a SMOOTH term, a level, weight or target that is not finite, a negative step.  A gradient or Hessian call
 * refuses a term whose step is beyond the trajectory and a stored mask whose length is no longer n_labels.
 *
 * Volumes of the DEFORMED configuration (glims_adjoint_observable_terms2, deformed = 1): a volume measured on a scan is a volume
 * of x = X + u(X).  Such a term measures every counted cell at y = X + scale u_k, u_k = K_el^-1 (G c_k + f) solved inside the
 * sweep (1e-12), as glims_observe(..., deformed = 1, scale) does:
 *     V = sum_T sigma_T vol(y_T) b0_T(c_k),    sigma_T = +-1 the reference orientation of the cell (a folded cell counts negatively),
 *     dJ/dc_k,i = weight (V - target) sum_{T holds i} sigma_T vol(y_T) d b0_T / d c_i,
 *     dJ/du_k,a = weight (V - target) scale sum_{T holds a} sigma_T b0_T d vol(y_T) / d y_a,
 * d vol / d y_a the cofactor vector of vertex a (csrc/observe_grad.h, glims_og_volume_grad; nothing is divided, a degenerate
 * displaced cell has finite cofactors).  V is a polynomial in u: no kink, no point location.  dJ/du_k joins the load of the
 * elastic adjoint of step k (one u_k solve and one adjoint solve per observed step, shared with the step's displacement and
 * deformed image terms), so volume data now carry the coupling, E and nu.  A SHARP term whose level lies below every
 * concentration (-1, say) has b0 = 1 and no c-partials: it is the deformed volume of the counted tissues -- the ventricles
 * under mass effect.  The terms stay ONE stored list: a batch of up to GLIMS_OBSERVE_MAX_QUERIES terms of a step may mix both
 * kinds, list order is kept, and a batch without a deformed term runs the kernels and gives the bits it gave before.  Extra
 * scratch of a list with a deformed term: 8 n_cells bytes per term of a pass (b0) and 8 (dim+1) dim n_cells bytes (the combined
 * load), through the same hipMemGetInfo refusal.  Second order through u is not built: while a deformed volume term is stored,
 * glims_adjoint_hessian, _hessian_spmd and _hessian_full return GLIMS_E_USAGE.  Further refusals of _terms2 (GLIMS_E_USAGE,
 * the old list left in place): a deformed term on a handle set up without mechanics, a scale that is not finite.
 *
 * CENTRE-OF-MASS terms (glims_adjoint_observable_terms3, moment = 1): the other number the workflow reports per scan and tissue.
 * With p = X, or p = y = X + scale u_k for a deformed term, T_T the signed measure factor of the volume terms (|T|, or
 * sigma_T vol(y_T)) and b_T[0 .. d+1] the barycentric values of the query (csrc/observe_clip.h),
 *     V = sum_T T_T b_T[0],   M_a = sum_T T_T sum_m b_T[1 + m] p_m,a,   X = M / V,   J_com = 1/2 weight |X - target_x|^2  (a < dim),
 * V and M the numbers glims_observe returns, summed over the counted labels.  With alpha = weight (X - target_x) / V and
 * psi_m,T = alpha . (p_m,T - X), both held fixed,
 *     dJ/dc_k,i = sum_{T holds i} T_T sum_m psi_m,T d b_T[1 + m] / d c_i,
 *     dJ/du_k,n = scale sum_{T holds n as vertex m} sigma_T (B_T cof_m(y_T) + vol(y_T) b_T[1 + m] alpha),   B_T = sum_m b_T[1 + m] psi_m,T.
 * A quotient needs V and M before any partial can be weighted: a batch with such a term first runs a moments pass over the
 * cells and a fixed-order sum that leave V, M, X, alpha and J on the device (no host round trip), then the gradient pass of
 * the volume terms, which writes the psi-weighted partials into the same planes (coefficient 1).  A batch may mix volume and
 * centre-of-mass terms of both configurations; one without a centre-of-mass term launches the kernels and gives the bits it
 * gave before.  EMPTY measure: if V is not > 0 at an evaluation the term adds J = 0 and zero gradients there (out[3] = 1 of
 * _info3); it is no error -- an optimiser may step there.  Extra scratch: 8 (dim+1) n_cells bytes per deformed centre-of-mass
 * term of a pass, through the same hipMemGetInfo refusal.  Second order is not built: while a centre-of-mass term is stored,
 * glims_adjoint_hessian, _hessian_spmd and _hessian_full return GLIMS_E_USAGE.  Further refusals of _terms3 (GLIMS_E_USAGE,
 * the old list left in place): moment outside 0 .. 1, a target_x entry (of the first dim) that is not finite; and everything
 * _terms2 refuses.
 * Not built: higher moments, partitioned handles, second order for SHARP, for deformed and for centre-of-mass terms. */
typedef struct glims_observable_misfit {
  int64_t step;              /* recorded step observed (0 = c_0) */
  int     kind;              /* GLIMS_OBSERVE_MASS / _SHARP / _SMOOTH */
  double  level, smooth;     /* as glims_observable */
  double  weight, target;    /* J_obs = 1/2 weight (V - target)^2 */
  const uint8_t* labels;     /* [n_labels of glims_set_materials]: non-zero = that label's cells are counted; NULL = all */
} glims_observable_misfit;
int glims_adjoint_observable_terms(glims_ctx* h, int n, const glims_observable_misfit* terms);   /* replaces the list; n = 0 clears */
/* stored term k: out[0] the number of counted cells, out[1] the cells the level set cut at the LAST evaluation (-1 before the
 * first, and for MASS / SMOOTH), *V the last V (NaN before the first) */
int glims_adjoint_observable_info(glims_ctx* h, int k, int64_t out[2], double* V);
/* the fields of glims_observable_misfit, then the configuration the cells are measured in */
typedef struct glims_observable_misfit2 {
  int64_t step;
  int     kind;
  double  level, smooth;
  double  weight, target;
  const uint8_t* labels;
  int     deformed;          /* 0: the reference configuration (as glims_observable_misfit); 1: the cells at X + scale u_k */
  double  scale;             /* deformed = 1: multiplies u_k (finite); ignored otherwise */
} glims_observable_misfit2;
/* replaces the SAME stored list as glims_adjoint_observable_terms (which stores its terms with deformed = 0); n = 0 clears */
int glims_adjoint_observable_terms2(glims_ctx* h, int n, const glims_observable_misfit2* terms);
/* stored term k: out[0] counted cells, out[1] cut cells (as _info), out[2] the counted cells folded (vol(y) / vol(X) not > 0)
 * at the LAST evaluation, out[3] = 0; *V the last V, *min_ratio the smallest vol(y) / vol(X) over the counted cells (NaN when
 * no cell is counted).  Before the first evaluation out[2] = -1, *V = NaN, *min_ratio = NaN; a reference term keeps
 * out[2] = -1 and *min_ratio = NaN. */
int glims_adjoint_observable_info2(glims_ctx* h, int k, int64_t out[4], double* V, double* min_ratio);
/* the fields of glims_observable_misfit2, then what the term compares */
typedef struct glims_observable_misfit3 {
  int64_t step;
  int     kind;
  double  level, smooth;
  double  weight, target;
  const uint8_t* labels;
  int     deformed;
  double  scale;
  int     moment;            /* 0: the volume term (target used), 1: centre of mass (target_x used) */
  double  target_x[3];       /* [dim] */
} glims_observable_misfit3;
/* replaces the SAME stored list as glims_adjoint_observable_terms / _terms2 (which store their terms with moment = 0); n = 0 clears */
int glims_adjoint_observable_terms3(glims_ctx* h, int n, const glims_observable_misfit3* terms);
/* as _info2, plus out[3] = 1 when the LAST evaluation found the measure of a centre-of-mass term empty (V not > 0), and
 * com[0 .. dim-1] = the last X = M / V: NaN before the first evaluation, when empty, for a volume term and in com[dim ..] */
int glims_adjoint_observable_info3(glims_ctx* h, int k, int64_t out[4], double* V, double* min_ratio, double com[3]);

/* ---- displacement-image misfit terms: a registration warp field or landmark displacements as data ----------------------------
 * The reference's third misfit term compares the displacement with the warp-field image of an ANTs registration, after
 * interpolating that image onto the mesh (optimization_workflow/image_based_optimization.py:660-708, :943-978).  Here the data
 * stay where they were measured: with P the operator of a FIXED (reference-configuration) sampler, p its points and
 * u_k = K_el^-1 (G c_k + f) the displacement of recorded step k (the adjoint's own solve, to 1e-12 ||rhs||),
 *   J_uimg        = 1/2 w sum_p q_p sum_a kappa_a (s (P u_k)_p,a - d_p,a)^2,
 *   dJ/du_k       = P^T R,    R_p,a  = w q_p kappa_a s (s (P u_k)_p,a - d_p,a)       [n_points][dim],
 *   d(dJ/du_k).du = P^T R2,   R2_p,a = w q_p kappa_a s^2 (P du)_p,a.
 * d is the target [n_points][dim], q_p >= 0 an optional point weight, kappa_a >= 0 the component weights (cweight; (1,0,0)
 * observes a midline shift alone), s a finite scale (warp fields come in both signs and in voxel or mm units).  A point is
 * OBSERVED iff the sampler found it, q_p != 0 and d_p,a is not NaN for every component with kappa_a != 0; a NaN in a
 * component with kappa_a = 0 is allowed and enters no arithmetic; the other points add nothing.  The term has no direct
 * c-derivative: dJ/du_k is added to the right-hand side of the elastic adjoint, the vector a GLIMS_MISFIT_U_L2 term of the
 * same step writes to, so u_k is solved ONCE per observed step and mu_k = K_el^-1 dJ/du_k once, whatever mix of terms needs
 * them; G^T mu_k and the gamma, E and nu sums follow as for a displacement term.
 *
 * The terms are a THIRD stored list with the semantics of glims_adjoint_image_terms: the call replaces its own list only
 * (n = 0 clears it), target and pweight are copied to the device once, the list survives glims_setup, glims_set_materials,
 * glims_set_state and a new recording, glims_sampler_destroy of a sampler it uses is refused, and with an empty list every
 * call issues exactly the work it issued before.  Per step glims_adjoint_gradient / _gradient_full evaluate the nodal terms,
 * the fixed image terms, the displacement image terms in list order, then the deformed image terms and the observable terms.
 * The term is quadratic in u and u is linear in c: glims_adjoint_hessian / _hessian_full add P^T R2 of each direction's own
 * tangent du (which holds the dK part of an E / nu direction) to the right-hand side of the second elastic adjoint -- the
 * products are exact, E and nu included.  No float atomics, sums in a fixed order: the same call gives the same bits.
 *
 * GLIMS_E_USAGE with a reason, the old list left in place: a partitioned handle (world > 1), a handle set up without
 * mechanics, an unknown or DEFORMED sampler, a non-finite weight or scale, a negative or non-finite q_p or kappa_a, all
 * kappa_a = 0, a null target, a negative step.  A step beyond the trajectory is refused by the gradient / Hessian call.
 * Not built: partitioned handles, a warp field defined on the deformed grid (u at the material point sitting at x_p),
 * interpolation other than the sampler's P1. */
typedef struct glims_displacement_image_misfit {
  int64_t step;            /* recorded step observed */
  int64_t sampler;         /* id of a fixed sampler (glims_sampler_create_grid / _points) on this handle */
  double  weight, scale;
  double  cweight[3];      /* kappa_a, the first dim are read */
  const double* target;    /* [n_points][dim], point order of the sampler */
  const double* pweight;   /* [n_points] q_p, or NULL = 1 */
} glims_displacement_image_misfit;
int glims_adjoint_displacement_image_terms(glims_ctx* h, int n, const glims_displacement_image_misfit* terms);
/* out = (sampler id, number of points, number of observed points) of stored term k */
int glims_adjoint_displacement_image_info(glims_ctx* h, int k, int64_t out[3]);

/* ---- anisotropic diffusion: a per-cell tensor ("Anisotropic diffusion") ---------------------- */

/* The flux of cell T with label t becomes D_t * TT_T grad c: D_t is still the per-tissue scalar of glims_set_materials
 * (and still the control of every gradient and Hessian), TT_T a dimensionless symmetric positive-definite dim x dim tensor
 * per cell, fixed during a fit.  T[n_cells][dim (dim + 1) / 2] in the CALLER's cell order, each tensor packed as its upper
 * triangle row by row (the ITK order): (xx, xy, yy) in 2-D, (xx, xy, xz, yy, yz, zz) in 3-D.  NULL clears the field: TT = I,
 * the isotropic kernels, the bits of a handle that never had one.
 *
 * The contract of glims_set_materials: the field is copied to the device (8 dim (dim + 1) / 2 bytes per cell, stored in the
 * internal cell order) and takes effect with the next glims_setup; the call forgets the mechanics operator and the derive
 * displacement, marks both multigrid hierarchies not ready, invalidates an adjoint recording and requires a new glims_setup.
 * What changes is the static operator S = M - dt M_rho + dt K with K_ij = sum_T D_t |T| grad phi_i^T TT_T grad phi_j, and
 * the gradient forms of the sensitivity passes (dJ/dD_t = -dt sum_{T in t} |T| grad lambda^T TT_T grad c, and the three forms
 * of the second order).  The time stepper, its solvers and fast paths read S alone and run the code they run without a field;
 * rho, gamma, E, nu, mechanics, every misfit term, the samplers, derive and observe do not see the tensor.
 *
 * A device pass validates the field: every entry finite and the leading principal minors > 0.  Otherwise GLIMS_E_USAGE, the
 * message naming the number of bad cells and the smallest caller's index among them, and the previous field (or none) stays
 * in place with the handle as it was.  On a partitioned handle the call is rank-local (the cells are the rank's cells) and
 * communicates nothing.
 *
 * Not built: single tensor entries per cell as controls (parameters of a tensor family are: the tangent fields below), tensors
 * that vary in time, anisotropic mechanics.  P1
 * elements with a strongly anisotropic tensor lose the discrete maximum principle (small negative concentrations are
 * possible); a Neumann load on the concentration (glims_set_rd_load) is passed as it is -- the natural condition
 * is on the tensor flux D_t TT grad c . n. */
int glims_set_diffusion_tensor(glims_ctx* h, const double* T);
/* out[0] = 1 if a field is set, else 0; out[1] = n_cells; *max_ratio = the largest lambda_max / lambda_min over the cells
 * (1 without a field).  Either pointer may be NULL. */
int glims_diffusion_tensor_info(const glims_ctx* h, int64_t out[2], double* max_ratio);

/* ---- tensor-field controls: tangent fields of the diffusion tensor ("Tangent fields") ---- */

#define GLIMS_DT_MAX_TANGENTS 4

/* For a tensor field TT(theta) the caller stores, next to TT itself, K <= GLIMS_DT_MAX_TANGENTS tangent fields
 * dTT/dtheta_k: dT[K][n_cells][dim (dim + 1) / 2] in the CALLER's cell order and the packed layout of
 * glims_set_diffusion_tensor, symmetric, not necessarily definite (a zero or indefinite tangent is fine).  K = 0 or
 * dT = NULL clears them.  Every backward sweep that follows -- glims_adjoint_gradient* and the glims_adjoint_hessian* entry
 * points run the same one -- then also adds up, per label t and tangent k,
 *     dJ/dtheta_k |_t = -dt D_t sum_steps sum_{T in t} |T| grad lambda_h^T (dTT_T/dtheta_k) grad c_h
 * (dJ/dD_t with the tangent in place of the tensor, times D_t), in a fixed order without atomics: the same call gives the
 * same bits.  First order only.
 *
 * Tangents are data of the sensitivity pass alone: the call does NOT invalidate the set-up, the multigrids, the prepared
 * step or an adjoint recording -- set them after a recorded run and ask for a gradient without a new run.  They work with
 * and without a base field (none: tangents about TT = I), are kept by glims_set_diffusion_tensor (they belong to the mesh's
 * cells), and cost 8 K dim (dim + 1) / 2 bytes per cell plus the handle-owned sums and partials.  A device pass checks every
 * entry for finiteness; otherwise GLIMS_E_USAGE, the message naming the first bad tangent, the number of bad entries' cells
 * and the smallest caller's index of a bad cell of that tangent, and the previously stored tangents stay.  K outside
 * 0..GLIMS_DT_MAX_TANGENTS is GLIMS_E_USAGE.  On a partitioned handle the call is rank-local (the rank's cells); every rank
 * must store the same K (the adjoint calls check it collectively). */
int glims_set_diffusion_tensor_tangents(glims_ctx* h, int K, const double* dT);
/* out[K][n_labels] = the sums above of the last completed backward sweep (on a partitioned handle gathered over the ranks
 * and added in rank order: every rank gets the same bits).  K and n_labels must be those of the stored tangents and of
 * glims_set_materials.  GLIMS_E_USAGE when no sweep has completed since the tangents were last set, or when the last sweep
 * stopped with a status. */
int glims_adjoint_tensor_gradient(glims_ctx* h, int K, int n_labels, double* out);

/* ---- single-node multi-GPU (one process per GPU, RCCL over xGMI) ------------------------------------- */

#define GLIMS_UNIQUE_ID_BYTES 256   /* two RCCL unique ids: halo communicator + reduction communicator */
int glims_comm_unique_id(char id[GLIMS_UNIQUE_ID_BYTES]);           /* rank 0; broadcast by the host program */
int glims_comm_init(glims_ctx* h, int rank, int world, const char id[GLIMS_UNIQUE_ID_BYTES]);

/* Node-local all-reduce for the scalars of the Krylov / Newton iterations: all ranks of ONE host map the POSIX
 * shared-memory object `shm_name` ("/name", created on first use, >= world * 128 bytes) into their GPU's address
 * space; the final block of each reduction kernel publishes its partial sums there and adds up everybody's in rank
 * order.  No launch and no RCCL kernel per iteration (the all-reduce of three doubles is pure latency; the halo
 * exchange stays on RCCL / xGMI).  Call after glims_comm_init or glims_set_transport (they set rank / world), from
 * every rank with the same name; the caller unlinks the object once every rank has returned.  Without this call the
 * reductions use ncclAllReduce (or the transport's allreduce callback).  shm_name = NULL switches it off again.
 * New in this build; the reference's counterpart is PETSc's MPI_Allreduce inside KSP/SNES. */
int glims_comm_mailbox(glims_ctx* h, const char* shm_name);
/* Collective check of the mailbox: one all-reduce of known values with a 5 s limit; every rank calls it.  A host
 * program that gets an error from ANY rank switches the mailbox off on ALL ranks (glims_comm_mailbox(h, NULL)). */
int glims_comm_mailbox_selftest(glims_ctx* h);

/* Diagnostic: runs the library's RCCL call sequence (pack -> event -> grouped ncclSend/ncclRecv on the communication
 * stream -> event -> compute stream, then ncclAllReduce on the compute stream) on a fresh ONE-rank communicator pair,
 * sending to itself, and checks the data.  Proves that the RCCL library the process resolved is usable with this
 * build (ABI, datatypes, stream/event ordering); it cannot prove multi-rank semantics. */
int glims_comm_selftest(glims_ctx* h);

/* Halo plan: for peer p (rank peer_rank[p]) this rank sends the values of its owned nodes
 * send_idx[send_ptr[p] .. send_ptr[p+1]) and receives recv_count[p] values into consecutive ghost slots;
 * ghost slots are laid out peer after peer in the order of peer_rank[], starting at node n_own, and the
 * k-th ghost of a peer is the k-th entry of that peer's send list for this rank.  Must precede glims_setup. */
int glims_set_halo(glims_ctx* h, int n_peers, const int32_t* peer_rank,
                   const int64_t* send_ptr, const int32_t* send_idx, const int64_t* recv_count);

/* Partitioned runs with mechanics: the bounding box lo[dim], hi[dim] of the WHOLE mesh (the same numbers on every rank).
 * The elasticity multigrid then lays one global frame of auxiliary grids over the partitioned mesh and replicates its
 * coarse levels (their operators are summed over the ranks once, the restricted residual once per cycle), so that the
 * low-frequency part of the error is corrected globally -- the counterpart of what a parallel AMG does inside PETSc
 * under mpirun (simulation_tumor_growth_brain_quad.py:116-119, README.md:142-183).  Without this call each rank
 * preconditions its own rows only (still correct, about three times the iterations at 2 ranks).  NULL clears. */
int glims_set_mg_frame(glims_ctx* h, const double* lo, const double* hi);

/* Optional host-provided transport instead of RCCL (e.g. the reference's own MPI communicator, which DOLFIN hands
 * around as mesh.mpi_comm(), helper_classes.py:1249-1267; also used by the 2-rank tests on a single GPU, where RCCL
 * refuses two ranks per device).  Both callbacks are invoked from the calling thread with device pointers and the
 * handle's HIP stream; they must return only when the exchange is complete and visible to later work on that stream
 * (e.g. hipStreamSynchronize, staged copies, hipMemcpy back).  Return 0 on success.
 *   halo:      sendbuf[(send_ptr[p] .. send_ptr[p+1]) * bs] goes to peer p; the values received from peer p must be
 *              stored at ghosts[(recv_ptr[p] .. recv_ptr[p+1]) * bs]  (ghosts = first ghost slot of the vector).
 *   allreduce: in-place sum of n doubles over all ranks.
 * Replaces glims_comm_init (sets rank / world); glims_set_halo is still required. */
typedef int (*glims_halo_fn)(void* user, const double* sendbuf_dev, const int64_t* send_ptr, double* ghosts_dev,
                             const int64_t* recv_ptr, int n_peers, const int32_t* peer_rank, int bs, void* hip_stream);
typedef int (*glims_allreduce_fn)(void* user, double* values_dev, int n, void* hip_stream);
int glims_set_transport(glims_ctx* h, int rank, int world, glims_halo_fn halo, glims_allreduce_fn allreduce,
                        void* user);

#ifdef __cplusplus
}
#endif
#endif /* GLIMS_HIP_H */
