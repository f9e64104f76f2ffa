// Tumour volumes and centres of mass per tissue, on the device (glims_observe): for every source (a
// recorded snapshot, the current state or host arrays), every query (MASS / SHARP / SMOOTH, observe_clip.h) and every label, the
// measure V = int q dx and the first moments M_a = int x_a q dx over the cells of that label, in the reference configuration or
// in the deformed one x = X + scale u.  Reference counterpart: compute_from_conc_for_each_time_step, compute_volume_thresholded
// and compute_com_all (optimization_workflow/image_based_optimization.py:1333-1397, :1262-1301, :1416-1430, :1470-1472).
//   k_observe_cells  one lane per cell over a fixed grid, ONE pass for all queries of a source: vertex ids, label, gathered c
//                    (positions and u only where some query can be non-zero); per query the lanes' contributions are reduced
//                    per label with a fixed shuffle tree and added to the wave's private table
//   k_observe_sum    one block per (label slot, value): the per-wave tables summed in a fixed order
// No float atomics; the same handle and arguments give the same bits on every call.
#include "glims_internal.h"
#include "observe_clip.h"
#include "observe_grad.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace {

#define GL_CHECK_LAUNCH() GL_HIP(hipGetLastError())

constexpr int GL_OBS_BLOCKS = 2048;          // fixed grid of the cell pass (as the derive / sensitivity passes)
constexpr int GL_OBS_WAVES = 4;              // waves per block
constexpr size_t GL_OBS_LDS_BYTES = 32768;   // per-wave tables live in LDS up to this size per block, else in the global tables
constexpr int64_t GL_OBS_PART_CAP = (int64_t)1 << 23;   // doubles of the global tables at 8 queries in 3-D (64 MB): bounds the grid

__constant__ double c_oq2_lam[GLIMS_DQ2_N][3] = GLIMS_DQ2_LAM;
__constant__ double c_oq2_w[GLIMS_DQ2_N] = GLIMS_DQ2_W;
__constant__ double c_oq3_lam[GLIMS_DQ3_N][4] = GLIMS_DQ3_LAM;
__constant__ double c_oq3_w[GLIMS_DQ3_N] = GLIMS_DQ3_W;

struct ObsQueries {
  int n;
  int kind[GLIMS_OBSERVE_MAX_QUERIES];
  double level[GLIMS_OBSERVE_MAX_QUERIES], smooth[GLIMS_OBSERVE_MAX_QUERIES];
};

// sum over the wave in a fixed order (every lane ends with the same bits)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = GL_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GL_WAVE);
  return v;
}

// Cell pass.  part: the per-wave tables [waves][n_slots][n_q][1 + D] (IN_LDS = 0: accumulated in place, zeroed by the caller;
// IN_LDS = 1: accumulated in LDS and written once).  DEF: positions X + scale u.  The reference orientation of a cell (the sign of
// its volume in X, whatever the vertex order the mesh came with) multiplies its contributions: a cell counts positively where it
// is not folded.
template <int D, int DEF, int IN_LDS>
__global__ __launch_bounds__(256) void k_observe_cells(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                       const uint8_t* __restrict__ label, const int32_t* __restrict__ label_slot,
                                                       int n_slots, const double* __restrict__ xyz, const double* __restrict__ c,
                                                       const double* __restrict__ u, double scale, ObsQueries qs,
                                                       double* __restrict__ part) {
  constexpr int NV = D + 1, NO = D + 1;
  extern __shared__ double lds[];
  const int lane = threadIdx.x & (GL_WAVE - 1), wave = threadIdx.x / GL_WAVE;
  const int64_t gwave = (int64_t)blockIdx.x * GL_OBS_WAVES + wave;
  const int tab_n = n_slots * qs.n * NO;
  double* gtab = part + gwave * tab_n;
  double* tab;
  if constexpr (IN_LDS) {
    tab = lds + (size_t)wave * tab_n;
    for (int i = lane; i < tab_n; i += GL_WAVE) tab[i] = 0.0;
  } else {
    tab = gtab;
  }
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // (wave-uniform trip count: the 64 cells of an iteration are consecutive)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + wave * GL_WAVE; base < n_cells; base += stride) {
    const int64_t e = base + lane;
    const bool valid = e < n_cells;
    int slot = -1;
    int nd[NV];
    double cv[NV], p[NV][D];
    double T = 0.0;
    bool live = false;
    if (valid) {
      slot = label_slot[label[e]];
      double cmax = -INFINITY;
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        nd[m] = cell_nodes[e * NV + m];
        cv[m] = c[nd[m]];
        cmax = fmax(cmax, cv[m]);
      }
      // a cell whose vertices are all out contributes nothing to a SHARP query: no positions are read for it
      for (int q = 0; q < qs.n; ++q) live = live || qs.kind[q] != GLIMS_OBSERVE_SHARP || cmax >= qs.level[q];
      live = live && slot >= 0;
    }
    if (!__any(live)) continue;
    if (live) {
      double X[NV][D];
#pragma unroll
      for (int m = 0; m < NV; ++m)
#pragma unroll
        for (int a = 0; a < D; ++a) {
          X[m][a] = xyz[(int64_t)nd[m] * D + a];
          p[m][a] = X[m][a];
          if constexpr (DEF) p[m][a] = X[m][a] + scale * u[(int64_t)nd[m] * D + a];
        }
      if constexpr (DEF) {
        T = glims_oc_volume<D>(p);
        if (glims_oc_volume<D>(X) < 0.0) T = -T;
      } else {
        T = fabs(glims_oc_volume<D>(p));
      }
    }
    for (int q = 0; q < qs.n; ++q) {
      double o[NO];
#pragma unroll
      for (int k = 0; k < NO; ++k) o[k] = 0.0;
      bool nz = false;
      if (live) {
        double b[D + 2];
        const int kind = qs.kind[q];
        if (kind == GLIMS_OBSERVE_MASS) {
          glims_oc_mass<D>(cv, b);
        } else if (kind == GLIMS_OBSERVE_SHARP) {
          glims_oc_sharp<D>(qs.level[q], cv, b);
        } else {
          if constexpr (D == 2) glims_oc_smooth<2, GLIMS_DQ2_N>(qs.level[q], qs.smooth[q], cv, c_oq2_lam, c_oq2_w, b);
          else glims_oc_smooth<3, GLIMS_DQ3_N>(qs.level[q], qs.smooth[q], cv, c_oq3_lam, c_oq3_w, b);
        }
        glims_oc_map<D>(T, p, b, o);
#pragma unroll
        for (int k = 0; k < NO; ++k) nz = nz || o[k] != 0.0;
      }
      // the distinct labels among the lanes that have something to add, one after the other (wave-uniform)
      unsigned long long todo = __ballot(nz);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int s = __shfl(slot, leader, GL_WAVE);
        const bool mine = nz && slot == s;
        todo &= ~__ballot(mine);
        double r[NO];
#pragma unroll
        for (int k = 0; k < NO; ++k) r[k] = wave_sum(mine ? o[k] : 0.0);
        if (lane == 0) {
          double* t = tab + ((size_t)s * qs.n + q) * NO;
#pragma unroll
          for (int k = 0; k < NO; ++k) t[k] += r[k];
        }
      }
    }
  }
  if constexpr (IN_LDS) {
    for (int i = lane; i < tab_n; i += GL_WAVE) gtab[i] = tab[i];
  }
}

// out[q][slot_label[s]][k] = sum over the waves, in a fixed order, of part[w][s][q][k]; one block per (s, q, k)
__global__ __launch_bounds__(256) void k_observe_sum(int64_t n_waves, int n_q, int no, int n_labels,
                                                     const int32_t* __restrict__ slot_label, const double* __restrict__ part,
                                                     double* __restrict__ out) {
  __shared__ double sm[256];
  const int i = blockIdx.x;                      // (s * n_q + q) * no + k
  const int64_t tab_n = (int64_t)gridDim.x;
  double acc = 0.0;
  for (int64_t w = threadIdx.x; w < n_waves; w += 256) acc += part[w * tab_n + i];
  sm[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int k = i % no, q = (i / no) % n_q, s = i / (no * n_q);
    out[((size_t)q * n_labels + slot_label[s]) * no + k] = sm[0];
  }
}

// ---- volume misfit terms (glims_adjoint_observable_terms; the per-cell mathematics is observe_grad.h) ---------------------------
//   k_observe_grad_cells  one lane per cell over the grid of k_observe_cells, ONE pass for up to GLIMS_OBSERVE_MAX_QUERIES stored
//                         terms of a step: per term the d+1 vertex partials |T| d b0 / d c_a as planes [term][a][cell] (exact
//                         zeros where the term's mask excludes the cell) and the wave's sum of V_T into its own row of `part`
//   k_observe_second_cells  the same pass for one Hessian direction: grad V_T . dc|_T summed per wave, (H_T dc)_a as planes
//   k_observe_grad_sum    one block per term: the per-wave rows summed in a fixed order; V, weight (V - target), the cut cells
//   k_observe_grad_rows   lane = row along cslice_ptr / celem (as k_derive_rows<NV, 1, 1>): g[row] += sum_t coef_t sum_incidences
//                         partial -- the row owns its sum, no atomics
// A batch with a term of the DEFORMED configuration (glims_adjoint_observable_terms2) runs k_observe_grad_cells<D, 1>, then
//   k_observe_def_load_cells  one lane per cell: the combined planes of dJ/du_k (coefficients times the cofactors of the cell)
//   k_observe_grad_rows<NV, D>  their row-owned gather into the load of the step's elastic adjoint
//   k_observe_def_sum     one block per term: the folded cells and the smallest volume ratio
// A batch with a CENTRE-OF-MASS term (glims_adjoint_observable_terms3) first runs
//   k_observe_mom_cells   one lane per cell: per such term the wave's sums of V_T and M_T (the arithmetic of k_observe_cells)
//   k_observe_mom_sum     one block per term: V, M in a fixed order, then X = M / V, alpha, J and the empty flag, left on the device
// and then the COM = 1 instances of k_observe_grad_cells / k_observe_def_load_cells, which weight the first-moment partials
// with psi = alpha . (p - X) and write them into the same planes; gather and u-gather are unchanged
struct ObsGradTerms {
  int n;
  int kind[GLIMS_OBSERVE_MAX_QUERIES];
  double level[GLIMS_OBSERVE_MAX_QUERIES], smooth[GLIMS_OBSERVE_MAX_QUERIES];
  double weight[GLIMS_OBSERVE_MAX_QUERIES], target[GLIMS_OBSERVE_MAX_QUERIES];
  int deformed[GLIMS_OBSERVE_MAX_QUERIES];   // the term measures the cells at X + scale u (k_observe_grad_cells<D, 1>)
  double scale[GLIMS_OBSERVE_MAX_QUERIES];
  unsigned long long mask[GLIMS_OBSERVE_MAX_QUERIES][GL_MAX_LABELS / 64];   // bit l: the cells of label l are counted
  int moment[GLIMS_OBSERVE_MAX_QUERIES];     // a centre-of-mass term (target_x in place of target)
  double target_x[GLIMS_OBSERVE_MAX_QUERIES][3];
};
// what k_observe_mom_sum leaves on the device per centre-of-mass term of a batch
constexpr int GL_OBS_MOM = 12;       // V, M[3], X[3], alpha[3], J, empty
constexpr int GL_OBS_MOM_X = 4, GL_OBS_MOM_ALPHA = 7, GL_OBS_MOM_J = 10, GL_OBS_MOM_EMPTY = 11;
static_assert(GL_MAX_LABELS == 256, "ObsGradTerms::mask is four 64-bit words per term");

__device__ __forceinline__ bool obs_counted(const ObsGradTerms& ts, int q, int lab) {
  const int w = lab >> 6;
  const unsigned long long m = w == 0 ? ts.mask[q][0] : w == 1 ? ts.mask[q][1] : w == 2 ? ts.mask[q][2] : ts.mask[q][3];
  return (m >> (lab & 63)) & 1ull;
}

// part / cut_part: rows [waves][MAX_QUERIES], every entry written here: a wave keeps its sums in its own row of LDS (lane 0 alone
// touches it) and stores the row once after the loop.
// DEF = 0: every term measures the reference cells (|T| = evol); xyz, u, b0p, fold_part and ratio_part are not touched.
// DEF = 1 (a batch with a deformed term): X and u_k at the cell's vertices are read once; a deformed term forms y = X + scale u
// with its OWN scale and takes T = sigma vol(y), sigma = the reference orientation (as k_observe_cells<D, 1>: a folded cell
// counts negatively); it also writes b0 as the plane b0p [term][cell] (what k_observe_def_load_cells multiplies the cofactors
// with; 0 where the cell is not counted) and the wave's count of counted cells with vol(y) / vol(X) not > 0 and its smallest
// such ratio into fold_part / ratio_part (rows as part).  A reference term of the same batch takes evol[e] as in DEF = 0.
// COM = 1 (a batch with a centre-of-mass term, after k_observe_mom_sum has left X and alpha in `mom`): X is read whatever DEF is;
// such a term forms psi_m = alpha . (p_m - X) at its own positions p (X, or y when deformed) and writes T sum_m psi_m
// d b[1 + m] / d c_a into the planes (glims_og_moment_*); its entry of `part` is V again.  A deformed one writes B = sum_m
// b[1 + m] psi_m in place of b0 and T b[1 + m] as the planes b1p [term][a][cell].  The volume terms of the batch are computed
// as with COM = 0.
template <int D, int DEF, int COM>
__global__ __launch_bounds__(256) void k_observe_grad_cells(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                            const uint8_t* __restrict__ label, const double* __restrict__ evol,
                                                            const double* __restrict__ c, ObsGradTerms ts,
                                                            double* __restrict__ planes, double* __restrict__ part,
                                                            unsigned int* __restrict__ cut_part,
                                                            const double* __restrict__ xyz, const double* __restrict__ u,
                                                            double* __restrict__ b0p, unsigned int* __restrict__ fold_part,
                                                            double* __restrict__ ratio_part, const double* __restrict__ mom,
                                                            double* __restrict__ b1p) {
  constexpr int NV = D + 1;
  const int lane = threadIdx.x & (GL_WAVE - 1), wave = threadIdx.x / GL_WAVE;
  const int64_t gwave = (int64_t)blockIdx.x * GL_OBS_WAVES + wave;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  __shared__ double acc[GL_OBS_WAVES][GLIMS_OBSERVE_MAX_QUERIES];
  __shared__ unsigned int acc_cut[GL_OBS_WAVES][GLIMS_OBSERVE_MAX_QUERIES];
  __shared__ unsigned int acc_fold[DEF ? GL_OBS_WAVES : 1][GLIMS_OBSERVE_MAX_QUERIES];
  __shared__ double acc_ratio[DEF ? GL_OBS_WAVES : 1][GLIMS_OBSERVE_MAX_QUERIES];
  if (lane == 0)
    for (int q = 0; q < GLIMS_OBSERVE_MAX_QUERIES; ++q) {
      acc[wave][q] = 0.0;
      acc_cut[wave][q] = 0u;
      if constexpr (DEF) {
        acc_fold[wave][q] = 0u;
        acc_ratio[wave][q] = INFINITY;
      }
    }
  // (wave-uniform trip count: the 64 cells of an iteration are consecutive)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + wave * GL_WAVE; base < n_cells; base += stride) {
    const int64_t e = base + lane;
    const bool valid = e < n_cells;
    int lab = 0;
    double cv[NV], T = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) cv[m] = 0.0;
    [[maybe_unused]] double X[NV][D], U[NV][D], volX = 1.0;
    if (valid) {
      lab = label[e];
      T = evol[e];
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        const int32_t nd = cell_nodes[e * NV + m];
        cv[m] = c[nd];
        if constexpr (DEF || COM) {
#pragma unroll
          for (int a = 0; a < D; ++a) {
            X[m][a] = xyz[(int64_t)nd * D + a];
            if constexpr (DEF) U[m][a] = u[(int64_t)nd * D + a];
          }
        }
      }
      if constexpr (DEF) volX = glims_oc_volume<D>(X);
    }
    for (int q = 0; q < ts.n; ++q) {
      double g[NV], v = 0.0;
      [[maybe_unused]] double b1_out[NV];
      [[maybe_unused]] bool is_mom = false;
      if constexpr (COM) is_mom = ts.moment[q] != 0;   // (wave-uniform)
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        g[m] = 0.0;
        if constexpr (COM) b1_out[m] = 0.0;
      }
      bool cut = false;
      [[maybe_unused]] bool folded = false;
      [[maybe_unused]] double ratio = INFINITY, b0_out = 0.0;
      if (valid && obs_counted(ts, q, lab)) {
        const int kind = ts.kind[q];
        if constexpr (DEF) {
          if (ts.deformed[q]) {
            double y[NV][D];
            const double sc = ts.scale[q];
#pragma unroll
            for (int m = 0; m < NV; ++m)
#pragma unroll
              for (int a = 0; a < D; ++a) y[m][a] = X[m][a] + sc * U[m][a];
            const double vy = glims_oc_volume<D>(y);
            T = volX < 0.0 ? -vy : vy;
            ratio = vy / volX;
            folded = !(ratio > 0.0);
          } else {
            T = evol[e];
          }
        }
        double b0 = 0.0;
        bool done = false;
        if constexpr (COM) {
          if (is_mom) {
            const double* mv = mom + q * GL_OBS_MOM;
            double psi[NV], b[D + 2];
#pragma unroll
            for (int m = 0; m < NV; ++m) {
              double s = 0.0;
#pragma unroll
              for (int a = 0; a < D; ++a) {
                double pa = X[m][a];
                if constexpr (DEF) {
                  if (ts.deformed[q]) pa = X[m][a] + ts.scale[q] * U[m][a];
                }
                s += mv[GL_OBS_MOM_ALPHA + a] * (pa - mv[GL_OBS_MOM_X + a]);
              }
              psi[m] = s;
            }
            if (kind == GLIMS_OBSERVE_MASS) {
              glims_og_moment_mass<D>(cv, psi, b, g);
            } else if (kind == GLIMS_OBSERVE_SHARP) {
              const int n_in = glims_og_moment_sharp<D>(ts.level[q], cv, psi, b, g);
              cut = n_in > 0 && n_in < NV;
            } else {
              if constexpr (D == 2)
                glims_og_moment_smooth<2, GLIMS_DQ2_N>(ts.level[q], ts.smooth[q], cv, c_oq2_lam, c_oq2_w, psi, b, g);
              else
                glims_og_moment_smooth<3, GLIMS_DQ3_N>(ts.level[q], ts.smooth[q], cv, c_oq3_lam, c_oq3_w, psi, b, g);
            }
            b0 = b[0];
            double B = 0.0;
#pragma unroll
            for (int m = 0; m < NV; ++m) {
              B += b[1 + m] * psi[m];
              b1_out[m] = T * b[1 + m];
            }
            if constexpr (DEF) b0_out = B;
            done = true;
          }
        }
        if (!done) {
          if (kind == GLIMS_OBSERVE_MASS) {
            b0 = glims_og_mass<D>(cv, g);
          } else if (kind == GLIMS_OBSERVE_SHARP) {
            int n_in = 0;
            b0 = glims_og_sharp<D>(ts.level[q], cv, g, &n_in);
            cut = n_in > 0 && n_in < NV;
          } else {
            if constexpr (D == 2)
              b0 = glims_og_smooth<2, GLIMS_DQ2_N>(ts.level[q], ts.smooth[q], cv, c_oq2_lam, c_oq2_w, g, nullptr, nullptr);
            else
              b0 = glims_og_smooth<3, GLIMS_DQ3_N>(ts.level[q], ts.smooth[q], cv, c_oq3_lam, c_oq3_w, g, nullptr, nullptr);
          }
          if constexpr (DEF) b0_out = b0;
        }
        v = T * b0;
#pragma unroll
        for (int m = 0; m < NV; ++m) g[m] *= T;
      }
      if (valid) {
#pragma unroll
        for (int m = 0; m < NV; ++m) planes[((int64_t)q * NV + m) * n_cells + e] = g[m];
        if constexpr (DEF) {
          if (ts.deformed[q]) {
            b0p[(int64_t)q * n_cells + e] = b0_out;
            if constexpr (COM) {
              if (is_mom) {
#pragma unroll
                for (int m = 0; m < NV; ++m) b1p[((int64_t)q * NV + m) * n_cells + e] = b1_out[m];
              }
            }
          }
        }
      }
      const double r = wave_sum(v);
      const unsigned int n_cut = (unsigned int)__popcll(__ballot(cut));
      if (lane == 0) {
        acc[wave][q] += r;
        acc_cut[wave][q] += n_cut;
      }
      if constexpr (DEF) {
        if (ts.deformed[q]) {   // (wave-uniform)
          const unsigned int n_fold = (unsigned int)__popcll(__ballot(folded));
          // a NaN ratio (a degenerate reference cell) counts as folded and is left out of the minimum
          double mr = ratio == ratio ? ratio : INFINITY;
#pragma unroll
          for (int o = GL_WAVE / 2; o > 0; o >>= 1) mr = fmin(mr, __shfl_xor(mr, o, GL_WAVE));
          if (lane == 0) {
            acc_fold[wave][q] += n_fold;
            acc_ratio[wave][q] = fmin(acc_ratio[wave][q], mr);
          }
        }
      }
    }
  }
  if (lane == 0)
    for (int q = 0; q < GLIMS_OBSERVE_MAX_QUERIES; ++q) {
      part[gwave * GLIMS_OBSERVE_MAX_QUERIES + q] = acc[wave][q];
      cut_part[gwave * GLIMS_OBSERVE_MAX_QUERIES + q] = acc_cut[wave][q];
      if constexpr (DEF) {
        fold_part[gwave * GLIMS_OBSERVE_MAX_QUERIES + q] = acc_fold[wave][q];
        ratio_part[gwave * GLIMS_OBSERVE_MAX_QUERIES + q] = acc_ratio[wave][q];
      }
    }
}

// The u-load of a batch's deformed terms, one lane per cell (launched after k_observe_grad_sum, which leaves coef_t = weight_t
// (V_t - target_t) on the device): lp [a][k][cell] = sum over the deformed terms t of coef_t s_t sigma b0_t d vol(y(s_t)) / d y_a,k
// with the cofactors of glims_og_volume_grad at the term's own y = X + s_t u -- 8 (d+1) d n_cells bytes whatever the number of
// terms.  Every entry is written (zeros where no term counts the cell); k_observe_grad_rows<NV, D> gathers the planes into murhs.
// COM = 1: a deformed centre-of-mass term has coef = 1 (0 when empty) and B in place of b0, and adds coef s T b[1 + m] alpha_k
// from the planes b1p and the alpha k_observe_mom_sum left in `mom`.
template <int D, int COM>
__global__ __launch_bounds__(256) void k_observe_def_load_cells(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                                const double* __restrict__ xyz, const double* __restrict__ u,
                                                                ObsGradTerms ts, const double* __restrict__ b0p,
                                                                const double* __restrict__ coef, double* __restrict__ lp,
                                                                const double* __restrict__ b1p, const double* __restrict__ mom) {
  constexpr int NV = D + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_cells) return;
  double X[NV][D], U[NV][D], acc[NV][D];
#pragma unroll
  for (int m = 0; m < NV; ++m) {
    const int32_t nd = cell_nodes[e * NV + m];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      X[m][a] = xyz[(int64_t)nd * D + a];
      U[m][a] = u[(int64_t)nd * D + a];
      acc[m][a] = 0.0;
    }
  }
  const double sigma = glims_oc_volume<D>(X) < 0.0 ? -1.0 : 1.0;
  for (int q = 0; q < ts.n; ++q) {
    if (!ts.deformed[q]) continue;
    const double sc = ts.scale[q];
    const double f = coef[q] * sc * sigma * b0p[(int64_t)q * n_cells + e];
    if constexpr (COM) {
      if (ts.moment[q]) {
        const double fs = coef[q] * sc;
#pragma unroll
        for (int m = 0; m < NV; ++m) {
          const double w = fs * b1p[((int64_t)q * NV + m) * n_cells + e];
#pragma unroll
          for (int a = 0; a < D; ++a) acc[m][a] += w * mom[q * GL_OBS_MOM + GL_OBS_MOM_ALPHA + a];
        }
      }
    }
    if (f == 0.0) continue;   // (a cell the term does not count, b0 = 0 or scale = 0: exact zeros are added nowhere)
    double y[NV][D], dv[NV][D];
#pragma unroll
    for (int m = 0; m < NV; ++m)
#pragma unroll
      for (int a = 0; a < D; ++a) y[m][a] = X[m][a] + sc * U[m][a];
    glims_og_volume_grad<D>(y, dv);
#pragma unroll
    for (int m = 0; m < NV; ++m)
#pragma unroll
      for (int a = 0; a < D; ++a) acc[m][a] += f * dv[m][a];
  }
#pragma unroll
  for (int m = 0; m < NV; ++m)
#pragma unroll
    for (int a = 0; a < D; ++a) lp[((int64_t)m * D + a) * n_cells + e] = acc[m][a];
}

// One block per term q of a batch with deformed terms: folds[q] = the folded counted cells, ratios[q] = the smallest ratio
// (+inf where no cell is counted), from the per-wave rows; integer sums and minima: the order does not matter
__global__ __launch_bounds__(256) void k_observe_def_sum(int64_t n_waves, const unsigned int* __restrict__ fold_part,
                                                         const double* __restrict__ ratio_part, long long* __restrict__ folds,
                                                         double* __restrict__ ratios) {
  __shared__ double sm[256];
  __shared__ long long sc[256];
  const int q = blockIdx.x;
  double mr = INFINITY;
  long long cnt = 0;
  for (int64_t w = threadIdx.x; w < n_waves; w += 256) {
    mr = fmin(mr, ratio_part[w * GLIMS_OBSERVE_MAX_QUERIES + q]);
    cnt += fold_part[w * GLIMS_OBSERVE_MAX_QUERIES + q];
  }
  sm[threadIdx.x] = mr;
  sc[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sm[threadIdx.x] = fmin(sm[threadIdx.x], sm[threadIdx.x + o]);
      sc[threadIdx.x] += sc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    folds[q] = sc[0];
    ratios[q] = sm[0];
  }
}

// The moments pass of a batch with a centre-of-mass term: the arithmetic of k_observe_cells restricted to the batch's masks.  One
// lane per cell over the grid of k_observe_grad_cells; per centre-of-mass term the wave's sums of V_T = T b[0] and
// M_T,a = T sum_m b[1 + m] p_m,a (glims_oc_*, glims_oc_map) into its own row of mom_part [waves][MAX_QUERIES][4], every entry
// written.  T and p as in k_observe_grad_cells: evol and X, or sigma vol(y) and y = X + scale u for a deformed term (DEF = 1).
template <int D, int DEF>
__global__ __launch_bounds__(256) void k_observe_mom_cells(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                           const uint8_t* __restrict__ label, const double* __restrict__ evol,
                                                           const double* __restrict__ c, ObsGradTerms ts,
                                                           const double* __restrict__ xyz, const double* __restrict__ u,
                                                           double* __restrict__ mom_part) {
  constexpr int NV = D + 1;
  const int lane = threadIdx.x & (GL_WAVE - 1), wave = threadIdx.x / GL_WAVE;
  const int64_t gwave = (int64_t)blockIdx.x * GL_OBS_WAVES + wave;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  __shared__ double acc[GL_OBS_WAVES][GLIMS_OBSERVE_MAX_QUERIES][4];
  if (lane == 0)
    for (int q = 0; q < GLIMS_OBSERVE_MAX_QUERIES; ++q)
      for (int k = 0; k < 4; ++k) acc[wave][q][k] = 0.0;
  // (wave-uniform trip count: the 64 cells of an iteration are consecutive)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + wave * GL_WAVE; base < n_cells; base += stride) {
    const int64_t e = base + lane;
    const bool valid = e < n_cells;
    int lab = 0;
    double cv[NV], X[NV][D], Tref = 0.0;
    [[maybe_unused]] double U[NV][D], volX = 1.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      cv[m] = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        X[m][a] = 0.0;
        if constexpr (DEF) U[m][a] = 0.0;
      }
    }
    if (valid) {
      lab = label[e];
      Tref = evol[e];
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        const int32_t nd = cell_nodes[e * NV + m];
        cv[m] = c[nd];
#pragma unroll
        for (int a = 0; a < D; ++a) {
          X[m][a] = xyz[(int64_t)nd * D + a];
          if constexpr (DEF) U[m][a] = u[(int64_t)nd * D + a];
        }
      }
      if constexpr (DEF) volX = glims_oc_volume<D>(X);
    }
    for (int q = 0; q < ts.n; ++q) {
      if (!ts.moment[q]) continue;   // (wave-uniform)
      double o[NV];
#pragma unroll
      for (int k = 0; k < NV; ++k) o[k] = 0.0;
      if (valid && obs_counted(ts, q, lab)) {
        double p[NV][D], T = Tref;
#pragma unroll
        for (int m = 0; m < NV; ++m)
#pragma unroll
          for (int a = 0; a < D; ++a) p[m][a] = X[m][a];
        if constexpr (DEF) {
          if (ts.deformed[q]) {
            const double sc = ts.scale[q];
#pragma unroll
            for (int m = 0; m < NV; ++m)
#pragma unroll
              for (int a = 0; a < D; ++a) p[m][a] = X[m][a] + sc * U[m][a];
            const double vy = glims_oc_volume<D>(p);
            T = volX < 0.0 ? -vy : vy;
          }
        }
        double b[D + 2];
        const int kind = ts.kind[q];
        if (kind == GLIMS_OBSERVE_MASS) {
          glims_oc_mass<D>(cv, b);
        } else if (kind == GLIMS_OBSERVE_SHARP) {
          glims_oc_sharp<D>(ts.level[q], cv, b);
        } else {
          if constexpr (D == 2) glims_oc_smooth<2, GLIMS_DQ2_N>(ts.level[q], ts.smooth[q], cv, c_oq2_lam, c_oq2_w, b);
          else glims_oc_smooth<3, GLIMS_DQ3_N>(ts.level[q], ts.smooth[q], cv, c_oq3_lam, c_oq3_w, b);
        }
        glims_oc_map<D>(T, p, b, o);
      }
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const double r = wave_sum(o[k]);
        if (lane == 0) acc[wave][q][k] += r;
      }
    }
  }
  if (lane == 0)
    for (int q = 0; q < GLIMS_OBSERVE_MAX_QUERIES; ++q)
      for (int k = 0; k < 4; ++k) mom_part[(gwave * GLIMS_OBSERVE_MAX_QUERIES + q) * 4 + k] = acc[wave][q][k];
}

// One block per term q of a batch with a centre-of-mass term: V and M = the per-wave rows summed in a fixed order, then, by one
// thread, X = M / V, alpha = weight (X - target_x) / V and J = 1/2 weight |X - target_x|^2 into mom [q][GL_OBS_MOM].  A measure
// that is not > 0 is EMPTY: X = alpha = J = 0 and the flag set, so that every partial of the term comes out as an exact zero.
// The rows of the batch's volume terms are zeroed.
__global__ __launch_bounds__(256) void k_observe_mom_sum(int64_t n_waves, int dim, const double* __restrict__ mom_part,
                                                         ObsGradTerms ts, double* __restrict__ mom) {
  __shared__ double sm[256];
  __shared__ double tot[4];
  const int q = blockIdx.x;
  if (!ts.moment[q]) {
    if (threadIdx.x < GL_OBS_MOM) mom[q * GL_OBS_MOM + threadIdx.x] = 0.0;
    return;
  }
  for (int k = 0; k <= dim; ++k) {
    double acc = 0.0;
    for (int64_t w = threadIdx.x; w < n_waves; w += 256) acc += mom_part[(w * GLIMS_OBSERVE_MAX_QUERIES + q) * 4 + k];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) tot[k] = sm[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* mv = mom + q * GL_OBS_MOM;
    const double V = tot[0];
    const bool empty = !(V > 0.0);
    double J = 0.0;
    mv[0] = V;
    for (int a = 0; a < 3; ++a) {
      const double M = a < dim ? tot[1 + a] : 0.0;
      double X = 0.0, al = 0.0;
      if (!empty && a < dim) {
        X = M / V;
        const double r = X - ts.target_x[q][a];
        al = ts.weight[q] * r / V;
        J += r * r;
      }
      mv[1 + a] = M;
      mv[GL_OBS_MOM_X + a] = X;
      mv[GL_OBS_MOM_ALPHA + a] = al;
    }
    mv[GL_OBS_MOM_J] = 0.5 * ts.weight[q] * J;
    mv[GL_OBS_MOM_EMPTY] = empty ? 1.0 : 0.0;
  }
}

// One Hessian direction dc: per term the wave's sum of grad V_T . dc|_T (from the planes of k_observe_grad_cells) into `part`,
// and planes2 [term][a][cell] = |T| (H_T dc)_a -- SMOOTH alone has one; zeros for the other kinds and the cells not counted
template <int D>
__global__ __launch_bounds__(256) void k_observe_second_cells(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                              const uint8_t* __restrict__ label, const double* __restrict__ evol,
                                                              const double* __restrict__ c, const double* __restrict__ dc,
                                                              ObsGradTerms ts, const double* __restrict__ planes,
                                                              double* __restrict__ planes2, double* __restrict__ part) {
  constexpr int NV = D + 1;
  const int lane = threadIdx.x & (GL_WAVE - 1), wave = threadIdx.x / GL_WAVE;
  const int64_t gwave = (int64_t)blockIdx.x * GL_OBS_WAVES + wave;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  __shared__ double acc[GL_OBS_WAVES][GLIMS_OBSERVE_MAX_QUERIES];   // (as k_observe_grad_cells)
  if (lane == 0)
    for (int q = 0; q < GLIMS_OBSERVE_MAX_QUERIES; ++q) acc[wave][q] = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + wave * GL_WAVE; base < n_cells; base += stride) {
    const int64_t e = base + lane;
    const bool valid = e < n_cells;
    int lab = 0;
    double cv[NV], dv[NV], T = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) cv[m] = dv[m] = 0.0;
    if (valid) {
      lab = label[e];
      T = evol[e];
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        const int32_t nd = cell_nodes[e * NV + m];
        cv[m] = c[nd];
        dv[m] = dc[nd];
      }
    }
    for (int q = 0; q < ts.n; ++q) {
      double Hd[NV], s = 0.0;
#pragma unroll
      for (int m = 0; m < NV; ++m) Hd[m] = 0.0;
      if (valid) {
#pragma unroll
        for (int m = 0; m < NV; ++m) s += planes[((int64_t)q * NV + m) * n_cells + e] * dv[m];
        if (ts.kind[q] == GLIMS_OBSERVE_SMOOTH && obs_counted(ts, q, lab)) {
          double g[NV];
          if constexpr (D == 2)
            (void)glims_og_smooth<2, GLIMS_DQ2_N>(ts.level[q], ts.smooth[q], cv, c_oq2_lam, c_oq2_w, g, dv, Hd);
          else
            (void)glims_og_smooth<3, GLIMS_DQ3_N>(ts.level[q], ts.smooth[q], cv, c_oq3_lam, c_oq3_w, g, dv, Hd);
#pragma unroll
          for (int m = 0; m < NV; ++m) Hd[m] *= T;
        }
#pragma unroll
        for (int m = 0; m < NV; ++m) planes2[((int64_t)q * NV + m) * n_cells + e] = Hd[m];
      }
      const double r = wave_sum(s);
      if (lane == 0) acc[wave][q] += r;
    }
  }
  if (lane == 0)
    for (int q = 0; q < GLIMS_OBSERVE_MAX_QUERIES; ++q) part[gwave * GLIMS_OBSERVE_MAX_QUERIES + q] = acc[wave][q];
}

// One block per term q: S = the per-wave rows summed in a fixed order.  mode 0: vals[q] = V = S, vals[MAXQ + q] = weight (V -
// target), cuts[q] = the cut cells;  mode 1: vals[2 MAXQ + q] = weight S  (weight g^T dc_j of a Hessian direction)
// mom != nullptr (a batch with a centre-of-mass term, mode 0): such a term's coefficient is 1, or 0 when its measure was empty
__global__ __launch_bounds__(256) void k_observe_grad_sum(int64_t n_waves, const double* __restrict__ part,
                                                          const unsigned int* __restrict__ cut_part, ObsGradTerms ts, int mode,
                                                          double* __restrict__ vals, long long* __restrict__ cuts,
                                                          const double* __restrict__ mom) {
  __shared__ double sm[256];
  __shared__ long long sc[256];
  const int q = blockIdx.x;
  double acc = 0.0;
  long long cnt = 0;
  for (int64_t w = threadIdx.x; w < n_waves; w += 256) {
    acc += part[w * GLIMS_OBSERVE_MAX_QUERIES + q];
    if (mode == 0) cnt += cut_part[w * GLIMS_OBSERVE_MAX_QUERIES + q];
  }
  sm[threadIdx.x] = acc;
  sc[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sm[threadIdx.x] += sm[threadIdx.x + o];
      sc[threadIdx.x] += sc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (mode == 0) {
      vals[q] = sm[0];
      vals[GLIMS_OBSERVE_MAX_QUERIES + q] = ts.weight[q] * (sm[0] - ts.target[q]);
      if (mom && ts.moment[q]) vals[GLIMS_OBSERVE_MAX_QUERIES + q] = mom[q * GL_OBS_MOM + GL_OBS_MOM_EMPTY] != 0.0 ? 0.0 : 1.0;
      cuts[q] = sc[0];
    } else {
      vals[2 * GLIMS_OBSERVE_MAX_QUERIES + q] = ts.weight[q] * sm[0];
    }
  }
}

// g[row] += sum_t (coef_a[t] A_t + coef_b[t] B_t), A_t / B_t = the row's sums, along its incidence list in list order, of the
// planes pa / pb [t][a][cell] at the vertex a the row is in that cell (pb == nullptr: the first part alone).  The terms' sum
// starts from 0 and is added to g once: a list sent in two parts gives the bits of the whole.
// NC = 1 is the gather of the c-partials.  NC = D gathers ONE combined term with NC components per vertex, planes pa
// [a][comp][cell], into g[row * NC + comp] (the u-load of k_observe_def_load_cells into murhs): n_t = 1, pb = nullptr.
template <int NV, int NC>
__global__ __launch_bounds__(256) void k_observe_grad_rows(int64_t n_own, int64_t n_cells,
                                                           const int64_t* __restrict__ cslice_ptr,
                                                           const int32_t* __restrict__ celem,
                                                           const int32_t* __restrict__ cell_nodes, int n_t,
                                                           const double* __restrict__ pa, const double* __restrict__ coef_a,
                                                           const double* __restrict__ pb, const double* __restrict__ coef_b,
                                                           double* __restrict__ g) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  if constexpr (NC > 1) {
    double A[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) A[q] = 0.0;
    for (int k = 0; k < clen; ++k) {
      const int32_t e = celem[cbase + (int64_t)k * GL_WAVE + lane];
      if (e < 0) continue;
      int a = -1;
#pragma unroll
      for (int m = 0; m < NV; ++m)
        if (cell_nodes[(int64_t)e * NV + m] == (int32_t)row) a = m;
      if (a < 0) continue;
#pragma unroll
      for (int q = 0; q < NC; ++q) A[q] += pa[((int64_t)a * NC + q) * n_cells + e];
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) g[row * NC + q] += A[q];
    return;
  }
  double A[GLIMS_OBSERVE_MAX_QUERIES], B[GLIMS_OBSERVE_MAX_QUERIES];
#pragma unroll
  for (int t = 0; t < GLIMS_OBSERVE_MAX_QUERIES; ++t) A[t] = B[t] = 0.0;
  for (int k = 0; k < clen; ++k) {
    const int32_t e = celem[cbase + (int64_t)k * GL_WAVE + lane];
    if (e < 0) continue;
    int a = -1;
#pragma unroll
    for (int m = 0; m < NV; ++m)
      if (cell_nodes[(int64_t)e * NV + m] == (int32_t)row) a = m;
    if (a < 0) continue;
#pragma unroll
    for (int t = 0; t < GLIMS_OBSERVE_MAX_QUERIES; ++t)
      if (t < n_t) {
        const int64_t at = ((int64_t)t * NV + a) * n_cells + e;
        A[t] += pa[at];
        if (pb) B[t] += pb[at];
      }
  }
  double sum = 0.0;
#pragma unroll
  for (int t = 0; t < GLIMS_OBSERVE_MAX_QUERIES; ++t)
    if (t < n_t) {
      sum += coef_a[t] * A[t];
      if (pb) sum += coef_b[t] * B[t];
    }
  g[row] += sum;
}

inline int worse(int a, int b) { return a == GLIMS_NAN || b == GLIMS_OK ? a : b; }

// which labels the cells carry, read from the device once per handle: compact slots in ascending label order
void ensure_slots(glims_ctx* h) {
  ObserveState& os = h->observe;
  if (!os.slot_label.empty() || h->n_cells == 0) return;
  std::vector<uint8_t> lab((size_t)h->n_cells);
  GL_HIP(hipMemcpyAsync(lab.data(), h->label.p, lab.size(), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  std::vector<uint8_t> used(GL_MAX_LABELS, 0);
  for (uint8_t l : lab) used[l] = 1;
  std::vector<int32_t> slot_of(GL_MAX_LABELS, -1), label_of;
  for (int l = 0; l < GL_MAX_LABELS; ++l)
    if (used[l]) {
      slot_of[l] = (int32_t)label_of.size();
      label_of.push_back(l);
    }
  os.label_slot.upload(slot_of, h->st);
  os.d_slot_label.upload(label_of, h->st);
  GL_HIP(hipStreamSynchronize(h->st));
  os.slot_label = label_of;
}

template <int D>
void launch_pass(glims_ctx* h, const ObsQueries& qs, const double* c, const double* u, double scale, int nb, bool in_lds,
                 double* out) {
  ObserveState& os = h->observe;
  const int n_slots = (int)os.slot_label.size(), no = D + 1;
  const int tab_n = n_slots * qs.n * no;
  const int64_t n_waves = (int64_t)nb * GL_OBS_WAVES;
  const size_t lds = in_lds ? (size_t)GL_OBS_WAVES * tab_n * sizeof(double) : 0;
  if (!in_lds) GL_HIP(hipMemsetAsync(os.part.p, 0, (size_t)n_waves * tab_n * sizeof(double), h->st));
#define GL_OBS_LAUNCH(DEF, L)                                                                                               \
  hipLaunchKernelGGL((k_observe_cells<D, DEF, L>), dim3(nb), dim3(256), lds, h->st, h->n_cells, h->adj.cell_nodes.p, h->label.p, \
                     os.label_slot.p, n_slots, h->xyz_new.p, c, u, scale, qs, os.part.p)
  if (u) {
    if (in_lds) GL_OBS_LAUNCH(1, 1);
    else GL_OBS_LAUNCH(1, 0);
  } else {
    if (in_lds) GL_OBS_LAUNCH(0, 1);
    else GL_OBS_LAUNCH(0, 0);
  }
#undef GL_OBS_LAUNCH
  GL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_observe_sum, dim3(tab_n), dim3(256), 0, h->st, n_waves, qs.n, no, h->n_labels, os.d_slot_label.p,
                     os.part.p, out);
  GL_CHECK_LAUNCH();
  os.n_cell_passes++;
}

}  // namespace

int gl_observe(glims_ctx* h, int n_src, const int64_t* src, const double* c_host, const double* u_host, int deformed,
               double scale, int n_q, const glims_observable* q, double* out) {
  ObserveState& os = h->observe;
  // ---- refusals: nothing is changed or written before the last of them ----
  GL_REQUIRE(h->world <= 1, "glims_observe: not available on a partitioned handle (world > 1); the host path computes the "
                            "observables there");
  GL_REQUIRE(h->is_setup, "glims_observe before glims_setup");
  GL_REQUIRE(n_src >= 1, "glims_observe: n_src must be at least 1");
  GL_REQUIRE(n_q >= 1 && n_q <= GLIMS_OBSERVE_MAX_QUERIES,
             "glims_observe: n_q = " + std::to_string(n_q) + " outside 1.." + std::to_string(GLIMS_OBSERVE_MAX_QUERIES));
  GL_REQUIRE(src && q && out, "glims_observe: src, q and out are required (null pointer)");
  GL_REQUIRE(std::isfinite(scale), "glims_observe: scale is not finite");
  ObsQueries qs;
  qs.n = n_q;
  for (int k = 0; k < GLIMS_OBSERVE_MAX_QUERIES; ++k) {
    qs.kind[k] = GLIMS_OBSERVE_MASS;
    qs.level[k] = 0.0;
    qs.smooth[k] = 1.0;
  }
  for (int k = 0; k < n_q; ++k) {
    GL_REQUIRE(q[k].kind >= GLIMS_OBSERVE_MASS && q[k].kind <= GLIMS_OBSERVE_SMOOTH,
               "glims_observe: unknown kind " + std::to_string(q[k].kind) + " of query " + std::to_string(k));
    GL_REQUIRE(std::isfinite(q[k].level), "glims_observe: level of query " + std::to_string(k) + " is not finite");
    GL_REQUIRE(q[k].kind != GLIMS_OBSERVE_SMOOTH || q[k].smooth > 0.0,
               "glims_observe: smooth of query " + std::to_string(k) + " must be positive");
    qs.kind[k] = q[k].kind;
    qs.level[k] = q[k].level;
    if (q[k].kind == GLIMS_OBSERVE_SMOOTH) qs.smooth[k] = q[k].smooth;
  }
  GL_REQUIRE(!deformed || (h->have_mech && h->U.p),
             "glims_observe: the deformed configuration needs the displacement: glims_setup(with_mechanics=1) first");
  for (int i = 0; i < n_src; ++i) {
    const int64_t s = src[i];
    if (s == GLIMS_DERIVE_HOST || s == GLIMS_DERIVE_CURRENT) {
      GL_REQUIRE(n_src == 1, "glims_observe: GLIMS_DERIVE_CURRENT / GLIMS_DERIVE_HOST take n_src = 1");
      if (s == GLIMS_DERIVE_HOST) {
        GL_REQUIRE(c_host, "glims_observe: GLIMS_DERIVE_HOST needs c_host (null pointer)");
        GL_REQUIRE(!deformed || u_host, "glims_observe: GLIMS_DERIVE_HOST in the deformed configuration needs u_host (null pointer)");
      } else {
        GL_REQUIRE(h->have_state, "glims_observe: GLIMS_DERIVE_CURRENT before glims_set_state");
      }
    } else {
      GL_REQUIRE(s >= 0 && s < (int64_t)h->snapshots.size() && h->snapshots[(size_t)s],
                 "glims_observe: unknown snapshot id " + std::to_string(s));
    }
  }
  GL_REQUIRE(h->n_labels > 0, "glims_observe before glims_set_materials");
  GL_REQUIRE(h->xyz_new.n == (size_t)h->n_nodes * h->dim, "glims_observe: mesh coordinates missing");
  ensure_slots(h);
  GL_REQUIRE(os.slot_label.empty() || os.slot_label.back() < h->n_labels,
             "glims_observe: a cell carries label " + std::to_string(os.slot_label.empty() ? 0 : os.slot_label.back()) +
                 ", glims_set_materials has " + std::to_string(h->n_labels) + " labels");
  const int d = h->dim, no = d + 1;
  const int64_t n = h->n_nodes;
  const size_t per_src = (size_t)n_q * h->n_labels * no;
  std::vector<double> host((size_t)n_src * per_src, 0.0);
  int status = GLIMS_OK;
  if (h->n_cells > 0) {
    gl_ensure_cell_nodes(h);
    const int n_slots = (int)os.slot_label.size();
    // the grid and where the per-wave tables live depend on the labels of the mesh alone, not on the queries
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(GL_OBS_BLOCKS, grid_of(h->n_cells)),
                                                               GL_OBS_PART_CAP / ((int64_t)GL_OBS_WAVES * n_slots * 32)));
    const bool in_lds = (size_t)GL_OBS_WAVES * n_slots * GLIMS_OBSERVE_MAX_QUERIES * no * sizeof(double) <= GL_OBS_LDS_BYTES;
    os.part.alloc((size_t)nb * GL_OBS_WAVES * n_slots * n_q * no);
    os.res.alloc((size_t)n_src * per_src);
    GL_HIP(hipMemsetAsync(os.res.p, 0, (size_t)n_src * per_src * sizeof(double), h->st));
    // GLIMS_OBSERVE_TIMING: an event pair around each source's pass (cell pass + sum), one line per source on stderr
    const bool timed = getenv("GLIMS_OBSERVE_TIMING") != nullptr;
    for (int i = 0; i < n_src; ++i) {
      const int64_t s = src[i];
      const double *c = nullptr, *u = nullptr;
      if (s == GLIMS_DERIVE_HOST) {
        os.sc.alloc((size_t)n);
        gl_to_device_perm(h, c_host, os.sc.p, 1);
        c = os.sc.p;
        if (deformed) {
          os.su.alloc((size_t)n * d);
          gl_to_device_perm(h, u_host, os.su.p, d);
          u = os.su.p;
        }
      } else if (s == GLIMS_DERIVE_CURRENT) {
        c = h->c.p;
        u = h->U.p;
      } else {
        c = h->snapshots[(size_t)s]->p;
        if (deformed && h->derive.u_snapshot != s) {
          // as glims_snapshot_mechanics solves it; glims_derive and the deformed samplers of this snapshot find U in place
          h->derive.forget_u();
          const int st = gl_solve_mechanics(h, c);
          os.n_elastic_solves++;
          h->derive.n_elastic_solves++;
          if (st == GLIMS_OK) h->derive.u_snapshot = s;
          status = worse(status, st);
        }
        u = h->U.p;
      }
      if (!deformed) u = nullptr;
      if (timed) GL_HIP(hipEventRecord(h->ev_a, h->st));
      if (d == 2) launch_pass<2>(h, qs, c, u, scale, nb, in_lds, os.res.p + (size_t)i * per_src);
      else launch_pass<3>(h, qs, c, u, scale, nb, in_lds, os.res.p + (size_t)i * per_src);
      if (timed) {
        float ms = 0.f;
        GL_HIP(hipEventRecord(h->ev_b, h->st));
        GL_HIP(hipEventSynchronize(h->ev_b));
        GL_HIP(hipEventElapsedTime(&ms, h->ev_a, h->ev_b));
        fprintf(stderr, "glims observe: source %lld  pass %.4f ms\n", (long long)s, ms);
      }
      os.n_sources++;
    }
    GL_HIP(hipMemcpyAsync(host.data(), os.res.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
  }
  std::copy(host.begin(), host.end(), out);
  return status;
}

// ---- volume misfit terms: the stored list and its passes -------------------------------------------------------------------------
namespace {

// cells per label, read from the device once per handle
void ensure_label_cells(glims_ctx* h) {
  ObsTermState& os = h->obs_terms;
  if (!os.label_cells.empty()) return;
  std::vector<uint8_t> lab((size_t)h->n_cells);
  if (h->n_cells > 0) {
    GL_HIP(hipMemcpyAsync(lab.data(), h->label.p, lab.size(), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
  }
  os.label_cells.assign(GL_MAX_LABELS, 0);
  for (uint8_t l : lab) os.label_cells[l]++;
}

// The scratch of the passes, sized from the mesh for nt terms per pass (the largest batch of the stored list; second: with the
// planes of a Hessian direction).  Grow-only: a buffer that is large enough stays, one that is too small is released before the
// free memory is asked for, so that its bytes count; GLIMS_E_HIP with the figures when the new size does not fit.
// gl_observable_terms_set releases the planes whenever the list is replaced or cleared.
void ensure_term_scratch(glims_ctx* h, int nt, bool second, int64_t n_waves) {
  ObsTermState& os = h->obs_terms;
  const size_t plane = (size_t)nt * (h->dim + 1) * (size_t)h->n_cells;
  const size_t rows = (size_t)n_waves * GLIMS_OBSERVE_MAX_QUERIES;
  size_t need = 0;
  if (os.planes.n < plane) {
    os.planes.release();
    need += plane * sizeof(double);
  }
  if (second && os.planes2.n < plane) {
    os.planes2.release();
    need += plane * sizeof(double);
  }
  if (os.part.n < rows) need += rows * (sizeof(double) + sizeof(unsigned int));
  if (need) {
    size_t fr = 0, tot = 0;
    GL_HIP(hipMemGetInfo(&fr, &tot));
    if (need > fr)
      throw glims_error(GLIMS_E_HIP, "glims_adjoint_observable_terms: the vertex partials of " + std::to_string(nt) +
                                         " volume terms over " + std::to_string(h->n_cells) + " cells need about " +
                                         std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(fr >> 20) +
                                         " MiB are free");
  }
  if (os.planes.n < plane) os.planes.alloc(plane);
  if (second && os.planes2.n < plane) os.planes2.alloc(plane);
  if (os.part.n < rows) {
    os.part.alloc(rows);
    os.cut_part.alloc(rows);
  }
  os.vals.alloc((size_t)3 * GLIMS_OBSERVE_MAX_QUERIES);
  os.cuts.alloc((size_t)GLIMS_OBSERVE_MAX_QUERIES);
}

// The further scratch of a list with a deformed term, with the same refusal: b0 per term of a pass and cell (8 n_cells bytes per
// term) and the combined u-load (8 (dim+1) dim n_cells bytes per pass), the per-wave folded counts and ratios.  A list without
// such a term never comes here.
void ensure_def_scratch(glims_ctx* h, int nt, int64_t n_waves) {
  ObsTermState& os = h->obs_terms;
  const size_t b0n = (size_t)nt * (size_t)h->n_cells;
  const size_t ldn = (size_t)(h->dim + 1) * h->dim * (size_t)h->n_cells;
  const size_t rows = (size_t)n_waves * GLIMS_OBSERVE_MAX_QUERIES;
  size_t need = 0;
  if (os.b0_planes.n < b0n) {
    os.b0_planes.release();
    need += b0n * sizeof(double);
  }
  if (os.load_planes.n < ldn) {
    os.load_planes.release();
    need += ldn * sizeof(double);
  }
  if (os.fold_part.n < rows) need += rows * (sizeof(double) + sizeof(unsigned int));
  if (need) {
    size_t fr = 0, tot = 0;
    GL_HIP(hipMemGetInfo(&fr, &tot));
    if (need > fr)
      throw glims_error(GLIMS_E_HIP, "glims_adjoint_observable_terms2: the b0 planes of " + std::to_string(nt) +
                                         " deformed volume terms and the displacement load over " + std::to_string(h->n_cells) +
                                         " cells need about " + std::to_string(need >> 20) + " MiB of device memory, " +
                                         std::to_string(fr >> 20) + " MiB are free");
  }
  if (os.b0_planes.n < b0n) os.b0_planes.alloc(b0n);
  if (os.load_planes.n < ldn) os.load_planes.alloc(ldn);
  if (os.fold_part.n < rows) {
    os.fold_part.alloc(rows);
    os.ratio_part.alloc(rows);
  }
  os.folds.alloc((size_t)GLIMS_OBSERVE_MAX_QUERIES);
  os.ratios.alloc((size_t)GLIMS_OBSERVE_MAX_QUERIES);
}

// The scratch of a list with a centre-of-mass term, with the same refusal: the per-wave moment rows, and with a DEFORMED such term
// the planes sigma vol(y) b[1 + m] (8 (dim+1) n_cells bytes per term of a pass).  A list without such a term never comes here.
void ensure_mom_scratch(glims_ctx* h, int nt, int64_t n_waves, bool deformed) {
  ObsTermState& os = h->obs_terms;
  const size_t b1n = deformed ? (size_t)nt * (h->dim + 1) * (size_t)h->n_cells : 0;
  const size_t rows = (size_t)n_waves * GLIMS_OBSERVE_MAX_QUERIES * 4;
  size_t need = 0;
  if (os.b1_planes.n < b1n) {
    os.b1_planes.release();
    need += b1n * sizeof(double);
  }
  if (os.mom_part.n < rows) need += rows * sizeof(double);
  if (need) {
    size_t fr = 0, tot = 0;
    GL_HIP(hipMemGetInfo(&fr, &tot));
    if (need > fr)
      throw glims_error(GLIMS_E_HIP, "glims_adjoint_observable_terms3: the moment rows and the first-moment planes of " +
                                         std::to_string(nt) + " centre-of-mass terms over " + std::to_string(h->n_cells) +
                                         " cells need about " + std::to_string(need >> 20) + " MiB of device memory, " +
                                         std::to_string(fr >> 20) + " MiB are free");
  }
  if (os.b1_planes.n < b1n) os.b1_planes.alloc(b1n);
  if (os.mom_part.n < rows) os.mom_part.alloc(rows);
  os.mom_vals.alloc((size_t)GLIMS_OBSERVE_MAX_QUERIES * GL_OBS_MOM);
}

template <int D>
void observable_batch(glims_ctx* h, const std::vector<int>& batch, int nt_alloc, const double* c, double* g, double* J, int P,
                      const double* dc, int64_t ld, double* dg, int step, const double* uk, double* murhs) {
  ObsTermState& os = h->obs_terms;
  constexpr int NV = D + 1, MQ = GLIMS_OBSERVE_MAX_QUERIES;
  const int nt = (int)batch.size();
  ObsGradTerms ts;
  ts.n = nt;
  for (int q = 0; q < MQ; ++q) {
    ts.kind[q] = GLIMS_OBSERVE_MASS;
    ts.level[q] = ts.weight[q] = ts.target[q] = 0.0;
    ts.smooth[q] = 1.0;
    ts.deformed[q] = 0;
    ts.scale[q] = 0.0;
    for (int w = 0; w < GL_MAX_LABELS / 64; ++w) ts.mask[q][w] = 0ull;
    ts.moment[q] = 0;
    for (int a = 0; a < 3; ++a) ts.target_x[q][a] = 0.0;
  }
  bool any_def = false, any_com = false;
  for (int q = 0; q < nt; ++q) {
    const GlObservableTerm& t = os.terms[(size_t)batch[(size_t)q]];
    ts.deformed[q] = t.deformed;
    ts.scale[q] = t.deformed ? t.scale : 0.0;
    any_def = any_def || t.deformed;
    ts.kind[q] = t.kind;
    ts.level[q] = t.level;
    ts.smooth[q] = t.kind == GLIMS_OBSERVE_SMOOTH ? t.smooth : 1.0;
    ts.weight[q] = t.weight;
    ts.target[q] = t.target;
    ts.moment[q] = t.moment;
    any_com = any_com || t.moment;
    for (int a = 0; a < 3; ++a) ts.target_x[q][a] = t.target_x[a];
    for (int l = 0; l < GL_MAX_LABELS; ++l)
      if (t.mask.empty() || (l < (int)t.mask.size() && t.mask[(size_t)l])) ts.mask[q][l >> 6] |= 1ull << (l & 63);
  }
  if (any_def && !(uk && murhs)) throw std::logic_error("observable_batch: a deformed volume term without u_k");
  if (any_com && P > 0) throw std::logic_error("observable_batch: second order with a centre-of-mass term");
  double vals[2 * MQ] = {0.0}, ratios[MQ], moms[MQ * GL_OBS_MOM] = {0.0};
  long long cuts[MQ] = {0}, folds[MQ] = {0};
  for (int q = 0; q < MQ; ++q) {
    ratios[q] = INFINITY;
    moms[q * GL_OBS_MOM + GL_OBS_MOM_EMPTY] = 1.0;   // (a mesh without cells: every measure is empty)
  }
  if (h->n_cells > 0) {
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(GL_OBS_BLOCKS, grid_of(h->n_cells)));
    const int64_t n_waves = (int64_t)nb * GL_OBS_WAVES;
    ensure_term_scratch(h, nt_alloc, P > 0, n_waves);
    if (gl_observable_terms_any_deformed(h)) ensure_def_scratch(h, nt_alloc, n_waves);   // (from the list: no step reallocates)
    bool list_com = false, list_def_com = false;
    for (const GlObservableTerm& t : os.terms) {
      list_com = list_com || t.moment;
      list_def_com = list_def_com || (t.moment && t.deformed);
    }
    if (list_com) ensure_mom_scratch(h, nt_alloc, n_waves, list_def_com);
    const int32_t* cn = gl_ensure_cell_nodes(h);
    // GLIMS_OBSERVABLE_TIMING: an event pair around the cell pass (with its sum) and one around the gather, one line per batch
    const bool timed = getenv("GLIMS_OBSERVABLE_TIMING") != nullptr;
    float ms_cells = 0.f, ms_rows = 0.f, ms_load = 0.f, ms_urows = 0.f, ms_mom = 0.f;
    auto tick = [&]() {
      if (timed) GL_HIP(hipEventRecord(h->ev_a, h->st));
    };
    auto tock = [&](float* ms) {
      if (!timed) return;
      GL_HIP(hipEventRecord(h->ev_b, h->st));
      GL_HIP(hipEventSynchronize(h->ev_b));
      GL_HIP(hipEventElapsedTime(ms, h->ev_a, h->ev_b));
    };
    const double* mom = any_com ? os.mom_vals.p : nullptr;
    if (any_com) {
      // the quotient needs V and M before any partial can be weighted: the moments pass and its sum leave them on the device
      tick();
      if (any_def)
        hipLaunchKernelGGL((k_observe_mom_cells<D, 1>), dim3(nb), dim3(256), 0, h->st, h->n_cells, cn, h->label.p, h->evol.p, c,
                           ts, h->xyz_new.p, uk, os.mom_part.p);
      else
        hipLaunchKernelGGL((k_observe_mom_cells<D, 0>), dim3(nb), dim3(256), 0, h->st, h->n_cells, cn, h->label.p, h->evol.p, c,
                           ts, h->xyz_new.p, (const double*)nullptr, os.mom_part.p);
      GL_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_observe_mom_sum, dim3(nt), dim3(256), 0, h->st, n_waves, D, os.mom_part.p, ts, os.mom_vals.p);
      GL_CHECK_LAUNCH();
      tock(&ms_mom);
      os.n_mom_passes++;
    }
    tick();
    if (any_def) {
      if (any_com)
        hipLaunchKernelGGL((k_observe_grad_cells<D, 1, 1>), dim3(nb), dim3(256), 0, h->st, h->n_cells, cn, h->label.p, h->evol.p,
                           c, ts, os.planes.p, os.part.p, os.cut_part.p, h->xyz_new.p, uk, os.b0_planes.p, os.fold_part.p,
                           os.ratio_part.p, mom, os.b1_planes.p);
      else
        hipLaunchKernelGGL((k_observe_grad_cells<D, 1, 0>), dim3(nb), dim3(256), 0, h->st, h->n_cells, cn, h->label.p, h->evol.p,
                           c, ts, os.planes.p, os.part.p, os.cut_part.p, h->xyz_new.p, uk, os.b0_planes.p, os.fold_part.p,
                           os.ratio_part.p, (const double*)nullptr, (double*)nullptr);
      os.n_def_passes++;
    } else if (any_com) {
      hipLaunchKernelGGL((k_observe_grad_cells<D, 0, 1>), dim3(nb), dim3(256), 0, h->st, h->n_cells, cn, h->label.p, h->evol.p, c,
                         ts, os.planes.p, os.part.p, os.cut_part.p, h->xyz_new.p, (const double*)nullptr, (double*)nullptr,
                         (unsigned int*)nullptr, (double*)nullptr, mom, (double*)nullptr);
    } else {
      hipLaunchKernelGGL((k_observe_grad_cells<D, 0, 0>), dim3(nb), dim3(256), 0, h->st, h->n_cells, cn, h->label.p, h->evol.p, c,
                         ts, os.planes.p, os.part.p, os.cut_part.p, (const double*)nullptr, (const double*)nullptr,
                         (double*)nullptr, (unsigned int*)nullptr, (double*)nullptr, (const double*)nullptr, (double*)nullptr);
    }
    GL_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_observe_grad_sum, dim3(nt), dim3(256), 0, h->st, n_waves, os.part.p, os.cut_part.p, ts, 0, os.vals.p,
                       os.cuts.p, mom);
    GL_CHECK_LAUNCH();
    tock(&ms_cells);
    tick();
    hipLaunchKernelGGL((k_observe_grad_rows<NV, 1>), dim3(grid_of(h->n_own)), dim3(256), 0, h->st, h->n_own, h->n_cells,
                       h->pat.cslice_ptr.p, h->pat.celem.p, cn, nt, os.planes.p, os.vals.p + MQ, (const double*)nullptr,
                       (const double*)nullptr, g);
    GL_CHECK_LAUNCH();
    tock(&ms_rows);
    os.n_cell_passes++;
    os.n_gathers++;
    if (timed)
      fprintf(stderr, "glims observable terms: step %d  terms %d  cells %.4f ms  gather %.4f ms\n", step, nt, ms_cells, ms_rows);
    if (timed && any_com) fprintf(stderr, "glims observable terms: step %d  moments pass %.4f ms\n", step, ms_mom);
    if (any_def) {
      // dJ/du_k of the batch's deformed terms: the combined cofactor planes (the coefficients are on the device), then their
      // row-owned gather into murhs; the folded counts and smallest ratios of the cell pass
      tick();
      if (any_com)
        hipLaunchKernelGGL((k_observe_def_load_cells<D, 1>), dim3(grid_of(h->n_cells)), dim3(256), 0, h->st, h->n_cells, cn,
                           h->xyz_new.p, uk, ts, os.b0_planes.p, os.vals.p + MQ, os.load_planes.p, os.b1_planes.p, mom);
      else
        hipLaunchKernelGGL((k_observe_def_load_cells<D, 0>), dim3(grid_of(h->n_cells)), dim3(256), 0, h->st, h->n_cells, cn,
                           h->xyz_new.p, uk, ts, os.b0_planes.p, os.vals.p + MQ, os.load_planes.p, (const double*)nullptr,
                           (const double*)nullptr);
      GL_CHECK_LAUNCH();
      tock(&ms_load);
      tick();
      hipLaunchKernelGGL((k_observe_grad_rows<NV, D>), dim3(grid_of(h->n_own)), dim3(256), 0, h->st, h->n_own, h->n_cells,
                         h->pat.cslice_ptr.p, h->pat.celem.p, cn, 1, os.load_planes.p, (const double*)nullptr,
                         (const double*)nullptr, (const double*)nullptr, murhs);
      GL_CHECK_LAUNCH();
      tock(&ms_urows);
      hipLaunchKernelGGL(k_observe_def_sum, dim3(nt), dim3(256), 0, h->st, n_waves, os.fold_part.p, os.ratio_part.p,
                         os.folds.p, os.ratios.p);
      GL_CHECK_LAUNCH();
      GL_HIP(hipMemcpyAsync(folds, os.folds.p, sizeof(folds), hipMemcpyDeviceToHost, h->st));
      GL_HIP(hipMemcpyAsync(ratios, os.ratios.p, sizeof(ratios), hipMemcpyDeviceToHost, h->st));
      if (timed)
        fprintf(stderr, "glims observable terms: step %d  deformed pass  load %.4f ms  u-gather %.4f ms\n", step, ms_load,
                ms_urows);
    }
    for (int p = 0; p < P; ++p) {
      // dg_p += sum_t (weight_t (g_t^T dc_p) G_t + weight_t (V_t - target_t) H_t dc_p)
      hipLaunchKernelGGL(k_observe_second_cells<D>, dim3(nb), dim3(256), 0, h->st, h->n_cells, cn, h->label.p, h->evol.p, c,
                         dc + (size_t)p * ld, ts, os.planes.p, os.planes2.p, os.part.p);
      GL_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_observe_grad_sum, dim3(nt), dim3(256), 0, h->st, n_waves, os.part.p, os.cut_part.p, ts, 1, os.vals.p,
                         os.cuts.p, (const double*)nullptr);
      GL_CHECK_LAUNCH();
      hipLaunchKernelGGL((k_observe_grad_rows<NV, 1>), dim3(grid_of(h->n_own)), dim3(256), 0, h->st, h->n_own, h->n_cells,
                         h->pat.cslice_ptr.p, h->pat.celem.p, cn, nt, os.planes.p, os.vals.p + 2 * MQ, os.planes2.p,
                         os.vals.p + MQ, dg + (size_t)p * ld);
      GL_CHECK_LAUNCH();
      os.n_cell_passes++;
      os.n_gathers++;
    }
    GL_HIP(hipMemcpyAsync(vals, os.vals.p, sizeof(vals), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipMemcpyAsync(cuts, os.cuts.p, sizeof(cuts), hipMemcpyDeviceToHost, h->st));
    if (any_com) GL_HIP(hipMemcpyAsync(moms, os.mom_vals.p, sizeof(moms), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
  }
  for (int q = 0; q < nt; ++q) {
    GlObservableTerm& t = os.terms[(size_t)batch[(size_t)q]];
    t.V = vals[q];
    t.n_cut = t.kind == GLIMS_OBSERVE_SHARP ? (int64_t)cuts[q] : -1;
    if (t.deformed) {
      t.n_folded = (int64_t)folds[q];
      t.min_ratio = std::isfinite(ratios[q]) ? ratios[q] : NAN;   // (no counted cell: nothing to take the minimum of)
    }
    if (t.moment) {
      const double* mv = moms + q * GL_OBS_MOM;
      t.V = mv[0];
      t.empty = mv[GL_OBS_MOM_EMPTY] != 0.0 ? 1 : 0;
      for (int a = 0; a < 3; ++a) t.com[a] = !t.empty && a < D ? mv[GL_OBS_MOM_X + a] : NAN;
      *J += mv[GL_OBS_MOM_J];
      continue;
    }
    const double r = t.V - t.target;
    *J += 0.5 * t.weight * (r * r);
  }
}

}  // namespace

void gl_observable_terms_set(glims_ctx* h, int n, const glims_observable_misfit* terms1,
                             const glims_observable_misfit2* terms2, const glims_observable_misfit3* terms3) {
  const std::string who = terms3   ? "glims_adjoint_observable_terms3"
                          : terms2 ? "glims_adjoint_observable_terms2"
                                   : "glims_adjoint_observable_terms";
  ObsTermState& os = h->obs_terms;
  GL_REQUIRE(n >= 0 && (n == 0 || terms1 || terms2 || terms3), who + ": bad term list");
  auto drop_planes = [&os]() {
    os.planes.release();
    os.planes2.release();
    os.b0_planes.release();
    os.load_planes.release();
    os.b1_planes.release();
  };
  if (n == 0) {   // clearing is always possible; the planes go with the list
    os.terms.clear();
    drop_planes();
    return;
  }
  // one internal form for the entry points: the first struct is a term of the reference configuration, the first two are
  // volume terms
  std::vector<glims_observable_misfit3> terms((size_t)n);
  for (int k = 0; k < n; ++k) {
    if (terms3) {
      terms[(size_t)k] = terms3[k];
    } else if (terms2) {
      const glims_observable_misfit2& t = terms2[k];
      terms[(size_t)k] = {t.step, t.kind, t.level, t.smooth, t.weight, t.target, t.labels, t.deformed, t.scale, 0,
                          {0.0, 0.0, 0.0}};
    } else {
      const glims_observable_misfit& t = terms1[k];
      terms[(size_t)k] = {t.step, t.kind, t.level, t.smooth, t.weight, t.target, t.labels, 0, 1.0, 0, {0.0, 0.0, 0.0}};
    }
  }
  GL_REQUIRE(h->world <= 1, who + ": not available on a partitioned handle (world > 1)");
  GL_REQUIRE(h->is_setup, who + " before glims_setup");
  GL_REQUIRE(h->n_labels > 0, who + " before glims_set_materials");
  for (int k = 0; k < n; ++k) {
    const glims_observable_misfit3& t = terms[(size_t)k];
    const std::string tk = " of term " + std::to_string(k);
    GL_REQUIRE(t.step >= 0, who + ": negative step" + tk);
    GL_REQUIRE(t.kind >= GLIMS_OBSERVE_MASS && t.kind <= GLIMS_OBSERVE_SMOOTH,
               who + ": unknown kind " + std::to_string(t.kind) + tk);
    GL_REQUIRE(std::isfinite(t.level), who + ": level" + tk + " is not finite");
    GL_REQUIRE(t.kind != GLIMS_OBSERVE_SMOOTH || t.smooth > 0.0, who + ": smooth" + tk + " must be positive");
    GL_REQUIRE(std::isfinite(t.weight), who + ": weight" + tk + " is not finite");
    GL_REQUIRE(t.moment >= 0 && t.moment <= 1, who + ": moment " + std::to_string(t.moment) + tk + " outside 0..1");
    if (t.moment) {
      for (int a = 0; a < h->dim; ++a)
        GL_REQUIRE(std::isfinite(t.target_x[a]), who + ": target_x[" + std::to_string(a) + "]" + tk + " is not finite");
    } else {
      GL_REQUIRE(std::isfinite(t.target), who + ": target" + tk + " is not finite");
    }
    GL_REQUIRE(!t.deformed || (h->have_mech && h->U.p),
               who + ": term " + std::to_string(k) + " is deformed: the deformed configuration needs the displacement, "
                     "glims_setup(with_mechanics=1) first");
    GL_REQUIRE(!t.deformed || std::isfinite(t.scale), who + ": scale" + tk + " is not finite");
  }
  ensure_label_cells(h);
  std::vector<GlObservableTerm> fresh((size_t)n);
  for (int k = 0; k < n; ++k) {
    const glims_observable_misfit3& t = terms[(size_t)k];
    GlObservableTerm& f = fresh[(size_t)k];
    f.moment = t.moment;
    for (int a = 0; a < h->dim; ++a) f.target_x[a] = t.moment ? t.target_x[a] : 0.0;
    f.deformed = t.deformed ? 1 : 0;
    f.scale = t.deformed ? t.scale : 1.0;
    f.step = t.step;
    f.kind = t.kind;
    f.level = t.level;
    f.smooth = t.kind == GLIMS_OBSERVE_SMOOTH ? t.smooth : 1.0;
    f.weight = t.weight;
    f.target = t.moment ? 0.0 : t.target;
    if (t.labels) {
      f.mask.assign(t.labels, t.labels + h->n_labels);
      for (int l = 0; l < h->n_labels; ++l)
        if (f.mask[(size_t)l]) f.n_counted += os.label_cells[(size_t)l];
    } else {
      f.n_counted = h->n_cells;
    }
  }
  os.terms.swap(fresh);
  // (the next call sizes the planes for the largest batch of THIS list)
  drop_planes();
}

void gl_observable_term_info2(glims_ctx* h, int k, int64_t out[4], double* V, double* min_ratio) {
  const ObsTermState& os = h->obs_terms;
  GL_REQUIRE(out && V && min_ratio, "glims_adjoint_observable_info2: null output");
  GL_REQUIRE(k >= 0 && k < (int)os.terms.size(), "glims_adjoint_observable_info2: no stored term " + std::to_string(k));
  const GlObservableTerm& t = os.terms[(size_t)k];
  out[0] = t.n_counted;
  out[1] = t.n_cut;
  out[2] = t.deformed ? t.n_folded : -1;
  out[3] = 0;
  *V = t.V;
  *min_ratio = t.deformed ? t.min_ratio : NAN;
}

void gl_observable_term_info3(glims_ctx* h, int k, int64_t out[4], double* V, double* min_ratio, double com[3]) {
  const ObsTermState& os = h->obs_terms;
  GL_REQUIRE(out && V && min_ratio && com, "glims_adjoint_observable_info3: null output");
  GL_REQUIRE(k >= 0 && k < (int)os.terms.size(), "glims_adjoint_observable_info3: no stored term " + std::to_string(k));
  gl_observable_term_info2(h, k, out, V, min_ratio);
  const GlObservableTerm& t = os.terms[(size_t)k];
  out[3] = t.moment && t.empty ? 1 : 0;
  for (int a = 0; a < 3; ++a) com[a] = t.moment && a < h->dim ? t.com[a] : NAN;
}

bool gl_observable_terms_any_deformed(const glims_ctx* h) {
  for (const GlObservableTerm& t : h->obs_terms.terms)
    if (t.deformed) return true;
  return false;
}

bool gl_observable_terms_need_u(const glims_ctx* h, int step) {
  for (const GlObservableTerm& t : h->obs_terms.terms)
    if (t.deformed && t.step == step) return true;
  return false;
}

void gl_observable_term_info(glims_ctx* h, int k, int64_t out[2], double* V) {
  const ObsTermState& os = h->obs_terms;
  GL_REQUIRE(out && V, "glims_adjoint_observable_info: null output");
  GL_REQUIRE(k >= 0 && k < (int)os.terms.size(), "glims_adjoint_observable_info: no stored term " + std::to_string(k));
  const GlObservableTerm& t = os.terms[(size_t)k];
  out[0] = t.n_counted;
  out[1] = t.n_cut;
  *V = t.V;
}

void gl_observable_terms_check(glims_ctx* h, int64_t N, const std::string& who, bool second_order) {
  const ObsTermState& os = h->obs_terms;
  for (size_t k = 0; k < os.terms.size(); ++k) {
    const GlObservableTerm& t = os.terms[k];
    GL_REQUIRE(t.step <= N, who + ": stored volume term " + std::to_string(k) + " observes step " + std::to_string(t.step) +
                                ", the recording has steps 0.." + std::to_string(N));
    GL_REQUIRE(t.mask.empty() || (int)t.mask.size() == h->n_labels,
               who + ": the label mask of stored volume term " + std::to_string(k) + " has " + std::to_string(t.mask.size()) +
                   " entries, glims_set_materials now has " + std::to_string(h->n_labels) + " labels");
    GL_REQUIRE(!second_order || t.kind != GLIMS_OBSERVE_SHARP,
               who + ": stored volume term " + std::to_string(k) + " is SHARP: its measure is piecewise smooth, with jumps in "
                     "the second derivative where the level set crosses a vertex; second order is built for MASS and SMOOTH");
    GL_REQUIRE(!t.deformed || h->have_mech,
               who + ": stored volume term " + std::to_string(k) + " is deformed: it needs glims_setup(with_mechanics=1)");
    GL_REQUIRE(!second_order || !t.moment,
               who + ": stored term " + std::to_string(k) + " is a centre-of-mass term: second order of the quotient M / V is "
                     "not built; clear the list with glims_adjoint_observable_terms3(h, 0, NULL) or store volume terms first");
    GL_REQUIRE(!second_order || !t.deformed,
               who + ": stored volume term " + std::to_string(k) + " is deformed: second order through the displacement is "
                     "not built (a Hessian without it would be wrong); clear the list with "
                     "glims_adjoint_observable_terms2(h, 0, NULL) or store reference-configuration terms first");
  }
}

void gl_observable_terms_of_step(glims_ctx* h, int step, const double* c, double* g, double* J, int P, const double* dc,
                                 int64_t ld, double* dg, const double* uk, double* murhs) {
  ObsTermState& os = h->obs_terms;
  std::vector<int> here;
  for (size_t k = 0; k < os.terms.size(); ++k)
    if (os.terms[k].step == step) here.push_back((int)k);
  if (here.empty()) return;
  // the planes serve the largest batch of the whole list: no step of this or a later call reallocates them
  std::vector<int> per_step;
  for (const GlObservableTerm& t : os.terms) {
    if ((size_t)t.step >= per_step.size()) per_step.resize((size_t)t.step + 1, 0);
    per_step[(size_t)t.step]++;
  }
  const int nt_alloc = std::min(GLIMS_OBSERVE_MAX_QUERIES, *std::max_element(per_step.begin(), per_step.end()));
  for (size_t b = 0; b < here.size(); b += GLIMS_OBSERVE_MAX_QUERIES) {
    const std::vector<int> batch(here.begin() + (long)b,
                                 here.begin() + (long)std::min(here.size(), b + GLIMS_OBSERVE_MAX_QUERIES));
    if (h->dim == 2) observable_batch<2>(h, batch, nt_alloc, c, g, J, P, dc, ld, dg, step, uk, murhs);
    else observable_batch<3>(h, batch, nt_alloc, c, g, J, P, dc, ld, dg, step, uk, murhs);
  }
}
