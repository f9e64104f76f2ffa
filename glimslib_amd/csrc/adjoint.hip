// Discrete adjoint of the backward-Euler / Newton scheme of gl_step: trajectory recording, the misfit
// terms, the parameter-sensitivity pass, the coupling adjoint G^T mu and the backward sweep.  Single GPU or partitioned
// (world > 1: every rank sweeps its sub-mesh, the adjoint vectors exchange their ghosts before every operator use, each
// cell enters the per-label sums on one rank only, and those sums are added over the ranks in rank order).
//
// Step n solves R_n = S c_n + dt N(c_n) c_n - M c_{n-1} - f_n = 0 (c_n fixed on the Dirichlet nodes).  Backwards from the last
// recorded step N:  mu_n = K_el^-1 dJ/du_n (observed displacement terms only),  g_n = dJ/dc_n + G^T mu_n,
// A(c_n) lambda_n = g_n + M lambda_{n+1} (masked: lambda = 0 on the constrained nodes), and per label t
//   dJ/dD_t = -dt sum_n int_t grad lambda_n . grad c_n,   dJ/drho_t = -dt sum_n int_t lambda_n (c_n^2 - c_n),
//   dJ/dgamma_t = sum_k mu_k^T G_t c_k,                   dJ/dc_0 = M lambda_1 + dJ/dc_0 (explicit),
//   dJ/dp_t = sum_k mu_k^T (dG/dp c_k - dK/dp u_k)  for p = E_t, nu_t  (u_k with its Dirichlet values).  K and G are linear
//   in the cell's Lame pair: A_t = sum int_t eps(mu):eps(u), B_t = sum int_t div mu div u and
//   C_t = dJ/dgamma_t / (2 mu_t + d lam_t) give dJ/dp_t = gamma_t (2 mu' + d lam') C_t - (2 mu' A_t + lam' B_t).
// (carrying capacity 1, as in the forward kernels: the reaction weights of k_corner_weights are rho |T| d!/(d+3)!.)
#include "glims_internal.h"
#include "diffusion_tensor.h"
#include "hessian_plan.h"
#include "lame_derivs.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include <omp.h>

namespace {

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Fixed-order epilogue of a 256-thread block that holds N per-thread sums: every wave's butterfly, then the block's four wave
// sums as (w0 + w1) + (w2 + w3), one store per sum into part[block][N].  No atomics: the partials are bitwise reproducible.
template <int N>
__device__ __forceinline__ void block_partials(double (&v)[N], double* __restrict__ part) {
  __shared__ double sm[4][N];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double t = wsum(v[k]);
    if (lane == 0) sm[wid][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    part[(size_t)blockIdx.x * N + k] = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
  }
}

// internal node of every cell vertex, from the row-owned incidence lists: the row whose diagonal slot is vertex m of cell e
template <int NV>
__global__ void k_cell_nodes(int64_t n_own, const int64_t* __restrict__ cslice_ptr, const uint32_t* __restrict__ cslots,
                             const int32_t* __restrict__ celem, const uint8_t* __restrict__ diag_k,
                             int32_t* __restrict__ cell_nodes) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  const uint32_t dk = diag_k[row];
  for (int q = 0; q < clen; ++q) {
    const int64_t ci = cbase + (int64_t)q * GL_WAVE + lane;
    const int32_t e = celem[ci];
    if (e < 0) continue;
    const uint32_t sl = cslots[ci];
#pragma unroll
    for (int m = 0; m < NV; ++m)
      if (((sl >> (8 * m)) & 255u) == dk) cell_nodes[(int64_t)e * NV + m] = (int32_t)row;
  }
}

// The same map on a partitioned handle: the rank holds every cell that touches an owned node, and the vertices of such a cell
// that are ghosts have no owned row of their own.  Every owned row writes ALL vertices of its cells from its own column list
// (the slot of vertex m is a column of the row); rows that share a cell write the same values.  seen[e] = 1 for every cell that
// some owned row lists.
template <int NV>
__global__ void k_cell_nodes_all(int64_t n_own, const int64_t* __restrict__ slice_ptr, const int32_t* __restrict__ cols,
                                 const int64_t* __restrict__ cslice_ptr, const uint32_t* __restrict__ cslots,
                                 const int32_t* __restrict__ celem, int32_t* __restrict__ cell_nodes,
                                 uint8_t* __restrict__ seen) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t base = slice_ptr[s];
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  for (int q = 0; q < clen; ++q) {
    const int64_t ci = cbase + (int64_t)q * GL_WAVE + lane;
    const int32_t e = celem[ci];
    if (e < 0) continue;
    const uint32_t sl = cslots[ci];
#pragma unroll
    for (int m = 0; m < NV; ++m)
      cell_nodes[(int64_t)e * NV + m] = cols[base + (int64_t)((sl >> (8 * m)) & 255u) * GL_WAVE + lane];
    seen[e] = 1;
  }
}

// Counting rule of the per-label sums on a partitioned handle: a cell is counted by the smallest rank that owns one of its
// vertices (that rank holds the cell).  owner of a local node: `rank` for the owned ones, ghost_owner[i - n_own] for the ghosts.
// In place: counted[e] holds `seen` on entry.
template <int NV>
__global__ void k_cell_counted(int64_t n_cells, int64_t n_own, int rank, const int32_t* __restrict__ ghost_owner,
                               const int32_t* __restrict__ cell_nodes, uint8_t* __restrict__ counted) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_cells) return;
  if (!counted[e]) return;   // listed by no owned row: not this rank's cell
  int lo = rank;
#pragma unroll
  for (int m = 0; m < NV; ++m) {
    const int64_t v = cell_nodes[e * NV + m];
    if (v >= n_own) lo = min(lo, ghost_owner[v - n_own]);
  }
  counted[e] = lo == rank ? 1 : 0;
}

// Parameter-sensitivity pass, one thread per cell (grid-stride over a FIXED grid), labels [l0, l0 + LT) per launch.
//   MODE 0 (c, lambda):  q0 = int_T grad lambda . grad c,  q1 = int_T lambda (c^2 - c)            (exact for P1)
//   MODE 1 (c, mu):      q2 = mu^T G_T c with gamma = 1 = (2 mu_T + d lam_T) |T| / (d+1) div mu_h (sum_a c_a);
//                        qcell[e] = gamma_T (2 mu_T + d lam_T) |T| / (d+1) div mu_h  (the cell's share of G^T mu)
//   MODE 2 (u, mu):      q0 = int_T eps(mu_h):eps(u_h),  q1 = int_T div mu_h div u_h  (both block size d; c is u here)
// counted (partitioned handles, else nullptr): cells with counted[e] = 0 stay out of the per-label sums (MODE 1 still writes
// their qcell: the owned rows of the cell need its share of G^T mu).
// Per-block partials [block][LT][3] in a fixed order (waves, then the block's four wave sums), no atomics: the sums are
// bitwise reproducible.  Bytes per cell: the geometry record (1 + NV D) x 8 (56 B in 2-D, 104 B in 3-D), NV x 4 B of vertex ids,
// 1 B of label (+ 8 B of qcell in MODE 1); the gathered vectors (2 x 8 B per node, mu: 8 d B; MODE 2: u and mu, 2 x 8 d B)
// mostly hit the caches.
// ANISO (MODE 0 alone): q0 = int_T grad lambda^T TT_T grad c with the cell's tensor dten[e] (diffusion_tensor.h), + 8 d (d + 1) / 2
// B per cell; ANISO = 0 is the kernel as it was: DT is empty there (the signature and kernel-argument layout of before), one
// `const double*` with ANISO.
template <int D, int MODE, int ANISO = 0, class... DT>
__global__ __launch_bounds__(256) void k_sens(int64_t n_cells, int l0, const int32_t* __restrict__ cell_nodes,
                                              const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                              const double* __restrict__ mat, const double* __restrict__ c,
                                              const double* __restrict__ v, const uint8_t* __restrict__ counted,
                                              double* __restrict__ qcell, double* __restrict__ partials, DT... dten) {
  static_assert(sizeof...(DT) == (ANISO ? 1 : 0), "the tensor field is passed with ANISO alone");
  constexpr int NV = D + 1, GE = 1 + NV * D;
  constexpr double f3 = D == 2 ? 1.0 / 60.0 : 1.0 / 120.0;   // d! / (d+3)!
  constexpr double f2 = D == 2 ? 1.0 / 12.0 : 1.0 / 20.0;    // d! / (d+2)!
  double acc[GL_ADJ_LT][2];
#pragma unroll
  for (int j = 0; j < GL_ADJ_LT; ++j) acc[j][0] = acc[j][1] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_cells; e += stride) {
    const int lab = label[e];
    const int j = lab - l0;
    if (MODE != 1 && (j < 0 || j >= GL_ADJ_LT || (counted && !counted[e]))) continue;
    const double* g = egeo + e * GE;
    const double vol = g[0];
    int nd[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) nd[m] = cell_nodes[e * NV + m];
    double a0 = 0.0, a1 = 0.0;
    if (MODE == 2) {
      // grad w_h [a][b] = d_a w_b = sum_m w_{m,b} dphi_m/dx_a
      double gm[D][D] = {}, gu[D][D] = {};
#pragma unroll
      for (int m = 0; m < NV; ++m)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          const double vm = v[(int64_t)nd[m] * D + b], um = c[(int64_t)nd[m] * D + b];
#pragma unroll
          for (int a = 0; a < D; ++a) {
            gm[a][b] += vm * g[1 + m * D + a];
            gu[a][b] += um * g[1 + m * D + a];
          }
        }
      double ee = 0.0, dm = 0.0, du = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        dm += gm[a][a];
        du += gu[a][a];
#pragma unroll
        for (int b = 0; b < D; ++b) ee += 0.25 * (gm[a][b] + gm[b][a]) * (gu[a][b] + gu[b][a]);
      }
      a0 = vol * ee;
      a1 = vol * dm * du;
    } else {
      double cv[NV];
#pragma unroll
      for (int m = 0; m < NV; ++m) cv[m] = c[nd[m]];
      if (MODE == 0) {
        double lv[NV], gc[D] = {0.0}, gl[D] = {0.0};
#pragma unroll
        for (int m = 0; m < NV; ++m) lv[m] = v[nd[m]];
        double Sl = 0.0, Sc = 0.0, lc = 0.0, cc = 0.0, lcc = 0.0;
#pragma unroll
        for (int m = 0; m < NV; ++m) {
#pragma unroll
          for (int a = 0; a < D; ++a) {
            gc[a] += cv[m] * g[1 + m * D + a];
            gl[a] += lv[m] * g[1 + m * D + a];
          }
          Sl += lv[m];
          Sc += cv[m];
          lc += lv[m] * cv[m];
          cc += cv[m] * cv[m];
          lcc += lv[m] * cv[m] * cv[m];
        }
        double gg = 0.0;
        if constexpr (ANISO != 0) {
          gg = glims_dt_form<D>(glims_dt_field(dten...) + e * glims_dt_size<D>(), gl, gc);
        } else {
#pragma unroll
          for (int a = 0; a < D; ++a) gg += gl[a] * gc[a];
        }
        a0 = vol * gg;
        // sum_{abc} l_a c_b c_c prod(alpha!) = Sl Sc^2 + 2 Sc (l.c) + Sl (c.c) + 2 sum l_a c_a^2;
        // sum_{ab} l_a c_b (1 + delta_ab)
        a1 = vol * (f3 * (Sl * Sc * Sc + 2.0 * Sc * lc + Sl * cc + 2.0 * lcc) - f2 * (Sl * Sc + lc));
      } else {
        double div = 0.0, Sc = 0.0;
#pragma unroll
        for (int m = 0; m < NV; ++m) {
          Sc += cv[m];
#pragma unroll
          for (int a = 0; a < D; ++a) div += v[(int64_t)nd[m] * D + a] * g[1 + m * D + a];
        }
        const double mu = mat[3 * GL_MAX_LABELS + lab], lam = mat[4 * GL_MAX_LABELS + lab];
        const double w = (2.0 * mu + D * lam) * vol * (1.0 / (D + 1)) * div;
        if (l0 == 0) qcell[e] = mat[2 * GL_MAX_LABELS + lab] * w;
        if (counted && !counted[e]) continue;
        a0 = w * Sc;
      }
    }
#pragma unroll
    for (int q = 0; q < GL_ADJ_LT; ++q)
      if (q == j) {
        acc[q][0] += a0;
        acc[q][1] += a1;
      }
  }
  // block_partials, written out: through the call MODE 1 loses the folding of its eight zero sums (acc[q][1]) and takes
  // 16 / 18 more VGPRs in 2-D / 3-D
  __shared__ double sm[4][GL_ADJ_LT * 2];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < GL_ADJ_LT; ++q)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double t = wsum(acc[q][k]);
      if (lane == 0) sm[wid][q * 2 + k] = t;
    }
  __syncthreads();
  if (threadIdx.x < GL_ADJ_LT * 2) {
    const int t = threadIdx.x;
    partials[(size_t)blockIdx.x * GL_ADJ_LT * 2 + t] = (sm[0][t] + sm[1][t]) + (sm[2][t] + sm[3][t]);
  }
}

// second stage, fixed order over the blocks: sums[(l0 + q) * ls + k_off + k] += sum_b partials[b][q][k] (ls sums per label).
// One wave per sum (16 waves): lane l adds blocks l, l + 64, ... in order, then the wave's butterfly -- the same order on every
// call
__global__ __launch_bounds__(1024) void k_sens_final(int n_blocks, int l0, int n_labels, int ls, int k_off,
                                                     const double* __restrict__ partials, double* __restrict__ sums) {
  const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (t >= GL_ADJ_LT * 2) return;
  double s = 0.0;
  for (int b = lane; b < n_blocks; b += 64) s += partials[(size_t)b * GL_ADJ_LT * 2 + t];
  s = wsum(s);
  const int q = t / 2, k = t % 2;
  if (lane == 0 && l0 + q < n_labels && k_off + k < ls) sums[(l0 + q) * ls + k_off + k] += s;
}

// Tangent-field sensitivities (glims_set_diffusion_tensor_tangents; DESIGN.md section 17, "Tangent fields"), next to
// k_sens<D, 0> with its grid, label windows and counting rule: per cell of label l0 + q and tangent k
//   q_k = |T| grad lambda^T (dTT_T / dtheta_k) grad c,     acc[q][k] += q_k
// The geometry record and the vertex ids are read once, grad lambda and grad c formed once, the K forms taken through
// glims_dt_form (a tangent need not be definite: the form does not care).  dtan: [K][n_cells][NT] planes, internal cell order.
// Per-block partials [block][LT][K] in the fixed order of block_partials; no atomics.  Bytes per cell: the geometry record
// (56 / 104 B), NV x 4 B of vertex ids, 1 B of label, 8 K d (d + 1) / 2 B of tangents (3-D: 104 + 16 + 1 + 48 K).
template <int D, int K>
__global__ __launch_bounds__(256) void k_sens_tangent(int64_t n_cells, int l0, const int32_t* __restrict__ cell_nodes,
                                                      const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                                      const double* __restrict__ c, const double* __restrict__ v,
                                                      const uint8_t* __restrict__ counted, const double* __restrict__ dtan,
                                                      double* __restrict__ partials) {
  constexpr int NV = D + 1, GE = 1 + NV * D, NT = glims_dt_size<D>();
  double acc[GL_ADJ_LT * K];   // flat: [q][k] at q * K + k
#pragma unroll
  for (int j = 0; j < GL_ADJ_LT * K; ++j) acc[j] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_cells; e += stride) {
    const int j = (int)label[e] - l0;
    if (j < 0 || j >= GL_ADJ_LT || (counted && !counted[e])) continue;
    const double* g = egeo + e * GE;
    const double vol = g[0];
    double gc[D] = {0.0}, gl[D] = {0.0};
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int nd = cell_nodes[e * NV + m];
      const double cm = c[nd], lm = v[nd];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        gc[a] += cm * g[1 + m * D + a];
        gl[a] += lm * g[1 + m * D + a];
      }
    }
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = vol * glims_dt_form<D>(dtan + ((int64_t)k * n_cells + e) * NT, gl, gc);
#pragma unroll
    for (int q = 0; q < GL_ADJ_LT; ++q)
      if (q == j) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[q * K + k] += a[k];
      }
  }
  block_partials(acc, partials);
}

// second stage of k_sens_tangent, the order of k_sens_final: one wave per sum (16 waves take the LT x K <= 32 sums in turn),
// lane l adds blocks l, l + 64, ... in order, then the wave's butterfly.  sums[k][GL_MAX_LABELS] += the partials of label l0 + q.
template <int K>
__global__ __launch_bounds__(1024) void k_sens_tangent_final(int n_blocks, int l0, int n_labels,
                                                             const double* __restrict__ partials, double* __restrict__ sums) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = w; t < GL_ADJ_LT * K; t += 16) {
    double s = 0.0;
    for (int b = lane; b < n_blocks; b += 64) s += partials[(size_t)b * GL_ADJ_LT * K + t];
    s = wsum(s);
    const int q = t / K, k = t % K;
    if (lane == 0 && l0 + q < n_labels) sums[k * GL_MAX_LABELS + l0 + q] += s;
  }
}

// g[row] += sum over the row's incidences of qcell[cell]  (G^T mu, atomics-free through the row-owned lists)
__global__ void k_gt_rows(int64_t n_own, const int64_t* __restrict__ cslice_ptr, const int32_t* __restrict__ celem,
                          const double* __restrict__ qcell, double* __restrict__ g) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  double acc = 0.0;
  for (int q = 0; q < clen; ++q) {
    const int32_t e = celem[cbase + (int64_t)q * GL_WAVE + lane];
    if (e >= 0) acc += qcell[e];
  }
  g[row] += acc;
}

// misfit of a concentration term: e = h(c) - t (kind THRESH) or c - t, hp = h'(c) or 1
__global__ void k_misfit_c(int64_t n, int kind, double level, double smooth, const double* __restrict__ c,
                           const double* __restrict__ t, double* __restrict__ e, double* __restrict__ hp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (kind == GLIMS_MISFIT_C_THRESH) {
    const double th = tanh((c[i] - level) / smooth);
    e[i] = 0.5 * (th + 1.0) - t[i];
    hp[i] = 0.5 * (1.0 - th * th) / smooth;
  } else {
    e[i] = c[i] - t[i];
    hp[i] = 1.0;
  }
}
__global__ void k_add_scaled_prod(int64_t n, double w, const double* __restrict__ a, const double* __restrict__ b,
                                  double* __restrict__ y) {   // y += w a b
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] += w * a[i] * b[i];
}
// component a of an interleaved [n][bs] vector: out = x[:, a] - t[:, a] (t may be null)
__global__ void k_component(int64_t n, int bs, int a, const double* __restrict__ x, const double* __restrict__ t,
                            double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[i * bs + a] - (t ? t[i * bs + a] : 0.0);
}
__global__ void k_add_component(int64_t n, int bs, int a, double w, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i * bs + a] += w * x[i];
}
__global__ void k_residual(int64_t n, const double* __restrict__ b, const double* __restrict__ Ax,
                           const uint8_t* __restrict__ fixed, double* __restrict__ r) {   // r = b - Ax, 0 on fixed
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) r[i] = (fixed && fixed[i]) ? 0.0 : b[i] - Ax[i];
}
__global__ void k_zero_fixed(int64_t n, const uint8_t* __restrict__ fixed, double* __restrict__ y,
                             const double* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && fixed[i]) y[i] = val ? val[i] : 0.0;
}
__global__ void k_perm(int64_t n, int bs, const int32_t* __restrict__ old2new, const double* __restrict__ src,
                       double* __restrict__ dst, int to_internal) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * bs) return;
  const int64_t o = i / bs;
  const int a = (int)(i - o * bs);
  const int64_t j = (int64_t)old2new[o] * bs + a;
  if (to_internal) dst[j] = src[i];
  else dst[i] = src[j];
}

#define GL_CHECK_LAUNCH() GL_HIP(hipGetLastError())

// device scratch of one gradient call (released on return)
struct AdjWork {
  dvec<double> lam, lam_next, rhs, g, r, u, w, p, s, e, hp, Me, tmp, qcell, part, sums, esums, vA, dinv, stage;
  dvec<uint8_t> lin;   // stays empty: the sweeps of the adjoint (which write wk.vA, ForwardGuard) keep no exact-linearity flags
  dvec<double> uk, murhs, mu, mr, mu_, mw, mp, ms, mKx;
  std::vector<std::unique_ptr<dvec<double>>> targets;
};

// Leaves the forward state as it was, also when an exception leaves gl_adjoint_gradient: the time stepper's Jacobian and
// diagonal are swapped out (not copied) for the call, kernel timing is off, statistics and V-cycle counters are restored.
struct ForwardGuard {
  glims_ctx* h;
  AdjWork& wk;
  glims_stats st;
  int64_t mg_cycles, mgrd_cycles;
  bool jac32;
  int time_kernels;
  bool mg_ready, mgrd_ready;
  ForwardGuard(glims_ctx* h_, AdjWork& w) : h(h_), wk(w) {
    st = h->stats;
    mg_ready = h->mg.ready;
    mgrd_ready = h->mg_rd.ready;
    mg_cycles = h->mg.cycles;
    mgrd_cycles = h->mg_rd.cycles;
    jac32 = h->jac32;
    time_kernels = h->opt.time_kernels;
    h->jac32 = false;   // the adjoint solves to 1e-12: the fp64 Jacobian, whatever GLIMS_FLAG_FP32_JACOBIAN says
    h->opt.time_kernels = 0;
    std::swap(h->vA.p, wk.vA.p);
    std::swap(h->vA.n, wk.vA.n);
    // (the exact-linearity flags describe the values of ONE buffer: the sweeps in here write wk.vA and so wk.lin)
    std::swap(h->lin.p, wk.lin.p);
    std::swap(h->lin.n, wk.lin.n);
    std::swap(h->dinv.p, wk.dinv.p);
    std::swap(h->dinv.n, wk.dinv.n);
  }
  ~ForwardGuard() {
    (void)hipStreamSynchronize(h->st);
    std::swap(h->vA.p, wk.vA.p);
    std::swap(h->vA.n, wk.vA.n);
    std::swap(h->lin.p, wk.lin.p);
    std::swap(h->lin.n, wk.lin.n);
    std::swap(h->dinv.p, wk.dinv.p);
    std::swap(h->dinv.n, wk.dinv.n);
    h->jac32 = jac32;
    h->opt.time_kernels = time_kernels;
    h->stats = st;
    h->mg.cycles = mg_cycles;
    h->mg_rd.cycles = mgrd_cycles;
    // a hierarchy the adjoint had to build goes again: the forward path builds it (the same one) when it needs it, with
    // its set-up statistics
    if (!mg_ready) h->mg.clear();
    if (!mgrd_ready) h->mg_rd.clear();
  }
};

void mass_apply(glims_ctx* h, const double* x, double* y) {
  gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vM.p, x, y, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
}

// Sums that every rank holds a share of (hessian_plan.h: RowPart), from src (device, or one host scalar) into dst at the same
// stride.  One GPU: the plain download.  Partitioned handles: every rank's W sums are gathered by an all-reduce of
// [world][W] (`count` doubles, from the call's buffer table) with zeros outside the own row -- x + 0 is exact: whatever order
// the transport adds in, every rank receives every row bit for bit -- and added in rank order on the host: the same bits on
// every rank.  Reached by every rank, also after a failed solve (the statuses are global; the parts are the same on every
// rank: the caller's outputs are SPMD).
struct SumPart {
  RowPart lay;
  const double* src;
  double* dst;
  bool host_src = false;
};
void gather_label_sums(glims_ctx* h, const std::vector<SumPart>& parts, size_t count) {
  if (h->world <= 1) {
    for (const SumPart& p : parts)
      if (p.lay.len)   // (the whole array, with the gaps between its runs)
        GL_HIP(hipMemcpyAsync(p.dst, p.src, p.lay.chunks * p.lay.stride * sizeof(double), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
    return;
  }
  std::vector<RowPart> lay;
  for (const SumPart& p : parts) lay.push_back(p.lay);
  const size_t W = row_width(lay);
  if (count < W * h->world) throw std::logic_error("adjoint: the gather of the per-label sums is larger than the call's table says");
  dvec<double> all;
  all.alloc_zero(count, h->st);
  double* row = all.p + W * h->rank;
  for (const SumPart& p : parts)
    for (size_t c = 0; c < p.lay.chunks && p.lay.len; ++c, row += p.lay.len)
      GL_HIP(hipMemcpyAsync(row, p.src + c * p.lay.stride, p.lay.len * sizeof(double),
                            p.host_src ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->st));
  if (!parts.empty() && parts[0].host_src) GL_HIP(hipStreamSynchronize(h->st));
  gl_allreduce_bulk(h, all.p, W * h->world);
  std::vector<double> rows(W * h->world), sum(W);
  if (W) GL_HIP(hipMemcpyAsync(rows.data(), all.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  add_rows_in_rank_order(h->world, W, rows.data(), sum.data());
  std::vector<double*> dst;
  for (const SumPart& p : parts) dst.push_back(p.dst);
  scatter_row(lay, sum.data(), dst.data());
}

// The stored image terms (glims_adjoint_image_terms) that observe `step`, in their list order, after the step's nodal terms:
// g += P^T r of each, J += 1/2 w sum_p q_p (h(v_p) - t_p)^2; with P > 0 also dg_j += P^T r2_j for the Hessian's directions
// dc (column-major [P][ld]).  No stored term: no launch.  Partitioned handles: a rank sums the points it COUNTS
// (glims_sampler_resolve), the ranks' sums are gathered and added in rank order -- one small all-reduce per term that observes
// the step, made by every rank (the stored list is SPMD: gl_adjoint_gradient has checked it).
double sum_over_ranks(glims_ctx* h, double mine) {
  double t = 0.0;
  gather_label_sums(h, {{{1, 1, 1}, &mine, &t, true}}, (size_t)h->world);
  return t;
}

void image_terms_of_step(glims_ctx* h, int step, const double* c, double* g, double* J, int P = 0,
                         const double* dc = nullptr, int64_t ld = 0, double* dg = nullptr) {
  for (const GlImageTerm* t : h->img_terms) {
    if (t->step != step) continue;
    double sum = gl_image_misfit_grad(h, *t, c, g);
    if (h->world > 1) sum = sum_over_ranks(h, sum);
    *J += 0.5 * t->weight * sum;
    if (P > 0) gl_image_misfit_second(h, *t, c, dc, P, ld, dg);
  }
}

inline int sens_blocks(const glims_ctx* h) { return (int)std::min<int64_t>(GL_ADJ_BLOCKS, grid_of(h->n_cells)); }

// k_sens<D, mode> over the labels, GL_ADJ_LT per launch, each followed by k_sens_final into sums[l][k_off + 0..1] (ls sums per
// label; the sums beyond ls are dropped).  sums == nullptr (mode 1, qcell alone): the l0 = 0 launch writes qcell, no other runs.
template <int D>
void sens_pass(glims_ctx* h, int mode, const double* mat, const double* c, const double* v, const uint8_t* counted,
               double* qcell, double* part, double* sums, int ls, int k_off) {
  const int nb = sens_blocks(h);
  const auto kern = mode == 0 ? k_sens<D, 0> : mode == 1 ? k_sens<D, 1> : k_sens<D, 2>;
  const bool aniso = mode == 0 && h->dten.p;   // a tensor field (glims_set_diffusion_tensor): the ANISO instance of mode 0
  for (int l0 = 0; l0 < h->n_labels; l0 += GL_ADJ_LT) {
    if (aniso)
      hipLaunchKernelGGL((k_sens<D, 0, 1, const double*>), dim3(nb), dim3(256), 0, h->st, h->n_cells, l0, h->adj.cell_nodes.p,
                         h->egeo.p, h->label.p, mat, c, v, counted, qcell, part, (const double*)h->dten.p);
    else
      hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, h->st, h->n_cells, l0, h->adj.cell_nodes.p, h->egeo.p, h->label.p, mat, c,
                         v, counted, qcell, part);
    GL_CHECK_LAUNCH();
    if (!sums) break;
    hipLaunchKernelGGL(k_sens_final, dim3(1), dim3(1024), 0, h->st, nb, l0, h->n_labels, ls, k_off, part, sums);
    GL_CHECK_LAUNCH();
  }
}

// k_sens_tangent<D, K> over the labels with the stored tangent fields, each launch followed by its second stage into the
// handle's sums; the grid and the label windows of sens_pass.  Nothing stored: no launch.
template <int D, int K>
void tangent_pass_k(glims_ctx* h, const double* c, const double* v, const uint8_t* counted) {
  const int nb = sens_blocks(h);
  GlTensorTangents& t = h->dtan;
  for (int l0 = 0; l0 < h->n_labels; l0 += GL_ADJ_LT) {
    hipLaunchKernelGGL((k_sens_tangent<D, K>), dim3(nb), dim3(256), 0, h->st, h->n_cells, l0, h->adj.cell_nodes.p, h->egeo.p,
                       h->label.p, c, v, counted, (const double*)t.planes.p, t.part.p);
    GL_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sens_tangent_final<K>, dim3(1), dim3(1024), 0, h->st, nb, l0, h->n_labels, t.part.p, t.sums.p);
    GL_CHECK_LAUNCH();
  }
}
template <int D>
void tangent_pass(glims_ctx* h, const double* c, const double* v, const uint8_t* counted) {
  switch (h->dtan.K) {
    case 0: return;
    case 1: return tangent_pass_k<D, 1>(h, c, v, counted);
    case 2: return tangent_pass_k<D, 2>(h, c, v, counted);
    case 3: return tangent_pass_k<D, 3>(h, c, v, counted);
    case 4: return tangent_pass_k<D, 4>(h, c, v, counted);
    default: throw std::logic_error("adjoint: more tangent fields than k_sens_tangent has instances for");
  }
}
static_assert(GLIMS_DT_MAX_TANGENTS == 4, "tangent_pass lists the instances of k_sens_tangent");

// The tangent sums of a sweep into the handle's host copy: the rows of the ranks gathered as gather_label_sums does (zeros
// outside the own row, one all-reduce, added in rank order: the same bits on every rank), from the handle's own buffers;
// out[k][t] = -dt D_t sums[k][t].  Reached by every rank, also after a failed solve (`status` then keeps the getter closed).
void finish_tangent_sums(glims_ctx* h, int status) {
  GlTensorTangents& t = h->dtan;
  if (t.K == 0) return;
  const int K = t.K, L = h->n_labels;
  const size_t W = (size_t)K * L;
  std::vector<double> sum(W);
  if (h->world <= 1) {
    for (int k = 0; k < K; ++k)
      GL_HIP(hipMemcpyAsync(sum.data() + (size_t)k * L, t.sums.p + (size_t)k * GL_MAX_LABELS, L * sizeof(double),
                            hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
  } else {
    t.gather.alloc((size_t)h->world * K * GL_MAX_LABELS);   // (the set call's size: allocates only if the transport came later)
    GL_HIP(hipMemsetAsync(t.gather.p, 0, W * h->world * sizeof(double), h->st));
    for (int k = 0; k < K; ++k)
      GL_HIP(hipMemcpyAsync(t.gather.p + W * h->rank + (size_t)k * L, t.sums.p + (size_t)k * GL_MAX_LABELS, L * sizeof(double),
                            hipMemcpyDeviceToDevice, h->st));
    gl_allreduce_bulk(h, t.gather.p, W * h->world);
    std::vector<double> rows(W * h->world);
    GL_HIP(hipMemcpyAsync(rows.data(), t.gather.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
    add_rows_in_rank_order(h->world, W, rows.data(), sum.data());
  }
  const double dt = h->opt.dt;
  t.grad.assign(W, 0.0);
  for (int k = 0; k < K; ++k)
    for (int l = 0; l < L; ++l) t.grad[(size_t)k * L + l] = -dt * h->mat_host[l] * sum[(size_t)k * L + l];
  t.grad_labels = L;
  t.have = status == GLIMS_OK;
  if (!t.have) t.why = "the last backward sweep stopped with status " + std::to_string(status);
}

// A host vector [n_nodes][bs] in the caller's numbering into dst in the internal numbering, and a scalar device vector back
// out, both through the staging buffer and synchronised (the buffer is free again on return)
void upload_permuted(glims_ctx* h, AdjWork& wk, const double* host, int bs, double* dst) {
  const int64_t nn = h->n_nodes;
  GL_HIP(hipMemcpyAsync(wk.stage.p, host, (size_t)nn * bs * sizeof(double), hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_perm, dim3(grid_of(nn * bs)), dim3(256), 0, h->st, nn, bs, h->d_old2new.p, wk.stage.p, dst, 1);
  GL_CHECK_LAUNCH();
  GL_HIP(hipStreamSynchronize(h->st));
}
void download_permuted(glims_ctx* h, AdjWork& wk, const double* src, double* host) {
  const int64_t nn = h->n_nodes;
  hipLaunchKernelGGL(k_perm, dim3(grid_of(nn)), dim3(256), 0, h->st, nn, 1, h->d_old2new.p, src, wk.stage.p, 0);
  GL_CHECK_LAUNCH();
  GL_HIP(hipMemcpyAsync(host, wk.stage.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
}

// K_el x = rhs with the Dirichlet dofs eliminated (x = xD there, or 0), to ||r|| <= rtol ||rhs||; the forward solve's
// displacement, its solve history and its hint are not touched (sibling of gl_solve_mechanics)
int solve_elastic(glims_ctx* h, AdjWork& wk, const double* rhs, double* x, const double* xD, double rtol, int64_t* its) {
  const int bs = h->dim;
  const int64_t nd = h->n_own * bs;
  const uint8_t* fx = h->have_fixed_u ? h->fixed_u.p : nullptr;
  const bool use_mg = gl_mech_precondition(h);
  // r = rhs - K xD on the free dofs, x = 0
  GL_HIP(hipMemsetAsync(x, 0, (size_t)h->n_nodes * bs * sizeof(double), h->st));
  if (fx && xD) {
    // (K xD reads the clamp values at the ghost columns; the same exchange, under the same condition, as gl_solve_mechanics)
    if (xD == h->m_uD.p) gl_halo_exchange(h, h->m_uD.p, bs);
    gl_launch_spmv_block(h, h->st, h->pat.n_slices, nullptr, xD, wk.mKx.p, fx, nullptr, nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_residual, dim3(grid_of(nd)), dim3(256), 0, h->st, nd, rhs, wk.mKx.p, fx, wk.mr.p);
  } else {
    GL_HIP(hipMemcpyAsync(wk.mr.p, rhs, (size_t)nd * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    if (fx) hipLaunchKernelGGL(k_zero_fixed, dim3(grid_of(nd)), dim3(256), 0, h->st, nd, fx, wk.mr.p, (const double*)nullptr);
  }
  GL_CHECK_LAUNCH();
  const double nb = std::sqrt(gl_dot(h, wk.mr.p, wk.mr.p, nd));
  int cs = GLIMS_OK;
  *its = 0;
  if (!std::isfinite(nb)) return GLIMS_NAN;
  if (nb > 0.0) {
    double res = 0.0;
    cs = gl_pcg(h, x, wk.mr.p, wk.mu_.p, wk.mw.p, wk.mp.p, wk.ms.p, h->m_dinv.p, nullptr, fx, bs, use_mg ? &h->mg : nullptr,
                h->opt.mg_smooth, rtol * nb, h->opt.mech_maxit, its, &res);
  }
  if (fx && xD) hipLaunchKernelGGL(k_zero_fixed, dim3(grid_of(nd)), dim3(256), 0, h->st, nd, fx, x, xD);
  GL_CHECK_LAUNCH();
  h->adj.mech_solves++;
  h->adj.mech_its += *its;
  return cs;
}

// cell -> vertex map in the internal numbering (AdjointState::cell_nodes; on partitioned handles also the counting rule of
// the per-label sums), built once per handle by whoever needs it first: a gradient, or a sampler (gl_ensure_cell_nodes)
template <int D>
void build_cell_nodes(glims_ctx* h) {
  AdjointState& a = h->adj;
  const int64_t n = h->n_own, nn = h->n_nodes;
  if (a.cell_nodes.n != (size_t)h->n_cells * (D + 1)) {
    a.cell_nodes.alloc_zero((size_t)h->n_cells * (D + 1), h->st);   // (every entry is written on one GPU; 0 keeps a gap in range)
    if (h->world <= 1) {
      hipLaunchKernelGGL(k_cell_nodes<D + 1>, dim3(grid_of(n)), dim3(256), 0, h->st, n, h->pat.cslice_ptr.p,
                         h->pat.cslots.p, h->pat.celem.p, h->pat.diag_k.p, a.cell_nodes.p);
      GL_CHECK_LAUNCH();
    } else {
      // ghost owners from the halo plan (ghosts grouped by owner: group p = peer_rank[p])
      std::vector<int32_t> gown((size_t)std::max<int64_t>(1, nn - n), 0);
      for (int p = 0; p < h->n_peers; ++p)
        for (int64_t i = h->recv_ptr[p]; i < h->recv_ptr[p + 1]; ++i) gown[(size_t)i] = h->peer_rank[p];
      dvec<int32_t> d_gown;
      d_gown.upload(gown, h->st);
      a.counted.alloc_zero((size_t)std::max<int64_t>(1, h->n_cells), h->st);
      hipLaunchKernelGGL(k_cell_nodes_all<D + 1>, dim3(grid_of(n)), dim3(256), 0, h->st, n, h->pat.slice_ptr.p, h->pat.cols.p,
                         h->pat.cslice_ptr.p, h->pat.cslots.p, h->pat.celem.p, a.cell_nodes.p, a.counted.p);
      GL_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_cell_counted<D + 1>, dim3(grid_of(h->n_cells)), dim3(256), 0, h->st, h->n_cells, n, h->rank,
                         d_gown.p, a.cell_nodes.p, a.counted.p);
      GL_CHECK_LAUNCH();
      GL_HIP(hipStreamSynchronize(h->st));   // d_gown goes out of scope
    }
  }
}

// What sizes a call (hessian_plan.h) but for the flags of the E / nu part, which the caller derives from its arguments
HessShape adjoint_shape(glims_ctx* h, int n_terms, const glims_misfit* terms, int P) {
  HessShape s;
  s.N = (int)h->adj.traj.size() - 1;
  s.P = P;
  s.dim = h->dim;
  s.n_labels = h->n_labels;
  s.world = h->world;
  s.n_nodes = h->n_nodes;
  s.n_cells = h->n_cells;
  s.total_entries = h->pat.total_entries;
  s.n_send = h->n_send;
  s.spmm_blocks = P > 0 ? gl_spmm_blocks(h) : 0;
  for (int k = 0; k < n_terms; ++k) s.term_is_u.push_back(terms[k].kind == GLIMS_MISFIT_U_L2);
  // (a displacement image term, a deformed image or volume term observes u_k as a displacement term does)
  s.any_u = hess_any_u(s.term_is_u, !h->uimg_terms.empty() || !h->dimg_terms.empty() || gl_observable_terms_any_deformed(h));
  return s;
}

// v = the call's buffer `name` (the k-th of that name), zeroed unless told otherwise; a buffer the call does not have
// (count 0) stays empty
template <class T>
void take(glims_ctx* h, const std::vector<HessBuffer>& table, const char* name, dvec<T>& v, bool zero = true, int k = 0) {
  const HessBuffer& b = hess_buffer(table, name, k);
  if (b.elem != sizeof(T)) throw std::logic_error(std::string("adjoint: element size of buffer '") + name + "'");
  if (zero) v.alloc_zero(b.count, h->st);
  else v.alloc(b.count);
}

// the work vectors, targets (internal numbering) and cell-vertex map of one gradient / Hessian call
template <int D>
void adjoint_setup(glims_ctx* h, const std::vector<HessBuffer>& table, int n_terms, const glims_misfit* terms, AdjWork& wk) {
  take(h, table, "vA", wk.vA, false);
  take(h, table, "dinv", wk.dinv, false);
  const std::pair<const char*, dvec<double>*> vecs[] = {
      {"lam", &wk.lam}, {"lam_next", &wk.lam_next}, {"rhs", &wk.rhs}, {"g", &wk.g}, {"r", &wk.r}, {"u", &wk.u}, {"w", &wk.w},
      {"p", &wk.p}, {"s", &wk.s}, {"e", &wk.e}, {"hp", &wk.hp}, {"Me", &wk.Me}, {"tmp", &wk.tmp}, {"qcell", &wk.qcell},
      {"part", &wk.part}, {"sums", &wk.sums}, {"esums", &wk.esums}, {"stage", &wk.stage},
      // with an observed displacement (a deformed image term observes u_k as a displacement term does)
      {"uk", &wk.uk}, {"murhs", &wk.murhs}, {"mu", &wk.mu}, {"mr", &wk.mr}, {"mu_", &wk.mu_}, {"mw", &wk.mw}, {"mp", &wk.mp},
      {"ms", &wk.ms}, {"mKx", &wk.mKx}};
  for (const auto& v : vecs) take(h, table, v.first, *v.second);
  // targets -> internal numbering
  for (int k = 0; k < n_terms; ++k) {
    wk.targets.push_back(std::make_unique<dvec<double>>());
    take(h, table, "target", *wk.targets.back(), true, k);
    upload_permuted(h, wk, terms[k].target, terms[k].kind == GLIMS_MISFIT_U_L2 ? D : 1, wk.targets.back()->p);
  }
  build_cell_nodes<D>(h);
}

// The first-order backward sweep, step by step: what glims_adjoint_gradient runs, and what glims_adjoint_hessian runs with
// its second-order work in between (same kernels, same order, same buffers: J and the gradient have the same bits in both).
// Construct it after the ForwardGuard (the lazy RD hierarchy is the guard's to drop).  A step is
//   c = begin_step;  have_u = nodal_terms;  [image terms: the caller]  have_u = deformed_image_terms;
//   if (have_u) coupling_adjoint;
//   step 0: c0_output, else lambda_solve -- each stops the sweep by setting `status`.
template <int D>
struct BackwardSweep {
  glims_ctx* h;
  AdjWork& wk;
  const int n_terms;
  const glims_misfit* terms;
  const bool elastic;   // the E / nu pass (mode 2) runs with the coupling adjoint
  const uint8_t* fxc;
  bool rd_mg;
  int rd_deg;
  double J = 0.0;
  int status = GLIMS_OK;

  BackwardSweep(glims_ctx* h_, AdjWork& w, int n_terms_, const glims_misfit* terms_, bool elastic_)
      : h(h_), wk(w), n_terms(n_terms_), terms(terms_), elastic(elastic_) {
    fxc = h->have_fixed_c ? h->fixed_c.p : nullptr;
    rd_mg = h->rd_precond_active == GLIMS_RD_PRECOND_MULTIGRID;
    if (rd_mg && !h->mg_rd.ready) gl_mg_setup_rd(h);
    rd_deg = h->opt.rd_mg_smooth > 0 ? h->opt.rd_mg_smooth : (h->mg_rd.lattice ? 1 : 3);
    if (h->dtan.K > 0) {   // stored tangent fields: their sums start at 0 and are this sweep's once it completes
      h->dtan.have = false;
      h->dtan.why = "the last backward sweep did not complete";
      GL_HIP(hipMemsetAsync(h->dtan.sums.p, 0, h->dtan.sums.n * sizeof(double), h->st));
    }
  }
  int last_step() const { return (int)h->adj.traj.size() - 1; }

  // mode 0: (c, lambda) -> sums[l][0..1];  mode 1: (c, mu) -> sums[l][2] and qcell;  mode 2: (u, mu) -> esums[l][0..1]
  void sens(int mode, const double* c, const double* v) {
    sens_pass<D>(h, mode, h->mat.p, c, v, h->world > 1 ? h->adj.counted.p : nullptr, wk.qcell.p, wk.part.p,
                 mode < 2 ? wk.sums.p : wk.esums.p, mode < 2 ? 3 : 2, mode == 1 ? 2 : 0);
    if (mode == 0) tangent_pass<D>(h, c, v, h->world > 1 ? h->adj.counted.p : nullptr);   // (no launch without tangents)
  }

  // c_n with current ghosts, g = 0
  const double* begin_step(int step) {
    // (c_n as recorded: gl_step leaves the ghosts of c current, but the adjoint does not rely on it -- one exchange per step)
    gl_halo_exchange(h, h->adj.traj[step]->p, 1);
    GL_HIP(hipMemsetAsync(wk.g.p, 0, (size_t)h->n_nodes * sizeof(double), h->st));
    return h->adj.traj[step]->p;
  }

  // u_k = K_el^-1 (G c_k + f) into wk.uk, murhs = 0: once per observed step, for its first displacement term or, when it has
  // none, its first deformed image term
  bool solve_uk(const double* c) {
    gl_apply_G(h, c, wk.murhs.p);
    int64_t its = 0;
    const bool timed = getenv("GLIMS_UIMG_TIMING") != nullptr;   // (next to the figures of the displacement image terms)
    const double t0 = timed ? omp_get_wtime() : 0.0;
    status = solve_elastic(h, wk, wk.murhs.p, wk.uk.p, h->have_fixed_u ? h->m_uD.p : nullptr, 1e-12, &its);
    if (timed) {
      GL_HIP(hipStreamSynchronize(h->st));
      fprintf(stderr, "glims displacement image terms: u_k solve %.4f ms  %lld iterations\n", 1e3 * (omp_get_wtime() - t0),
              (long long)its);
    }
    if (status != GLIMS_OK) return false;
    GL_HIP(hipMemsetAsync(wk.murhs.p, 0, (size_t)h->n_nodes * D * sizeof(double), h->st));
    return true;
  }

  // The stored displacement image terms (glims_adjoint_displacement_image_terms) that observe `step`, in their list order,
  // after the step's nodal and fixed image terms: J += 1/2 w sum_p q_p sum_a kappa_a (s (P u_k)_p,a - d_p,a)^2 and
  // murhs += P^T R.  have_u: u_k is solved already; returns whether it is now (the coupling adjoint follows then).  No stored
  // term: no launch.
  bool displacement_image_terms(int step, const double* c, bool have_u) {
    for (const GlDisplacementImageTerm* t : h->uimg_terms) {
      if (t->step != step) continue;
      if (!have_u) {
        if (!solve_uk(c)) return have_u;
        have_u = true;
      }
      J += 0.5 * t->weight * gl_displacement_image_misfit_grad(h, *t, wk.uk.p, wk.murhs.p);
    }
    return have_u;
  }

  // The stored deformed image terms (glims_adjoint_deformed_image_terms) that observe `step`, in their list order, after the
  // step's nodal, fixed image and displacement image terms: the points are located in the mesh at X + scale u_k, J += 1/2 w sum_p q_p (h(v_p) -
  // t_p)^2, g += P^T r and murhs += P^T S (the load through the location).  have_u: u_k is solved already; returns whether
  // it is now (the coupling adjoint follows then).  No stored term: no launch.
  bool deformed_image_terms(int step, const double* c, bool have_u) {
    for (GlDeformedImageTerm* t : h->dimg_terms) {
      if (t->step != step) continue;
      if (!have_u) {
        if (!solve_uk(c)) return have_u;
        have_u = true;
      }
      J += 0.5 * t->weight * gl_deformed_image_misfit_grad(h, *t, c, wk.uk.p, wk.g.p, wk.murhs.p);
    }
    return have_u;
  }

  // The nodal terms that observe `step`, in list order: J and g += dJ/dc_n of the concentration terms (after each,
  // after_c_term(term) runs while wk.Me still holds M (h(c) - t)); the displacement terms solve u_k once and add dJ/du_n to
  // murhs.  True when the step has a displacement term (the coupling adjoint follows).
  template <class Hook>
  bool nodal_terms(int step, const double* c, Hook&& after_c_term) {
    const int64_t n = h->n_own;
    bool have_u = false;
    for (int k = 0; k < n_terms; ++k) {
      const glims_misfit& tm = terms[k];
      if (tm.step != step) continue;
      const double* t = wk.targets[k]->p;
      if (tm.kind != GLIMS_MISFIT_U_L2) {
        hipLaunchKernelGGL(k_misfit_c, dim3(grid_of(n)), dim3(256), 0, h->st, n, tm.kind, tm.level, tm.smooth, c, t, wk.e.p,
                           wk.hp.p);
        GL_CHECK_LAUNCH();
        gl_halo_exchange(h, wk.e.p, 1);   // the mass SpMV reads e at the ghost columns
        mass_apply(h, wk.e.p, wk.Me.p);
        J += 0.5 * tm.weight * gl_dot(h, wk.e.p, wk.Me.p, n);
        hipLaunchKernelGGL(k_add_scaled_prod, dim3(grid_of(n)), dim3(256), 0, h->st, n, tm.weight, wk.hp.p, wk.Me.p, wk.g.p);
        GL_CHECK_LAUNCH();
        after_c_term(tm);
        continue;
      }
      if (!have_u) {
        if (!solve_uk(c)) return have_u;
        have_u = true;
      }
      for (int comp = 0; comp < D; ++comp) {   // dJ/du = w M_vec (u - t), component by component through the scalar M
        hipLaunchKernelGGL(k_component, dim3(grid_of(n)), dim3(256), 0, h->st, n, D, comp, wk.uk.p, t, wk.e.p);
        GL_CHECK_LAUNCH();
        gl_halo_exchange(h, wk.e.p, 1);
        mass_apply(h, wk.e.p, wk.Me.p);
        J += 0.5 * tm.weight * gl_dot(h, wk.e.p, wk.Me.p, n);
        hipLaunchKernelGGL(k_add_component, dim3(grid_of(n)), dim3(256), 0, h->st, n, D, comp, tm.weight, wk.Me.p,
                           wk.murhs.p);
        GL_CHECK_LAUNCH();
      }
    }
    return have_u;
  }

  // mu = K_el^-1 dJ/du (0 on the constrained dofs); g += G^T mu; dJ/dgamma_t += mu^T G_t c
  bool coupling_adjoint(const double* c) {
    const int64_t n = h->n_own;
    int64_t its = 0;
    status = solve_elastic(h, wk, wk.murhs.p, wk.mu.p, nullptr, 1e-12, &its);
    if (status != GLIMS_OK) return false;
    gl_halo_exchange(h, wk.mu.p, D);   // qcell of every local cell, also those whose other vertices are ghosts
    sens(1, c, wk.mu.p);
    hipLaunchKernelGGL(k_gt_rows, dim3(grid_of(n)), dim3(256), 0, h->st, n, h->pat.cslice_ptr.p, h->pat.celem.p, wk.qcell.p,
                       wk.g.p);
    GL_CHECK_LAUNCH();
    if (elastic) {   // A_t, B_t from u_k (its clamp values in place: solve_elastic wrote them) and mu_k
      gl_halo_exchange(h, wk.uk.p, D);   // PCG updates the owned rows: the cells at the cut read u_k at their ghosts
      sens(2, wk.uk.p, wk.mu.p);
    }
    return true;
  }

  // dJ/dc_0 = M lambda_1 + g_0, in the caller's numbering
  void c0_output(double* dc0) {
    if (last_step() > 0) gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vM.p, wk.lam_next.p, wk.rhs.p, nullptr, wk.g.p,
                                        nullptr, nullptr, 0, nullptr);
    else GL_HIP(hipMemcpyAsync(wk.rhs.p, wk.g.p, (size_t)h->n_own * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    download_permuted(h, wk, wk.rhs.p, dc0);
  }

  // lambda_n: A(c_n) lambda_n = g_n + M lambda_{n+1} (masked) by PCG from lambda_{n+1}, then its D / rho sums.  Leaves
  // lambda_n in wk.lam and A(c_n) with its diagonal in the swapped-in buffers; the caller ends the step with end_step().
  bool lambda_solve(const double* c) {
    AdjointState& a = h->adj;
    const int64_t n = h->n_own, nn = h->n_nodes;
    // rhs = g_n + M lambda_{n+1}, 0 on the constrained nodes
    gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vM.p, wk.lam_next.p, wk.rhs.p, fxc, wk.g.p, nullptr, nullptr, 0,
                   nullptr);
    if (fxc) hipLaunchKernelGGL(k_zero_fixed, dim3(grid_of(n)), dim3(256), 0, h->st, n, fxc, wk.rhs.p, (const double*)nullptr);
    GL_CHECK_LAUNCH();
    // A(c_n) (and its diagonal) into the swapped-in buffers; the residual output is scratch (b = 0)
    GL_HIP(hipMemsetAsync(wk.tmp.p, 0, (size_t)nn * sizeof(double), h->st));
    gl_rd_assemble(h, c, wk.tmp.p, nullptr, wk.w.p, nullptr, h->partials.p);
    GL_HIP(hipMemcpyAsync(wk.lam.p, wk.lam_next.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vA.p, wk.lam.p, wk.w.p, fxc, nullptr, nullptr, nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_residual, dim3(grid_of(n)), dim3(256), 0, h->st, n, wk.rhs.p, wk.w.p, fxc, wk.r.p);
    GL_CHECK_LAUNCH();
    const double nb = std::sqrt(gl_dot(h, wk.rhs.p, wk.rhs.p, n));
    if (!std::isfinite(nb)) {
      status = GLIMS_NAN;
      return false;
    }
    if (nb > 0.0) {
      int64_t its = 0;
      double res = 0.0;
      status = gl_pcg(h, wk.lam.p, wk.r.p, wk.u.p, wk.w.p, wk.p.p, wk.s.p, h->dinv.p, h->vA.p, fxc, 1,
                      rd_mg ? &h->mg_rd : nullptr, rd_deg, 1e-12 * nb, std::max(h->opt.cg_maxit, 20000), &its, &res);
      a.pcg_its += its;
      if (status != GLIMS_OK) return false;
      gl_halo_exchange(h, wk.lam.p, 1);   // PCG updates the owned rows: the sensitivity pass and M lambda read the ghosts
      sens(0, c, wk.lam.p);
    } else {
      GL_HIP(hipMemsetAsync(wk.lam.p, 0, (size_t)nn * sizeof(double), h->st));
    }
    return true;
  }
  void end_step() {   // lambda_n becomes lambda_{n+1}
    std::swap(wk.lam.p, wk.lam_next.p);
    h->adj.steps++;
  }

  // dJ/dD_t, dJ/drho_t, dJ/dgamma_t from the [L][3] sums
  void write_labels(const double* sums, double* dD, double* drho, double* dgamma) const {
    const double dt = h->opt.dt;
    for (int l = 0; l < h->n_labels; ++l) {
      if (dD) dD[l] = -dt * sums[l * 3 + 0];
      if (drho) drho[l] = -dt * sums[l * 3 + 1];
      if (dgamma) dgamma[l] = sums[l * 3 + 2];
    }
  }
};

template <int D>
int gradient_t(glims_ctx* h, int n_terms, const glims_misfit* terms, double* J_out, double* dD, double* drho,
               double* dgamma, double* dc0, double* dE, double* dnu) {
  AdjointState& a = h->adj;
  const double t0 = omp_get_wtime();
  AdjWork wk;
  const bool elastic = dE || dnu;   // the E / nu pass runs only when asked for
  HessShape shape = adjoint_shape(h, n_terms, terms, 0);
  shape.el = elastic;
  const std::vector<HessBuffer> table = hessian_buffers(shape);
  adjoint_setup<D>(h, table, n_terms, terms, wk);
  ForwardGuard guard(h, wk);
  BackwardSweep<D> sw(h, wk, n_terms, terms, elastic);
  for (int step = sw.last_step(); step >= 0; --step) {
    const double* c = sw.begin_step(step);
    bool have_u = sw.nodal_terms(step, c, [](const glims_misfit&) {});
    if (sw.status != GLIMS_OK) break;
    image_terms_of_step(h, step, c, wk.g.p, &sw.J);
    if (!h->uimg_terms.empty()) {
      have_u = sw.displacement_image_terms(step, c, have_u);
      if (sw.status != GLIMS_OK) break;
    }
    if (!h->dimg_terms.empty()) {
      have_u = sw.deformed_image_terms(step, c, have_u);
      if (sw.status != GLIMS_OK) break;
    }
    // a deformed volume term of a step that has no u_k yet: one solve, before the step's volume terms
    if (!have_u && gl_observable_terms_need_u(h, step)) {
      if (!sw.solve_uk(c)) break;
      have_u = true;
    }
    gl_observable_terms_of_step(h, step, c, wk.g.p, &sw.J, 0, nullptr, 0, nullptr, wk.uk.p, wk.murhs.p);
    if (have_u && !sw.coupling_adjoint(c)) break;
    if (step == 0) {
      if (dc0) sw.c0_output(dc0);
      break;
    }
    if (!sw.lambda_solve(c)) break;
    sw.end_step();
  }
  const int status = sw.status;
  // sums: [L][3] (D, rho, gamma), then [L][2] (A, B) when the E / nu pass ran
  const std::vector<RowPart> lay = label_row_parts(h->n_labels, elastic, 0);
  std::vector<double> sums(lay[0].len), esums(lay[1].len);
  gather_label_sums(h, {{lay[0], wk.sums.p, sums.data()}, {lay[1], wk.esums.p, esums.data()}},
                    hess_buffer(table, "gather").count);
  sw.write_labels(sums.data(), dD, drho, dgamma);
  if (elastic) write_elastic_labels(h->mat_host.data(), h->n_labels, D, sums.data(), esums.data(), dE, dnu);
  finish_tangent_sums(h, status);
  *J_out = sw.J;
  a.gradients++;
  a.ms_backward += 1e3 * (omp_get_wtime() - t0);
  return status;
}

// ---- second order: Hessian-vector products ("Second order") ----------------------------------------
// P <= GL_HESS_MAXDIR directions per call.  Per-label direction tables dir[p][3][GL_MAX_LABELS] = (dD, drho, dgamma); node
// vectors of the directions are stored column after column, [p][n_nodes].  Every column runs through the same arithmetic
// whatever P is: column p of a P-direction call has the bits of a one-direction call.

// Row-owned right-hand-side terms of the tangent-linear (MODE 0) and the second-order adjoint (MODE 1) solves, P columns per
// launch, atomics-free through the incidence lists (each row adds its cells' shares in list order).  Cell T of label t,
// vertex i = the row, f3 / f2 as in k_sens:
//   MODE 0:  y_p[i] += -dt (dD_p[t] int_T grad c . grad phi_i + drho_p[t] int_T (c^2 - c) phi_i)
//   MODE 1:  y_p[i] += -dt (2 rho_t int_T dc_p lam phi_i + dD_p[t] int_T grad lam . grad phi_i
//                           + drho_p[t] int_T (2c - 1) lam phi_i)
// Bytes per row and incidence: the slot word, cell id, geometry record and label as in the assembly; the gathered c / lam /
// dc_p values mostly hit the caches.
// ANISO: grad phi_i is replaced by TT_T grad phi_i once per incidence (the cell's tensor dten[e] is dead after that: no more
// live registers in the direction loop), so gg[m] = grad phi_m^T TT_T grad phi_i.  ANISO = 0 is the kernel as it was (DT empty,
// as in k_sens).
template <int D, int MODE, int ANISO = 0, class... DT>
__global__ __launch_bounds__(256) void k_hess_rows(int64_t n_own, int P, int64_t ld, const int64_t* __restrict__ cslice_ptr,
                                                   const uint32_t* __restrict__ cslots, const int32_t* __restrict__ celem,
                                                   const uint8_t* __restrict__ diag_k, const int32_t* __restrict__ cell_nodes,
                                                   const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                                   const double* __restrict__ mat, const double* __restrict__ dir, double dt,
                                                   const double* __restrict__ c, const double* __restrict__ lam,
                                                   const double* __restrict__ dc, double* __restrict__ y, DT... dten) {
  static_assert(sizeof...(DT) == (ANISO ? 1 : 0), "the tensor field is passed with ANISO alone");
  constexpr int NV = D + 1, GE = 1 + NV * D;
  constexpr double f3 = D == 2 ? 1.0 / 60.0 : 1.0 / 120.0;   // d! / (d+3)!
  constexpr double f2 = D == 2 ? 1.0 / 12.0 : 1.0 / 20.0;    // d! / (d+2)!
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  const uint32_t dk = diag_k[row];
  double acc[GL_HESS_MAXDIR];
#pragma unroll
  for (int p = 0; p < GL_HESS_MAXDIR; ++p) acc[p] = 0.0;
  for (int q = 0; q < clen; ++q) {
    const int64_t ci = cbase + (int64_t)q * GL_WAVE + lane;
    const int32_t e = celem[ci];
    if (e < 0) continue;
    const uint32_t sl = cslots[ci];
    const double* g = egeo + (int64_t)e * GE;
    const double vol = g[0];
    const int lab = label[e];
    double gi[D];   // grad phi_i (the row's vertex of the cell)
#pragma unroll
    for (int a = 0; a < D; ++a) gi[a] = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m)
      if (((sl >> (8 * m)) & 255u) == dk)
#pragma unroll
        for (int a = 0; a < D; ++a) gi[a] = g[1 + m * D + a];
    if constexpr (ANISO != 0) {   // gi <- TT_T gi
      double t[D];
      glims_dt_apply<D>(glims_dt_field(dten...) + (int64_t)e * glims_dt_size<D>(), gi, t);
#pragma unroll
      for (int a = 0; a < D; ++a) gi[a] = t[a];
    }
    int nd[NV];
    double cv[NV], gg[NV];   // gg[m] = grad phi_m . grad phi_i
    double Sc = 0.0, cc = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      nd[m] = cell_nodes[(int64_t)e * NV + m];
      cv[m] = c[nd[m]];
      Sc += cv[m];
      cc += cv[m] * cv[m];
      double t = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) t += g[1 + m * D + a] * gi[a];
      gg[m] = t;
    }
    const double c_i = c[row];
    if (MODE == 0) {
      double Kc = 0.0;
#pragma unroll
      for (int m = 0; m < NV; ++m) Kc += cv[m] * gg[m];
      Kc *= vol;
      // sum_{jk} c_j c_k prod(alpha!) with i fixed = Sc^2 + c.c + 2 c_i Sc + 2 c_i^2;  sum_j c_j (1 + delta_ij) = Sc + c_i
      const double Nc = vol * (f3 * (Sc * Sc + cc + 2.0 * c_i * Sc + 2.0 * c_i * c_i) - f2 * (Sc + c_i));
#pragma unroll
      for (int p = 0; p < GL_HESS_MAXDIR; ++p)
        if (p < P) {
          const double* dp = dir + (size_t)p * 3 * GL_MAX_LABELS;
          acc[p] += -dt * (dp[lab] * Kc + dp[GL_MAX_LABELS + lab] * Nc);
        }
    } else {
      double lv[NV], Sl = 0.0, Kl = 0.0, cl = 0.0;
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        lv[m] = lam[nd[m]];
        Sl += lv[m];
        Kl += lv[m] * gg[m];
        cl += cv[m] * lv[m];
      }
      Kl *= vol;
      const double l_i = lam[row];
      const double Q = vol * (2.0 * f3 * (Sc * Sl + cl + c_i * Sl + l_i * Sc + 2.0 * c_i * l_i) - f2 * (Sl + l_i));
      const double rho = mat[GL_MAX_LABELS + lab];
#pragma unroll
      for (int p = 0; p < GL_HESS_MAXDIR; ++p)
        if (p < P) {
          const double* dcp = dc + (size_t)p * ld;
          double Sd = 0.0, dl = 0.0;
#pragma unroll
          for (int m = 0; m < NV; ++m) {
            const double dv = dcp[nd[m]];
            Sd += dv;
            dl += dv * lv[m];
          }
          const double d_i = dcp[row];
          const double R = vol * f3 * (Sd * Sl + dl + d_i * Sl + l_i * Sd + 2.0 * d_i * l_i);
          const double* dp = dir + (size_t)p * 3 * GL_MAX_LABELS;
          acc[p] += -dt * (2.0 * rho * R + dp[lab] * Kl + dp[GL_MAX_LABELS + lab] * Q);
        }
    }
  }
#pragma unroll
  for (int p = 0; p < GL_HESS_MAXDIR; ++p)
    if (p < P) y[(size_t)p * ld + row] += acc[p];
}

// Per-label Hessian sums of one direction, the layout, grid and fixed-order reduction of k_sens (then k_sens_final):
//   q0 = int_T grad nu . grad c + grad lam . grad dc,   q1 = int_T nu (c^2 - c) + lam (2c - 1) dc   (exact for P1)
// counted: as in k_sens (partitioned handles, else nullptr)
// ANISO: both gradient forms take the cell's tensor dten[e] in the middle; ANISO = 0 is the kernel as it was (DT empty, as in
// k_sens).
template <int D, int ANISO = 0, class... DT>
__global__ __launch_bounds__(256) void k_hsens(int64_t n_cells, int l0, const int32_t* __restrict__ cell_nodes,
                                               const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                               const double* __restrict__ c, const double* __restrict__ lam,
                                               const double* __restrict__ dc, const double* __restrict__ nu,
                                               const uint8_t* __restrict__ counted, double* __restrict__ partials, DT... dten) {
  static_assert(sizeof...(DT) == (ANISO ? 1 : 0), "the tensor field is passed with ANISO alone");
  constexpr int NV = D + 1, GE = 1 + NV * D;
  constexpr double f3 = D == 2 ? 1.0 / 60.0 : 1.0 / 120.0;
  constexpr double f2 = D == 2 ? 1.0 / 12.0 : 1.0 / 20.0;
  double acc[GL_ADJ_LT][2];
#pragma unroll
  for (int j = 0; j < GL_ADJ_LT; ++j) acc[j][0] = acc[j][1] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_cells; e += stride) {
    const int j = label[e] - l0;
    if (j < 0 || j >= GL_ADJ_LT || (counted && !counted[e])) continue;
    const double* g = egeo + e * GE;
    const double vol = g[0];
    double gc[D] = {0.0}, gl[D] = {0.0}, gd[D] = {0.0}, gv[D] = {0.0};
    double Sc = 0.0, Sl = 0.0, Sd = 0.0, Sv = 0.0, cc = 0.0, vc = 0.0, vcc = 0.0, cd = 0.0, ld = 0.0, lc = 0.0, lcd = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int64_t k = cell_nodes[e * NV + m];
      const double cm = c[k], lm = lam[k], dm = dc[k], vm = nu[k];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        const double gm = g[1 + m * D + a];
        gc[a] += cm * gm;
        gl[a] += lm * gm;
        gd[a] += dm * gm;
        gv[a] += vm * gm;
      }
      Sc += cm;
      Sl += lm;
      Sd += dm;
      Sv += vm;
      cc += cm * cm;
      vc += vm * cm;
      vcc += vm * cm * cm;
      cd += cm * dm;
      ld += lm * dm;
      lc += lm * cm;
      lcd += lm * cm * dm;
    }
    double gg = 0.0;
    if constexpr (ANISO != 0) {
      const double* T = glims_dt_field(dten...) + e * glims_dt_size<D>();
      gg = glims_dt_form<D>(T, gv, gc) + glims_dt_form<D>(T, gl, gd);
    } else {
#pragma unroll
      for (int a = 0; a < D; ++a) gg += gv[a] * gc[a] + gl[a] * gd[a];
    }
    const double a0 = vol * gg;
    // sum_{abc} x_a y_b z_c prod(alpha!) = Sx Sy Sz + Sx (y.z) + Sy (x.z) + Sz (x.y) + 2 sum x y z
    const double a1 = vol * (f3 * (Sv * Sc * Sc + 2.0 * Sc * vc + Sv * cc + 2.0 * vcc) - f2 * (Sv * Sc + vc) +
                             2.0 * f3 * (Sl * Sc * Sd + Sl * cd + Sc * ld + Sd * lc + 2.0 * lcd) - f2 * (Sl * Sd + ld));
#pragma unroll
    for (int q = 0; q < GL_ADJ_LT; ++q)
      if (q == j) {
        acc[q][0] += a0;
        acc[q][1] += a1;
      }
  }
  block_partials(reinterpret_cast<double (&)[GL_ADJ_LT * 2]>(acc), partials);   // flat: [q][k] at q * 2 + k
}

// y[row][a] = (G dc + sum_t dgamma_t G_t c)[row][a] = sum over the row's cells of
//   (2 mu_T + d lam_T) |T| / (d+1) (gamma_T sum_m dc_m + dgamma_T sum_m c_m) dphi_row / dx_a     (owned rows; row-owned)
// EL (a direction in E / nu): plus dkap_T |T| / (d+1) sum_m c_m dphi_row / dx_a with the per-label table
// dkap_t = gamma_t (2 dm_t + d dl_t), the E / nu part of dG c, and the row's entries of `sub` (dK u_k, from k_dkel_rows) are
// subtracted on the way out: y = G dc + dG c - dK u_k from one pass.  The terms of EL = false keep their arithmetic and its
// order.
template <int D, bool EL>
__global__ void k_gdir_rows(int64_t n_own, const int64_t* __restrict__ cslice_ptr, const uint32_t* __restrict__ cslots,
                            const int32_t* __restrict__ celem, const uint8_t* __restrict__ diag_k,
                            const int32_t* __restrict__ cell_nodes, const double* __restrict__ egeo,
                            const uint8_t* __restrict__ label, const double* __restrict__ mat,
                            const double* __restrict__ dgam, const double* __restrict__ dkap,
                            const double* __restrict__ sub, const double* __restrict__ c, const double* __restrict__ dc,
                            double* __restrict__ y) {
  constexpr int NV = D + 1, GE = 1 + NV * D;
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  const uint32_t dk = diag_k[row];
  double acc[D];
#pragma unroll
  for (int a = 0; a < D; ++a) acc[a] = 0.0;
  for (int q = 0; q < clen; ++q) {
    const int64_t ci = cbase + (int64_t)q * GL_WAVE + lane;
    const int32_t e = celem[ci];
    if (e < 0) continue;
    const uint32_t sl = cslots[ci];
    const double* g = egeo + (int64_t)e * GE;
    const int lab = label[e];
    double Sc = 0.0, Sd = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int32_t k = cell_nodes[(int64_t)e * NV + m];
      Sc += c[k];
      Sd += dc[k];
    }
    const double mu = mat[3 * GL_MAX_LABELS + lab], lam = mat[4 * GL_MAX_LABELS + lab];
    double w = (2.0 * mu + D * lam) * g[0] * (1.0 / (D + 1)) * (mat[2 * GL_MAX_LABELS + lab] * Sd + dgam[lab] * Sc);
    if (EL) w += dkap[lab] * g[0] * (1.0 / (D + 1)) * Sc;
#pragma unroll
    for (int m = 0; m < NV; ++m)
      if (((sl >> (8 * m)) & 255u) == dk)
#pragma unroll
        for (int a = 0; a < D; ++a) acc[a] += w * g[1 + m * D + a];
  }
#pragma unroll
  for (int a = 0; a < D; ++a) y[row * D + a] = EL ? acc[a] - sub[row * D + a] : acc[a];
}

// y_p[row][b] = (dK_p v)[row][b] = sum over the row's cells T of |T| (2 dm_p,T eps(v)|_T + dl_p,T div v|_T I) grad phi_row, the
// stiffness operator along the E / nu part of direction p applied to a displacement-like vector v (u_k with its Dirichlet
// values, or mu_k).  Row-owned through the incidence lists, no atomics, P <= GL_HESS_MAXDIR columns per launch: the cell's
// strain is formed once, each column adds two products per component.  dlame[p][2][GL_MAX_LABELS] = (dm, dl) per label;
// columns stored one after the other, ld apart.  Bytes per row and incidence: the slot word, cell id, geometry record and
// label as in k_hess_rows; the gathered v (8 d B per vertex) mostly hits the caches; 8 d P B written per row.
template <int D>
__global__ __launch_bounds__(256) void k_dkel_rows(int64_t n_own, int P, int64_t ld, const int64_t* __restrict__ cslice_ptr,
                                                   const uint32_t* __restrict__ cslots, const int32_t* __restrict__ celem,
                                                   const uint8_t* __restrict__ diag_k, const int32_t* __restrict__ cell_nodes,
                                                   const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                                   const double* __restrict__ dlame, const double* __restrict__ v,
                                                   double* __restrict__ y) {
  constexpr int NV = D + 1, GE = 1 + NV * D;
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  const uint32_t dk = diag_k[row];
  double acc[GL_HESS_MAXDIR][D];
#pragma unroll
  for (int p = 0; p < GL_HESS_MAXDIR; ++p)
#pragma unroll
    for (int b = 0; b < D; ++b) acc[p][b] = 0.0;
  for (int q = 0; q < clen; ++q) {
    const int64_t ci = cbase + (int64_t)q * GL_WAVE + lane;
    const int32_t e = celem[ci];
    if (e < 0) continue;
    const uint32_t sl = cslots[ci];
    const double* g = egeo + (int64_t)e * GE;
    const double vol = g[0];
    const int lab = label[e];
    double gi[D];   // grad phi_i (the row's vertex of the cell)
#pragma unroll
    for (int a = 0; a < D; ++a) gi[a] = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m)
      if (((sl >> (8 * m)) & 255u) == dk)
#pragma unroll
        for (int a = 0; a < D; ++a) gi[a] = g[1 + m * D + a];
    // grad v_h [a][b] = d_a v_b = sum_m v_{m,b} dphi_m/dx_a
    double gv[D][D] = {};
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int64_t k = cell_nodes[(int64_t)e * NV + m];
#pragma unroll
      for (int b = 0; b < D; ++b) {
        const double vm = v[k * D + b];
#pragma unroll
        for (int a = 0; a < D; ++a) gv[a][b] += vm * g[1 + m * D + a];
      }
    }
    double tr = 0.0, se[D];   // se = 2 eps(v) grad phi_i
#pragma unroll
    for (int a = 0; a < D; ++a) tr += gv[a][a];
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double t = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) t += (gv[a][b] + gv[b][a]) * gi[a];
      se[b] = t;
    }
#pragma unroll
    for (int p = 0; p < GL_HESS_MAXDIR; ++p)
      if (p < P) {
        const double* dp = dlame + (size_t)p * 2 * GL_MAX_LABELS;
        const double dm = dp[lab], dl = dp[GL_MAX_LABELS + lab];
#pragma unroll
        for (int b = 0; b < D; ++b) acc[p][b] += vol * (dm * se[b] + dl * tr * gi[b]);
      }
  }
#pragma unroll
  for (int p = 0; p < GL_HESS_MAXDIR; ++p)
    if (p < P)
#pragma unroll
      for (int b = 0; b < D; ++b) y[(size_t)p * ld + row * D + b] = acc[p][b];
}

// Per-label second-order sums of the E / nu rows, one direction: the layout, grid and fixed-order reduction of k_sens (then
// k_sens_final), with a partials buffer of its own.  Geometry and vertex ids are read once for both pairs:
//   q0 = int_T eps(dmu):eps(u) + eps(mu):eps(du),   q1 = int_T div dmu div u + div mu div du
// counted: as in k_sens (partitioned handles, else nullptr)
template <int D>
__global__ __launch_bounds__(256) void k_hesens(int64_t n_cells, int l0, const int32_t* __restrict__ cell_nodes,
                                                const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                                const double* __restrict__ u, const double* __restrict__ mu,
                                                const double* __restrict__ du, const double* __restrict__ dmu,
                                                const uint8_t* __restrict__ counted, double* __restrict__ partials) {
  constexpr int NV = D + 1, GE = 1 + NV * D;
  double acc[GL_ADJ_LT][2];
#pragma unroll
  for (int j = 0; j < GL_ADJ_LT; ++j) acc[j][0] = acc[j][1] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_cells; e += stride) {
    const int j = label[e] - l0;
    if (j < 0 || j >= GL_ADJ_LT || (counted && !counted[e])) continue;
    const double* g = egeo + e * GE;
    const double vol = g[0];
    // grad w_h [a][b] = d_a w_b = sum_m w_{m,b} dphi_m/dx_a
    double gu[D][D] = {}, gm[D][D] = {}, gdu[D][D] = {}, gdm[D][D] = {};
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int64_t k = cell_nodes[e * NV + m];
#pragma unroll
      for (int b = 0; b < D; ++b) {
        const double um = u[k * D + b], mm = mu[k * D + b], dum = du[k * D + b], dmm = dmu[k * D + b];
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double ga = g[1 + m * D + a];
          gu[a][b] += um * ga;
          gm[a][b] += mm * ga;
          gdu[a][b] += dum * ga;
          gdm[a][b] += dmm * ga;
        }
      }
    }
    double ee = 0.0, tu = 0.0, tm = 0.0, tdu = 0.0, tdm = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      tu += gu[a][a];
      tm += gm[a][a];
      tdu += gdu[a][a];
      tdm += gdm[a][a];
#pragma unroll
      for (int b = 0; b < D; ++b)
        ee += 0.25 * ((gdm[a][b] + gdm[b][a]) * (gu[a][b] + gu[b][a]) + (gm[a][b] + gm[b][a]) * (gdu[a][b] + gdu[b][a]));
    }
    const double a0 = vol * ee, a1 = vol * (tdm * tu + tm * tdu);
#pragma unroll
    for (int q = 0; q < GL_ADJ_LT; ++q)
      if (q == j) {
        acc[q][0] += a0;
        acc[q][1] += a1;
      }
  }
  block_partials(reinterpret_cast<double (&)[GL_ADJ_LT * 2]>(acc), partials);   // flat: [q][k] at q * 2 + k
}

__global__ void k_sub(int64_t n, const double* __restrict__ x, double* __restrict__ y) {   // y -= x
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] -= x[i];
}

// h'(c) and h''(c) of a concentration term (1 and 0 for C_L2)
__device__ __forceinline__ void misfit_derivs(int kind, double level, double smooth, double c, double* hp, double* h2) {
  if (kind == GLIMS_MISFIT_C_THRESH) {
    const double th = tanh((c - level) / smooth);
    *hp = 0.5 * (1.0 - th * th) / smooth;
    *h2 = -th * (1.0 - th * th) / (smooth * smooth);
  } else {
    *hp = 1.0;
    *h2 = 0.0;
  }
}
__global__ void k_misfit_dir(int64_t n, int kind, double level, double smooth, const double* __restrict__ c,
                             const double* __restrict__ dc, double* __restrict__ out) {   // out = h'(c) dc
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double hp, h2;
  misfit_derivs(kind, level, smooth, c[i], &hp, &h2);
  out[i] = hp * dc[i];
}
// dg += w (h' M(h' dc) + h'' M(h - t) dc), nodewise (Mhd = M(h' dc), Me = M(h - t))
__global__ void k_misfit_second(int64_t n, int kind, double level, double smooth, double w, const double* __restrict__ c,
                                const double* __restrict__ dc, const double* __restrict__ Me,
                                const double* __restrict__ Mhd, double* __restrict__ dg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double hp, h2;
  misfit_derivs(kind, level, smooth, c[i], &hp, &h2);
  dg[i] += w * (hp * Mhd[i] + h2 * Me[i] * dc[i]);
}

// A(c_n) x = rhs (0 on the constrained nodes) by the PCG of the first-order adjoint's lambda solve; x holds the initial
// guess on entry (its constrained entries are set to 0)
int rd_solve(glims_ctx* h, AdjWork& wk, const uint8_t* fxc, bool rd_mg, int rd_deg, const double* rhs, double* x,
             int64_t* its) {
  const int64_t n = h->n_own;
  if (fxc) hipLaunchKernelGGL(k_zero_fixed, dim3(grid_of(n)), dim3(256), 0, h->st, n, fxc, x, (const double*)nullptr);
  gl_halo_exchange(h, x, 1);   // (partitioned handles: the guess at the ghost columns, with its zeros on the constrained nodes)
  gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vA.p, x, wk.w.p, fxc, nullptr, nullptr, nullptr, 0, nullptr);
  hipLaunchKernelGGL(k_residual, dim3(grid_of(n)), dim3(256), 0, h->st, n, rhs, wk.w.p, fxc, wk.r.p);
  GL_CHECK_LAUNCH();
  const double nb = std::sqrt(gl_dot(h, rhs, rhs, n));
  *its = 0;
  if (!std::isfinite(nb)) return GLIMS_NAN;
  if (nb == 0.0) {
    GL_HIP(hipMemsetAsync(x, 0, (size_t)h->n_nodes * sizeof(double), h->st));
    return GLIMS_OK;
  }
  double res = 0.0;
  const int st = gl_pcg(h, x, wk.r.p, wk.u.p, wk.w.p, wk.p.p, wk.s.p, h->dinv.p, h->vA.p, fxc, 1,
                        rd_mg ? &h->mg_rd : nullptr, rd_deg, 1e-12 * nb, std::max(h->opt.cg_maxit, 20000), its, &res);
  if (fxc) hipLaunchKernelGGL(k_zero_fixed, dim3(grid_of(n)), dim3(256), 0, h->st, n, fxc, x, (const double*)nullptr);
  GL_CHECK_LAUNCH();
  return st;
}

// ---- P-column Jacobi-PCG: P independent solves A x_j = b_j sharing one k_spmm per iteration ------------------------------
// Vectors interleaved [node][P].  Each column has its own alpha, beta, stopping test (||r_j|| <= tol_j) and done flag; a done
// column is frozen (no update of x, r or p).  The 2P dot products (r.z, r.r) of an iteration come from one fixed-order
// reduction (block partials on a fixed grid, then one wave per sum), p.Ap from k_spmm's fused partials: no float atomics,
// and the arithmetic of column j does not depend on P.  State sc[6][P]: rz, rr, alpha, beta, tol, pq.
enum { MP_RZ = 0, MP_RR, MP_ALPHA, MP_BETA, MP_TOL, MP_PQ, MP_N };
static_assert(MP_N == GL_MP_SCALARS, "hessian_plan.h sizes the scalar buffer");

// column-major [P][ld] <-> interleaved [n][P]; fixed rows give 0 (pack)
template <int P>
__global__ void k_mp_pack(int64_t n, int64_t ld, const double* __restrict__ src, const uint8_t* __restrict__ fixed,
                          double* __restrict__ dst, int to_interleaved) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    if (to_interleaved) dst[i * P + q] = (fixed && fixed[i]) ? 0.0 : src[(int64_t)q * ld + i];
    else dst[(int64_t)q * ld + i] = src[i * P + q];
  }
}

// mode 0 (start): r = b - Ax (Ax in q), p = z = Dinv r;  mode 1 (iteration): x += alpha p, r -= alpha q, z = Dinv r.
// Both leave the block partials of (r.z, r.r) per column.
template <int P>
__global__ __launch_bounds__(256) void k_mp_vec(int mode, int64_t n, const uint8_t* __restrict__ fixed,
                                                const double* __restrict__ dinv, const double* __restrict__ b,
                                                double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                const double* __restrict__ q, const double* __restrict__ sc,
                                                const int* __restrict__ done, double* __restrict__ part) {
  double v[2 * P], al[P];
  bool dn[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {   // the column scalars, once per thread
    dn[j] = done[j] != 0;
    al[j] = sc[MP_ALPHA * P + j];
  }
#pragma unroll
  for (int k = 0; k < 2 * P; ++k) v[k] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const bool fx = fixed && fixed[i];
    const double di = dinv[i];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (dn[j]) continue;
      const int64_t o = i * P + j;
      double rr;
      if (mode == 0) {
        rr = fx ? 0.0 : b[o] - q[o];
      } else {
        const double a = al[j];
        x[o] += a * p[o];
        rr = r[o] - a * q[o];
      }
      r[o] = rr;
      const double z = fx ? 0.0 : di * rr;
      if (mode == 0) p[o] = z;
      v[2 * j] += rr * z;
      v[2 * j + 1] += rr * rr;
    }
  }
  block_partials(v, part);
}

// p = Dinv r + beta p (columns still running)
template <int P>
__global__ void k_mp_dir(int64_t n, const uint8_t* __restrict__ fixed, const double* __restrict__ dinv,
                         const double* __restrict__ r, double* __restrict__ p, const double* __restrict__ sc,
                         const int* __restrict__ done) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool fx = fixed && fixed[i];
  const double di = fx ? 0.0 : dinv[i];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const bool dn = done[j] != 0;
    const double be = sc[MP_BETA * P + j];
    if (dn) continue;
    const int64_t o = i * P + j;
    p[o] = di * r[o] + be * p[o];
  }
}

// The scalar step, one wave per sum (fixed order: lane l adds blocks l, l + 64, ..., then the butterfly), thread 0 per column:
//   stage 0 (after the start):      rz, rr; done when ||r|| <= tol
//   stage 1 (after k_spmm):          pq = p.Ap, alpha = rz / pq (breakdown: flags[1])
//   stage 2 (after the update):      done when ||r|| <= tol (its[j] = it), else beta = rz' / rz;  flags[0] = all done
template <int P>
__device__ __forceinline__ void mp_scalar_step(int stage, int it, const double* s, double* __restrict__ sc,
                                               int* __restrict__ done, int* __restrict__ its, int* __restrict__ flags) {
  int all = 1;
  for (int j = 0; j < P; ++j) {
    if (!done[j]) {
      if (stage == 1) {
        const double pq = s[j];
        sc[MP_PQ * P + j] = pq;
        if (!(pq > 0.0) || !isfinite(pq)) {
          flags[1] = 1;
          done[j] = 1;
        } else {
          sc[MP_ALPHA * P + j] = sc[MP_RZ * P + j] / pq;
        }
      } else {
        const double rz = s[2 * j], rr = s[2 * j + 1];
        if (!isfinite(rr)) {
          flags[1] = 1;
          done[j] = 1;
        } else if (sqrt(rr) <= sc[MP_TOL * P + j]) {
          done[j] = 1;
          its[j] = it;
        } else if (stage == 2) {
          sc[MP_BETA * P + j] = rz / sc[MP_RZ * P + j];
        }
        sc[MP_RZ * P + j] = rz;
        sc[MP_RR * P + j] = rr;
      }
    }
    all = all && done[j];
  }
  flags[0] = all;
}
template <int P>
__global__ __launch_bounds__(1024) void k_mp_scalar(int stage, int it, int nb, const double* __restrict__ part,
                                                    double* __restrict__ sc, int* __restrict__ done, int* __restrict__ its,
                                                    int* __restrict__ flags) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ns = stage == 1 ? P : 2 * P;
  __shared__ double s[2 * P];
  if (w < ns) {
    double t = 0.0;
    for (int bk = lane; bk < nb; bk += 64) t += part[(size_t)bk * ns + w];
    t = wsum(t);
    if (lane == 0) s[w] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  mp_scalar_step<P>(stage, it, s, sc, done, its, flags);
}

// Partitioned handles: the sums of an iteration are over all ranks and the same bits on all of them.  k_mp_rank_sums reduces
// this rank's block partials in k_mp_scalar's order into row `rank` of rows[world][ns] and zeroes the other rows; the
// all-reduce of rows then is a gather (x + 0 is exact in every transport); k_mp_scalar_ranks adds the rows in rank order and
// takes the scalar step.  Every rank holds the same sc, done, its and flags afterwards.
__global__ __launch_bounds__(1024) void k_mp_rank_sums(int ns, int nb, int rank, int world, const double* __restrict__ part,
                                                       double* __restrict__ rows) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __shared__ double s[2 * 8];
  if (w < ns) {
    double t = 0.0;
    for (int bk = lane; bk < nb; bk += 64) t += part[(size_t)bk * ns + w];
    t = wsum(t);
    if (lane == 0) s[w] = t;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < world * ns; i += blockDim.x) rows[i] = i / ns == rank ? s[i - rank * ns] : 0.0;
}
template <int P>
__global__ void k_mp_scalar_ranks(int stage, int it, int world, const double* __restrict__ rows, double* __restrict__ sc,
                                  int* __restrict__ done, int* __restrict__ its, int* __restrict__ flags) {
  const int ns = stage == 1 ? P : 2 * P;
  __shared__ double s[2 * P];
  if (threadIdx.x < ns) {
    double t = 0.0;
    for (int r = 0; r < world; ++r) t += rows[r * ns + threadIdx.x];
    s[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  mp_scalar_step<P>(stage, it, s, sc, done, its, flags);
}

struct MultiPcg {
  dvec<double> X, B, R, Pv, Q, part, part2, sc;
  dvec<int> done, its, flags;
  // partitioned handles: the send buffer of the [n_nodes][P] ghost exchanges (n_send x P: the handle's own holds n_send x dim)
  // and the [world][2 P] rows of the cross-rank sums
  dvec<double> sendbuf, rows;
};

// the scalar step after a reduction of `nb` block partials (stage as in k_mp_scalar); on a partitioned handle through the
// gather of every rank's sums
template <int P>
void mp_scalar(glims_ctx* h, MultiPcg& m, int stage, int it, int nb, const double* part) {
  if (h->world <= 1) {
    hipLaunchKernelGGL(k_mp_scalar<P>, dim3(1), dim3(1024), 0, h->st, stage, it, nb, part, m.sc.p, m.done.p, m.its.p,
                       m.flags.p);
    GL_CHECK_LAUNCH();
    return;
  }
  const int ns = stage == 1 ? P : 2 * P;
  hipLaunchKernelGGL(k_mp_rank_sums, dim3(1), dim3(1024), 0, h->st, ns, nb, h->rank, h->world, part, m.rows.p);
  GL_CHECK_LAUNCH();
  gl_allreduce_bulk(h, m.rows.p, (size_t)h->world * ns);
  hipLaunchKernelGGL(k_mp_scalar_ranks<P>, dim3(1), dim3(64), 0, h->st, stage, it, h->world, (const double*)m.rows.p, m.sc.p,
                     m.done.p, m.its.p, m.flags.p);
  GL_CHECK_LAUNCH();
}
// ghosts of an interleaved [n_nodes][P] operand of k_spmm
void mp_exchange(glims_ctx* h, MultiPcg& m, double* v, int P) {
  if (h->world <= 1) return;
  gl_halo_exchange_buf(h, v, P, m.sendbuf.p);
}

template <int P>
int mp_solve_t(glims_ctx* h, MultiPcg& m, const uint8_t* fxc, const double* rhs, double* x, int64_t ld,
               const std::vector<double>& nb, int64_t* its_out) {
  const int64_t n = h->n_own;
  const unsigned g = grid_of(n);
  const int nbk = (int)std::min<int64_t>(GL_MP_BLOCKS, g);
  std::vector<double> sc((size_t)MP_N * P, 0.0);
  std::vector<int> done(P, 0), its(P, 0), flags(2, 0);
  for (int j = 0; j < P; ++j) {
    sc[MP_TOL * P + j] = 1e-12 * nb[j];
    done[j] = nb[j] == 0.0;   // a zero right-hand side: x_j = 0 (below), no iteration
  }
  m.sc.upload(sc, h->st);
  m.done.upload(done, h->st);
  m.its.upload(its, h->st);
  m.flags.upload(flags, h->st);
  for (int j = 0; j < P; ++j)
    if (done[j]) GL_HIP(hipMemsetAsync(x + (size_t)j * ld, 0, (size_t)h->n_nodes * sizeof(double), h->st));
  hipLaunchKernelGGL(k_mp_pack<P>, dim3(g), dim3(256), 0, h->st, n, ld, rhs, fxc, m.B.p, 1);
  hipLaunchKernelGGL(k_mp_pack<P>, dim3(g), dim3(256), 0, h->st, n, ld, (const double*)x, fxc, m.X.p, 1);
  GL_CHECK_LAUNCH();
  mp_exchange(h, m, m.X.p, P);
  gl_launch_spmm(h, P, h->vA.p, m.X.p, m.Q.p, fxc, nullptr);
  hipLaunchKernelGGL(k_mp_vec<P>, dim3(nbk), dim3(256), 0, h->st, 0, n, fxc, h->dinv.p, m.B.p, m.X.p, m.R.p, m.Pv.p, m.Q.p,
                     m.sc.p, m.done.p, m.part2.p);
  GL_CHECK_LAUNCH();
  mp_scalar<P>(h, m, 0, 0, nbk, m.part2.p);
  const int maxit = std::max(h->opt.cg_maxit, 20000), nbs = gl_spmm_blocks(h);
  int it = 0;
  for (;;) {
    GL_HIP(hipMemcpyAsync(flags.data(), m.flags.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
    if (flags[0] || it >= maxit) break;
    for (int k = 0; k < 4 && it < maxit; ++k) {   // (done columns stay frozen: checking every 4 iterations changes no bit)
      ++it;
      mp_exchange(h, m, m.Pv.p, P);
      gl_launch_spmm(h, P, h->vA.p, m.Pv.p, m.Q.p, fxc, m.part.p);
      mp_scalar<P>(h, m, 1, it, nbs, m.part.p);
      hipLaunchKernelGGL(k_mp_vec<P>, dim3(nbk), dim3(256), 0, h->st, 1, n, fxc, h->dinv.p, m.B.p, m.X.p, m.R.p, m.Pv.p,
                         m.Q.p, m.sc.p, m.done.p, m.part2.p);
      GL_CHECK_LAUNCH();
      mp_scalar<P>(h, m, 2, it, nbk, m.part2.p);
      hipLaunchKernelGGL(k_mp_dir<P>, dim3(g), dim3(256), 0, h->st, n, fxc, h->dinv.p, m.R.p, m.Pv.p, m.sc.p, m.done.p);
      GL_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(k_mp_pack<P>, dim3(g), dim3(256), 0, h->st, n, ld, (const double*)m.X.p, fxc, x, 0);
  GL_CHECK_LAUNCH();
  GL_HIP(hipMemcpyAsync(its.data(), m.its.p, P * sizeof(int), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  for (int j = 0; j < P; ++j) *its_out += its[j];
  if (flags[1]) return GLIMS_NAN;
  return flags[0] ? GLIMS_OK : GLIMS_NOT_CONVERGED;
}

// A(c_n) x_j = rhs_j for P columns (column-major [P][ld], rhs 0 on the constrained nodes; x holds the initial guesses): one
// P-column Jacobi-PCG with the Jacobi preconditioner; with the RD multigrid (stiff steps) the V-cycle PCG of rd_solve runs
// column by column (no batched V-cycle).  Stops column j at ||r|| <= 1e-12 ||rhs_j||.
int rd_solve_cols(glims_ctx* h, AdjWork& wk, MultiPcg& m, const uint8_t* fxc, bool rd_mg, int rd_deg, int P,
                  const double* rhs, double* x, int64_t ld, int64_t* its) {
  if (rd_mg) {
    int st = GLIMS_OK;
    for (int j = 0; j < P && st == GLIMS_OK; ++j) {
      int64_t k = 0;
      st = rd_solve(h, wk, fxc, rd_mg, rd_deg, rhs + (size_t)j * ld, x + (size_t)j * ld, &k);
      *its += k;
    }
    return st;
  }
  std::vector<double> nb(P);
  for (int j = 0; j < P; ++j) {
    nb[j] = std::sqrt(gl_dot(h, rhs + (size_t)j * ld, rhs + (size_t)j * ld, h->n_own));
    if (!std::isfinite(nb[j])) return GLIMS_NAN;
  }
  switch (P) {
    case 1: return mp_solve_t<1>(h, m, fxc, rhs, x, ld, nb, its);
    case 2: return mp_solve_t<2>(h, m, fxc, rhs, x, ld, nb, its);
    case 3: return mp_solve_t<3>(h, m, fxc, rhs, x, ld, nb, its);
    case 4: return mp_solve_t<4>(h, m, fxc, rhs, x, ld, nb, its);
    case 5: return mp_solve_t<5>(h, m, fxc, rhs, x, ld, nb, its);
    case 6: return mp_solve_t<6>(h, m, fxc, rhs, x, ld, nb, its);
    case 7: return mp_solve_t<7>(h, m, fxc, rhs, x, ld, nb, its);
    default: return mp_solve_t<8>(h, m, fxc, rhs, x, ld, nb, its);
  }
}

// glims_adjoint_stats counts gradient calls only: what the shared solves of a Hessian call add goes back on return
struct AdjCountGuard {
  AdjointState& a;
  int64_t gradients, steps, pcg_its, mech_solves, mech_its;
  double ms;
  explicit AdjCountGuard(AdjointState& a_)
      : a(a_), gradients(a_.gradients), steps(a_.steps), pcg_its(a_.pcg_its), mech_solves(a_.mech_solves),
        mech_its(a_.mech_its), ms(a_.ms_backward) {}
  ~AdjCountGuard() {
    a.gradients = gradients;
    a.steps = steps;
    a.pcg_its = pcg_its;
    a.mech_solves = mech_solves;
    a.mech_its = mech_its;
    a.ms_backward = ms;
  }
};

// The arguments of a Hessian call.  el (glims_adjoint_hessian_full, one GPU; nullptr otherwise): the E / nu directions,
// gradient rows and products.
struct ElasticSecond {
  const double *dir_E, *dir_nu;
  double *dE, *dnu, *hv_E, *hv_nu;
};
struct HessCall {
  int n_terms;
  const glims_misfit* terms;
  int P;
  const double *dir_D, *dir_rho, *dir_gamma, *dir_c0;
  double *J, *dD, *drho, *dgamma, *dc0, *hv_D, *hv_rho, *hv_gamma, *hv_c0, *stats;
  bool mem_checked = false;   // glims_adjoint_hessian_spmd has taken the memory verdict of all ranks
  const ElasticSecond* el = nullptr;
};

HessShape hessian_shape(glims_ctx* h, const HessCall& c) {
  HessShape s = adjoint_shape(h, c.n_terms, c.terms, c.P);
  s.el = c.el != nullptr;
  s.el_dirs = hess_el_dirs(s.el, s.any_u, c.el && (c.el->dir_E || c.el->dir_nu));
  s.el_sums = hess_el_sums(s.el, s.any_u, c.el && (c.el->hv_E || c.el->hv_nu));
  return s;
}

// Device memory of a Hessian call on top of the trajectory -- the sum of its buffer table (hessian_plan.h) -- and what is
// free now: the stored tangent-linear states dominate, 8 P B per node and recorded state (see glims_hip.h)
bool hessian_fits(const HessShape& s, std::string* why) {
  const size_t need = hessian_bytes(s);
  size_t fr = 0, tot = 0;
  GL_HIP(hipMemGetInfo(&fr, &tot));
  if (need <= fr) return true;
  *why = "glims_adjoint_hessian: " + std::to_string(s.P) + " directions over " + std::to_string(s.N + 1) +
         " recorded states need about " + std::to_string(need >> 20) + " MiB of device memory, " + std::to_string(fr >> 20) +
         " MiB are free";
  return false;
}

// Every device buffer of a Hessian call, allocated from the call's table: the first-order work vectors (filled by
// adjoint_setup), the P-column solver's, the direction tables and the second-order vectors.  Node vectors of the directions
// are stored column after column, [p][n_nodes].
struct HessMemory {
  const int P;
  const int64_t nn, nd;
  const std::vector<HessBuffer> table;
  AdjWork wk;
  MultiPcg mp;
  dvec<double> d_dir, d_dmat, d_dlame, d_dkap, d_dmat2, dKu, dKmu, hesums, hepart;
  dvec<double> dcs, nu, nu_next, dg, hrhs, hd, Mhd, hsums, hpart, hqcell, urhs, du, dmurhs, dmu, ue, uMe;

  HessMemory(glims_ctx* h, const HessShape& s)
      : P(s.P), nn(s.n_nodes), nd(s.n_nodes * s.dim), table(hessian_buffers(s)) {
    const std::pair<const char*, dvec<double>*> vecs[] = {
        {"dKu", &dKu}, {"dKmu", &dKmu}, {"hesums", &hesums}, {"hepart", &hepart}, {"dcs", &dcs}, {"nu", &nu},
        {"nu_next", &nu_next}, {"dg", &dg}, {"hrhs", &hrhs}, {"hd", &hd}, {"Mhd", &Mhd}, {"hsums", &hsums}, {"hpart", &hpart},
        {"hqcell", &hqcell}, {"urhs", &urhs}, {"du", &du}, {"dmurhs", &dmurhs}, {"dmu", &dmu}, {"ue", &ue}, {"uMe", &uMe},
        {"mp.X", &mp.X}, {"mp.B", &mp.B}, {"mp.R", &mp.R}, {"mp.Pv", &mp.Pv}, {"mp.Q", &mp.Q}, {"mp.part", &mp.part},
        {"mp.part2", &mp.part2}, {"mp.sendbuf", &mp.sendbuf}, {"mp.rows", &mp.rows}};
    for (const auto& v : vecs) take(h, table, v.first, *v.second);
    // written before they are read: the direction tables (upload_directions) and the solver's scalars (mp_solve_t)
    const std::pair<const char*, dvec<double>*> filled[] = {{"d_dir", &d_dir}, {"d_dmat", &d_dmat}, {"d_dlame", &d_dlame},
                                                            {"d_dkap", &d_dkap}, {"d_dmat2", &d_dmat2}, {"mp.sc", &mp.sc}};
    for (const auto& v : filled) take(h, table, v.first, *v.second, false);
    take(h, table, "mp.done", mp.done, false);
    take(h, table, "mp.its", mp.its, false);
    take(h, table, "mp.flags", mp.flags, false);
  }
  void upload_directions(glims_ctx* h, const HessDirections& d) {
    const std::pair<dvec<double>*, const std::vector<double>*> tabs[] = {
        {&d_dir, &d.dir}, {&d_dmat, &d.dmat}, {&d_dlame, &d.dlame}, {&d_dkap, &d.dkap}, {&d_dmat2, &d.dmat2}};
    for (const auto& t : tabs) {
      if (t.first->n != t.second->size()) throw std::logic_error("adjoint: a direction table and its buffer differ in size");
      t.first->upload(*t.second, h->st);
    }
  }
  double* col(dvec<double>& v, int p) const { return v.p + (size_t)p * nn; }                 // column p of nu, dg, hrhs ...
  double* dc_of(int step, int p) const { return dcs.p + ((size_t)step * P + p) * nn; }       // dc_step of direction p
  double* hsums_of(int p) const { return hsums.p + (size_t)p * GL_MAX_LABELS * 3; }
  double* hesums_of(int p) const { return hesums.p + (size_t)p * GL_MAX_LABELS * 2; }
  const double* dgamma_of(int p) const { return d_dir.p + ((size_t)p * 3 + 2) * GL_MAX_LABELS; }
  const double* dmat_of(const dvec<double>& t, int p) const { return t.p + (size_t)p * 5 * GL_MAX_LABELS; }
};

// The second-order work of a Hessian call, phase by phase, between the parts of gradient_t's backward sweep (BackwardSweep:
// J and the gradient keep its bits, which tests/test_gpu_adjoint_hessian.py checks).  Every phase stops the call by setting
// sw.status.
// Partitioned handles: dc_n, nu_n, du and dmu exchange their ghosts after their solves, hd and ue before the mass product,
// the per-label sums count a cell on one rank (AdjointState::counted) and are gathered with the gradient's.
// el: the sweep runs the gradient's E / nu pass (mode 2) as glims_adjoint_gradient_full does; with a direction in E / nu
// (el_dirs) du and dmu take -dK u_k and -dK mu_k on their right-hand sides, dG carries its E / nu part, and k_hesens sums the
// E / nu rows.  Without one, every launch of the other outputs is the one glims_adjoint_hessian issues: the same bits.
template <int D>
struct HessianSweep {
  glims_ctx* h;
  const HessCall& call;
  const HessShape& s;
  HessMemory& m;
  BackwardSweep<D>& sw;
  AdjWork& wk;
  const DevPattern& pt;
  const int P, L, N;
  const int64_t n, nn, nd;
  const double dt;
  const uint8_t *fxc, *counted;
  int64_t tlm_its = 0, soa_its = 0, extra_mech = 0;

  HessianSweep(glims_ctx* h_, const HessCall& c, const HessShape& s_, HessMemory& m_, BackwardSweep<D>& sw_)
      : h(h_), call(c), s(s_), m(m_), sw(sw_), wk(m_.wk), pt(h_->pat), P(s_.P), L(s_.n_labels), N(s_.N), n(h_->n_own),
        nn(m_.nn), nd(m_.nd), dt(h_->opt.dt), fxc(sw_.fxc), counted(s_.world > 1 ? h_->adj.counted.p : nullptr) {}

  // ghosts of P vectors stored column after column (no-ops on one GPU)
  void exchange_cols(double* v) {
    for (int p = 0; s.world > 1 && p < P; ++p) gl_halo_exchange(h, v + (size_t)p * nn, 1);
  }
  // y = M x (+ add); fixed: the rows of the constrained nodes are left out
  void mass_col(const double* x, const double* add, double* y, const uint8_t* fixed) {
    gl_launch_spmv(h, h->st, pt.n_slices, nullptr, h->vM.p, x, y, fixed, add, nullptr, nullptr, 0, nullptr);
  }
  // 0 on the constrained nodes of every column of v
  void zero_fixed_cols(double* v) {
    for (int p = 0; fxc && p < P; ++p) {
      hipLaunchKernelGGL(k_zero_fixed, dim3(grid_of(n)), dim3(256), 0, h->st, n, fxc, v + (size_t)p * nn, (const double*)nullptr);
      GL_CHECK_LAUNCH();
    }
  }
  template <int MODE>
  void hess_rows(const double* c, const double* lam, const double* dc) {
    if (h->dten.p)   // a tensor field (glims_set_diffusion_tensor)
      hipLaunchKernelGGL((k_hess_rows<D, MODE, 1, const double*>), dim3(grid_of(n)), dim3(256), 0, h->st, n, P, nn,
                         pt.cslice_ptr.p, pt.cslots.p, pt.celem.p, pt.diag_k.p, h->adj.cell_nodes.p, h->egeo.p, h->label.p,
                         h->mat.p, m.d_dir.p, dt, c, lam, dc, m.hrhs.p, (const double*)h->dten.p);
    else
      hipLaunchKernelGGL((k_hess_rows<D, MODE>), dim3(grid_of(n)), dim3(256), 0, h->st, n, P, nn, pt.cslice_ptr.p, pt.cslots.p,
                         pt.celem.p, pt.diag_k.p, h->adj.cell_nodes.p, h->egeo.p, h->label.p, h->mat.p, m.d_dir.p, dt, c, lam, dc,
                         m.hrhs.p);
    GL_CHECK_LAUNCH();
  }
  // mode 1 of the sensitivity pass into the directions' own qcell and partials: qcell of every cell, into `sums` (if any) the
  // cells this rank counts
  void gt_pass(const double* mat, const double* x, const double* v, double* sums) {
    sens_pass<D>(h, 1, mat, x, v, counted, m.hqcell.p, m.hpart.p, sums, 3, 2);
  }
  void gt_rows(double* dgp) {   // dg_p += the rows' sums of hqcell
    hipLaunchKernelGGL(k_gt_rows, dim3(grid_of(n)), dim3(256), 0, h->st, n, pt.cslice_ptr.p, pt.celem.p, m.hqcell.p, dgp);
    GL_CHECK_LAUNCH();
  }

  // A(c_n) dc_n = M dc_{n-1} - dt sum_t dD_t K_t c_n - dt sum_t drho_t int_t (c_n^2 - c_n) phi, all directions.
  // Reads traj[step], dcs[step - 1], d_dir; writes the swapped-in A(c_n), hrhs, dcs[step].
  void tangent_linear_step(int step) {
    gl_halo_exchange(h, h->adj.traj[step]->p, 1);   // (as BackwardSweep::begin_step)
    const double* c = h->adj.traj[step]->p;
    GL_HIP(hipMemsetAsync(wk.tmp.p, 0, (size_t)nn * sizeof(double), h->st));
    gl_rd_assemble(h, c, wk.tmp.p, nullptr, wk.w.p, nullptr, h->partials.p);
    for (int p = 0; p < P; ++p) mass_col(m.dc_of(step - 1, p), nullptr, m.col(m.hrhs, p), fxc);
    hess_rows<0>(c, nullptr, nullptr);
    zero_fixed_cols(m.hrhs.p);
    // warm start from dc_{n-1} (its constrained entries -- dc_0 may have some -- start at 0)
    GL_HIP(hipMemcpyAsync(m.dc_of(step, 0), m.dc_of(step - 1, 0), (size_t)P * nn * sizeof(double), hipMemcpyDeviceToDevice,
                          h->st));
    zero_fixed_cols(m.dc_of(step, 0));
    sw.status = rd_solve_cols(h, wk, m.mp, fxc, sw.rd_mg, sw.rd_deg, P, m.hrhs.p, m.dc_of(step, 0), nn, &tlm_its);
    // the solve updates the owned rows: the next step's M dc, the row and cell passes of the second sweep read the ghosts
    if (sw.status == GLIMS_OK) exchange_cols(m.dc_of(step, 0));
  }

  // After a concentration term, while wk.Me holds M (h - t):  dg_p += w (h' M(h' dc_p) + h'' M(h - t) dc_p).
  // Reads dcs[step], wk.Me; writes hd, Mhd, dg.
  void concentration_second(int step, const double* c, const glims_misfit& tm) {
    for (int p = 0; p < P; ++p) {
      hipLaunchKernelGGL(k_misfit_dir, dim3(grid_of(n)), dim3(256), 0, h->st, n, tm.kind, tm.level, tm.smooth, c,
                         m.dc_of(step, p), m.hd.p);
      GL_CHECK_LAUNCH();
      gl_halo_exchange(h, m.hd.p, 1);
      mass_apply(h, m.hd.p, m.Mhd.p);
      hipLaunchKernelGGL(k_misfit_second, dim3(grid_of(n)), dim3(256), 0, h->st, n, tm.kind, tm.level, tm.smooth, tm.weight,
                         c, m.dc_of(step, p), wk.Me.p, m.Mhd.p, m.col(m.dg, p));
      GL_CHECK_LAUNCH();
    }
  }

  // dK_p u_k (u_k with its Dirichlet values: the lifting term is differentiated too) and dK_p mu_k into dKu, dKmu
  void dkel_products() {
    for (const auto& vy : {std::make_pair((const double*)wk.uk.p, m.dKu.p), std::make_pair((const double*)wk.mu.p, m.dKmu.p)}) {
      hipLaunchKernelGGL(k_dkel_rows<D>, dim3(grid_of(n)), dim3(256), 0, h->st, n, P, nd, pt.cslice_ptr.p, pt.cslots.p,
                         pt.celem.p, pt.diag_k.p, h->adj.cell_nodes.p, h->egeo.p, h->label.p, m.d_dlame.p, vy.first, vy.second);
      GL_CHECK_LAUNCH();
    }
  }
  // du = K_el^-1 (G dc + sum_t dgamma_t G_t c), with el_dirs G dc + dG c - dK u_k: urhs, then du with current ghosts
  bool du_solve(int step, const double* c, int p) {
    const auto kern = s.el_dirs ? k_gdir_rows<D, true> : k_gdir_rows<D, false>;
    hipLaunchKernelGGL(kern, dim3(grid_of(n)), dim3(256), 0, h->st, n, pt.cslice_ptr.p, pt.cslots.p, pt.celem.p, pt.diag_k.p,
                       h->adj.cell_nodes.p, h->egeo.p, h->label.p, h->mat.p, m.dgamma_of(p),
                       s.el_dirs ? m.d_dkap.p + (size_t)p * GL_MAX_LABELS : (const double*)nullptr,
                       s.el_dirs ? m.dKu.p + (size_t)p * nd : (const double*)nullptr, c, m.dc_of(step, p), m.urhs.p);
    GL_CHECK_LAUNCH();
    int64_t its = 0;
    sw.status = solve_elastic(h, wk, m.urhs.p, m.du.p, nullptr, 1e-12, &its);
    if (sw.status != GLIMS_OK) return false;
    gl_halo_exchange(h, m.du.p, D);
    return true;
  }
  // dmu = K_el^-1 (sum w M_vec du + sum P^T R2(du)) (0 on the constrained dofs), with el_dirs - dK mu_k: dmurhs through ue,
  // uMe and the samplers' staging, then dmu with current ghosts
  bool dmu_solve(int step, int p) {
    GL_HIP(hipMemsetAsync(m.dmurhs.p, 0, (size_t)nd * sizeof(double), h->st));
    for (int k = 0; k < call.n_terms; ++k) {
      const glims_misfit& tm = call.terms[k];
      if (tm.step != step || tm.kind != GLIMS_MISFIT_U_L2) continue;
      for (int comp = 0; comp < D; ++comp) {
        hipLaunchKernelGGL(k_component, dim3(grid_of(n)), dim3(256), 0, h->st, n, D, comp, m.du.p, (const double*)nullptr,
                           m.ue.p);
        GL_CHECK_LAUNCH();
        gl_halo_exchange(h, m.ue.p, 1);
        mass_apply(h, m.ue.p, m.uMe.p);
        hipLaunchKernelGGL(k_add_component, dim3(grid_of(n)), dim3(256), 0, h->st, n, D, comp, tm.weight, m.uMe.p, m.dmurhs.p);
        GL_CHECK_LAUNCH();
      }
    }
    // the stored displacement image terms of the step, in list order: dmurhs += P^T R2 of this direction's du.  The call holds
    // one tangent du at a time, so the P-column kernel runs with one column per direction.
    for (const GlDisplacementImageTerm* t : h->uimg_terms)
      if (t->step == step) gl_displacement_image_misfit_second(h, *t, m.du.p, 1, nd, m.dmurhs.p);
    if (s.el_dirs) {   // - dK mu_k
      hipLaunchKernelGGL(k_sub, dim3(grid_of(n * D)), dim3(256), 0, h->st, n * D, m.dKmu.p + (size_t)p * nd, m.dmurhs.p);
      GL_CHECK_LAUNCH();
    }
    int64_t its = 0;
    sw.status = solve_elastic(h, wk, m.dmurhs.p, m.dmu.p, nullptr, 1e-12, &its);
    if (sw.status != GLIMS_OK) return false;
    gl_halo_exchange(h, m.dmu.p, D);   // qcell of the cells at the cut
    return true;
  }
  // dg_p += G^T dmu + sum_t dgamma_t G_t^T mu (+ the E / nu part of dG^T mu);  H_gamma_t += dmu^T G_t c + mu^T G_t dc
  void gt_contributions(int step, const double* c, int p) {
    gt_pass(h->mat.p, c, m.dmu.p, m.hsums_of(p));
    gt_rows(m.col(m.dg, p));
    gt_pass(h->mat.p, m.dc_of(step, p), wk.mu.p, m.hsums_of(p));
    gt_pass(m.dmat_of(m.d_dmat, p), c, wk.mu.p, nullptr);
    gt_rows(m.col(m.dg, p));
    if (s.el_dirs) {   // gamma_t (2 dm_t + d dl_t) |T|/(d+1) div mu per cell, then the rows
      gt_pass(m.dmat_of(m.d_dmat2, p), c, wk.mu.p, nullptr);
      gt_rows(m.col(m.dg, p));
    }
  }
  // A_t(dmu, u) + A_t(mu, du), B_t(dmu, u) + B_t(mu, du) of step k (u_k's ghosts: coupling_adjoint exchanged them)
  void elastic_sums(int p) {
    for (int l0 = 0; l0 < L; l0 += GL_ADJ_LT) {
      hipLaunchKernelGGL(k_hesens<D>, dim3(sens_blocks(h)), dim3(256), 0, h->st, h->n_cells, l0, h->adj.cell_nodes.p, h->egeo.p,
                         h->label.p, wk.uk.p, wk.mu.p, m.du.p, m.dmu.p, counted, m.hepart.p);
      GL_CHECK_LAUNCH();
      hipLaunchKernelGGL(k_sens_final, dim3(1), dim3(1024), 0, h->st, sens_blocks(h), l0, L, 2, 0, m.hepart.p, m.hesums_of(p));
      GL_CHECK_LAUNCH();
    }
  }
  // The displacement part of a step that has one, after the coupling adjoint (wk.uk, wk.mu): per direction two elastic solves,
  // their share of dg and of the gamma (and E / nu) sums.  Reads dcs[step]; writes dg, hsums, hesums.
  bool coupling_second(int step, const double* c) {
    if (s.el_dirs) dkel_products();
    for (int p = 0; p < P; ++p) {
      if (!du_solve(step, c, p) || !dmu_solve(step, p)) return false;
      extra_mech += 2;
      gt_contributions(step, c, p);
      if (s.el_sums) elastic_sums(p);
    }
    return true;
  }

  // Step 0: dJ/dc_0, and (H dm)_c0 = M nu_1 + dg_0 of every direction through hrhs
  void c0_rows() {
    if (call.dc0) sw.c0_output(call.dc0);
    for (int p = 0; call.hv_c0 && p < P; ++p) {
      double* y = m.col(m.hrhs, p);
      if (N > 0) mass_col(m.col(m.nu_next, p), m.col(m.dg, p), y, nullptr);
      else GL_HIP(hipMemcpyAsync(y, m.col(m.dg, p), (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->st));
      download_permuted(h, wk, y, call.hv_c0 + (size_t)p * nn);
    }
  }

  // nu_n: A(c_n) nu_n = M nu_{n+1} + dg_n - 2 dt sum_t rho_t int_t dc_n lam_n phi - dt sum_t dD_t K_t lam_n
  //                     - dt sum_t drho_t int_t (2 c_n - 1) lam_n phi,   PCG from nu_{n+1}; then the (H dm)_{D,rho} sums of step n.
  // After lambda_solve (wk.lam, A(c_n) in the swapped-in buffers).  Reads dg, dcs[step], nu_next; writes hrhs, nu (which
  // becomes nu_next), hsums.
  void second_adjoint_step(int step, const double* c) {
    for (int p = 0; p < P; ++p) mass_col(m.col(m.nu_next, p), m.col(m.dg, p), m.col(m.hrhs, p), fxc);
    hess_rows<1>(c, wk.lam.p, m.dc_of(step, 0));
    zero_fixed_cols(m.hrhs.p);
    GL_HIP(hipMemcpyAsync(m.nu.p, m.nu_next.p, (size_t)P * nn * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    sw.status = rd_solve_cols(h, wk, m.mp, fxc, sw.rd_mg, sw.rd_deg, P, m.hrhs.p, m.nu.p, nn, &soa_its);
    if (sw.status == GLIMS_OK) exchange_cols(m.nu.p);   // k_hsens and M nu_{n+1} read the ghosts
    for (int p = 0; p < P && sw.status == GLIMS_OK; ++p)
      for (int l0 = 0; l0 < L; l0 += GL_ADJ_LT) {
        if (h->dten.p)
          hipLaunchKernelGGL((k_hsens<D, 1, const double*>), dim3(sens_blocks(h)), dim3(256), 0, h->st, h->n_cells, l0,
                             h->adj.cell_nodes.p, h->egeo.p, h->label.p, c, wk.lam.p, m.dc_of(step, p), m.col(m.nu, p), counted,
                             m.hpart.p, (const double*)h->dten.p);
        else
          hipLaunchKernelGGL(k_hsens<D>, dim3(sens_blocks(h)), dim3(256), 0, h->st, h->n_cells, l0, h->adj.cell_nodes.p, h->egeo.p,
                             h->label.p, c, wk.lam.p, m.dc_of(step, p), m.col(m.nu, p), counted, m.hpart.p);
        GL_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_sens_final, dim3(1), dim3(1024), 0, h->st, sens_blocks(h), l0, L, 3, 0, m.hpart.p, m.hsums_of(p));
        GL_CHECK_LAUNCH();
      }
    std::swap(m.nu.p, m.nu_next.p);
  }

  // The gather of the per-label sums (every rank reaches it, also after a failed solve) and the rows of every output
  void label_outputs(const HessDirections& dirs) {
    const size_t LM = GL_MAX_LABELS;
    const std::vector<RowPart> lay = label_row_parts(L, s.el, P, s.el_sums);
    std::vector<double> sums((size_t)L * 3), hs((size_t)P * LM * 3), esums((size_t)L * 2, 0.0), hes((size_t)P * LM * 2, 0.0);
    gather_label_sums(h, {{lay[0], wk.sums.p, sums.data()}, {lay[1], wk.esums.p, esums.data()},
                          {lay[2], m.hsums.p, hs.data()}, {lay[3], m.hesums.p, hes.data()}},
                      hess_buffer(m.table, "gather").count);
    const ElasticSecond none = {}, &el = call.el ? *call.el : none;
    sw.write_labels(sums.data(), call.dD, call.drho, call.dgamma);
    if (call.el) write_elastic_labels(h->mat_host.data(), L, D, sums.data(), esums.data(), el.dE, el.dnu);
    hessian_label_rows(dirs, call.el != nullptr, dt, h->mat_host.data(), sums.data(), hs.data(), esums.data(), hes.data(),
                       call.hv_D, call.hv_rho, call.hv_gamma, el.hv_E, el.hv_nu);
    finish_tangent_sums(h, sw.status);
  }
};

// The tangent-linear sweep, then gradient_t's backward sweep with the second-order adjoint work of every direction between
// its parts (HessianSweep).  The guards' order matters: the counters, then the forward state, then the sweep (the lazy RD
// hierarchy is the ForwardGuard's to drop).
template <int D>
int hessian_t(glims_ctx* h, const HessCall& call) {
  const double t0 = omp_get_wtime();
  const HessShape shape = hessian_shape(h, call);
  if (!call.mem_checked) {
    std::string why;
    if (!hessian_fits(shape, &why)) throw glims_error(GLIMS_E_HIP, why);
  }
  const int P = shape.P, N = shape.N;
  const int64_t nn = shape.n_nodes;
  const ElasticSecond none = {}, &el = call.el ? *call.el : none;
  AdjCountGuard counts(h->adj);
  HessMemory mem(h, shape);
  AdjWork& wk = mem.wk;
  adjoint_setup<D>(h, mem.table, call.n_terms, call.terms, wk);
  const HessDirections dirs(P, shape.n_labels, D, h->mat_host.data(), call.dir_D, call.dir_rho, call.dir_gamma, el.dir_E,
                            el.dir_nu, shape.el_dirs);
  mem.upload_directions(h, dirs);
  for (int p = 0; call.dir_c0 && p < P; ++p) upload_permuted(h, wk, call.dir_c0 + (size_t)p * nn, 1, mem.dc_of(0, p));
  ForwardGuard guard(h, wk);
  BackwardSweep<D> sw(h, wk, call.n_terms, call.terms, shape.el);
  HessianSweep<D> hs(h, call, shape, mem, sw);
  if (call.dir_c0) hs.exchange_cols(mem.dcs.p);   // (the caller's ghost entries are not trusted; under the guard: glims_stats stay)
  // 1. the tangent-linear sweep
  for (int step = 1; step <= N && sw.status == GLIMS_OK; ++step) hs.tangent_linear_step(step);
  // 2. the first-order sweep with the second-order adjoint nu_n of every direction
  for (int step = N; step >= 0 && sw.status == GLIMS_OK; --step) {
    const double* c = sw.begin_step(step);
    GL_HIP(hipMemsetAsync(mem.dg.p, 0, (size_t)P * nn * sizeof(double), h->st));
    bool have_u = sw.nodal_terms(step, c, [&](const glims_misfit& tm) { hs.concentration_second(step, c, tm); });
    if (sw.status != GLIMS_OK) break;
    image_terms_of_step(h, step, c, wk.g.p, &sw.J, P, mem.dc_of(step, 0), nn, mem.dg.p);
    if (!h->uimg_terms.empty()) {   // (their second order: dmu_solve, from each direction's du)
      have_u = sw.displacement_image_terms(step, c, have_u);
      if (sw.status != GLIMS_OK) break;
    }
    gl_observable_terms_of_step(h, step, c, wk.g.p, &sw.J, P, mem.dc_of(step, 0), nn, mem.dg.p);
    if (have_u && !(sw.coupling_adjoint(c) && hs.coupling_second(step, c))) break;
    if (step == 0) {
      hs.c0_rows();
      break;
    }
    if (!sw.lambda_solve(c)) break;
    hs.second_adjoint_step(step, c);
    sw.end_step();
  }
  hs.label_outputs(dirs);
  *call.J = sw.J;
  if (call.stats) {
    call.stats[0] = (double)hs.tlm_its;
    call.stats[1] = (double)hs.soa_its;
    call.stats[2] = (double)hs.extra_mech;
    call.stats[3] = 1e3 * (omp_get_wtime() - t0);
  }
  return sw.status;
}

}  // namespace

const int32_t* gl_ensure_cell_nodes(glims_ctx* h) {
  if (h->dim == 2) build_cell_nodes<2>(h);
  else build_cell_nodes<3>(h);
  return h->adj.cell_nodes.p;
}

void gl_adjoint_start(glims_ctx* h) {
  AdjointState& a = h->adj;
  a.clear();
  a.valid = false;
  a.why = "no trajectory recorded";
  GL_REQUIRE(h->have_state, "glims_adjoint_record before glims_set_state: c_0 is the current state");
  a.had_fixed = h->have_fixed_c;
  a.fixed0 = h->have_fixed_c ? h->fixed_c_host : std::vector<uint8_t>();
  a.recording = true;
  a.valid = true;
  gl_adjoint_after_step(h, GLIMS_OK);   // c_0
}

void gl_adjoint_after_step(glims_ctx* h, int status) {
  AdjointState& a = h->adj;
  if (status != GLIMS_OK) {
    a.invalidate("the recorded run has a failed step");
    return;
  }
  if (!a.valid) return;   // invalidated while recording: stays so until the next glims_adjoint_record / glims_set_state
  auto d = std::make_unique<dvec<double>>();
  try {
    d->alloc((size_t)h->n_nodes);
  } catch (const glims_error& e) {
    a.invalidate("device memory exhausted while recording the trajectory");
    throw glims_error(GLIMS_E_HIP, std::string("adjoint trajectory: step ") + std::to_string(a.traj.size()) +
                                       " does not fit in device memory (" + e.what() + "); the trajectory is dropped");
  }
  GL_HIP(hipMemcpyAsync(d->p, h->c.p, (size_t)h->n_nodes * sizeof(double), hipMemcpyDeviceToDevice, h->st));
  a.traj.push_back(std::move(d));
}

namespace {
// The argument and state checks of one rank (GLIMS_E_USAGE with the reason)
void check_gradient_call(glims_ctx* h, int n_terms, const glims_misfit* terms, const double* J,
                         const std::string& who = "glims_adjoint_gradient", bool second_order = false) {
  const AdjointState& a = h->adj;
  GL_REQUIRE(J, who + ": null J");
  GL_REQUIRE(n_terms >= 0 && (n_terms == 0 || terms), who + ": bad term list");
  GL_REQUIRE(h->is_setup, who + " before glims_setup");
  GL_REQUIRE(a.valid && !a.traj.empty(), who + ": no valid trajectory (" + a.why + ")");
  if (a.had_fixed != h->have_fixed_c || (a.had_fixed && a.fixed0 != h->fixed_c_host))
    throw glims_error(GLIMS_E_USAGE, who + ": the Dirichlet node set changed since recording started");
  const int64_t N = (int64_t)a.traj.size() - 1;
  for (int k = 0; k < n_terms; ++k) {
    const glims_misfit& t = terms[k];
    GL_REQUIRE(t.step >= 0 && t.step <= N, who + ": term " + std::to_string(k) + " observes step " +
                                               std::to_string(t.step) + ", the recording has steps 0.." + std::to_string(N));
    GL_REQUIRE(t.kind >= GLIMS_MISFIT_C_L2 && t.kind <= GLIMS_MISFIT_U_L2, who + ": unknown misfit kind");
    GL_REQUIRE(t.target, who + ": null target");
    GL_REQUIRE(std::isfinite(t.weight), who + ": non-finite weight");
    GL_REQUIRE(t.kind != GLIMS_MISFIT_C_THRESH || (t.smooth > 0.0 && std::isfinite(t.level)),
               who + ": threshold term needs smooth > 0");
    GL_REQUIRE(t.kind != GLIMS_MISFIT_U_L2 || h->have_mech,
               who + ": a displacement term needs glims_setup(with_mechanics=1)");
  }
  for (size_t k = 0; k < h->img_terms.size(); ++k)
    GL_REQUIRE(h->img_terms[k]->step <= N, who + ": stored image term " + std::to_string(k) + " observes step " +
                                               std::to_string(h->img_terms[k]->step) + ", the recording has steps 0.." +
                                               std::to_string(N));
  for (size_t k = 0; k < h->uimg_terms.size(); ++k) {
    GL_REQUIRE(h->uimg_terms[k]->step <= N, who + ": stored displacement image term " + std::to_string(k) + " observes step " +
                                                std::to_string(h->uimg_terms[k]->step) + ", the recording has steps 0.." +
                                                std::to_string(N));
    GL_REQUIRE(h->have_mech, who + ": a stored displacement image term needs glims_setup(with_mechanics=1)");
  }
  for (size_t k = 0; k < h->dimg_terms.size(); ++k)
    GL_REQUIRE(h->dimg_terms[k]->step <= N, who + ": stored deformed image term " + std::to_string(k) + " observes step " +
                                                std::to_string(h->dimg_terms[k]->step) + ", the recording has steps 0.." +
                                                std::to_string(N));
  gl_observable_terms_check(h, N, who, second_order);
}
}  // namespace

int gl_adjoint_gradient(glims_ctx* h, int n_terms, const glims_misfit* terms, double* J, double* dD, double* drho,
                        double* dgamma, double* dc0, double* dE, double* dnu) {
  if (h->world <= 1) {
    check_gradient_call(h, n_terms, terms, J);
  } else {
    // Collective: a rank that refused alone would leave the others waiting in the first halo exchange of the sweep.  Every
    // rank's verdict goes through one all-reduce ([2][world] flags, 1 = refused), and every rank returns the same status.
    std::string why;
    try {
      check_gradient_call(h, n_terms, terms, J);
    } catch (const glims_error& e) {
      if (e.code != GLIMS_E_USAGE) throw;
      why = e.what();
    }
    // (second row: whether the rank asks for dJ/dE or dJ/dnu -- the size of the final all-reduce follows it; third and fourth:
    // the stored image terms, their count and a checksum of their steps -- the all-reduces of the sweep follow them)
    std::vector<double> flag((size_t)h->world * 5, 0.0);
    flag[(size_t)h->rank] = why.empty() ? 0.0 : 1.0;
    flag[(size_t)(h->world + h->rank)] = (dE || dnu) ? 1.0 : 0.0;
    uint64_t sum_steps = 0;
    for (const GlImageTerm* t : h->img_terms) sum_steps = (sum_steps * 1000003ull + (uint64_t)t->step + 1) & ((1ull << 52) - 1);
    flag[(size_t)(2 * h->world + h->rank)] = (double)h->img_terms.size();
    flag[(size_t)(3 * h->world + h->rank)] = (double)sum_steps;
    flag[(size_t)(4 * h->world + h->rank)] = (double)h->dtan.K;   // fifth: the stored tangent fields -- their gather follows the sweep
    dvec<double> d_flag;
    d_flag.upload(flag, h->st);
    gl_allreduce_bulk(h, d_flag.p, flag.size());
    GL_HIP(hipMemcpyAsync(flag.data(), d_flag.p, flag.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
    std::string refused;
    for (int r = 0; r < h->world; ++r)
      if (flag[(size_t)r] != 0.0) refused += (refused.empty() ? "" : ", ") + std::to_string(r);
    if (!why.empty()) throw glims_error(GLIMS_E_USAGE, why + " (ranks that refused: " + refused + ")");
    if (!refused.empty())
      throw glims_error(GLIMS_E_USAGE, "glims_adjoint_gradient: refused on rank(s) " + refused + " (see their messages)");
    for (int r = 1; r < h->world; ++r)
      if (flag[(size_t)(h->world + r)] != flag[(size_t)h->world])
        throw glims_error(GLIMS_E_USAGE, "glims_adjoint_gradient_full: the ranks disagree on asking for dJ_dE / dJ_dnu");
    for (int r = 1; r < h->world; ++r)
      if (flag[(size_t)(2 * h->world + r)] != flag[(size_t)(2 * h->world)] ||
          flag[(size_t)(3 * h->world + r)] != flag[(size_t)(3 * h->world)])
        throw glims_error(GLIMS_E_USAGE, "glims_adjoint_gradient: the ranks disagree on the stored image terms (their count "
                                         "or the steps they observe)");
    for (int r = 1; r < h->world; ++r)
      if (flag[(size_t)(4 * h->world + r)] != flag[(size_t)(4 * h->world)])
        throw glims_error(GLIMS_E_USAGE, "glims_adjoint_gradient: the ranks disagree on the number of stored tangent fields "
                                         "(glims_set_diffusion_tensor_tangents)");
  }
  return h->dim == 2 ? gradient_t<2>(h, n_terms, terms, J, dD, drho, dgamma, dc0, dE, dnu)
                     : gradient_t<3>(h, n_terms, terms, J, dD, drho, dgamma, dc0, dE, dnu);
}

namespace {
int hessian_dispatch(glims_ctx* h, const HessCall& call) {
  return h->dim == 2 ? hessian_t<2>(h, call) : hessian_t<3>(h, call);
}
void check_n_dir(int n_dir, const std::string& who = "glims_adjoint_hessian") {
  GL_REQUIRE(n_dir >= 1 && n_dir <= GL_HESS_MAXDIR, who + ": n_dir = " + std::to_string(n_dir) + ", 1.." +
                                                        std::to_string(GL_HESS_MAXDIR) + " directions per call");
}
}  // namespace

int gl_adjoint_hessian(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                       const double* dir_rho, const double* dir_gamma, const double* dir_c0, double* J, double* dD,
                       double* drho, double* dgamma, double* dc0, double* hv_D, double* hv_rho, double* hv_gamma,
                       double* hv_c0, double* stats) {
  // (every rank of a partitioned handle refuses alike: no collective is entered)
  GL_REQUIRE(h->world <= 1, "glims_adjoint_hessian: not available on partitioned handles (world > 1)");
  GL_REQUIRE(h->dimg_terms.empty(), "glims_adjoint_hessian: second order through the location of the stored deformed image "
                                    "terms is not built (a Hessian without them would be wrong): clear them with "
                                    "glims_adjoint_deformed_image_terms(h, 0, NULL) first");
  check_gradient_call(h, n_terms, terms, J, "glims_adjoint_hessian", true);
  check_n_dir(n_dir);
  return hessian_dispatch(h, {n_terms, terms, n_dir, dir_D, dir_rho, dir_gamma, dir_c0, J, dD, drho, dgamma, dc0, hv_D, hv_rho,
                              hv_gamma, hv_c0, stats});
}

int gl_adjoint_hessian_full(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                            const double* dir_rho, const double* dir_gamma, const double* dir_c0, const double* dir_E,
                            const double* dir_nu, double* J, double* dD, double* drho, double* dgamma, double* dc0, double* dE,
                            double* dnu, double* hv_D, double* hv_rho, double* hv_gamma, double* hv_c0, double* hv_E,
                            double* hv_nu, double* stats) {
  const std::string who = "glims_adjoint_hessian_full";
  // (every rank of a partitioned handle refuses alike, before any collective)
  GL_REQUIRE(h->world <= 1, who + ": not available on partitioned handles (world > 1): E / nu are first order there");
  GL_REQUIRE(h->dimg_terms.empty(), who + ": second order through the location of the stored deformed image terms is not "
                                          "built (a Hessian without them would be wrong): clear them with "
                                          "glims_adjoint_deformed_image_terms(h, 0, NULL) first");
  check_gradient_call(h, n_terms, terms, J, who, true);
  check_n_dir(n_dir, who);
  GL_REQUIRE(h->have_mech || !(dir_E || dir_nu || hv_E || hv_nu),
             who + ": dir_E / dir_nu / hv_E / hv_nu need glims_setup(with_mechanics=1)");
  const ElasticSecond el = {dir_E, dir_nu, dE, dnu, hv_E, hv_nu};
  return hessian_dispatch(h, {n_terms, terms, n_dir, dir_D, dir_rho, dir_gamma, dir_c0, J, dD, drho, dgamma, dc0, hv_D, hv_rho,
                              hv_gamma, hv_c0, stats, false, &el});
}

int gl_adjoint_hessian_spmd(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                            const double* dir_rho, const double* dir_gamma, const double* dir_c0, double* J, double* dD,
                            double* drho, double* dgamma, double* dc0, double* hv_D, double* hv_rho, double* hv_gamma,
                            double* hv_c0, double* stats) {
  if (h->world <= 1)
    return gl_adjoint_hessian(h, n_terms, terms, n_dir, dir_D, dir_rho, dir_gamma, dir_c0, J, dD, drho, dgamma, dc0, hv_D,
                              hv_rho, hv_gamma, hv_c0, stats);
  // Collective, as the partitioned gl_adjoint_gradient: every rank's verdict on its arguments and trajectory, its n_dir, the
  // NULL pattern of its direction arrays, its stored image terms and its memory verdict go through ONE all-reduce
  // ([7][world], the last row the number of stored tangent fields; zeros outside the own column) before any other collective; every rank returns the same status.
  const std::string who = "glims_adjoint_hessian_spmd";
  std::string why, why_mem;
  try {
    check_gradient_call(h, n_terms, terms, J, who);
    check_n_dir(n_dir);
  } catch (const glims_error& e) {
    if (e.code != GLIMS_E_USAGE) throw;
    why = e.what();
  }
  const HessCall call = {n_terms, terms, n_dir, dir_D, dir_rho, dir_gamma, dir_c0, J, dD, drho, dgamma, dc0, hv_D, hv_rho,
                         hv_gamma, hv_c0, stats, true};
  const bool fits = !why.empty() || hessian_fits(hessian_shape(h, call), &why_mem);
  const size_t w = (size_t)h->world, r0 = (size_t)h->rank;
  std::vector<double> flag(w * 7, 0.0);
  uint64_t sum_steps = 0;
  for (const GlImageTerm* t : h->img_terms) sum_steps = (sum_steps * 1000003ull + (uint64_t)t->step + 1) & ((1ull << 52) - 1);
  flag[r0] = why.empty() ? 0.0 : 1.0;
  flag[w + r0] = (double)n_dir;
  flag[2 * w + r0] = (dir_D ? 1.0 : 0.0) + (dir_rho ? 2.0 : 0.0) + (dir_gamma ? 4.0 : 0.0) + (dir_c0 ? 8.0 : 0.0);
  flag[3 * w + r0] = (double)h->img_terms.size();
  flag[4 * w + r0] = (double)sum_steps;
  flag[5 * w + r0] = fits ? 0.0 : 1.0;
  flag[6 * w + r0] = (double)h->dtan.K;
  dvec<double> d_flag;
  d_flag.upload(flag, h->st);
  gl_allreduce_bulk(h, d_flag.p, flag.size());
  GL_HIP(hipMemcpyAsync(flag.data(), d_flag.p, flag.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  auto ranks_with = [&](size_t row) {
    std::string s;
    for (size_t r = 0; r < w; ++r)
      if (flag[row * w + r] != 0.0) s += (s.empty() ? "" : ", ") + std::to_string(r);
    return s;
  };
  auto differs = [&](size_t row) {
    for (size_t r = 1; r < w; ++r)
      if (flag[row * w + r] != flag[row * w]) return true;
    return false;
  };
  const std::string refused = ranks_with(0);
  if (!why.empty()) throw glims_error(GLIMS_E_USAGE, why + " (ranks that refused: " + refused + ")");
  if (!refused.empty()) throw glims_error(GLIMS_E_USAGE, who + ": refused on rank(s) " + refused + " (see their messages)");
  if (differs(1)) throw glims_error(GLIMS_E_USAGE, who + ": the ranks disagree on n_dir");
  if (differs(2))
    throw glims_error(GLIMS_E_USAGE, who + ": the ranks disagree on which of dir_D / dir_rho / dir_gamma / dir_c0 are NULL");
  if (differs(3) || differs(4))
    throw glims_error(GLIMS_E_USAGE, who + ": the ranks disagree on the stored image terms (their count or the steps they "
                                         "observe)");
  if (differs(6))
    throw glims_error(GLIMS_E_USAGE, who + ": the ranks disagree on the number of stored tangent fields "
                                           "(glims_set_diffusion_tensor_tangents)");
  const std::string short_mem = ranks_with(5);
  if (!fits) throw glims_error(GLIMS_E_HIP, why_mem + " (ranks short of memory: " + short_mem + ")");
  if (!short_mem.empty()) throw glims_error(GLIMS_E_HIP, who + ": rank(s) " + short_mem + " are short of device memory");
  return hessian_dispatch(h, call);
}
