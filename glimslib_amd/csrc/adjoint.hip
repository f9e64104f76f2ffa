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

#include <algorithm>
#include <cmath>
#include <cstring>

#include <omp.h>

namespace {

inline unsigned grid_of(int64_t n, int bs = 256) { return (unsigned)std::max<int64_t>(1, (n + bs - 1) / bs); }

// labels per sensitivity launch: per-thread accumulators live in registers (LT x 3 doubles)
constexpr int GL_ADJ_LT = 8;
constexpr int GL_ADJ_BLOCKS = 2048;   // fixed grid of the sensitivity pass: the reduction order does not depend on the mesh

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
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
template <int D, int MODE>
__global__ __launch_bounds__(256) void k_sens(int64_t n_cells, int l0, const int32_t* __restrict__ cell_nodes,
                                              const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                              const double* __restrict__ mat, const double* __restrict__ c,
                                              const double* __restrict__ v, const uint8_t* __restrict__ counted,
                                              double* __restrict__ qcell, double* __restrict__ partials) {
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
#pragma unroll
        for (int a = 0; a < D; ++a) gg += gl[a] * gc[a];
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
  dvec<double> uk, murhs, mu, mr, mu_, mw, mp, ms, mKx;
  std::vector<dvec<double>*> targets;
  ~AdjWork() {
    for (auto* t : targets) delete t;
  }
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
    std::swap(h->dinv.p, wk.dinv.p);
    std::swap(h->dinv.n, wk.dinv.n);
  }
  ~ForwardGuard() {
    (void)hipStreamSynchronize(h->st);
    std::swap(h->vA.p, wk.vA.p);
    std::swap(h->vA.n, wk.vA.n);
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

// mode 0: (c, lambda) -> sums[l][0..1];  mode 1: (c, mu) -> sums[l][2] and qcell;  mode 2: (u, mu) -> esums[l][0..1]
template <int D>
void sens_pass(glims_ctx* h, int mode, const double* c, const double* v, AdjWork& wk) {
  const AdjointState& a = h->adj;
  const int nb = (int)std::min<int64_t>(GL_ADJ_BLOCKS, grid_of(h->n_cells));
  const uint8_t* counted = h->world > 1 ? a.counted.p : nullptr;
  for (int l0 = 0; l0 < h->n_labels; l0 += GL_ADJ_LT) {
    if (mode == 0)
      hipLaunchKernelGGL((k_sens<D, 0>), dim3(nb), dim3(256), 0, h->st, h->n_cells, l0, a.cell_nodes.p, h->egeo.p,
                         h->label.p, h->mat.p, c, v, counted, wk.qcell.p, wk.part.p);
    else if (mode == 1)
      hipLaunchKernelGGL((k_sens<D, 1>), dim3(nb), dim3(256), 0, h->st, h->n_cells, l0, a.cell_nodes.p, h->egeo.p,
                         h->label.p, h->mat.p, c, v, counted, wk.qcell.p, wk.part.p);
    else
      hipLaunchKernelGGL((k_sens<D, 2>), dim3(nb), dim3(256), 0, h->st, h->n_cells, l0, a.cell_nodes.p, h->egeo.p,
                         h->label.p, h->mat.p, c, v, counted, wk.qcell.p, wk.part.p);
    GL_CHECK_LAUNCH();
    if (mode < 2)
      hipLaunchKernelGGL(k_sens_final, dim3(1), dim3(1024), 0, h->st, nb, l0, h->n_labels, 3, mode == 0 ? 0 : 2, wk.part.p,
                         wk.sums.p);
    else
      hipLaunchKernelGGL(k_sens_final, dim3(1), dim3(1024), 0, h->st, nb, l0, h->n_labels, 2, 0, wk.part.p, wk.esums.p);
    GL_CHECK_LAUNCH();
  }
}

// K_el x = rhs with the Dirichlet dofs eliminated (x = xD there, or 0), to ||r|| <= rtol ||rhs||; the forward solve's
// displacement, its solve history and its hint are not touched (sibling of gl_solve_mechanics)
int solve_elastic(glims_ctx* h, AdjWork& wk, const double* rhs, double* x, const double* xD, double rtol, int64_t* its) {
  const int bs = h->dim;
  const int64_t nd = h->n_own * bs;
  const uint8_t* fx = h->have_fixed_u ? h->fixed_u.p : nullptr;
  const bool use_mg = h->opt.mech_precond == GLIMS_PRECOND_MULTIGRID;
  if (use_mg && !h->mg.ready) gl_mg_setup_mech(h);
  else if (!use_mg) gl_block_dinv(h);
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

template <int D>
int gradient_t(glims_ctx* h, int n_terms, const glims_misfit* terms, double* J_out, double* dD, double* drho,
               double* dgamma, double* dc0, double* dE, double* dnu) {
  AdjointState& a = h->adj;
  const int64_t n = h->n_own, nn = h->n_nodes, nd = nn * D;
  const int N = (int)a.traj.size() - 1;
  const double t0 = omp_get_wtime();
  AdjWork wk;
  const size_t ne = (size_t)h->pat.total_entries;
  wk.vA.alloc(ne);
  wk.dinv.alloc((size_t)nn);
  for (auto* v : {&wk.lam, &wk.lam_next, &wk.rhs, &wk.g, &wk.r, &wk.u, &wk.w, &wk.p, &wk.s, &wk.e, &wk.hp, &wk.Me, &wk.tmp})
    v->alloc_zero((size_t)nn, h->st);
  wk.qcell.alloc_zero((size_t)h->n_cells, h->st);
  wk.part.alloc_zero((size_t)GL_ADJ_BLOCKS * GL_ADJ_LT * 2, h->st);
  wk.sums.alloc_zero((size_t)GL_MAX_LABELS * 3, h->st);
  const bool elastic = dE || dnu;   // the E / nu pass runs only when asked for
  if (elastic) wk.esums.alloc_zero((size_t)GL_MAX_LABELS * 2, h->st);
  wk.stage.alloc_zero((size_t)nd, h->st);
  bool any_u = false;
  for (int k = 0; k < n_terms; ++k) any_u = any_u || terms[k].kind == GLIMS_MISFIT_U_L2;
  if (any_u)
    for (auto* v : {&wk.uk, &wk.murhs, &wk.mu, &wk.mr, &wk.mu_, &wk.mw, &wk.mp, &wk.ms, &wk.mKx})
      v->alloc_zero((size_t)nd, h->st);
  // targets -> internal numbering
  for (int k = 0; k < n_terms; ++k) {
    const int bs = terms[k].kind == GLIMS_MISFIT_U_L2 ? D : 1;
    auto* t = new dvec<double>();
    wk.targets.push_back(t);
    t->alloc_zero((size_t)nn * bs, h->st);
    GL_HIP(hipMemcpyAsync(wk.stage.p, terms[k].target, (size_t)nn * bs * sizeof(double), hipMemcpyHostToDevice, h->st));
    hipLaunchKernelGGL(k_perm, dim3(grid_of(nn * bs)), dim3(256), 0, h->st, nn, bs, h->d_old2new.p, wk.stage.p, t->p, 1);
    GL_CHECK_LAUNCH();
    GL_HIP(hipStreamSynchronize(h->st));   // the staging buffer is reused by the next target
  }
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
  ForwardGuard guard(h, wk);
  const uint8_t* fxc = h->have_fixed_c ? h->fixed_c.p : nullptr;
  const bool rd_mg = h->rd_precond_active == GLIMS_RD_PRECOND_MULTIGRID;
  if (rd_mg && !h->mg_rd.ready) gl_mg_setup_rd(h);
  const int rd_deg = h->opt.rd_mg_smooth > 0 ? h->opt.rd_mg_smooth : (h->mg_rd.lattice ? 1 : 3);
  double J = 0.0;
  int status = GLIMS_OK;
  for (int step = N; step >= 0 && status == GLIMS_OK; --step) {
    // (c_n as recorded: gl_step leaves the ghosts of c current, but the adjoint does not rely on it -- one exchange per step)
    gl_halo_exchange(h, a.traj[step]->p, 1);
    const double* c = a.traj[step]->p;
    GL_HIP(hipMemsetAsync(wk.g.p, 0, (size_t)nn * sizeof(double), h->st));
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
        continue;
      }
      if (!have_u) {   // u_k = K_el^-1 (G c_k + f), once per observed step
        gl_apply_G(h, c, wk.murhs.p);
        int64_t its = 0;
        status = solve_elastic(h, wk, wk.murhs.p, wk.uk.p, h->have_fixed_u ? h->m_uD.p : nullptr, 1e-12, &its);
        if (status != GLIMS_OK) break;
        GL_HIP(hipMemsetAsync(wk.murhs.p, 0, (size_t)nd * sizeof(double), h->st));
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
    if (status != GLIMS_OK) break;
    if (have_u) {   // mu = K_el^-1 dJ/du (0 on the constrained dofs); g += G^T mu; dJ/dgamma_t += mu^T G_t c
      int64_t its = 0;
      status = solve_elastic(h, wk, wk.murhs.p, wk.mu.p, nullptr, 1e-12, &its);
      if (status != GLIMS_OK) break;
      gl_halo_exchange(h, wk.mu.p, D);   // qcell of every local cell, also those whose other vertices are ghosts
      sens_pass<D>(h, 1, c, wk.mu.p, wk);
      hipLaunchKernelGGL(k_gt_rows, dim3(grid_of(n)), dim3(256), 0, h->st, n, h->pat.cslice_ptr.p, h->pat.celem.p,
                         wk.qcell.p, wk.g.p);
      GL_CHECK_LAUNCH();
      if (elastic) {   // A_t, B_t from u_k (its clamp values in place: solve_elastic wrote them) and mu_k
        gl_halo_exchange(h, wk.uk.p, D);   // PCG updates the owned rows: the cells at the cut read u_k at their ghosts
        sens_pass<D>(h, 2, wk.uk.p, wk.mu.p, wk);
      }
    }
    if (step == 0) {   // dJ/dc_0 = M lambda_1 + g_0
      if (dc0) {
        if (N > 0) gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vM.p, wk.lam_next.p, wk.rhs.p, nullptr, wk.g.p,
                                  nullptr, nullptr, 0, nullptr);
        else GL_HIP(hipMemcpyAsync(wk.rhs.p, wk.g.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->st));
        hipLaunchKernelGGL(k_perm, dim3(grid_of(nn)), dim3(256), 0, h->st, nn, 1, h->d_old2new.p, wk.rhs.p, wk.stage.p, 0);
        GL_CHECK_LAUNCH();
        GL_HIP(hipMemcpyAsync(dc0, wk.stage.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, h->st));
      }
      break;
    }
    // rhs = g_n + M lambda_{n+1}, 0 on the constrained nodes
    gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vM.p, wk.lam_next.p, wk.rhs.p, fxc, wk.g.p, nullptr, nullptr, 0,
                   nullptr);
    if (fxc) hipLaunchKernelGGL(k_zero_fixed, dim3(grid_of(n)), dim3(256), 0, h->st, n, fxc, wk.rhs.p, (const double*)nullptr);
    GL_CHECK_LAUNCH();
    // A(c_n) (and its diagonal) into the swapped-in buffers; the residual output is scratch (b = 0)
    GL_HIP(hipMemsetAsync(wk.tmp.p, 0, (size_t)nn * sizeof(double), h->st));
    gl_rd_assemble(h, c, wk.tmp.p, nullptr, wk.w.p, nullptr, h->partials.p);
    // lambda_n: PCG from lambda_{n+1}
    GL_HIP(hipMemcpyAsync(wk.lam.p, wk.lam_next.p, (size_t)nn * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    gl_launch_spmv(h, h->st, h->pat.n_slices, nullptr, h->vA.p, wk.lam.p, wk.w.p, fxc, nullptr, nullptr, nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_residual, dim3(grid_of(n)), dim3(256), 0, h->st, n, wk.rhs.p, wk.w.p, fxc, wk.r.p);
    GL_CHECK_LAUNCH();
    const double nb = std::sqrt(gl_dot(h, wk.rhs.p, wk.rhs.p, n));
    if (!std::isfinite(nb)) {
      status = GLIMS_NAN;
      break;
    }
    if (nb > 0.0) {
      int64_t its = 0;
      double res = 0.0;
      status = gl_pcg(h, wk.lam.p, wk.r.p, wk.u.p, wk.w.p, wk.p.p, wk.s.p, h->dinv.p, h->vA.p, fxc, 1,
                      rd_mg ? &h->mg_rd : nullptr, rd_deg, 1e-12 * nb, std::max(h->opt.cg_maxit, 20000), &its, &res);
      a.pcg_its += its;
      if (status != GLIMS_OK) break;
      gl_halo_exchange(h, wk.lam.p, 1);   // PCG updates the owned rows: the sensitivity pass and M lambda read the ghosts
      sens_pass<D>(h, 0, c, wk.lam.p, wk);
    } else {
      GL_HIP(hipMemsetAsync(wk.lam.p, 0, (size_t)nn * sizeof(double), h->st));
    }
    std::swap(wk.lam.p, wk.lam_next.p);
    a.steps++;
  }
  // sums: [L][3] (D, rho, gamma), then [L][2] (A, B) when the E / nu pass ran
  const size_t L3 = (size_t)h->n_labels * 3, L2 = elastic ? (size_t)h->n_labels * 2 : 0, W = L3 + L2;
  std::vector<double> sums(W);
  if (h->world <= 1) {
    GL_HIP(hipMemcpyAsync(sums.data(), wk.sums.p, L3 * sizeof(double), hipMemcpyDeviceToHost, h->st));
    if (L2) GL_HIP(hipMemcpyAsync(sums.data() + L3, wk.esums.p, L2 * sizeof(double), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
  } else {
    // Every rank's W = 3 (or 5) x n_labels sums, gathered by an all-reduce of [world][W] with zeros outside the own row
    // (x + 0 is exact: whatever order the transport adds in, every rank receives every row bit for bit), then added in rank
    // order on the host: the same bits on every rank.  Reached by every rank, also after a failed solve (the statuses are
    // global; `elastic` is the same on every rank: the caller's outputs are SPMD).
    dvec<double> all;
    all.alloc_zero(std::max<size_t>(1, W * h->world), h->st);
    if (L3) GL_HIP(hipMemcpyAsync(all.p + W * h->rank, wk.sums.p, L3 * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    if (L2) GL_HIP(hipMemcpyAsync(all.p + W * h->rank + L3, wk.esums.p, L2 * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    gl_allreduce_bulk(h, all.p, W * h->world);
    std::vector<double> rows(W * h->world);
    if (W) GL_HIP(hipMemcpyAsync(rows.data(), all.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
    for (size_t k = 0; k < W; ++k) {
      double t = 0.0;
      for (int r = 0; r < h->world; ++r) t += rows[W * r + k];
      sums[k] = t;
    }
  }
  const double dt = h->opt.dt;
  for (int l = 0; l < h->n_labels; ++l) {
    if (dD) dD[l] = -dt * sums[l * 3 + 0];
    if (drho) drho[l] = -dt * sums[l * 3 + 1];
    if (dgamma) dgamma[l] = sums[l * 3 + 2];
  }
  for (int l = 0; elastic && l < h->n_labels; ++l) {
    // C_t = sum_k int_t |T|/(d+1) div mu_k sum_a c_k,a = (dJ/dgamma sum) / (2 mu_t + d lam_t): mode 1's sum carries the factor
    const double* mh = h->mat_host.data();
    const double gam = mh[2 * GL_MAX_LABELS + l], mu = mh[3 * GL_MAX_LABELS + l], lam = mh[4 * GL_MAX_LABELS + l];
    const double E = mh[5 * GL_MAX_LABELS + l], nu = mh[6 * GL_MAX_LABELS + l];
    const double den = 2.0 * mu + D * lam;
    const double Ct = den != 0.0 ? sums[l * 3 + 2] / den : 0.0;
    const double At = sums[L3 + l * 2 + 0], Bt = sums[L3 + l * 2 + 1];
    const double q = (1.0 + nu) * (1.0 - 2.0 * nu);
    if (dE) {
      const double mp = 1.0 / (2.0 * (1.0 + nu)), lp = nu / q;
      dE[l] = gam * (2.0 * mp + D * lp) * Ct - (2.0 * mp * At + lp * Bt);
    }
    if (dnu) {
      const double mp = -E / (2.0 * (1.0 + nu) * (1.0 + nu)), lp = E * (1.0 + 2.0 * nu * nu) / (q * q);
      dnu[l] = gam * (2.0 * mp + D * lp) * Ct - (2.0 * mp * At + lp * Bt);
    }
  }
  *J_out = J;
  a.gradients++;
  a.ms_backward += 1e3 * (omp_get_wtime() - t0);
  return status;
}

}  // namespace

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
  auto* d = new dvec<double>();
  try {
    d->alloc((size_t)h->n_nodes);
  } catch (const glims_error& e) {
    delete d;
    a.invalidate("device memory exhausted while recording the trajectory");
    throw glims_error(GLIMS_E_HIP, std::string("adjoint trajectory: step ") + std::to_string(a.traj.size()) +
                                       " does not fit in device memory (" + e.what() + "); the trajectory is dropped");
  }
  GL_HIP(hipMemcpyAsync(d->p, h->c.p, (size_t)h->n_nodes * sizeof(double), hipMemcpyDeviceToDevice, h->st));
  a.traj.push_back(d);
}

namespace {
// The argument and state checks of one rank (GLIMS_E_USAGE with the reason)
void check_gradient_call(glims_ctx* h, int n_terms, const glims_misfit* terms, const double* J) {
  const AdjointState& a = h->adj;
  GL_REQUIRE(J, "glims_adjoint_gradient: null J");
  GL_REQUIRE(n_terms >= 0 && (n_terms == 0 || terms), "glims_adjoint_gradient: bad term list");
  GL_REQUIRE(h->is_setup, "glims_adjoint_gradient before glims_setup");
  GL_REQUIRE(a.valid && !a.traj.empty(), "glims_adjoint_gradient: no valid trajectory (" + a.why + ")");
  if (a.had_fixed != h->have_fixed_c || (a.had_fixed && a.fixed0 != h->fixed_c_host))
    throw glims_error(GLIMS_E_USAGE, "glims_adjoint_gradient: the Dirichlet node set changed since recording started");
  const int64_t N = (int64_t)a.traj.size() - 1;
  for (int k = 0; k < n_terms; ++k) {
    const glims_misfit& t = terms[k];
    GL_REQUIRE(t.step >= 0 && t.step <= N, "glims_adjoint_gradient: term " + std::to_string(k) + " observes step " +
                                               std::to_string(t.step) + ", the recording has steps 0.." + std::to_string(N));
    GL_REQUIRE(t.kind >= GLIMS_MISFIT_C_L2 && t.kind <= GLIMS_MISFIT_U_L2, "glims_adjoint_gradient: unknown misfit kind");
    GL_REQUIRE(t.target, "glims_adjoint_gradient: null target");
    GL_REQUIRE(std::isfinite(t.weight), "glims_adjoint_gradient: non-finite weight");
    GL_REQUIRE(t.kind != GLIMS_MISFIT_C_THRESH || (t.smooth > 0.0 && std::isfinite(t.level)),
               "glims_adjoint_gradient: threshold term needs smooth > 0");
    GL_REQUIRE(t.kind != GLIMS_MISFIT_U_L2 || h->have_mech,
               "glims_adjoint_gradient: a displacement term needs glims_setup(with_mechanics=1)");
  }
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
    // (second row: whether the rank asks for dJ/dE or dJ/dnu -- the size of the final all-reduce follows it)
    std::vector<double> flag((size_t)h->world * 2, 0.0);
    flag[(size_t)h->rank] = why.empty() ? 0.0 : 1.0;
    flag[(size_t)(h->world + h->rank)] = (dE || dnu) ? 1.0 : 0.0;
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
  }
  return h->dim == 2 ? gradient_t<2>(h, n_terms, terms, J, dD, drho, dgamma, dc0, dE, dnu)
                     : gradient_t<3>(h, n_terms, terms, J, dD, drho, dgamma, dc0, dE, dnu);
}
