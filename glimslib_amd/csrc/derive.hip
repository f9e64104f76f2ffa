// Derived fields of a recorded step on the device (glims_derive): the strain and stress tensors, pressure,
// von Mises stress, displacement norm, logistic growth, growth strain, total and growth-induced Jacobians and the concentration
// in the deformed configuration -- the fields of the PostProcess classes (simulation_helpers/postprocess.py is the statement in
// numpy).  Every field is the L2 projection M p = int f phi_i dx of an integrand f:
//   k_derive_cells   one thread per cell: the cell's constant times |T| / (d+1), or its local load vector from the quadrature rule
//   k_derive_rows    lane = row: the right-hand side summed along the row's incidence list, in list order (no atomics)
//   gl_project       the mass solves, component by component
#include "glims_internal.h"
#include "derive_quadrature.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace {

#define GL_CHECK_LAUNCH() GL_HIP(hipGetLastError())

constexpr int GL_DERIVE_BLOCKS = 2048;   // fixed grid of the cell pass (as the sensitivity pass of the adjoint)

__constant__ double c_q2_lam[GLIMS_DQ2_N][3] = GLIMS_DQ2_LAM;
__constant__ double c_q2_w[GLIMS_DQ2_N] = GLIMS_DQ2_W;
__constant__ double c_q3_lam[GLIMS_DQ3_N][4] = GLIMS_DQ3_LAM;
__constant__ double c_q3_w[GLIMS_DQ3_N] = GLIMS_DQ3_W;

// what the cell pass evaluates (the entry point's kinds map onto these; the second stages read first-stage P1 planes)
enum {
  CK_STRAIN = 0,   // eps(u_h)                              cell-constant, NS components
  CK_STRESS,       // 2 mu eps + lambda tr(eps) I           cell-constant, NS components
  CK_JTOT,         // det(I + grad u_h)                     cell-constant
  CK_VM,           // sqrt(3/2 dev:dev) of P1 planes [NS]   quadrature
  CK_UNORM,        // |u_h|                                 quadrature
  CK_LOGG,         // rho_T c_h (1 - c_h)                   quadrature
  CK_GAMC,         // gamma_T c_h                           quadrature
  CK_GROWJ,        // (1 + s_h)^d of a P1 plane s           quadrature
  CK_CDEF          // c_h (1 + gamma_T c_h)^d / J_T         quadrature
};
constexpr bool ck_is_const(int ck) { return ck == CK_STRAIN || ck == CK_STRESS || ck == CK_JTOT; }
constexpr bool ck_needs_u(int ck) {
  return ck == CK_STRAIN || ck == CK_STRESS || ck == CK_JTOT || ck == CK_UNORM || ck == CK_CDEF;
}

template <int D>
__device__ __forceinline__ double det_i_plus(const double (&G)[D][D]) {
  if constexpr (D == 2) {
    return (1.0 + G[0][0]) * (1.0 + G[1][1]) - G[0][1] * G[1][0];
  } else {
    const double a = 1.0 + G[0][0], e = 1.0 + G[1][1], i = 1.0 + G[2][2];
    return a * (e * i - G[1][2] * G[2][1]) - G[0][1] * (G[1][0] * i - G[1][2] * G[2][0]) +
           G[0][2] * (G[1][0] * G[2][1] - e * G[2][0]);
  }
}

// symmetric components in the order xx, yy, (zz,) xy, (xz, yz)
template <int D>
__device__ __forceinline__ void sym_of(const double (&G)[D][D], double* s) {
#pragma unroll
  for (int a = 0; a < D; ++a) s[a] = G[a][a];
  s[D] = 0.5 * (G[0][1] + G[1][0]);
  if constexpr (D == 3) {
    s[4] = 0.5 * (G[0][2] + G[2][0]);
    s[5] = 0.5 * (G[1][2] + G[2][1]);
  }
}

// Cell pass, one thread per cell over a fixed grid.  Reads the geometry record (1 + NV D doubles), NV vertex ids, the label, and
// gathers the vertex values it needs (f0: u [node][D], c [node] or P1 planes [NS][n_nodes]; c: the concentration where CK_CDEF
// needs both).  Writes planes out[k][n_cells]: the NC cell constants times |T| / (d+1), or the NV entries of the local load
// vector |T| sum_q w_q lambda_qa f_q.
template <int D, int CK>
__global__ __launch_bounds__(256) void k_derive_cells(int64_t n_cells, int64_t n_nodes, const int32_t* __restrict__ cell_nodes,
                                                      const double* __restrict__ egeo, const uint8_t* __restrict__ label,
                                                      const double* __restrict__ mat, const double* __restrict__ f0,
                                                      const double* __restrict__ c, double* __restrict__ out) {
  constexpr int NV = D + 1, GE = 1 + NV * D, NS = D * (D + 1) / 2;
  constexpr int NQ = D == 2 ? GLIMS_DQ2_N : GLIMS_DQ3_N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_cells; e += stride) {
    const double* g = egeo + e * GE;
    const double vol = g[0];
    const int lab = label[e];
    int nd[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) nd[m] = cell_nodes[e * NV + m];
    double G[D][D] = {};   // G[b][a] = d u_b / d x_a
    double uv[NV][D];
    if constexpr (ck_needs_u(CK)) {
      const double* u = f0;
#pragma unroll
      for (int m = 0; m < NV; ++m)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          uv[m][b] = u[(int64_t)nd[m] * D + b];
#pragma unroll
          for (int a = 0; a < D; ++a) G[b][a] += uv[m][b] * g[1 + m * D + a];
        }
    }
    if constexpr (ck_is_const(CK)) {
      const double wv = vol * (1.0 / NV);
      if constexpr (CK == CK_JTOT) {
        out[e] = det_i_plus<D>(G) * wv;
      } else {
        double s[NS];
        sym_of<D>(G, s);
        if constexpr (CK == CK_STRESS) {
          const double mu = mat[3 * GL_MAX_LABELS + lab], lam = mat[4 * GL_MAX_LABELS + lab];
          double tr = 0.0;
#pragma unroll
          for (int a = 0; a < D; ++a) tr += s[a];
#pragma unroll
          for (int k = 0; k < NS; ++k) s[k] = 2.0 * mu * s[k] + (k < D ? lam * tr : 0.0);
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) out[(int64_t)k * n_cells + e] = s[k] * wv;
      }
    } else {
      // vertex values of what is interpolated to the quadrature points
      constexpr int NF = CK == CK_VM ? NS : CK == CK_UNORM ? D : 1;
      double fv[NV][NF];
      if constexpr (CK == CK_VM) {
#pragma unroll
        for (int m = 0; m < NV; ++m)
#pragma unroll
          for (int k = 0; k < NS; ++k) fv[m][k] = f0[(int64_t)k * n_nodes + nd[m]];
      } else if constexpr (CK == CK_UNORM) {
#pragma unroll
        for (int m = 0; m < NV; ++m)
#pragma unroll
          for (int b = 0; b < D; ++b) fv[m][b] = uv[m][b];
      } else {
        const double* s = CK == CK_CDEF ? c : f0;
#pragma unroll
        for (int m = 0; m < NV; ++m) fv[m][0] = s[nd[m]];
      }
      double coef = 0.0, jt = 1.0;
      if constexpr (CK == CK_LOGG) coef = mat[1 * GL_MAX_LABELS + lab];
      if constexpr (CK == CK_GAMC || CK == CK_CDEF) coef = mat[2 * GL_MAX_LABELS + lab];
      if constexpr (CK == CK_CDEF) jt = det_i_plus<D>(G);
      double loc[NV];
#pragma unroll
      for (int a = 0; a < NV; ++a) loc[a] = 0.0;
      for (int q = 0; q < NQ; ++q) {
        double lq[NV];
#pragma unroll
        for (int a = 0; a < NV; ++a) lq[a] = D == 2 ? c_q2_lam[q][a] : c_q3_lam[q][a];
        const double wq = D == 2 ? c_q2_w[q] : c_q3_w[q];
        double v[NF];
#pragma unroll
        for (int k = 0; k < NF; ++k) {
          double t = 0.0;
#pragma unroll
          for (int a = 0; a < NV; ++a) t += lq[a] * fv[a][k];
          v[k] = t;
        }
        double fq;
        if constexpr (CK == CK_VM) {
          double tr = 0.0;
#pragma unroll
          for (int a = 0; a < D; ++a) tr += v[a];
          const double third = tr * (1.0 / 3.0);   // 1/3 in 2-D too: math_linear_elasticity.compute_deviatoric_stress_tensor
          double dd = 0.0;
#pragma unroll
          for (int a = 0; a < D; ++a) dd += (v[a] - third) * (v[a] - third);
#pragma unroll
          for (int k = D; k < NS; ++k) dd += 2.0 * v[k] * v[k];
          fq = sqrt(1.5 * dd);
        } else if constexpr (CK == CK_UNORM) {
          double dd = 0.0;
#pragma unroll
          for (int b = 0; b < D; ++b) dd += v[b] * v[b];
          fq = sqrt(dd);
        } else if constexpr (CK == CK_LOGG) {
          fq = coef * v[0] * (1.0 - v[0]);
        } else if constexpr (CK == CK_GAMC) {
          fq = coef * v[0];
        } else if constexpr (CK == CK_GROWJ) {
          const double t = 1.0 + v[0];
          fq = D == 2 ? t * t : t * t * t;
        } else {
          const double t = 1.0 + coef * v[0];
          fq = v[0] * (D == 2 ? t * t : t * t * t) / jt;
        }
        const double wf = wq * fq;
#pragma unroll
        for (int a = 0; a < NV; ++a) loc[a] += lq[a] * wf;
      }
#pragma unroll
      for (int a = 0; a < NV; ++a) out[(int64_t)a * n_cells + e] = vol * loc[a];
    }
  }
}

// Gather, lane = row: rhs[k][row] = sum over the row's incidences, in list order, of cellv[k][cell] (LOC = 0, NC components in
// one launch) or of cellv[a][cell] with a the row's position among the cell's vertices (LOC = 1).  Per incidence 4 B of cell id
// + NC gathered doubles (LOC: the NV vertex ids of the cell, one 16-byte load in 3-D, + 1 double).
template <int NV, int NC, int LOC>
__global__ __launch_bounds__(256) void k_derive_rows(int64_t n_own, int64_t n_nodes, int64_t n_cells,
                                                     const int64_t* __restrict__ cslice_ptr, const int32_t* __restrict__ celem,
                                                     const int32_t* __restrict__ cell_nodes, const double* __restrict__ cellv,
                                                     double* __restrict__ rhs) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0;
  for (int q = 0; q < clen; ++q) {
    const int32_t e = celem[cbase + (int64_t)q * GL_WAVE + lane];
    if (e < 0) continue;
    if constexpr (LOC) {
      int a = 0;
#pragma unroll
      for (int m = 1; m < NV; ++m)
        if (cell_nodes[(int64_t)e * NV + m] == (int32_t)row) a = m;
      acc[0] += cellv[(int64_t)a * n_cells + e];
    } else {
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] += cellv[(int64_t)k * n_cells + e];
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) rhs[(int64_t)k * n_nodes + row] = acc[k];
}

// nodal algebra: out = 1/3 (s_0 + .. + s_{d-1}) of the stress planes (pressure), or out = gamma c
__global__ void k_derive_pressure(int64_t n, int d, const double* __restrict__ s, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double tr = 0.0;
  for (int a = 0; a < d; ++a) tr += s[(int64_t)a * n + i];
  out[i] = 1.0 / 3.0 * tr;
}
__global__ void k_derive_scale(int64_t n, double gamma, const double* __restrict__ c, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = c[i] * gamma;
}

// internal -> caller's order: ext[o][k] = planes[k][new(o)] (FULL = 0), or the full tensor ext[o][a][b] from the symmetric planes (FULL = 1)
template <int D, int FULL>
__global__ void k_derive_out(int64_t n, int ncomp, const int32_t* __restrict__ old2new, const double* __restrict__ planes,
                             double* __restrict__ ext) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;
  const int64_t nw = old2new[o];
  if constexpr (FULL) {
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        const int k = a == b ? a : (D == 2 ? 2 : a + b + 2);   // (0,1) -> 3, (0,2) -> 4, (1,2) -> 5
        ext[(o * D + a) * D + b] = planes[(int64_t)k * n + nw];
      }
  } else {
    for (int k = 0; k < ncomp; ++k) ext[o * ncomp + k] = planes[(int64_t)k * n + nw];
  }
}
__global__ void k_derive_interleave(int64_t n, int ncomp, const double* __restrict__ planes, double* __restrict__ il) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * ncomp) return;
  const int64_t node = i / ncomp;
  il[i] = planes[(i - node * ncomp) * n + node];
}

template <int D, int CK>
void launch_cells(glims_ctx* h, const double* f0, const double* c) {
  DeriveState& ds = h->derive;
  constexpr int NS = D * (D + 1) / 2;
  ds.cellv.alloc((size_t)h->n_cells * (D + 1 > NS ? D + 1 : NS));
  const int nb = (int)std::min<int64_t>(GL_DERIVE_BLOCKS, grid_of(h->n_cells));
  hipLaunchKernelGGL((k_derive_cells<D, CK>), dim3(nb), dim3(256), 0, h->st, h->n_cells, h->n_nodes, h->adj.cell_nodes.p,
                     h->egeo.p, h->label.p, h->mat.p, f0, c, ds.cellv.p);
  GL_CHECK_LAUNCH();
  ds.n_cell_passes++;
}

template <int D>
void cells_of(glims_ctx* h, int ck, const double* f0, const double* c) {
  switch (ck) {
    case CK_STRAIN: return launch_cells<D, CK_STRAIN>(h, f0, c);
    case CK_STRESS: return launch_cells<D, CK_STRESS>(h, f0, c);
    case CK_JTOT: return launch_cells<D, CK_JTOT>(h, f0, c);
    case CK_VM: return launch_cells<D, CK_VM>(h, f0, c);
    case CK_UNORM: return launch_cells<D, CK_UNORM>(h, f0, c);
    case CK_LOGG: return launch_cells<D, CK_LOGG>(h, f0, c);
    case CK_GAMC: return launch_cells<D, CK_GAMC>(h, f0, c);
    case CK_GROWJ: return launch_cells<D, CK_GROWJ>(h, f0, c);
    default: return launch_cells<D, CK_CDEF>(h, f0, c);
  }
}

template <int NV, int NC, int LOC>
void launch_rows(glims_ctx* h) {
  DeriveState& ds = h->derive;
  hipLaunchKernelGGL((k_derive_rows<NV, NC, LOC>), dim3(grid_of(h->n_own)), dim3(256), 0, h->st, h->n_own, h->n_nodes,
                     h->n_cells, h->pat.cslice_ptr.p, h->pat.celem.p, h->adj.cell_nodes.p, ds.cellv.p, ds.rhs.p);
  GL_CHECK_LAUNCH();
}

// cell pass + gather + mass solves of one projection: x planes [ncomp][n_nodes].  Returns the worst status of the solves.
int project_integrand(glims_ctx* h, int ck, const double* f0, const double* c, double rtol, double* x) {
  DeriveState& ds = h->derive;
  const int d = h->dim, ns = d * (d + 1) / 2;
  const int ncomp = (ck == CK_STRAIN || ck == CK_STRESS) ? ns : 1;
  const bool loc = !ck_is_const(ck);
  ds.rhs.alloc((size_t)h->n_nodes * ns);
  // GLIMS_DERIVE_TIMING (tools/derive_cost.py): event pairs around the two passes, one line per projection on stderr
  const bool timed = getenv("GLIMS_DERIVE_TIMING") != nullptr;
  float ms_cells = 0.f, ms_rows = 0.f;
  if (timed) GL_HIP(hipEventRecord(h->ev_a, h->st));
  if (d == 2) cells_of<2>(h, ck, f0, c);
  else cells_of<3>(h, ck, f0, c);
  if (timed) {
    GL_HIP(hipEventRecord(h->ev_b, h->st));
    GL_HIP(hipEventSynchronize(h->ev_b));
    GL_HIP(hipEventElapsedTime(&ms_cells, h->ev_a, h->ev_b));
    GL_HIP(hipEventRecord(h->ev_a, h->st));
  }
  if (d == 2) {
    if (loc) launch_rows<3, 1, 1>(h);
    else if (ncomp == 1) launch_rows<3, 1, 0>(h);
    else launch_rows<3, 3, 0>(h);
  } else {
    if (loc) launch_rows<4, 1, 1>(h);
    else if (ncomp == 1) launch_rows<4, 1, 0>(h);
    else launch_rows<4, 6, 0>(h);
  }
  if (timed) {
    GL_HIP(hipEventRecord(h->ev_b, h->st));
    GL_HIP(hipEventSynchronize(h->ev_b));
    GL_HIP(hipEventElapsedTime(&ms_rows, h->ev_a, h->ev_b));
    fprintf(stderr, "glims derive: integrand %d  cell pass %.4f ms  gather %.4f ms\n", ck, ms_cells, ms_rows);
  }
  int status = GLIMS_OK;
  for (int k = 0; k < ncomp; ++k) {
    const int st = gl_project(h, ds.rhs.p + (size_t)k * h->n_nodes, x + (size_t)k * h->n_nodes, rtol);
    ds.n_mass_solves++;
    if (st != GLIMS_OK && status != GLIMS_NAN) status = st;
  }
  return status;
}

inline int worse(int a, int b) { return a == GLIMS_NAN || b == GLIMS_OK ? a : b; }

// is gamma one value over all cells?  (which labels the cells use is read from the device once per handle)
bool gamma_uniform(glims_ctx* h, double* gamma) {
  std::vector<uint8_t>& used = h->derive.label_used;
  if (used.empty()) {
    std::vector<uint8_t> lab((size_t)h->n_cells);
    GL_HIP(hipMemcpyAsync(lab.data(), h->label.p, lab.size(), hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
    used.assign(GL_MAX_LABELS, 0);
    for (uint8_t l : lab) used[l] = 1;
  }
  bool first = true, uniform = true;
  for (int l = 0; l < GL_MAX_LABELS; ++l) {
    if (!used[l]) continue;
    const double g = h->mat_host[2 * GL_MAX_LABELS + l];
    if (first) *gamma = g;
    else if (g != *gamma) uniform = false;
    first = false;
  }
  return uniform;
}

}  // namespace

int gl_derive(glims_ctx* h, int kind, int64_t snapshot, const double* c_host, const double* u_host, double rtol,
              double* out) {
  DeriveState& ds = h->derive;
  // ---- refusals: nothing is changed before the last of them ----
  GL_REQUIRE(h->world <= 1, "glims_derive: not available on a partitioned handle (world > 1); the host path computes the derived "
                            "fields there");
  GL_REQUIRE(kind >= GLIMS_DERIVE_STRAIN && kind <= GLIMS_DERIVE_CONC_DEFORMED,
             "glims_derive: unknown kind " + std::to_string(kind));
  GL_REQUIRE(h->is_setup, "glims_derive before glims_setup");
  GL_REQUIRE(rtol > 0.0, "glims_derive: rtol must be positive");
  const bool need_u = kind == GLIMS_DERIVE_STRAIN || kind == GLIMS_DERIVE_STRESS || kind == GLIMS_DERIVE_PRESSURE ||
                      kind == GLIMS_DERIVE_VON_MISES || kind == GLIMS_DERIVE_DISP_NORM ||
                      kind == GLIMS_DERIVE_TOTAL_JACOBIAN || kind == GLIMS_DERIVE_CONC_DEFORMED;
  const bool need_c = kind == GLIMS_DERIVE_LOG_GROWTH || kind == GLIMS_DERIVE_MECH_EXPANSION ||
                      kind == GLIMS_DERIVE_GROWTH_JACOBIAN || kind == GLIMS_DERIVE_CONC_DEFORMED;
  GL_REQUIRE(!need_u || (h->have_mech && h->U.p),
             "glims_derive: this kind needs the displacement: glims_setup(with_mechanics=1) first");
  if (snapshot == GLIMS_DERIVE_HOST) {
    GL_REQUIRE(!need_c || c_host, "glims_derive: GLIMS_DERIVE_HOST needs c_host for this kind (null pointer)");
    GL_REQUIRE(!need_u || u_host, "glims_derive: GLIMS_DERIVE_HOST needs u_host for this kind (null pointer)");
  } else if (snapshot == GLIMS_DERIVE_CURRENT) {
    GL_REQUIRE(h->have_state, "glims_derive: GLIMS_DERIVE_CURRENT before glims_set_state");
  } else {
    GL_REQUIRE(snapshot >= 0 && snapshot < (int64_t)h->snapshots.size() && h->snapshots[(size_t)snapshot],
               "glims_derive: unknown snapshot id " + std::to_string(snapshot));
  }
  const int d = h->dim, ns = d * (d + 1) / 2;
  const int64_t n = h->n_nodes;
  gl_ensure_cell_nodes(h);
  int status = GLIMS_OK;
  // ---- the source ----
  const double *c = nullptr, *u = nullptr;
  if (snapshot == GLIMS_DERIVE_HOST) {
    if (need_c) {
      ds.sc.alloc((size_t)n);
      gl_to_device_perm(h, c_host, ds.sc.p, 1);
      c = ds.sc.p;
    }
    if (need_u) {
      ds.su.alloc((size_t)n * d);
      gl_to_device_perm(h, u_host, ds.su.p, d);
      u = ds.su.p;
    }
  } else if (snapshot == GLIMS_DERIVE_CURRENT) {
    c = h->c.p;
    u = h->U.p;
  } else {
    c = h->snapshots[(size_t)snapshot]->p;
    if (need_u && ds.u_snapshot != snapshot) {
      ds.forget_u();
      const int st = gl_solve_mechanics(h, c);
      ds.n_elastic_solves++;
      if (st == GLIMS_OK) ds.u_snapshot = snapshot;
      status = worse(status, st);
    }
    u = h->U.p;
  }
  // ---- the field ----
  const bool tensor = kind == GLIMS_DERIVE_STRAIN || kind == GLIMS_DERIVE_STRESS;
  const int ncomp = tensor ? ns : 1;
  ds.ncomp = 0;   // (no result while this call is under way: a failure below leaves none)
  ds.res_il_valid = false;
  ds.res.alloc((size_t)n * ns);
  // the P1 stress of this source, through the one-entry cache
  auto stress_planes = [&]() -> const double* {
    const bool cacheable = snapshot != GLIMS_DERIVE_HOST;
    if (cacheable && ds.stress_valid && ds.stress_src == snapshot && ds.stress_gen == ds.u_gen && ds.stress_rtol <= rtol) {
      ds.n_cache_hits++;
      return ds.stress.p;
    }
    ds.stress.alloc((size_t)n * ns);
    ds.stress_valid = false;
    const int st = project_integrand(h, CK_STRESS, u, nullptr, rtol, ds.stress.p);
    status = worse(status, st);
    if (cacheable && st == GLIMS_OK) {
      ds.stress_valid = true;
      ds.stress_src = snapshot;
      ds.stress_gen = ds.u_gen;
      ds.stress_rtol = rtol;
    }
    return ds.stress.p;
  };
  switch (kind) {
    case GLIMS_DERIVE_STRAIN: status = worse(status, project_integrand(h, CK_STRAIN, u, nullptr, rtol, ds.res.p)); break;
    case GLIMS_DERIVE_STRESS: {
      const double* s = stress_planes();
      GL_HIP(hipMemcpyAsync(ds.res.p, s, (size_t)n * ns * sizeof(double), hipMemcpyDeviceToDevice, h->st));
      break;
    }
    case GLIMS_DERIVE_PRESSURE: {
      const double* s = stress_planes();
      hipLaunchKernelGGL(k_derive_pressure, dim3(grid_of(n)), dim3(256), 0, h->st, n, d, s, ds.res.p);
      GL_CHECK_LAUNCH();
      break;
    }
    case GLIMS_DERIVE_VON_MISES: {
      const double* s = stress_planes();
      status = worse(status, project_integrand(h, CK_VM, s, nullptr, rtol, ds.res.p));
      break;
    }
    case GLIMS_DERIVE_DISP_NORM: status = worse(status, project_integrand(h, CK_UNORM, u, nullptr, rtol, ds.res.p)); break;
    case GLIMS_DERIVE_LOG_GROWTH: status = worse(status, project_integrand(h, CK_LOGG, c, nullptr, rtol, ds.res.p)); break;
    case GLIMS_DERIVE_TOTAL_JACOBIAN: status = worse(status, project_integrand(h, CK_JTOT, u, nullptr, rtol, ds.res.p)); break;
    case GLIMS_DERIVE_CONC_DEFORMED: status = worse(status, project_integrand(h, CK_CDEF, u, c, rtol, ds.res.p)); break;
    case GLIMS_DERIVE_MECH_EXPANSION:
    case GLIMS_DERIVE_GROWTH_JACOBIAN: {
      // the class's two branches: gamma c nodewise where gamma is one value over all cells, else the projection of gamma_T c_h
      if (kind == GLIMS_DERIVE_GROWTH_JACOBIAN) ds.p1.alloc((size_t)n);
      double* s = kind == GLIMS_DERIVE_MECH_EXPANSION ? ds.res.p : ds.p1.p;
      double gamma = 0.0;
      if (gamma_uniform(h, &gamma)) {
        hipLaunchKernelGGL(k_derive_scale, dim3(grid_of(n)), dim3(256), 0, h->st, n, gamma, c, s);
        GL_CHECK_LAUNCH();
      } else {
        status = worse(status, project_integrand(h, CK_GAMC, c, nullptr, rtol, s));
      }
      if (kind == GLIMS_DERIVE_GROWTH_JACOBIAN)
        status = worse(status, project_integrand(h, CK_GROWJ, s, nullptr, rtol, ds.res.p));
      break;
    }
  }
  // ---- the caller's copy ----
  if (out) {
    const int nout = tensor ? d * d : 1;
    ds.out_stage.alloc((size_t)n * d * d);
    if (!tensor) hipLaunchKernelGGL((k_derive_out<2, 0>), dim3(grid_of(n)), dim3(256), 0, h->st, n, 1, h->d_old2new.p, ds.res.p, ds.out_stage.p);
    else if (d == 2) hipLaunchKernelGGL((k_derive_out<2, 1>), dim3(grid_of(n)), dim3(256), 0, h->st, n, ncomp, h->d_old2new.p, ds.res.p, ds.out_stage.p);
    else hipLaunchKernelGGL((k_derive_out<3, 1>), dim3(grid_of(n)), dim3(256), 0, h->st, n, ncomp, h->d_old2new.p, ds.res.p, ds.out_stage.p);
    GL_CHECK_LAUNCH();
    GL_HIP(hipMemcpyAsync(out, ds.out_stage.p, (size_t)n * nout * sizeof(double), hipMemcpyDeviceToHost, h->st));
  }
  GL_HIP(hipStreamSynchronize(h->st));
  ds.ncomp = ncomp;
  return status;
}

const double* gl_derive_sampled(glims_ctx* h, int ncomp) {
  DeriveState& ds = h->derive;
  GL_REQUIRE(ds.ncomp > 0, "glims_sampler_apply: GLIMS_FIELD_DERIVED with nothing derived (glims_derive first)");
  GL_REQUIRE(ncomp == ds.ncomp, "glims_sampler_apply: GLIMS_FIELD_DERIVED holds " + std::to_string(ds.ncomp) +
                                    " component(s), ncomp = " + std::to_string(ncomp));
  if (ds.ncomp == 1) return ds.res.p;
  if (!ds.res_il_valid) {
    const int64_t nn = h->n_nodes * ds.ncomp;
    ds.res_il.alloc((size_t)nn);
    hipLaunchKernelGGL(k_derive_interleave, dim3(grid_of(nn)), dim3(256), 0, h->st, h->n_nodes, ds.ncomp, ds.res.p, ds.res_il.p);
    GL_CHECK_LAUNCH();
    ds.res_il_valid = true;
  }
  return ds.res_il.p;
}
