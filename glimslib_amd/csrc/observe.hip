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
