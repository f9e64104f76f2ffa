// The host side of one adjoint call (gl_adjoint_gradient, gl_adjoint_hessian*, adjoint.hip): the scalars that size it, the
// table of every device buffer it allocates (the memory estimate is the table's sum), the per-label direction tables of a
// Hessian call, the fold of the ranks' per-label sums and their combination into the Hessian rows.  Plain C++17 -- no device
// types, no handle -- so that tests/hessian_plan_check.cpp exercises it on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "lame_derivs.h"

#ifndef GL_MAX_LABELS
#define GL_MAX_LABELS 256
#endif

constexpr int GL_ADJ_LT = 8;          // labels per sensitivity launch: per-thread accumulators live in registers (LT x 3 doubles)
constexpr int GL_ADJ_BLOCKS = 2048;   // fixed grid of the sensitivity pass: the reduction order does not depend on the mesh
constexpr int GL_HESS_MAXDIR = 8;     // directions per Hessian call
constexpr int GL_MP_BLOCKS = 1024;    // fixed grid of the P-column solver's dot products
constexpr int GL_MP_SCALARS = 6;      // its per-column scalars (rz, rr, alpha, beta, tol, pq)

// ---- shape ---------------------------------------------------------------------------------------------------------------
struct HessShape {
  int N = 0;     // the recording holds the states 0..N
  int P = 0;     // directions; 0: a gradient call, which allocates the first-order buffers alone
  int dim = 2, n_labels = 0, world = 1;
  int64_t n_nodes = 0, n_cells = 0, total_entries = 0, n_send = 0;
  int spmm_blocks = 0;                 // block partials of one k_spmm launch (gl_spmm_blocks)
  std::vector<uint8_t> term_is_u;      // per misfit term: 1 = a displacement term (its target has dim entries per node)
  bool any_u = false;                  // the sweep solves u_k and mu_k
  bool el = false;                     // the gradient's E / nu pass runs (mode 2: A_t, B_t)
  bool el_dirs = false;                // some direction has a part in E / nu
  bool el_sums = false;                // the E / nu rows of the Hessian are summed (k_hesens)
};

// A step is observed through the displacement when a nodal term is a displacement term, or a stored term observes u_k: a
// displacement image term (gradient and Hessian calls) or a deformed image / volume term (gradient calls only: the Hessian
// calls refuse those)
inline bool hess_any_u(const std::vector<uint8_t>& term_is_u, bool deformed_terms = false) {
  bool any = deformed_terms;
  for (uint8_t u : term_is_u) any = any || u != 0;
  return any;
}
// A direction in E / nu acts through K_el and G alone: without an observed displacement it changes nothing
inline bool hess_el_dirs(bool el, bool any_u, bool dir_E_or_nu) { return el && any_u && dir_E_or_nu; }
// The rows H[E, .], H[nu, .] are summed whenever they are asked for, also without a direction in E / nu: the mixed rows
// H[E, D] ... are not 0
inline bool hess_el_sums(bool el, bool any_u, bool hv_E_or_nu) { return el && any_u && hv_E_or_nu; }

// ---- the ranks' per-label sums -------------------------------------------------------------------------------------------
// A part of a rank's row: `chunks` runs of `len` sums, which lie `stride` apart where they are produced and where they are
// combined (device and host), and one after the other in the row
struct RowPart {
  size_t chunks, len, stride;
};
inline size_t row_width(const std::vector<RowPart>& parts) {
  size_t w = 0;
  for (const RowPart& p : parts) w += p.chunks * p.len;
  return w;
}
// The row of an adjoint call: [L][3] (D, rho, gamma), then [L][2] (A, B) when the E / nu pass ran, then the directions'
// [P][L][3], which live at stride GL_MAX_LABELS ([P][GL_MAX_LABELS][3]), and [P][L][2] of their E / nu rows (one GPU only)
inline std::vector<RowPart> label_row_parts(int L, bool el, int P, bool el_sums = false) {
  const size_t l = (size_t)L, LM = GL_MAX_LABELS;
  return {{1, 3 * l, 3 * l}, {1, el ? 2 * l : 0, 2 * l}, {(size_t)P, 3 * l, 3 * LM}, {(size_t)P, el_sums ? 2 * l : 0, 2 * LM}};
}
// out[k] = rows[0][k] + rows[1][k] + ... in rank order (rows: [world][W]): the same bits on every rank
inline void add_rows_in_rank_order(int world, size_t W, const double* rows, double* out) {
  for (size_t k = 0; k < W; ++k) {
    double t = 0.0;
    for (int r = 0; r < world; ++r) t += rows[W * r + k];
    out[k] = t;
  }
}
// the folded row into the parts' own arrays, each at its stride (dst[i] may be null where part i is empty)
inline void scatter_row(const std::vector<RowPart>& parts, const double* row, double* const* dst) {
  for (size_t i = 0; i < parts.size(); ++i)
    for (size_t c = 0; c < parts[i].chunks; ++c, row += parts[i].len)
      if (parts[i].len) std::memcpy(dst[i] + c * parts[i].stride, row, parts[i].len * sizeof(double));
}

// ---- buffers -------------------------------------------------------------------------------------------------------------
struct HessBuffer {
  const char* name;
  size_t count, elem;   // elements and bytes per element; count = 0: not allocated in this call
};

// Every device buffer of a call: the first-order work vectors (AdjWork), one "target" per misfit term in list order, the
// gather of the per-label sums and, with P > 0, the Hessian's own.  The allocations take their sizes from here
// (hess_buffer), so that hessian_bytes is what a call allocates.  Not listed: what belongs to the handle and outlives the
// call (the trajectory, the cell-vertex map) and the scratch of the stored image / observable terms.
inline std::vector<HessBuffer> hessian_buffers(const HessShape& s) {
  const size_t nn = (size_t)s.n_nodes, nd = nn * s.dim, nc = (size_t)s.n_cells, P = (size_t)s.P, LM = GL_MAX_LABELS;
  const size_t part = (size_t)GL_ADJ_BLOCKS * GL_ADJ_LT * 2, d = sizeof(double), i = sizeof(int);
  std::vector<HessBuffer> t;
  t.push_back({"vA", (size_t)s.total_entries, d});
  t.push_back({"dinv", nn, d});
  for (const char* v : {"lam", "lam_next", "rhs", "g", "r", "u", "w", "p", "s", "e", "hp", "Me", "tmp"}) t.push_back({v, nn, d});
  t.push_back({"qcell", nc, d});
  t.push_back({"part", part, d});
  t.push_back({"sums", LM * 3, d});
  t.push_back({"esums", s.el ? LM * 2 : 0, d});
  t.push_back({"stage", nd, d});
  for (const char* v : {"uk", "murhs", "mu", "mr", "mu_", "mw", "mp", "ms", "mKx"}) t.push_back({v, s.any_u ? nd : 0, d});
  for (uint8_t u : s.term_is_u) t.push_back({"target", nn * (u ? s.dim : 1), d});
  // [world][W] of the final gather (gather_label_sums allocates it when the sweep is over)
  t.push_back({"gather", s.world > 1 ? std::max<size_t>(1, row_width(label_row_parts(s.n_labels, s.el, s.P)) * s.world) : 0, d});
  if (s.P == 0) return t;
  t.push_back({"d_dir", P * 3 * LM, d});
  t.push_back({"d_dmat", P * 5 * LM, d});
  t.push_back({"d_dlame", s.el_dirs ? P * 2 * LM : 0, d});
  t.push_back({"d_dkap", s.el_dirs ? P * LM : 0, d});
  t.push_back({"d_dmat2", s.el_dirs ? P * 5 * LM : 0, d});
  t.push_back({"dKu", s.el_dirs ? P * nd : 0, d});
  t.push_back({"dKmu", s.el_dirs ? P * nd : 0, d});
  t.push_back({"hesums", s.el_sums ? P * LM * 2 : 0, d});
  t.push_back({"hepart", s.el_sums ? part : 0, d});
  t.push_back({"dcs", (size_t)(s.N + 1) * P * nn, d});   // dc_n of direction p at dcs[(n P + p) nn]
  for (const char* v : {"nu", "nu_next", "dg", "hrhs"}) t.push_back({v, P * nn, d});
  t.push_back({"hd", nn, d});
  t.push_back({"Mhd", nn, d});
  t.push_back({"hsums", P * LM * 3, d});
  t.push_back({"hpart", part, d});
  t.push_back({"hqcell", nc, d});
  for (const char* v : {"urhs", "du", "dmurhs", "dmu"}) t.push_back({v, s.any_u ? nd : 0, d});
  t.push_back({"ue", s.any_u ? nn : 0, d});
  t.push_back({"uMe", s.any_u ? nn : 0, d});
  // the P-column solver: interleaved vectors [n_nodes][P], block partials, scalars; on partitioned handles the send buffer of
  // its ghost exchanges and the [world][2 P] rows of its cross-rank sums
  for (const char* v : {"mp.X", "mp.B", "mp.R", "mp.Pv", "mp.Q"}) t.push_back({v, P * nn, d});
  t.push_back({"mp.part", (size_t)s.spmm_blocks * P, d});
  t.push_back({"mp.part2", (size_t)GL_MP_BLOCKS * 2 * P, d});
  t.push_back({"mp.sc", (size_t)GL_MP_SCALARS * P, d});
  t.push_back({"mp.done", P, i});
  t.push_back({"mp.its", P, i});
  t.push_back({"mp.flags", 2, i});
  t.push_back({"mp.sendbuf", s.world > 1 ? (size_t)std::max<int64_t>(s.n_send, 1) * P : 0, d});
  t.push_back({"mp.rows", s.world > 1 ? (size_t)s.world * 2 * P : 0, d});
  return t;
}
inline size_t hessian_bytes(const HessShape& s) {
  size_t b = 0;
  for (const HessBuffer& e : hessian_buffers(s)) b += e.count * e.elem;
  return b;
}
// the k-th entry called `name`: a buffer that is not in the table cannot be allocated
inline const HessBuffer& hess_buffer(const std::vector<HessBuffer>& t, const char* name, int k = 0) {
  for (const HessBuffer& e : t)
    if (!std::strcmp(e.name, name) && k-- == 0) return e;
  throw std::logic_error(std::string("adjoint: no buffer '") + name + "' in the call's table");
}

// ---- directions ----------------------------------------------------------------------------------------------------------
// Per-label tables of the P directions, LM = GL_MAX_LABELS entries per row (labels >= L: 0):
//   dir  [P][3][LM] = (dD, drho, dgamma);   dmat [P][5][LM]: the material table with the gamma row replaced by dgamma_p (the
//   dgamma_t G_t^T mu pass);   with el_dirs   dlame [P][2][LM] = (dm, dl)_p,   dkap [P][LM] = gamma (2 dm_p + d dl_p) (the
//   E / nu part of dG c),   dmat2 [P][5][LM]: the material table with the Lame rows replaced by (dm_p, dl_p) (the E / nu part
//   of dG^T mu through mode 1 and k_gt_rows).
// mat_host: [7][LM] = D, rho, gamma, mu, lambda, E, nu.  The caller's arrays are [P][L]; any of them may be null (= 0).
struct HessDirections {
  int P, L, dim;
  bool el_dirs;
  const double *dir_gamma, *dir_E, *dir_nu;   // the caller's, as given
  std::vector<double> dir, dmat, dlame, dkap, dmat2;

  HessDirections(int P_, int L_, int dim_, const double* mh, const double* dir_D, const double* dir_rho,
                 const double* dir_gamma_, const double* dir_E_, const double* dir_nu_, bool el_dirs_)
      : P(P_), L(L_), dim(dim_), el_dirs(el_dirs_), dir_gamma(dir_gamma_), dir_E(dir_E_), dir_nu(dir_nu_) {
    const size_t LM = GL_MAX_LABELS;
    dir.assign((size_t)P * 3 * LM, 0.0);
    dmat.assign((size_t)P * 5 * LM, 0.0);
    for (int p = 0; p < P; ++p) {
      for (int l = 0; l < L; ++l) {
        dir[(p * 3 + 0) * LM + l] = dir_D ? dir_D[(size_t)p * L + l] : 0.0;
        dir[(p * 3 + 1) * LM + l] = dir_rho ? dir_rho[(size_t)p * L + l] : 0.0;
        dir[(p * 3 + 2) * LM + l] = dir_gamma ? dir_gamma[(size_t)p * L + l] : 0.0;
      }
      std::copy(mh, mh + 5 * LM, dmat.begin() + (size_t)p * 5 * LM);
      std::copy(dir.begin() + (p * 3 + 2) * LM, dir.begin() + (p * 3 + 3) * LM, dmat.begin() + ((size_t)p * 5 + 2) * LM);
    }
    if (!el_dirs) return;
    dlame.assign((size_t)P * 2 * LM, 0.0);
    dkap.assign((size_t)P * LM, 0.0);
    dmat2.assign((size_t)P * 5 * LM, 0.0);
    for (int p = 0; p < P; ++p) {
      std::copy(mh, mh + 5 * LM, dmat2.begin() + (size_t)p * 5 * LM);
      for (int l = 0; l < L; ++l) {
        const LameDerivs d = lame_derivs(mh[5 * LM + l], mh[6 * LM + l]);
        double dm, dl;
        lame_direction(d, dir_E ? dir_E[(size_t)p * L + l] : 0.0, dir_nu ? dir_nu[(size_t)p * L + l] : 0.0, &dm, &dl);
        dlame[((size_t)p * 2 + 0) * LM + l] = dm;
        dlame[((size_t)p * 2 + 1) * LM + l] = dl;
        dkap[(size_t)p * LM + l] = mh[2 * LM + l] * (2.0 * dm + dim * dl);
      }
      std::copy(dlame.begin() + (size_t)p * 2 * LM, dlame.begin() + ((size_t)p * 2 + 2) * LM,
                dmat2.begin() + ((size_t)p * 5 + 3) * LM);
    }
  }
};

// ---- per-label rows ------------------------------------------------------------------------------------------------------
// The totals (A_t, B_t, C_t) of label l from the gradient's sums: sums3 [L][3] (D, rho, gamma), esums [L][2] (A, B).
// C_t = sum_k int_t |T|/(d+1) div mu_k sum_a c_k,a = (dJ/dgamma sum) / (2 mu_t + d lam_t): mode 1's sum carries the factor
inline ElasticSums elastic_totals(const double* mh, int dim, int l, const double* sums3, const double* esums) {
  const double den = 2.0 * mh[3 * GL_MAX_LABELS + l] + dim * mh[4 * GL_MAX_LABELS + l];
  return {esums[l * 2 + 0], esums[l * 2 + 1], den != 0.0 ? sums3[l * 3 + 2] / den : 0.0};
}

// dJ/dE_t, dJ/dnu_t in label order (lame_derivs.h)
inline void write_elastic_labels(const double* mh, int L, int dim, const double* sums3, const double* esums, double* dE,
                                 double* dnu) {
  for (int l = 0; l < L; ++l) {
    const double gam = mh[2 * GL_MAX_LABELS + l];
    const LameDerivs d = lame_derivs(mh[5 * GL_MAX_LABELS + l], mh[6 * GL_MAX_LABELS + l]);
    const ElasticSums tot = elastic_totals(mh, dim, l, sums3, esums);
    if (dE) dE[l] = elastic_gradient_row(dim, gam, d.m_E, d.l_E, tot);
    if (dnu) dnu[l] = elastic_gradient_row(dim, gam, d.m_nu, d.l_nu, tot);
  }
}

// The Hessian rows [P][L] of every direction from the gathered sums: sums [L][3] and esums [L][2] of the gradient,
// hs [P][LM][3] = (q0, q1, q2) and hes [P][LM][2] (A, B) of the directions.  hv_D = -dt q0, hv_rho = -dt q1, hv_gamma = q2.
// el (the E / nu rows next to the first-order combination, lame_derivs.h): the gradient's totals (A_t, B_t, C_t), the
// direction's sums (mode 1's sums carry kappa_t, as C_t does), and with el_dirs the extra term kappa(dm, dl) C_t of the gamma
// row.  Any output may be null.
inline void hessian_label_rows(const HessDirections& dd, bool el, double dt, const double* mh, const double* sums,
                               const double* hs, const double* esums, const double* hes, double* hv_D, double* hv_rho,
                               double* hv_gamma, double* hv_E, double* hv_nu) {
  const size_t LM = GL_MAX_LABELS;
  const int P = dd.P, L = dd.L, D = dd.dim;
  for (int p = 0; p < P; ++p)
    for (int l = 0; l < L; ++l) {
      const double* q = hs + ((size_t)p * LM + l) * 3;
      if (hv_D) hv_D[(size_t)p * L + l] = -dt * q[0];
      if (hv_rho) hv_rho[(size_t)p * L + l] = -dt * q[1];
      if (hv_gamma) hv_gamma[(size_t)p * L + l] = q[2];
    }
  if (!el) return;
  for (int p = 0; p < P; ++p)
    for (int l = 0; l < L; ++l) {
      const size_t o = (size_t)p * L + l;
      const double dEl = dd.dir_E ? dd.dir_E[o] : 0.0, dnul = dd.dir_nu ? dd.dir_nu[o] : 0.0;
      const LameDerivs d = lame_derivs(mh[5 * LM + l], mh[6 * LM + l]);
      const ElasticSums tot = elastic_totals(mh, D, l, sums, esums);
      const double den = 2.0 * mh[3 * LM + l] + D * mh[4 * LM + l];
      const ElasticSums sd = {hes[((size_t)p * LM + l) * 2 + 0], hes[((size_t)p * LM + l) * 2 + 1],
                              den != 0.0 ? hs[((size_t)p * LM + l) * 3 + 2] / den : 0.0};
      const double gam = mh[2 * LM + l], dgam = dd.dir_gamma ? dd.dir_gamma[o] : 0.0;
      if (hv_E) hv_E[o] = elastic_hessian_row(D, 0, d, gam, dgam, dEl, dnul, tot, sd);
      if (hv_nu) hv_nu[o] = elastic_hessian_row(D, 1, d, gam, dgam, dEl, dnul, tot, sd);
      if (dd.el_dirs && hv_gamma) {
        double dm, dl;
        lame_direction(d, dEl, dnul, &dm, &dl);
        hv_gamma[o] += (2.0 * dm + D * dl) * tot.C;
      }
    }
}
