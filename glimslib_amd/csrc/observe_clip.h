// Per-cell mathematics of the observables (observe.hip, glims_observe): for one simplex with vertex
// positions p_0 .. p_d and P1 vertex values c_0 .. c_d, the measure V = int_T q dx and the first moments M_a = int_T x_a q dx of
//   MASS    q = c_h                                        exact
//   SHARP   q = 1 where c_h >= level, else 0               exact, by clipping the simplex at the level set
//   SMOOTH  q = 1/2 (tanh((c_h - level) / smooth) + 1)     the 16 / 64-point degree-7 rule of derive_quadrature.h
// -- what the reference's compute_from_conc_for_each_time_step / compute_volume_thresholded / compute_com_all integrate over dx
// and dx(subdomain_id) (optimization_workflow/image_based_optimization.py:1333-1397, :1262-1301, :1416-1430, :1470-1472).
//
// Every query is evaluated in the cell's barycentric coordinates first: b[0] = V / |T| and b[1 + k] = (int_T lambda_k q dx) / |T|.
// glims_oc_map turns these into V = |T| b[0] and M_a = |T| sum_k b[1 + k] p_k[a].  |T| is the SIGNED volume of the positions
// passed in (glims_oc_volume): the same code serves the reference configuration (p_i = X_i) and the deformed one
// (p_i = X_i + scale u_i), where the measure is int q det(I + grad u) dX, the moments are those of x = X + u and a folded cell
// counts negatively, as in the total Jacobian of glims_derive.
//
// SHARP.  A vertex is "in" when c_i >= level (a tie counts as in).  The cut point on the edge from an in-vertex a to an
// out-vertex b is p_a + t (p_b - p_a) with t = (c_a - level) / (c_a - c_b) in [0, 1]; the denominator is > 0 by construction.
//   0 in: zeros.  All in: the cell.  1 in: the corner simplex at that vertex.  1 out: the cell minus the corner simplex at the
//   out-vertex.  3-D with a, b in and e, f out: the prism {a, P_ae, P_af | b, P_be, P_bf} as the three tetrahedra
//   (A0, A1, A2, B0), (A1, A2, B0, B1), (A2, B0, B1, B2).
// A sub-simplex contributes its volume fraction and that fraction times the mean of its vertices.  The fractions are computed
// from the edge parameters t alone (products of t for a corner, 3 x 3 determinants of barycentric coordinates for the prism), so
// their rounding error is a few units in the last place of |T| whatever the shape of the cell.  The closed form
// sum_i (c_i - level)^d / prod_{j != i} (c_i - c_j) is NOT used: it cancels catastrophically for nearly equal vertex values.
//
// SMOOTH is the discrete statement of the quadrature rule, not a converged integral: where `smooth` is far below the range of c
// over a cell the integrand is a step on the scale of the cell and the rule resolves it only to O(1) of the cell's volume.
//
// Plain C++17 templates over the dimension; usable from host and device code (tests/observe_clip_check.cpp runs them on the host).
#pragma once
#include <math.h>

#include "derive_quadrature.h"

#if defined(__HIP__) || defined(__CUDACC__)
#define GLIMS_OC_HD __host__ __device__ inline
#else
#define GLIMS_OC_HD inline
#endif

#define GLIMS_OC_MASS 0
#define GLIMS_OC_SHARP 1
#define GLIMS_OC_SMOOTH 2

// signed volume det(p_1 - p_0, .., p_d - p_0) / d!
template <int D>
GLIMS_OC_HD double glims_oc_volume(const double (&p)[D + 1][D]) {
  if constexpr (D == 2) {
    return 0.5 * ((p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0]));
  } else {
    const double a0 = p[1][0] - p[0][0], a1 = p[1][1] - p[0][1], a2 = p[1][2] - p[0][2];
    const double b0 = p[2][0] - p[0][0], b1 = p[2][1] - p[0][1], b2 = p[2][2] - p[0][2];
    const double c0 = p[3][0] - p[0][0], c1 = p[3][1] - p[0][1], c2 = p[3][2] - p[0][2];
    return (1.0 / 6.0) * (a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0));
  }
}

// one tetrahedron of the prism: vertices Q_0 .. Q_3 in barycentric coordinates; adds its volume fraction to b[0] and the fraction
// times the mean of its vertices to b[1 ..]
GLIMS_OC_HD void glims_oc_add_tet(const double* q0, const double* q1, const double* q2, const double* q3, double (&b)[5]) {
  // the coordinates sum to 1: the volume ratio is the determinant of the differences in coordinates 1 .. 3
  const double a0 = q1[1] - q0[1], a1 = q1[2] - q0[2], a2 = q1[3] - q0[3];
  const double b0 = q2[1] - q0[1], b1 = q2[2] - q0[2], b2 = q2[3] - q0[3];
  const double c0 = q3[1] - q0[1], c1 = q3[2] - q0[2], c2 = q3[3] - q0[3];
  const double f = fabs(a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0));
  b[0] += f;
  for (int k = 0; k < 4; ++k) b[1 + k] += f * (0.25 * (q0[k] + q1[k] + q2[k] + q3[k]));
}

// SHARP in barycentric terms
template <int D>
GLIMS_OC_HD void glims_oc_sharp(double level, const double (&c)[D + 1], double (&b)[D + 2]) {
  constexpr int NV = D + 1;
  int n_in = 0;
  for (int i = 0; i < NV; ++i) n_in += c[i] >= level ? 1 : 0;
  for (int k = 0; k < NV + 1; ++k) b[k] = 0.0;
  if (n_in == 0) return;
  if (n_in == NV) {
    b[0] = 1.0;
    for (int k = 0; k < NV; ++k) b[1 + k] = 1.0 / NV;
    return;
  }
  if (n_in == 1 || n_in == NV - 1) {
    // the corner simplex at vertex v: the single in-vertex, or the single out-vertex; s_j = its extent along the edge v -> j
    const bool corner_in = n_in == 1;
    int v = 0;
    for (int i = 0; i < NV; ++i)
      if ((c[i] >= level) == corner_in) v = i;
    double s[NV];
    double frac = 1.0, sum_rest = 0.0;
    for (int j = 0; j < NV; ++j) {
      if (j == v) {
        s[j] = 0.0;
        continue;
      }
      // in-vertex a, out-vertex o of this edge; t from the in-vertex
      const int a = corner_in ? v : j, o = corner_in ? j : v;
      const double t = (c[a] - level) / (c[a] - c[o]);
      s[j] = corner_in ? t : 1.0 - t;
      frac *= s[j];
      sum_rest += 1.0 - s[j];
    }
    // mean of the corner simplex's vertices: e_v and (1 - s_j) e_v + s_j e_j
    double m[NV];
    for (int j = 0; j < NV; ++j) m[j] = (j == v ? 1.0 + sum_rest : s[j]) * (1.0 / NV);
    if (corner_in) {
      b[0] = frac;
      for (int k = 0; k < NV; ++k) b[1 + k] = frac * m[k];
    } else {
      b[0] = 1.0 - frac;
      for (int k = 0; k < NV; ++k) b[1 + k] = 1.0 / NV - frac * m[k];
    }
    return;
  }
  if constexpr (D == 3) {
    // 2 in (ia < ib), 2 out (oe < of): the prism
    int in[2], out[2], ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) {
      if (c[i] >= level) in[ni++] = i;
      else out[no++] = i;
    }
    double A[3][4] = {}, B[3][4] = {};
    A[0][in[0]] = 1.0;
    B[0][in[1]] = 1.0;
    for (int k = 0; k < 2; ++k) {
      const double ta = (c[in[0]] - level) / (c[in[0]] - c[out[k]]);
      const double tb = (c[in[1]] - level) / (c[in[1]] - c[out[k]]);
      A[1 + k][in[0]] = 1.0 - ta;
      A[1 + k][out[k]] = ta;
      B[1 + k][in[1]] = 1.0 - tb;
      B[1 + k][out[k]] = tb;
    }
    glims_oc_add_tet(A[0], A[1], A[2], B[0], b);
    glims_oc_add_tet(A[1], A[2], B[0], B[1], b);
    glims_oc_add_tet(A[2], B[0], B[1], B[2], b);
  }
}

// MASS in barycentric terms: V = |T| mean(c), int lambda_k c_h = |T| (sum_i c_i + c_k) / ((d+1)(d+2))
template <int D>
GLIMS_OC_HD void glims_oc_mass(const double (&c)[D + 1], double (&b)[D + 2]) {
  constexpr int NV = D + 1;
  double s = 0.0;
  for (int i = 0; i < NV; ++i) s += c[i];
  b[0] = s * (1.0 / NV);
  for (int k = 0; k < NV; ++k) b[1 + k] = (s + c[k]) * (1.0 / (NV * (NV + 1)));
}

// SMOOTH in barycentric terms with the rule (lam [NQ][d+1], w [NQ]) handed in (device code keeps the rule in constant memory)
template <int D, int NQ>
GLIMS_OC_HD void glims_oc_smooth(double level, double smooth, const double (&c)[D + 1], const double (*lam)[D + 1],
                                 const double* w, double (&b)[D + 2]) {
  constexpr int NV = D + 1;
  for (int k = 0; k < NV + 1; ++k) b[k] = 0.0;
  for (int q = 0; q < NQ; ++q) {
    double cq = 0.0;
    for (int a = 0; a < NV; ++a) cq += lam[q][a] * c[a];
    const double f = w[q] * (0.5 * (tanh((cq - level) / smooth) + 1.0));
    b[0] += f;
    for (int k = 0; k < NV; ++k) b[1 + k] += f * lam[q][k];
  }
}

// V = T b[0], M_a = T sum_k b[1 + k] p_k[a]  ->  out[0 .. d]
template <int D>
GLIMS_OC_HD void glims_oc_map(double T, const double (&p)[D + 1][D], const double (&b)[D + 2], double (&out)[D + 1]) {
  out[0] = T * b[0];
  for (int a = 0; a < D; ++a) {
    double m = 0.0;
    for (int k = 0; k < D + 1; ++k) m += b[1 + k] * p[k][a];
    out[1 + a] = T * m;
  }
}

// one query of one simplex, host side (the rule from derive_quadrature.h's static tables): out = (V, M_0 .. M_{d-1})
template <int D>
inline void glims_oc_observe(int kind, double level, double smooth, const double (&p)[D + 1][D], const double (&c)[D + 1],
                             double (&out)[D + 1]) {
  double b[D + 2];
  if (kind == GLIMS_OC_MASS) glims_oc_mass<D>(c, b);
  else if (kind == GLIMS_OC_SHARP) glims_oc_sharp<D>(level, c, b);
  else if constexpr (D == 2) glims_oc_smooth<2, GLIMS_DQ2_N>(level, smooth, c, glims_dq2_lam, glims_dq2_w, b);
  else glims_oc_smooth<3, GLIMS_DQ3_N>(level, smooth, c, glims_dq3_lam, glims_dq3_w, b);
  glims_oc_map<D>(glims_oc_volume<D>(p), p, b, out);
}
