// Per-cell derivatives of the observables' measure (observe.hip, glims_adjoint_observable_terms): for one
// simplex with P1 vertex values c_0 .. c_d and the query (MASS / SHARP / SMOOTH) of observe_clip.h, the fraction b0 = V_T / |T| and
//   g[i]  = d b0 / d c_i                          (the measure's gradient is |T| g)
//   Hd[i] = sum_j d2 b0 / (d c_i d c_j) dc_j      (MASS: 0; SMOOTH: the rule's own second derivative; SHARP: not defined here)
// Everything is in barycentric terms: no positions enter, |T| multiplies at the caller's.  For the terms of the deformed
// configuration, whose |T| depends on the displacement, glims_og_volume_grad gives the derivative of the cell volume by the
// vertex positions (tests/observe_def_grad_check.cpp runs it on the host).
//
//   MASS    b0 = mean(c):  g[i] = 1 / (d+1).
//   SMOOTH  b0 = sum_q w_q h(v_q), v_q = sum_a lam_qa c_a, h(v) = 1/2 (tanh((v - level) / smooth) + 1):
//           g[i] = sum_q w_q h'(v_q) lam_qi,   Hd[i] = sum_q w_q h''(v_q) lam_qi (sum_j lam_qj dc_j)
//           with h' = (1 - th^2) / (2 smooth), h'' = -th (1 - th^2) / smooth^2 -- the derivative of the discrete rule of
//           glims_oc_smooth (same points and weights), not of a converged integral.
//   SHARP   the derivative of the fraction formulas of observe_clip.h THROUGH their edge parameters.  With a the in-vertex and o
//           the out-vertex of a cut edge, t = (c_a - level) / (c_a - c_o):
//               dt/dc_a = (1 - t) / (c_a - c_o),   dt/dc_o = t / (c_a - c_o)        (c_a - c_o > 0 by construction)
//             1 in (v):   b0 = prod_j t_j over the edges v -> j
//             1 out (v):  b0 = 1 - prod_j (1 - t_j) over the edges j -> v
//             3-D, a, b in and e, f out: the three tetrahedra of the prism have the fractions (their 3 x 3 determinants, expanded)
//                         t_ae t_af,   t_af t_be (1 - t_ae),   t_be t_bf (1 - t_af)
//                         -- each a product of factors in [0, 1]: b0 has no cancellation.  Its partials by the t are short
//                         polynomials of the same factors; d b0 / d t_af = t_ae + t_be (1 - t_ae) - t_be t_bf holds one
//                         subtraction of terms of size <= 1 (an absolute error of a few roundings).
//           0 or d+1 vertices in: g = 0.  A tie c_i == level counts as in, as in the forward rule; the gradient is that of the
//           smooth piece the evaluation sits on (b0 is continuous and piecewise rational in c, with a jump in the SECOND
//           derivative where the level set crosses a vertex).  The products that leave one factor out are formed explicitly: a
//           factor that is 0 (a tie) divides nothing.  The closed form observe_clip.h warns against is not differentiated.
//
// Plain C++17 templates over the dimension; usable from host and device code (tests/observe_grad_check.cpp runs them on the host).
#pragma once
#include "observe_clip.h"

// MASS: returns b0
template <int D>
GLIMS_OC_HD double glims_og_mass(const double (&c)[D + 1], double (&g)[D + 1]) {
  constexpr int NV = D + 1;
  double s = 0.0;
  for (int i = 0; i < NV; ++i) {
    s += c[i];
    g[i] = 1.0 / NV;
  }
  return s * (1.0 / NV);
}

// SHARP: returns b0; *n_in = the number of vertices with c_i >= level (the cell is cut iff 0 < n_in < d+1)
template <int D>
GLIMS_OC_HD double glims_og_sharp(double level, const double (&c)[D + 1], double (&g)[D + 1], int* n_in_out) {
  constexpr int NV = D + 1;
  int n_in = 0;
  for (int i = 0; i < NV; ++i) {
    n_in += c[i] >= level ? 1 : 0;
    g[i] = 0.0;
  }
  *n_in_out = n_in;
  if (n_in == 0) return 0.0;
  if (n_in == NV) return 1.0;
  if (n_in == 1 || n_in == NV - 1) {
    // the corner simplex at vertex v (observe_clip.h): s_j = its extent along the edge v -> j
    const bool corner_in = n_in == 1;
    int v = 0;
    for (int i = 0; i < NV; ++i)
      if ((c[i] >= level) == corner_in) v = i;
    double s[NV], ds_j[NV], ds_v[NV];   // s_j and its partials by c_j and by c_v
    double frac = 1.0;
    for (int j = 0; j < NV; ++j) {
      s[j] = 1.0;
      ds_j[j] = ds_v[j] = 0.0;
      if (j == v) continue;
      const int a = corner_in ? v : j, o = corner_in ? j : v;
      const double den = c[a] - c[o];
      const double t = (c[a] - level) / den;
      if (corner_in) {   // s = t, a = v, o = j
        s[j] = t;
        ds_j[j] = t / den;
        ds_v[j] = (1.0 - t) / den;
      } else {           // s = 1 - t, a = j, o = v
        s[j] = 1.0 - t;
        ds_j[j] = -(1.0 - t) / den;
        ds_v[j] = -t / den;
      }
      frac *= s[j];
    }
    const double sign = corner_in ? 1.0 : -1.0;   // b0 = frac or 1 - frac
    double gv = 0.0;
    for (int j = 0; j < NV; ++j) {
      if (j == v) continue;
      double rest = 1.0;   // prod of s_k over the edges other than j
      for (int k = 0; k < NV; ++k)
        if (k != v && k != j) rest *= s[k];
      g[j] = sign * rest * ds_j[j];
      gv += rest * ds_v[j];
    }
    g[v] = sign * gv;
    return corner_in ? frac : 1.0 - frac;
  }
  if constexpr (D == 3) {
    // 2 in (a < b), 2 out (e < f), in the vertex order of glims_oc_sharp's prism
    int in[2], out[2], ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) {
      if (c[i] >= level) in[ni++] = i;
      else out[no++] = i;
    }
    double t[2][2], dt_in[2][2], dt_out[2][2];   // [in vertex][out vertex]
    for (int x = 0; x < 2; ++x)
      for (int k = 0; k < 2; ++k) {
        const double den = c[in[x]] - c[out[k]];
        t[x][k] = (c[in[x]] - level) / den;
        dt_in[x][k] = (1.0 - t[x][k]) / den;
        dt_out[x][k] = t[x][k] / den;
      }
    const double ta0 = t[0][0], ta1 = t[0][1], tb0 = t[1][0], tb1 = t[1][1];
    const double b0 = ta0 * ta1 + ta1 * tb0 * (1.0 - ta0) + tb0 * tb1 * (1.0 - ta1);
    double db[2][2];   // d b0 / d t
    db[0][0] = ta1 * (1.0 - tb0);
    db[0][1] = ta0 + tb0 * (1.0 - ta0) - tb0 * tb1;
    db[1][0] = ta1 * (1.0 - ta0) + tb1 * (1.0 - ta1);
    db[1][1] = tb0 * (1.0 - ta1);
    for (int x = 0; x < 2; ++x)
      for (int k = 0; k < 2; ++k) {
        g[in[x]] += db[x][k] * dt_in[x][k];
        g[out[k]] += db[x][k] * dt_out[x][k];
      }
    return b0;
  }
  return 0.0;
}

// SMOOTH with the rule (lam [NQ][d+1], w [NQ]) handed in: returns b0.  dc != nullptr: also Hd (the second derivative applied to dc).
template <int D, int NQ>
GLIMS_OC_HD double glims_og_smooth(double level, double smooth, const double (&c)[D + 1], const double (*lam)[D + 1],
                                   const double* w, double (&g)[D + 1], const double* dc, double* Hd) {
  constexpr int NV = D + 1;
  double b0 = 0.0;
  for (int i = 0; i < NV; ++i) {
    g[i] = 0.0;
    if (dc) Hd[i] = 0.0;
  }
  const double inv = 1.0 / smooth;
  for (int q = 0; q < NQ; ++q) {
    double cq = 0.0, dq = 0.0;
    for (int a = 0; a < NV; ++a) {
      cq += lam[q][a] * c[a];
      if (dc) dq += lam[q][a] * dc[a];
    }
    const double th = tanh((cq - level) / smooth);
    b0 += w[q] * (0.5 * (th + 1.0));
    const double sech2 = 1.0 - th * th;
    const double h1 = w[q] * (0.5 * sech2 * inv);
    const double h2 = w[q] * (-th * sech2 * inv * inv) * dq;
    for (int i = 0; i < NV; ++i) {
      g[i] += h1 * lam[q][i];
      if (dc) Hd[i] += h2 * lam[q][i];
    }
  }
  return b0;
}

// The signed volume of observe_clip.h by the vertex positions: dvol[a][k] = d glims_oc_volume(p) / d p[a][k], the cofactor vector
// of vertex a.  2-D: half the opposite edge rotated by a quarter turn; 3-D: one sixth of the cross product of two edges of the
// opposite face, with the sign of the vertex.  Every vertex gets its own expression (none is minus the sum of the others) and
// nothing is divided: a degenerate simplex has finite cofactors, and sum_a dvol[a] = 0 holds to rounding.  The volume is
// multilinear in the vertex positions, so a central difference in one component reproduces dvol up to rounding.
template <int D>
GLIMS_OC_HD void glims_og_volume_grad(const double (&p)[D + 1][D], double (&dvol)[D + 1][D]) {
  if constexpr (D == 2) {
    dvol[0][0] = 0.5 * (p[1][1] - p[2][1]);
    dvol[0][1] = 0.5 * (p[2][0] - p[1][0]);
    dvol[1][0] = 0.5 * (p[2][1] - p[0][1]);
    dvol[1][1] = 0.5 * (p[0][0] - p[2][0]);
    dvol[2][0] = 0.5 * (p[0][1] - p[1][1]);
    dvol[2][1] = 0.5 * (p[1][0] - p[0][0]);
  } else {
    // vertex a: sign_a / 6 (p_j - p_i) x (p_k - p_i) with (i, j, k) the other three in ascending order, sign = -, +, -, +
    constexpr int oth[4][3] = {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}};
    for (int a = 0; a < 4; ++a) {
      const int i = oth[a][0], j = oth[a][1], k = oth[a][2];
      const double e0 = p[j][0] - p[i][0], e1 = p[j][1] - p[i][1], e2 = p[j][2] - p[i][2];
      const double f0 = p[k][0] - p[i][0], f1 = p[k][1] - p[i][1], f2 = p[k][2] - p[i][2];
      const double s = (a & 1) ? (1.0 / 6.0) : (-1.0 / 6.0);
      dvol[a][0] = s * (e1 * f2 - e2 * f1);
      dvol[a][1] = s * (e2 * f0 - e0 * f2);
      dvol[a][2] = s * (e0 * f1 - e1 * f0);
    }
  }
}

// one query of one simplex, host side (the rule from derive_quadrature.h's static tables): b0, g and (dc != nullptr, MASS / SMOOTH)
// Hd; returns the in-count of a SHARP query, -1 for the other kinds
template <int D>
inline int glims_og_cell(int kind, double level, double smooth, const double (&c)[D + 1], double* b0, double (&g)[D + 1],
                         const double* dc, double* Hd) {
  int n_in = -1;
  if (dc)
    for (int i = 0; i < D + 1; ++i) Hd[i] = 0.0;
  if (kind == GLIMS_OC_MASS) *b0 = glims_og_mass<D>(c, g);
  else if (kind == GLIMS_OC_SHARP) *b0 = glims_og_sharp<D>(level, c, g, &n_in);
  else if constexpr (D == 2) *b0 = glims_og_smooth<2, GLIMS_DQ2_N>(level, smooth, c, glims_dq2_lam, glims_dq2_w, g, dc, Hd);
  else *b0 = glims_og_smooth<3, GLIMS_DQ3_N>(level, smooth, c, glims_dq3_lam, glims_dq3_w, g, dc, Hd);
  return n_in;
}
