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

// ---- first moments (centre-of-mass terms) ------------------------------------------------------------------------------------------
// With D1[m][i] = d b[1 + m] / d c_i and weights psi_m handed in, the glims_og_moment_* give the values b[0 .. d+1] of
// observe_clip.h (the same formulas, to rounding) and the contraction g[i] = sum_m psi_m D1[m][i] -- the gradient of the scalar
// S(c) = sum_m psi_m b[1 + m](c).  psi knows the positions; nothing here does.
//   MASS    D1[m][i] = (1 + delta_mi) / ((d+1)(d+2)):  g[i] = (sum_m psi_m + psi_i) / ((d+1)(d+2))
//   SMOOTH  D1[m][i] = sum_q w_q h'(v_q) lam_qi lam_qm:  g[i] = sum_q w_q h'(v_q) lam_qi (sum_m lam_qm psi_m)
//   SHARP   glims_oc_sharp's formulas differentiated through the edge parameters t (dt/dc as in glims_og_sharp):
//             corner simplex at v, s_j its extent along v -> j:  F = frac Q,  frac = prod_j s_j,
//               Q = (psi_v (1 + sum_j (1 - s_j)) + sum_j psi_j s_j) / (d+1),   dF/ds_j = (prod_{k != j} s_k) Q + frac (psi_j - psi_v) / (d+1),
//               S = F (1 in) or sum_m psi_m / (d+1) - F (1 out); the products that leave one factor out are formed explicitly
//             3-D prism: the three tetrahedra of glims_oc_add_tet in forward mode over the four t (glims_og_d4: a value and its
//               four partials), in the local vertex order (a, b, e, f) so that every index is a constant.  The three
//               determinants are sigma times products of factors in [0, 1] with ONE sign sigma, that of the vertex order
//               (a, e, f, b) -- +1 in the local order: |det| = sigma det is differentiated as such, so that a factor that is 0
//               (a tie: a tetrahedron of zero volume) still has the derivative of the piece the evaluation sits on
//           0 or d+1 vertices in: g = 0.  A tie counts as in.  The only divisions are those by c_a - c_o > 0.

// MASS
template <int D>
GLIMS_OC_HD void glims_og_moment_mass(const double (&c)[D + 1], const double (&psi)[D + 1], double (&b)[D + 2],
                                      double (&g)[D + 1]) {
  constexpr int NV = D + 1;
  glims_oc_mass<D>(c, b);
  double sp = 0.0;
  for (int m = 0; m < NV; ++m) sp += psi[m];
  for (int i = 0; i < NV; ++i) g[i] = (sp + psi[i]) * (1.0 / (NV * (NV + 1)));
}

// SMOOTH with the rule handed in (as glims_og_smooth)
template <int D, int NQ>
GLIMS_OC_HD void glims_og_moment_smooth(double level, double smooth, const double (&c)[D + 1], const double (*lam)[D + 1],
                                        const double* w, const double (&psi)[D + 1], double (&b)[D + 2], double (&g)[D + 1]) {
  constexpr int NV = D + 1;
  for (int k = 0; k < NV + 1; ++k) b[k] = 0.0;
  for (int i = 0; i < NV; ++i) g[i] = 0.0;
  const double inv = 1.0 / smooth;
  for (int q = 0; q < NQ; ++q) {
    double cq = 0.0, pq = 0.0;
    for (int a = 0; a < NV; ++a) {
      cq += lam[q][a] * c[a];
      pq += lam[q][a] * psi[a];
    }
    const double th = tanh((cq - level) / smooth);
    const double f = w[q] * (0.5 * (th + 1.0));
    b[0] += f;
    for (int k = 0; k < NV; ++k) b[1 + k] += f * lam[q][k];
    const double h1 = w[q] * (0.5 * (1.0 - th * th) * inv) * pq;
    for (int i = 0; i < NV; ++i) g[i] += h1 * lam[q][i];
  }
}

// a value and its partials by the four edge parameters of the prism
struct glims_og_d4 {
  double v, d[4];
};
GLIMS_OC_HD glims_og_d4 glims_og_d4_const(double v) { return {v, {0.0, 0.0, 0.0, 0.0}}; }
GLIMS_OC_HD glims_og_d4 glims_og_d4_add(const glims_og_d4& x, const glims_og_d4& y) {
  glims_og_d4 r;
  r.v = x.v + y.v;
  for (int k = 0; k < 4; ++k) r.d[k] = x.d[k] + y.d[k];
  return r;
}
GLIMS_OC_HD glims_og_d4 glims_og_d4_sub(const glims_og_d4& x, const glims_og_d4& y) {
  glims_og_d4 r;
  r.v = x.v - y.v;
  for (int k = 0; k < 4; ++k) r.d[k] = x.d[k] - y.d[k];
  return r;
}
GLIMS_OC_HD glims_og_d4 glims_og_d4_mul(const glims_og_d4& x, const glims_og_d4& y) {
  glims_og_d4 r;
  r.v = x.v * y.v;
  for (int k = 0; k < 4; ++k) r.d[k] = x.d[k] * y.v + x.v * y.d[k];
  return r;
}

// glims_oc_add_tet in forward mode: adds the tetrahedron's b and, to S, sum_k psi_k (its fraction times the mean of its vertices)_k;
// sigma = the sign its determinant has wherever it is not 0
GLIMS_OC_HD void glims_og_add_tet(const glims_og_d4* q0, const glims_og_d4* q1, const glims_og_d4* q2, const glims_og_d4* q3,
                                  double sigma, const double (&psi)[4], double (&b)[5], glims_og_d4& S) {
  const glims_og_d4 a0 = glims_og_d4_sub(q1[1], q0[1]), a1 = glims_og_d4_sub(q1[2], q0[2]), a2 = glims_og_d4_sub(q1[3], q0[3]);
  const glims_og_d4 b0 = glims_og_d4_sub(q2[1], q0[1]), b1 = glims_og_d4_sub(q2[2], q0[2]), b2 = glims_og_d4_sub(q2[3], q0[3]);
  const glims_og_d4 c0 = glims_og_d4_sub(q3[1], q0[1]), c1 = glims_og_d4_sub(q3[2], q0[2]), c2 = glims_og_d4_sub(q3[3], q0[3]);
  const glims_og_d4 m0 = glims_og_d4_sub(glims_og_d4_mul(b1, c2), glims_og_d4_mul(b2, c1));
  const glims_og_d4 m1 = glims_og_d4_sub(glims_og_d4_mul(b0, c2), glims_og_d4_mul(b2, c0));
  const glims_og_d4 m2 = glims_og_d4_sub(glims_og_d4_mul(b0, c1), glims_og_d4_mul(b1, c0));
  glims_og_d4 f = glims_og_d4_add(glims_og_d4_sub(glims_og_d4_mul(a0, m0), glims_og_d4_mul(a1, m1)), glims_og_d4_mul(a2, m2));
  f.v *= sigma;
  for (int k = 0; k < 4; ++k) f.d[k] *= sigma;
  b[0] += f.v;
  for (int k = 0; k < 4; ++k) {
    glims_og_d4 mean = glims_og_d4_add(glims_og_d4_add(q0[k], q1[k]), glims_og_d4_add(q2[k], q3[k]));
    mean.v *= 0.25;
    for (int j = 0; j < 4; ++j) mean.d[j] *= 0.25;
    const glims_og_d4 fm = glims_og_d4_mul(f, mean);
    b[1 + k] += fm.v;
    S.v += psi[k] * fm.v;
    for (int j = 0; j < 4; ++j) S.d[j] += psi[k] * fm.d[j];
  }
}

// SHARP: returns the in-count (the cell is cut iff 0 < n_in < d+1)
template <int D>
GLIMS_OC_HD int glims_og_moment_sharp(double level, const double (&c)[D + 1], const double (&psi)[D + 1], double (&b)[D + 2],
                                      double (&g)[D + 1]) {
  constexpr int NV = D + 1;
  int n_in = 0;
  for (int i = 0; i < NV; ++i) {
    n_in += c[i] >= level ? 1 : 0;
    g[i] = 0.0;
  }
  for (int k = 0; k < NV + 1; ++k) b[k] = 0.0;
  if (n_in == 0) return n_in;
  if (n_in == NV) {
    b[0] = 1.0;
    for (int k = 0; k < NV; ++k) b[1 + k] = 1.0 / NV;
    return n_in;
  }
  if (n_in == 1 || n_in == NV - 1) {
    const bool corner_in = n_in == 1;
    int v = 0;
    for (int i = 0; i < NV; ++i)
      if ((c[i] >= level) == corner_in) v = i;
    double s[NV], ds_j[NV], ds_v[NV];   // s_j and its partials by c_j and by c_v (as glims_og_sharp)
    double frac = 1.0, sum_rest = 0.0;
    for (int j = 0; j < NV; ++j) {
      s[j] = 0.0;
      ds_j[j] = ds_v[j] = 0.0;
      if (j == v) continue;
      const int a = corner_in ? v : j, o = corner_in ? j : v;
      const double den = c[a] - c[o];
      const double t = (c[a] - level) / den;
      if (corner_in) {
        s[j] = t;
        ds_j[j] = t / den;
        ds_v[j] = (1.0 - t) / den;
      } else {
        s[j] = 1.0 - t;
        ds_j[j] = -(1.0 - t) / den;
        ds_v[j] = -t / den;
      }
      frac *= s[j];
      sum_rest += 1.0 - s[j];
    }
    double m[NV], Q = 0.0;
    for (int j = 0; j < NV; ++j) {
      m[j] = (j == v ? 1.0 + sum_rest : s[j]) * (1.0 / NV);
      Q += psi[j] * m[j];
    }
    if (corner_in) {
      b[0] = frac;
      for (int k = 0; k < NV; ++k) b[1 + k] = frac * m[k];
    } else {
      b[0] = 1.0 - frac;
      for (int k = 0; k < NV; ++k) b[1 + k] = 1.0 / NV - frac * m[k];
    }
    const double sign = corner_in ? 1.0 : -1.0;   // S = F or sum psi / (d+1) - F
    double gv = 0.0;
    for (int j = 0; j < NV; ++j) {
      if (j == v) continue;
      double rest = 1.0;
      for (int k = 0; k < NV; ++k)
        if (k != v && k != j) rest *= s[k];
      const double dF = rest * Q + frac * ((psi[j] - psi[v]) * (1.0 / NV));
      g[j] = sign * dF * ds_j[j];
      gv += dF * ds_v[j];
    }
    g[v] = sign * gv;
    return n_in;
  }
  if constexpr (D == 3) {
    int in[2], out[2], ni = 0, no = 0;
    for (int i = 0; i < 4; ++i) {
      if (c[i] >= level) in[ni++] = i;
      else out[no++] = i;
    }
    // The prism of glims_oc_sharp in the LOCAL vertex order (a, b, e, f) = (in[0], in[1], out[0], out[1]): every index below is
    // a constant, so the forward-mode values stay in registers; only c, psi, b and g are addressed through in / out.  The
    // parameter t[x][k] (in-vertex x, out-vertex k) is direction 2 x + k.
    const double cl[4] = {c[in[0]], c[in[1]], c[out[0]], c[out[1]]};
    const double pl[4] = {psi[in[0]], psi[in[1]], psi[out[0]], psi[out[1]]};
    glims_og_d4 A[3][4], B[3][4];
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 4; ++k) A[r][k] = B[r][k] = glims_og_d4_const(0.0);
    A[0][0].v = 1.0;
    B[0][1].v = 1.0;
    double dt_in[2][2], dt_out[2][2];
    for (int k = 0; k < 2; ++k) {
      const double dena = cl[0] - cl[2 + k], denb = cl[1] - cl[2 + k];
      const double ta = (cl[0] - level) / dena;
      const double tb = (cl[1] - level) / denb;
      dt_in[0][k] = (1.0 - ta) / dena;
      dt_out[0][k] = ta / dena;
      dt_in[1][k] = (1.0 - tb) / denb;
      dt_out[1][k] = tb / denb;
      A[1 + k][0].v = 1.0 - ta;
      A[1 + k][0].d[k] = -1.0;
      A[1 + k][2 + k].v = ta;
      A[1 + k][2 + k].d[k] = 1.0;
      B[1 + k][1].v = 1.0 - tb;
      B[1 + k][1].d[2 + k] = -1.0;
      B[1 + k][2 + k].v = tb;
      B[1 + k][2 + k].d[2 + k] = 1.0;
    }
    // sigma: the determinant of (e_a, e_e, e_f, e_b) in the local coordinates 1 .. 3 -- rows (e_2 - e_0, e_3 - e_0, e_1 - e_0)
    // = ((0, 1, 0), (0, 0, 1), (1, 0, 0)), an even permutation
    const double sigma = 1.0;
    double bl[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    glims_og_d4 S = glims_og_d4_const(0.0);
    glims_og_add_tet(A[0], A[1], A[2], B[0], sigma, pl, bl, S);
    glims_og_add_tet(A[1], A[2], B[0], B[1], sigma, pl, bl, S);
    glims_og_add_tet(A[2], B[0], B[1], B[2], sigma, pl, bl, S);
    b[0] = bl[0];
    b[1 + in[0]] = bl[1];
    b[1 + in[1]] = bl[2];
    b[1 + out[0]] = bl[3];
    b[1 + out[1]] = bl[4];
    for (int x = 0; x < 2; ++x)
      for (int k = 0; k < 2; ++k) {
        g[in[x]] += S.d[2 * x + k] * dt_in[x][k];
        g[out[k]] += S.d[2 * x + k] * dt_out[x][k];
      }
  }
  return n_in;
}

// one query of one simplex, host side: b[0 .. d+1] and g = the psi-contraction of D1; returns the in-count of a SHARP query,
// -1 for the other kinds
template <int D>
inline int glims_og_moment_cell(int kind, double level, double smooth, const double (&c)[D + 1], const double (&psi)[D + 1],
                                double (&b)[D + 2], double (&g)[D + 1]) {
  if (kind == GLIMS_OC_MASS) glims_og_moment_mass<D>(c, psi, b, g);
  else if (kind == GLIMS_OC_SHARP) return glims_og_moment_sharp<D>(level, c, psi, b, g);
  else if constexpr (D == 2) glims_og_moment_smooth<2, GLIMS_DQ2_N>(level, smooth, c, glims_dq2_lam, glims_dq2_w, psi, b, g);
  else glims_og_moment_smooth<3, GLIMS_DQ3_N>(level, smooth, c, glims_dq3_lam, glims_dq3_w, psi, b, g);
  return -1;
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
