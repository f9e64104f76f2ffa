// The per-cell diffusion tensor of the anisotropic model ("Anisotropic diffusion"): the flux of cell T with label t
// is D_t * TT_T grad c, with D_t the per-tissue scalar of glims_set_materials and TT_T a dimensionless symmetric
// positive-definite d x d tensor that glims_set_diffusion_tensor stores per cell.
//
// Packed layout, d (d + 1) / 2 doubles per cell -- the upper triangle row by row (the order of ITK's symmetric tensors):
//   2-D:  (xx, xy, yy)
//   3-D:  (xx, xy, xz, yy, yz, zz)
//
// The kernels that read the diffusion coefficient (k_assemble_static, k_sens, k_hess_rows, k_hsens) take the tensor through
// glims_dt_apply / glims_dt_form alone, so the contraction order is stated once: out_a = sum_b T_ab g_b with b ascending, then
// a^T (T b) = sum_a a_a out_a with a ascending.  Plain C++ -- host and device share this one definition
// (tests/diffusion_tensor_check.cpp exercises it on the host).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GL_DT_HD __host__ __device__ __forceinline__
#else
#define GL_DT_HD inline
#endif

// doubles per cell
template <int D>
constexpr int glims_dt_size() {
  return D * (D + 1) / 2;
}

// index of entry (a, b), a <= b, in the packed upper triangle
template <int D>
GL_DT_HD constexpr int glims_dt_index(int a, int b) {
  return a * D - a * (a - 1) / 2 + (b - a);
}

// entry (a, b) of the symmetric tensor, any order of a and b
template <int D>
GL_DT_HD double glims_dt_at(const double* T, int a, int b) {
  return a <= b ? T[glims_dt_index<D>(a, b)] : T[glims_dt_index<D>(b, a)];
}

// The tensor field of a kernel whose LAST parameters are a pack `const double*... dten`: empty in the isotropic instance, whose
// signature and kernel-argument layout therefore stay those of the kernel without the feature; one pointer otherwise
GL_DT_HD const double* glims_dt_field() { return nullptr; }
GL_DT_HD const double* glims_dt_field(const double* p) { return p; }

// out = TT g
template <int D>
GL_DT_HD void glims_dt_apply(const double* T, const double* g, double* out) {
#pragma unroll
  for (int a = 0; a < D; ++a) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < D; ++b) t += glims_dt_at<D>(T, a, b) * g[b];
    out[a] = t;
  }
}

// a^T TT b
template <int D>
GL_DT_HD double glims_dt_form(const double* T, const double* a, const double* b) {
  double Tb[D];
  glims_dt_apply<D>(T, b, Tb);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) s += a[k] * Tb[k];
  return s;
}

// every entry finite: the whole test of a TANGENT field dTT/dtheta (glims_set_diffusion_tensor_tangents), which is symmetric by
// its layout and need not be definite.  glims_dt_form takes a tangent as it takes a tensor.
template <int D>
GL_DT_HD bool glims_dt_finite(const double* T) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < glims_dt_size<D>(); ++k) ok = ok && std::isfinite(T[k]);
  return ok;
}

// symmetric positive definite: every entry finite and the leading principal minors > 0 (Sylvester's criterion)
template <int D>
GL_DT_HD bool glims_dt_spd(const double* T) {
#pragma unroll
  for (int k = 0; k < glims_dt_size<D>(); ++k)
    if (!std::isfinite(T[k])) return false;
  if (D == 2) {
    const double m2 = T[0] * T[2] - T[1] * T[1];
    return T[0] > 0.0 && m2 > 0.0;
  }
  const double xx = T[0], xy = T[1], xz = T[2], yy = T[3], yz = T[4], zz = T[5];
  const double m2 = xx * yy - xy * xy;
  const double m3 = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
  return xx > 0.0 && m2 > 0.0 && m3 > 0.0;
}

// lambda_max / lambda_min of an SPD tensor: the quadratic in 2-D, cyclic Jacobi rotations in 3-D (a fixed number of sweeps,
// accurate to rounding also where two eigenvalues coincide, as in a fibre tensor I + (r - 1) e e^T);
// glims_diffusion_tensor_info reports the largest over the cells
template <int D>
GL_DT_HD double glims_dt_ratio(const double* T) {
  if (D == 2) {
    const double m = 0.5 * (T[0] + T[2]), h = 0.5 * (T[0] - T[2]);
    const double r = std::sqrt(h * h + T[1] * T[1]);
    return (m + r) / (m - r);
  }
  double d0 = T[0], d1 = T[3], d2 = T[5], o01 = T[1], o02 = T[2], o12 = T[4];
  for (int sweep = 0; sweep < 8; ++sweep) {
    // rotate (p, q) to zero its off-diagonal entry; r is the third index: (0,1;2), (0,2;1), (1,2;0)
#define GL_DT_ROT(dp, dq, opq, opr, oqr)                                  \
    if (opq != 0.0) {                                                      \
      const double th = (dq - dp) / (2.0 * opq);                          \
      const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0)); \
      const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;        \
      dp -= t * opq;                                                       \
      dq += t * opq;                                                       \
      opq = 0.0;                                                           \
      const double pr = opr, qr = oqr;                                     \
      opr = cs * pr - sn * qr;                                             \
      oqr = sn * pr + cs * qr;                                             \
    }
    GL_DT_ROT(d0, d1, o01, o02, o12)
    GL_DT_ROT(d0, d2, o02, o01, o12)
    GL_DT_ROT(d1, d2, o12, o01, o02)
#undef GL_DT_ROT
  }
  const double lmax = std::fmax(d0, std::fmax(d1, d2)), lmin = std::fmin(d0, std::fmin(d1, d2));
  return lmax / lmin;
}
