// First and second derivatives of the Lame pair (m, l) = (E / (2 (1 + nu)), E nu / ((1 + nu)(1 - 2 nu))) in (E, nu), and the
// host combination of the per-label sums of the elastic adjoint into dJ/dE, dJ/dnu and their Hessian rows (DESIGN.md section
// 13, "Second order in E and nu").  Plain C++ -- no device types, no handle -- so that tests/lame_derivs_check.cpp exercises
// it on the host; device code may include it too (GL_LAME_HD).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GL_LAME_HD __host__ __device__
#else
#define GL_LAME_HD
#endif

struct LameDerivs {
  double m_E, l_E, m_nu, l_nu;               // first derivatives
  double m_EE, l_EE, m_Enu, l_Enu, m_nunu, l_nunu;   // second derivatives (m, l are linear in E)
};

// With q = (1 + nu)(1 - 2 nu) = 1 - nu - 2 nu^2, q' = -(1 + 4 nu):
//   m_E = 1 / (2 (1 + nu)),   m_nu = -E / (2 (1 + nu)^2),   m_Enu = -1 / (2 (1 + nu)^2),   m_nunu = E / (1 + nu)^3
//   l_E = nu / q,             l_nu = E (q - nu q') / q^2 = E (1 + 2 nu^2) / q^2,            l_Enu = (1 + 2 nu^2) / q^2
//   l_nunu = E (4 nu q - 2 (1 + 2 nu^2) q') / q^3 = 2 E (1 + 6 nu + 4 nu^3) / q^3
GL_LAME_HD inline LameDerivs lame_derivs(double E, double nu) {
  LameDerivs d;
  const double q = (1.0 + nu) * (1.0 - 2.0 * nu);
  d.m_E = 1.0 / (2.0 * (1.0 + nu));
  d.l_E = nu / q;
  d.m_nu = -E / (2.0 * (1.0 + nu) * (1.0 + nu));
  d.l_nu = E * (1.0 + 2.0 * nu * nu) / (q * q);
  d.m_EE = 0.0;
  d.l_EE = 0.0;
  d.m_Enu = -1.0 / (2.0 * (1.0 + nu) * (1.0 + nu));
  d.l_Enu = (1.0 + 2.0 * nu * nu) / (q * q);
  d.m_nunu = E / ((1.0 + nu) * (1.0 + nu) * (1.0 + nu));
  d.l_nunu = 2.0 * E * (1.0 + 6.0 * nu + 4.0 * nu * nu * nu) / (q * q * q);
  return d;
}

// The direction's change of a label's Lame pair: (dm, dl) = dE d_E(m, l) + dnu d_nu(m, l)
GL_LAME_HD inline void lame_direction(const LameDerivs& d, double dE, double dnu, double* dm, double* dl) {
  *dm = dE * d.m_E + dnu * d.m_nu;
  *dl = dE * d.l_E + dnu * d.l_nu;
}

// The per-label sums of the steps that a displacement term observes (u_k with its Dirichlet values, mu_k = 0 on the
// constrained dofs):  A = sum_k int_t eps(mu_k):eps(u_k),  B = sum_k int_t div mu_k div u_k,
// C = sum_k sum_T |T|/(d+1) div mu_k sum_v c_k,v
struct ElasticSums {
  double A, B, C;
};

// dJ/dp_t = gamma_t (2 m_p + d l_p) C_t - (2 m_p A_t + l_p B_t)  for (m_p, l_p) = d_p(m, l)_t
GL_LAME_HD inline double elastic_gradient_row(int dim, double gamma, double mp, double lp, const ElasticSums& s) {
  return gamma * (2.0 * mp + dim * lp) * s.C - (2.0 * mp * s.A + lp * s.B);
}

// (H dm)_{p_t}, p = E (which = 0) or nu (which = 1), from the totals `tot` of the gradient and the direction's sums `dir`
// (dir.A = sum_k A_t(dmu_k, u_k) + A_t(mu_k, du_k), dir.B likewise, dir.C = sum_k C_t(dmu_k, c_k) + C_t(mu_k, dc_k)):
//   gamma_t kappa(m_p, l_p) dir.C - 2 m_p dir.A - l_p dir.B
//   + [dgamma_t kappa(m_p, l_p) + gamma_t kappa(dm_p, dl_p)] tot.C - 2 dm_p tot.A - dl_p tot.B,
// kappa(m, l) = 2 m + d l and (dm_p, dl_p) = dE d_pE(m, l) + dnu d_pnu(m, l).
GL_LAME_HD inline double elastic_hessian_row(int dim, int which, const LameDerivs& d, double gamma, double dgamma, double dE,
                                             double dnu, const ElasticSums& tot, const ElasticSums& dir) {
  const double mp = which == 0 ? d.m_E : d.m_nu, lp = which == 0 ? d.l_E : d.l_nu;
  const double dmp = which == 0 ? dE * d.m_EE + dnu * d.m_Enu : dE * d.m_Enu + dnu * d.m_nunu;
  const double dlp = which == 0 ? dE * d.l_EE + dnu * d.l_Enu : dE * d.l_Enu + dnu * d.l_nunu;
  const double kp = 2.0 * mp + dim * lp, dkp = 2.0 * dmp + dim * dlp;
  return gamma * kp * dir.C - (2.0 * mp * dir.A + lp * dir.B) + (dgamma * kp + gamma * dkp) * tot.C -
         (2.0 * dmp * tot.A + dlp * tot.B);
}
