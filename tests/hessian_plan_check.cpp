// Host-side check of the adjoint calls' plan (glimslib_amd/csrc/hessian_plan.h): the buffer table against the memory formula
// it replaces, the direction tables, the per-label rows and the rank-ordered fold.  Built and run by
// tests/test_hessian_plan_cpu.py; exit status 0 = every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "hessian_plan.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static const size_t LM = GL_MAX_LABELS;

// uniform numbers in (-1, 1) from a fixed seed (64-bit LCG: the same on every host)
struct Uniform {
  uint64_t state = 0x9E3779B97F4A7C15ull;
  double operator()() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return 2.0 * (((state >> 11) + 0.5) / 9007199254740992.0) - 1.0;
  }
};

// a material table [7][LM] = D, rho, gamma, mu, lambda, E, nu with L labels
static std::vector<double> materials(Uniform& rnd, int L) {
  std::vector<double> mh(7 * LM, 0.0);
  for (int l = 0; l < L; ++l) {
    for (int row = 0; row < 3; ++row) mh[row * LM + l] = 0.6 + 0.5 * rnd();
    const double E = 1.5 + rnd(), nu = 0.2 + 0.2 * rnd();
    mh[3 * LM + l] = E / (2.0 * (1.0 + nu));
    mh[4 * LM + l] = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu));
    mh[5 * LM + l] = E;
    mh[6 * LM + l] = nu;
  }
  return mh;
}
static std::vector<double> randoms(Uniform& rnd, size_t n) {
  std::vector<double> v(n);
  for (double& x : v) x = rnd();
  return v;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// ---- the buffer table ----------------------------------------------------------------------------------------------------
// The estimate of hessian_fits as it stood at commit 2ced451 ("Volume misfit terms: fit D, rho to tumour-volume series on the
// device"), which the table's sum replaces:
//   8 ((N+1) P nn + (9P + 16) nn + [any_u] 14 nd + [any_u and el_dirs] 2 P nd + 2 n_cells + total_entries)
static size_t old_formula(const HessShape& s) {
  const size_t nn = (size_t)s.n_nodes, nd = nn * s.dim, P = (size_t)s.P;
  return 8 * ((size_t)(s.N + 1) * P * nn + (9 * P + 16) * nn + (s.any_u ? 14 * nd : 0) + (s.any_u && s.el_dirs ? 2 * P * nd : 0) +
              2 * (size_t)s.n_cells + (size_t)s.total_entries);
}
// What it stood for: (N+1) P nn = dcs;  9 P nn = nu, nu_next, dg, hrhs and the solver's five;  16 nn = dinv, the 13 node
// vectors of the first-order sweep, hd, Mhd;  14 nd = the 9 vectors of the elastic solves, urhs, du, dmurhs, dmu and the
// staging buffer (which is allocated without a displacement term too: then it was not counted);  2 P nd = dKu, dKmu;
// 2 n_cells = qcell, hqcell;  total_entries = vA.
static const std::set<std::string> counted = {
    "dcs", "nu", "nu_next", "dg", "hrhs", "mp.X", "mp.B", "mp.R", "mp.Pv", "mp.Q", "dinv", "lam", "lam_next", "rhs", "g", "r", "u",
    "w", "p", "s", "e", "hp", "Me", "tmp", "hd", "Mhd", "uk", "murhs", "mu", "mr", "mu_", "mw", "mp", "ms", "mKx", "urhs", "du",
    "dmurhs", "dmu", "stage", "dKu", "dKmu", "qcell", "hqcell", "vA"};
// What it left out
static const std::set<std::string> uncounted = {
    "ue", "uMe", "target", "part", "sums", "esums", "gather", "d_dir", "d_dmat", "d_dlame", "d_dkap", "d_dmat2", "hesums",
    "hepart", "hsums", "hpart", "mp.part", "mp.part2", "mp.sc", "mp.done", "mp.its", "mp.flags", "mp.sendbuf", "mp.rows"};
// when a buffer is allocated
static bool wanted(const std::string& n, const HessShape& s) {
  static const std::set<std::string> with_u = {"uk", "murhs", "mu", "mr", "mu_", "mw", "mp", "ms", "mKx", "urhs", "du", "dmurhs",
                                               "dmu", "ue", "uMe"};
  static const std::set<std::string> with_dirs = {"d_dlame", "d_dkap", "d_dmat2", "dKu", "dKmu"};
  static const std::set<std::string> with_ranks = {"gather", "mp.sendbuf", "mp.rows"};
  if (n == "esums") return s.el;
  if (n == "hesums" || n == "hepart") return s.el_sums;
  if (with_u.count(n)) return s.any_u;
  if (with_dirs.count(n)) return s.el_dirs;
  if (with_ranks.count(n)) return s.world > 1;
  return true;
}

static void table_against_the_old_formula() {
  const int flags[][3] = {{0, 0, 0}, {1, 1, 1}, {1, 0, 1}, {1, 1, 0}, {1, 0, 0}};   // el, a direction in E / nu, hv_E / hv_nu asked for
  for (int dim = 2; dim <= 3; ++dim)
    for (int world : {1, 4})
      for (int big = 0; big < 2; ++big)
        for (int with_u = 0; with_u < 2; ++with_u)
          for (const auto& f : flags) {
            HessShape s;
            s.N = big ? 6 : 0;
            s.P = big ? 8 : 1;
            s.dim = dim;
            s.n_labels = big ? 9 : 3;
            s.world = world;
            s.n_nodes = 1003;
            s.n_cells = dim == 2 ? 1900 : 5021;
            s.total_entries = 64 * (dim == 2 ? 117 : 251);
            s.n_send = world > 1 ? 37 : 0;
            s.spmm_blocks = 16;
            s.term_is_u = with_u ? std::vector<uint8_t>{0, 1, 0} : std::vector<uint8_t>{0, 0};
            s.any_u = hess_any_u(s.term_is_u);
            s.el = f[0];
            s.el_dirs = hess_el_dirs(s.el, s.any_u, f[1]);
            s.el_sums = hess_el_sums(s.el, s.any_u, f[2]);
            CHECK(s.any_u == (with_u != 0));
            CHECK(s.el_dirs == (f[0] && f[1] && with_u));
            CHECK(s.el_sums == (f[0] && f[2] && with_u));
            size_t extra = 0, total = 0;
            int targets = 0;
            for (const HessBuffer& b : hessian_buffers(s)) {
              const std::string n = b.name;
              CHECK(counted.count(n) + uncounted.count(n) == 1);   // a new buffer is put on one of the lists with thought
              CHECK((b.count != 0) == wanted(n, s));
              CHECK(b.elem == (n == "mp.done" || n == "mp.its" || n == "mp.flags" ? 4u : 8u));
              total += b.count * b.elem;
              if (uncounted.count(n) || (n == "stage" && !s.any_u)) extra += b.count * b.elem;
              if (n == "target") CHECK(b.count == (size_t)s.n_nodes * (s.term_is_u[targets++] ? dim : 1));
            }
            CHECK(targets == (int)s.term_is_u.size());
            CHECK(hessian_bytes(s) == total);
            CHECK(hessian_bytes(s) >= old_formula(s));
            CHECK(hessian_bytes(s) - old_formula(s) == extra);
            CHECK(hess_buffer(hessian_buffers(s), "dcs").count == (size_t)(s.N + 1) * s.P * s.n_nodes);
            // a gradient call (P = 0) takes the first-order part of the same table
            HessShape g = s;
            g.P = 0;
            g.el_dirs = g.el_sums = false;
            const std::vector<HessBuffer> full = hessian_buffers(s), first = hessian_buffers(g);
            for (size_t k = 0; k < first.size(); ++k) {
              CHECK(std::string(first[k].name) == full[k].name);
              CHECK(first[k].count == full[k].count || std::string(first[k].name) == "gather");
            }
            CHECK(std::string(first.back().name) == "gather" && std::string(full[first.size()].name) == "d_dir");
          }
  // a deformed image term observes u_k as a displacement term does; a buffer outside the table cannot be asked for
  CHECK(hess_any_u({0, 0}, true) && !hess_any_u({}, false));
  bool thrown = false;
  try {
    hess_buffer(hessian_buffers(HessShape()), "no_such_buffer");
  } catch (const std::logic_error&) {
    thrown = true;
  }
  CHECK(thrown);
}

// ---- the direction tables ------------------------------------------------------------------------------------------------
static void direction_tables() {
  Uniform rnd;
  for (int dim = 2; dim <= 3; ++dim)
    for (int L : {3, 9})
      for (int P : {1, 4})
        for (int set = 0; set < 3; ++set) {   // every direction array given, every one null, dir_nu alone
          const std::vector<double> mh = materials(rnd, L);
          const std::vector<double> vD = randoms(rnd, P * L), vrho = randoms(rnd, P * L), vgam = randoms(rnd, P * L),
                                    vE = randoms(rnd, P * L), vnu = randoms(rnd, P * L);
          const double* dD = set == 0 ? vD.data() : nullptr;
          const double* drho = set == 0 ? vrho.data() : nullptr;
          const double* dgam = set == 0 ? vgam.data() : nullptr;
          const double* dE = set == 0 ? vE.data() : nullptr;
          const double* dnu = set != 1 ? vnu.data() : nullptr;
          for (int el_dirs = 0; el_dirs < 2; ++el_dirs) {
            const HessDirections t(P, L, dim, mh.data(), dD, drho, dgam, dE, dnu, el_dirs != 0);
            CHECK(t.dir.size() == (size_t)P * 3 * LM && t.dmat.size() == (size_t)P * 5 * LM);
            CHECK(t.dlame.size() == (el_dirs ? (size_t)P * 2 * LM : 0) && t.dkap.size() == (el_dirs ? (size_t)P * LM : 0) &&
                  t.dmat2.size() == (el_dirs ? (size_t)P * 5 * LM : 0));
            CHECK(t.dir_gamma == dgam && t.dir_E == dE && t.dir_nu == dnu);
            for (int p = 0; p < P; ++p)
              for (size_t l = 0; l < LM; ++l) {
                const bool in = l < (size_t)L;
                const size_t o = (size_t)p * L + l;
                CHECK(same_bits(t.dir[(p * 3 + 0) * LM + l], in && dD ? dD[o] : 0.0));
                CHECK(same_bits(t.dir[(p * 3 + 1) * LM + l], in && drho ? drho[o] : 0.0));
                CHECK(same_bits(t.dir[(p * 3 + 2) * LM + l], in && dgam ? dgam[o] : 0.0));
                for (int row = 0; row < 5; ++row)   // the material table with the gamma row replaced by dgamma_p
                  CHECK(same_bits(t.dmat[(p * 5 + row) * LM + l], row == 2 ? (in && dgam ? dgam[o] : 0.0) : mh[row * LM + l]));
                if (!el_dirs) continue;
                double dm = 0.0, dl = 0.0;
                if (in) lame_direction(lame_derivs(mh[5 * LM + l], mh[6 * LM + l]), dE ? dE[o] : 0.0, dnu ? dnu[o] : 0.0, &dm, &dl);
                CHECK(same_bits(t.dlame[(p * 2 + 0) * LM + l], dm) && same_bits(t.dlame[(p * 2 + 1) * LM + l], dl));
                CHECK(same_bits(t.dkap[p * LM + l], in ? mh[2 * LM + l] * (2.0 * dm + dim * dl) : 0.0));
                for (int row = 0; row < 5; ++row)   // ... with the Lame rows replaced by (dm_p, dl_p)
                  CHECK(same_bits(t.dmat2[(p * 5 + row) * LM + l], row == 3 ? dm : row == 4 ? dl : mh[row * LM + l]));
              }
          }
        }
}

// ---- the per-label rows --------------------------------------------------------------------------------------------------
static void label_rows() {
  Uniform rnd;
  const int L = 3, P = 2, CAN = 4;
  const double dt = 0.37, canary = -777.25;
  for (int dim = 2; dim <= 3; ++dim)
    for (int el_dirs = 0; el_dirs < 2; ++el_dirs) {
      std::vector<double> mh = materials(rnd, L);
      mh[3 * LM + 1] = -(double)dim;   // label 1: 2 mu + d lambda == 0
      mh[4 * LM + 1] = 2.0;
      CHECK(2.0 * mh[3 * LM + 1] + dim * mh[4 * LM + 1] == 0.0);
      const std::vector<double> vgam = randoms(rnd, P * L), vE = randoms(rnd, P * L), vnu = randoms(rnd, P * L);
      const std::vector<double> sums = randoms(rnd, L * 3), esums = randoms(rnd, L * 2), hs = randoms(rnd, P * LM * 3),
                                hes = randoms(rnd, P * LM * 2);
      const HessDirections dd(P, L, dim, mh.data(), nullptr, nullptr, vgam.data(), el_dirs ? vE.data() : nullptr,
                              el_dirs ? vnu.data() : nullptr, el_dirs != 0);
      // the five outputs, each between canaries
      std::vector<double> out[5], want[5];
      for (int k = 0; k < 5; ++k) want[k].assign(P * L, 0.0);
      for (int p = 0; p < P; ++p)
        for (int l = 0; l < L; ++l) {
          const size_t o = (size_t)p * L + l;
          const double* q = &hs[(p * LM + l) * 3];
          const double gam = mh[2 * LM + l], dgam = vgam[o], dE = el_dirs ? vE[o] : 0.0, dnu = el_dirs ? vnu[o] : 0.0;
          const LameDerivs d = lame_derivs(mh[5 * LM + l], mh[6 * LM + l]);
          const double den = 2.0 * mh[3 * LM + l] + dim * mh[4 * LM + l];
          const double totA = esums[l * 2 + 0], totB = esums[l * 2 + 1], totC = den != 0.0 ? sums[l * 3 + 2] / den : 0.0;
          const double dirA = hes[(p * LM + l) * 2 + 0], dirB = hes[(p * LM + l) * 2 + 1], dirC = den != 0.0 ? q[2] / den : 0.0;
          if (l == 1) CHECK(totC == 0.0 && dirC == 0.0);
          const double dm = dE * d.m_E + dnu * d.m_nu, dl = dE * d.l_E + dnu * d.l_nu;
          want[0][o] = -dt * q[0];
          want[1][o] = -dt * q[1];
          want[2][o] = q[2];
          if (el_dirs) want[2][o] += (2.0 * dm + dim * dl) * totC;
          for (int which = 0; which < 2; ++which) {   // elastic_hessian_row of lame_derivs.h, written out
            const double mp = which == 0 ? d.m_E : d.m_nu, lp = which == 0 ? d.l_E : d.l_nu;
            const double dmp = which == 0 ? dE * d.m_EE + dnu * d.m_Enu : dE * d.m_Enu + dnu * d.m_nunu;
            const double dlp = which == 0 ? dE * d.l_EE + dnu * d.l_Enu : dE * d.l_Enu + dnu * d.l_nunu;
            const double kp = 2.0 * mp + dim * lp, dkp = 2.0 * dmp + dim * dlp;
            want[3 + which][o] =
                gam * kp * dirC - (2.0 * mp * dirA + lp * dirB) + (dgam * kp + gam * dkp) * totC - (2.0 * dmp * totA + dlp * totB);
          }
        }
      // every subset of the outputs: what is asked for is written, canaries and what is not asked for stay
      for (int mask = 0; mask < 32; ++mask) {
        double* ptr[5];
        for (int k = 0; k < 5; ++k) {
          out[k].assign(P * L + 2 * CAN, canary);
          ptr[k] = (mask >> k) & 1 ? out[k].data() + CAN : nullptr;
        }
        hessian_label_rows(dd, true, dt, mh.data(), sums.data(), hs.data(), esums.data(), hes.data(), ptr[0], ptr[1], ptr[2],
                           ptr[3], ptr[4]);
        for (int k = 0; k < 5; ++k)
          for (int i = 0; i < P * L + 2 * CAN; ++i) {
            const bool inside = i >= CAN && i < CAN + P * L;
            if (inside && ptr[k]) CHECK(same_bits(out[k][i], want[k][i - CAN]) && std::isfinite(out[k][i]));
            else CHECK(same_bits(out[k][i], canary));
          }
      }
      // without the E / nu part (glims_adjoint_hessian): the three rows alone, no extra term of the gamma row
      std::vector<double> g(P * L, canary);
      hessian_label_rows(dd, false, dt, mh.data(), sums.data(), hs.data(), nullptr, nullptr, nullptr, nullptr, g.data(), nullptr,
                         nullptr);
      for (int p = 0; p < P; ++p)
        for (int l = 0; l < L; ++l) CHECK(same_bits(g[p * L + l], hs[(p * LM + l) * 3 + 2]));
      // the first-order E / nu rows: elastic_gradient_row of lame_derivs.h, written out
      std::vector<double> gE(L + 2 * CAN, canary), gnu(L + 2 * CAN, canary);
      write_elastic_labels(mh.data(), L, dim, sums.data(), esums.data(), gE.data() + CAN, nullptr);
      write_elastic_labels(mh.data(), L, dim, sums.data(), esums.data(), nullptr, gnu.data() + CAN);
      for (int l = 0; l < L; ++l) {
        const LameDerivs d = lame_derivs(mh[5 * LM + l], mh[6 * LM + l]);
        const double den = 2.0 * mh[3 * LM + l] + dim * mh[4 * LM + l], C = den != 0.0 ? sums[l * 3 + 2] / den : 0.0;
        const double gam = mh[2 * LM + l], A = esums[l * 2], B = esums[l * 2 + 1];
        CHECK(same_bits(gE[CAN + l], gam * (2.0 * d.m_E + dim * d.l_E) * C - (2.0 * d.m_E * A + d.l_E * B)));
        CHECK(same_bits(gnu[CAN + l], gam * (2.0 * d.m_nu + dim * d.l_nu) * C - (2.0 * d.m_nu * A + d.l_nu * B)));
        CHECK(std::isfinite(gE[CAN + l]) && std::isfinite(gnu[CAN + l]));
      }
      for (int i = 0; i < CAN; ++i)
        CHECK(same_bits(gE[i], canary) && same_bits(gE[CAN + L + i], canary) && same_bits(gnu[i], canary) &&
              same_bits(gnu[CAN + L + i], canary));
    }
}

// ---- the fold of the ranks' rows -----------------------------------------------------------------------------------------
static void rank_ordered_fold() {
  Uniform rnd;
  const double big[] = {1e16, 1.0, -1e16, 1.0, 3.0};   // (1e16 + 1) - 1e16 is not 1 + (1e16 - 1e16): the order shows
  for (int world : {1, 2, 5})
    for (int L : {3, 9})
      for (int el = 0; el < 2; ++el) {
        const int P = 2;
        const std::vector<RowPart> lay = label_row_parts(L, el != 0, P);
        const size_t W = row_width(lay);
        CHECK(W == (size_t)L * 3 + (el ? (size_t)L * 2 : 0) + (size_t)P * L * 3);
        std::vector<double> rows(W * world);
        for (int r = 0; r < world; ++r)
          for (size_t k = 0; k < W; ++k) rows[W * r + k] = big[(r + k) % 5] * (1.0 + 0.25 * rnd());
        std::vector<double> out(W, -1.0);
        add_rows_in_rank_order(world, W, rows.data(), out.data());
        bool order_shows = world < 3;
        for (size_t k = 0; k < W; ++k) {
          double t = 0.0;
          for (int r = 0; r < world; ++r) t += rows[W * r + k];
          CHECK(same_bits(out[k], t));
          double back = 0.0;
          for (int r = world - 1; r >= 0; --r) back += rows[W * r + k];
          order_shows = order_shows || !same_bits(back, t);
        }
        CHECK(order_shows);
        // the row's layout: [L][3], then [L][2] with el, then [P][L][3] into [P][GL_MAX_LABELS][3]
        std::vector<double> sums(L * 3, -1.0), esums(L * 2, -1.0), hs(P * LM * 3, -1.0), hes(P * LM * 2, -1.0);
        double* dst[] = {sums.data(), esums.data(), hs.data(), hes.data()};
        scatter_row(lay, out.data(), dst);
        const size_t o_hs = (size_t)L * 3 + (el ? (size_t)L * 2 : 0);
        for (int l = 0; l < L; ++l) {
          for (int k = 0; k < 3; ++k) CHECK(same_bits(sums[l * 3 + k], out[l * 3 + k]));
          for (int k = 0; k < 2; ++k) CHECK(same_bits(esums[l * 2 + k], el ? out[L * 3 + l * 2 + k] : -1.0));
        }
        for (int p = 0; p < P; ++p)
          for (size_t l = 0; l < LM; ++l)
            for (int k = 0; k < 3; ++k)
              CHECK(same_bits(hs[(p * LM + l) * 3 + k], l < (size_t)L ? out[o_hs + ((size_t)p * L + l) * 3 + k] : -1.0));
        for (double v : hes) CHECK(v == -1.0);   // (the E / nu rows of the directions: one GPU, not part of a rank's row)
      }
}

int main() {
  table_against_the_old_formula();
  direction_tables();
  label_rows();
  rank_ordered_fold();
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  else std::printf("hessian_plan: all checks held\n");
  return failures ? 1 : 0;
}
