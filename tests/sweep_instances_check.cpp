// Host-side check of the instance policy of the incidence-list kernels (glimslib_amd/csrc/sweep_instances.h): every input of
// gl_sweep_key and gl_quad_key against tables written down here as literals.  Built and run by
// tests/test_sweep_instances_cpu.py; exit status 0 = every check held.
#include <cstdio>
#include <set>
#include <tuple>

#include "sweep_instances.h"

static int failures = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      if (++failures <= 20)                                                                                            \
        std::fprintf(stderr, "line %d: %s  [nv %d cap %d idx16 %d jac32 %d fg %d mass %d stream %d]\n", __LINE__, #cond, nv, \
                     cc, idx16, jac32, fg, mass, st);                                                                  \
    }                                                                                                                  \
  } while (0)

// the tables: longest row of the class -> bound of the straight-line instance (0: the looped kernel), records per round trip
static int expect_cap(int cc) {
  if (cc <= 16) return 16;
  if (cc <= 20) return 20;
  if (cc <= 24) return 24;
  if (cc <= 32) return 32;
  return 0;
}
static int sweep_records(int cap) {
  switch (cap) {
    case 16: return 26;
    case 20: return 24;
    case 24: return 24;
    case 32: return 24;
    default: return 24;   // looped
  }
}
static int quad_records(int cap) {
  switch (cap) {
    case 16: return 28;
    case 20: return 32;
    case 24: return 32;
    case 32: return 32;
    default: return 24;   // looped
  }
}

typedef std::tuple<int, int, int, int, int, int, int, int> Key;
static Key tup(const GlSweepKey& k) { return Key(k.nv, k.cap, k.rb, k.cidx, k.at, k.fg, k.mb, k.st); }

int main() {
  std::set<Key> sweep, plain_s, looped, fused, quad;
  int n25 = 0;
  for (int nv = 3; nv <= 4; ++nv)
    for (int cc = 1; cc <= 64; ++cc)
      for (int idx16 = 0; idx16 <= 1; ++idx16) {
        int jac32 = 0, fg = 0, mass = 0, st = 0;
        {
          const GlSweepKey q = gl_quad_key(nv, cc, idx16 != 0);
          const int cap = expect_cap(cc);
          CHECK(q.ok && q.nv == nv && q.cap == cap && q.cidx == idx16 && q.rb == quad_records(cap));
          CHECK(q.at == GL_AT_F64 && q.fg == 0 && q.mb == 0 && q.st == GL_ST_U32);
          CHECK(gl_quad_instance(q.nv, q.cap, q.cidx));
          CHECK(gl_quad_lds(cc) == (size_t)cc * 64 * 8 && gl_sweep_lds(cc) == (size_t)2 * cc * 64 * 8);
          quad.insert(tup(q));
        }
        for (jac32 = 0; jac32 <= 1; ++jac32)
          for (fg = 0; fg <= 2; ++fg)
            for (mass = 0; mass <= 1; ++mass)
              for (st = 0; st <= 2; ++st) {
                const GlSweepKey k = gl_sweep_key(nv, cc, idx16 != 0, jac32 != 0, fg, mass != 0, st);
                const int cap = expect_cap(cc);
                // refusals: the guess pass and the mass product where gl_rd_fusable says no (an fp32 Jacobian, a class of the
                // looped kernel); the compact records without an fp64 Jacobian and 16-bit column codes, or on a looped class
                const bool fusable = !jac32 && cc <= 32;
                const bool refused = ((fg != 0 || mass) && !fusable) || (st == GL_ST_REC32 && (jac32 || !idx16 || cc > 32));
                CHECK(k.ok == !refused);
                CHECK(k.ok == gl_sweep_instance(k.nv, k.cap, k.cidx, k.at, k.fg, k.mb, k.st));
                if (!k.ok) continue;
                CHECK(k.nv == nv && k.cap == cap && k.cidx == idx16 && k.at == (jac32 ? GL_AT_F32 : GL_AT_F64));
                CHECK(k.fg == fg && k.mb == mass);
                // the looped kernel reads cs2 whatever the 16-bit words offer
                CHECK(k.st == (cap == 0 ? GL_ST_U32 : st));
                const bool one_fewer = nv == 4 && !idx16 && fg == 1 && mass && cc <= 16 && st == GL_ST_U32;
                CHECK(k.rb == (one_fewer ? 25 : sweep_records(cap)));
                n25 += k.rb == 25;
                sweep.insert(tup(k));
                (cap == 0 ? looped : fg != 0 ? fused : plain_s).insert(tup(k));
              }
      }
  // refusals outside the handles' range
  {
    int nv = 5, cc = 12, idx16 = 1, jac32 = 0, fg = 0, mass = 0, st = 3;
    CHECK(!gl_sweep_key(5, 12, true, false, 0, false, GL_ST_U16).ok && !gl_quad_key(5, 12, true).ok);
    CHECK(!gl_sweep_key(3, 0, true, false, 0, false, GL_ST_U16).ok && !gl_quad_key(3, 0, true).ok);
    CHECK(!gl_sweep_key(3, 12, true, false, 3, false, GL_ST_U16).ok && !gl_sweep_key(3, 12, true, false, 0, false, 3).ok);
    // the sixteen classes of at most 16 entries of that one combination: the only 25s
    CHECK(n25 == 16);
    CHECK(plain_s.size() == 112 && looped.size() == 8 && fused.size() == 160 && sweep.size() == 280);
    CHECK(quad.size() == 20);
  }
  if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
