// Host-side check of the coded entry word of exactly-linear Jacobian slices (glimslib_amd/csrc/value_codes.h): packing, decoding
// and the dictionary rule as the header's comments state them, compared exactly.  Built and run by
// tests/test_value_codes_cpu.py; exit status 0 = every check held.
#include <cstdio>
#include <vector>

#include "value_codes.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static void round_trip() {
  // entries of S of the flagship lattice's size, both signs (the diagonal is positive, most off-diagonals negative), every
  // dictionary index, offsets over the whole range, column codes at their corners
  const double vals[] = {0.731, -0.0468, 1.0e-300, -1.0e300, 0.0};
  const int64_t offs[] = {0, 1, -1, 356, -356, 1022, 1023, -1022, -1023};
  const uint32_t cols[] = {0u, 1u, 0x8000u, 0xFFFFu, 0x5A5Au};
  for (double v0 : vals)
    for (int64_t off : offs)
      for (uint32_t col : cols)
        for (int idx = 0; idx < GL_VC_BASES; ++idx) {
          const int64_t base = gl_vc_bits(v0);
          const double v = gl_vc_double((int64_t)((uint64_t)base + (uint64_t)off));
          const int64_t dl = gl_vc_delta(base, v);
          CHECK(dl == off && gl_vc_fits(dl));
          const uint32_t word = gl_vc_pack(col, idx, dl);
          CHECK(gl_vc_col(word) == col);
          CHECK(gl_vc_index(word) == idx);
          CHECK(gl_vc_delta_of(word) == (int32_t)off);
          CHECK(gl_vc_bits(gl_vc_value(word, base)) == gl_vc_bits(v));
        }
  // the whole delta range, one by one
  const int64_t base = gl_vc_bits(-2.0);
  for (int64_t off = -GL_VC_DELTA_MAX; off <= GL_VC_DELTA_MAX; ++off) {
    const uint32_t word = gl_vc_pack(0x1234u, 17, off);
    CHECK(gl_vc_delta_of(word) == (int32_t)off && gl_vc_index(word) == 17 && gl_vc_col(word) == 0x1234u);
    CHECK(gl_vc_bits(gl_vc_value(word, base)) == base + off);
  }
  // a padding entry: its column code, value code 0
  CHECK(gl_vc_pack_padding(0xBEEFu) == 0xBEEFu && gl_vc_index(0xBEEFu) == 0 && gl_vc_delta_of(0xBEEFu) == 0);
}

static void limits() {
  CHECK(GL_VC_BASES == 32 && GL_VC_DELTA_MAX == 1023 && GL_VC_SPAN == 2046);
  CHECK(GL_VC_INDEX_SHIFT == 27 && GL_VC_DELTA_SHIFT == 16 && GL_VC_DELTA_BITS == 11);
  CHECK(gl_vc_fits(1023) && gl_vc_fits(-1023));
  CHECK(!gl_vc_fits(1024) && !gl_vc_fits(-1024));   // -1024 has a bit pattern but is never written
  const int64_t b = gl_vc_bits(0.25);
  CHECK(gl_vc_fits(gl_vc_delta(b, gl_vc_double(b + 1023))) && !gl_vc_fits(gl_vc_delta(b, gl_vc_double(b + 1024))));
  CHECK(!gl_vc_fits(gl_vc_delta(b, 0.0)) && !gl_vc_fits(gl_vc_delta(b, -0.25)) && !gl_vc_fits(gl_vc_delta(b, 0.5)));
  CHECK(gl_vc_base_for(b) == b + 1023);
}

static void dictionary() {
  int64_t base[GL_VC_BASES];
  const int64_t v0 = gl_vc_bits(0.0468);
  // one cluster exactly as wide as a base covers; one ulp more needs a second base
  std::vector<int64_t> a = {v0 + 2046, v0, v0 + 7};
  CHECK(gl_vc_build_dictionary(a.data(), a.size(), base) == 1 && base[0] == v0 + 1023);
  std::vector<int64_t> b = {v0 + 2047, v0, v0 + 7};
  CHECK(gl_vc_build_dictionary(b.data(), b.size(), base) == 2 && base[0] == v0 + 1023 && base[1] == v0 + 2047 + 1023);
  // negative values sort below positive ones (signed patterns); zero between them
  std::vector<int64_t> c = {gl_vc_bits(0.5), gl_vc_bits(-0.5), 0};
  CHECK(gl_vc_build_dictionary(c.data(), c.size(), base) == 3 && base[0] == gl_vc_bits(-0.5) + 1023 && base[1] == 1023);
  // 32 well-separated values fit, 33 do not; every value is then found with a fitting offset from exactly one base
  for (int n : {32, 33}) {
    std::vector<int64_t> d;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < 5; ++j) d.push_back(v0 + (int64_t)i * 100000 + j * 400);
    const int nb = gl_vc_build_dictionary(d.data(), d.size(), base);
    CHECK(nb == n);
    if (nb <= GL_VC_BASES)
      for (int64_t p : d) {
        int hits = 0;
        for (int i = 0; i < nb; ++i) hits += gl_vc_fits(gl_vc_delta(base[i], gl_vc_double(p))) ? 1 : 0;
        CHECK(hits == 1);
      }
  }
  CHECK(gl_vc_build_dictionary(nullptr, 0, base) == 0);
}

int main() {
  round_trip();
  limits();
  dictionary();
  if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
