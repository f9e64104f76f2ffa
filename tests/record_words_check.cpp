// Host-side check of the compact incidence record word (glimslib_amd/csrc/record_words.h): packing and decoding as the header's
// comments state them, compared exactly.  Built and run by tests/test_record_words_cpu.py; exit status 0 = every check held.
#include <cstdio>
#include <vector>

#include "record_words.h"

static int failures = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static void round_trip() {
  // a weight of the flagship lattice's size, offsets over the whole range, every slot pattern of three 5-bit fields' corners
  const double w0 = 0.05 * 1.5537 * (1.0 / 120.0);
  const int64_t base = gl_rw_bits(w0);
  const int64_t offs[] = {0, 1, -1, 533, -533, 65534, 65535, -65534, -65535};
  const uint32_t slots[] = {0u, 1u, 31u, 31u << 5, 31u << 10, 0x7FFFu, 0x5A5Au, 0x2B67u};
  for (int64_t off : offs)
    for (uint32_t sl : slots) {
      const double w = gl_rw_double(base + off);
      const int64_t dl = gl_rw_delta(base, w);
      CHECK(dl == off && gl_rw_fits(dl));
      const uint32_t word = gl_rw_pack(sl, dl);
      CHECK(gl_rw_slots(word) == sl);
      CHECK(gl_rw_delta_of(word) == (int32_t)off);
      CHECK(gl_rw_delta_of(word) != GL_RW_DELTA_ZERO);
      CHECK(gl_rw_bits(gl_rw_weight(word, base)) == base + off);
      for (int m = 1; m <= 3; ++m) CHECK(gl_rw_slot_field(word, m) == (int)((sl >> (5 * (m - 1))) & 31u));
    }
}

static void limit() {
  const int64_t base = gl_rw_bits(3.0e-4);
  CHECK(gl_rw_fits((1 << 16) - 1) && gl_rw_fits(-((1 << 16) - 1)));
  CHECK(!gl_rw_fits(1 << 16) && !gl_rw_fits(-(1 << 16)));   // -2^16 is the reserved code
  CHECK(!gl_rw_fits((1 << 16) + 1) && !gl_rw_fits(-(1 << 16) - 1));
  CHECK(gl_rw_fits(gl_rw_delta(base, gl_rw_double(base + 65535))));
  CHECK(!gl_rw_fits(gl_rw_delta(base, gl_rw_double(base + 65536))));
  CHECK(!gl_rw_fits(gl_rw_delta(base, gl_rw_double(base + 65537))));
  CHECK(!gl_rw_fits(gl_rw_delta(base, 0.0)));               // a zero weight next to non-zero ones: a full slice
  CHECK(!gl_rw_fits(gl_rw_delta(base, -3.0e-4)));
  CHECK(!gl_rw_fits(gl_rw_delta(base, 6.0e-4)));
}

static void zero() {
  const int64_t bases[] = {0, gl_rw_bits(1.25e-3), gl_rw_bits(-3.0), gl_rw_bits(1e300)};
  for (int64_t base : bases) {
    const double w = gl_rw_weight(gl_rw_pack_zero(), base);
    CHECK(gl_rw_bits(w) == 0);   // +0.0, not -0.0
    CHECK(gl_rw_slots(gl_rw_pack_zero()) == 0u);
  }
  // a tissue with rho = 0: base 0, every offset 0, the word is the slot fields alone
  CHECK(gl_rw_delta(0, 0.0) == 0 && gl_rw_pack(0x1234u, 0) == 0x1234u);
  CHECK(gl_rw_bits(gl_rw_weight(0x1234u, 0)) == 0);
}

int main() {
  round_trip();
  limit();
  zero();
  // (records in a heap array: out-of-bounds or misaligned accesses of the helpers would show under a sanitizer)
  std::vector<uint32_t> words;
  const int64_t base = gl_rw_bits(2.0);
  for (int i = -65535; i <= 65535; i += 257) words.push_back(gl_rw_pack((uint32_t)(i & 0x7FFF), i));
  int k = 0;
  for (int i = -65535; i <= 65535; i += 257, ++k) CHECK(gl_rw_bits(gl_rw_weight(words[(size_t)k], base)) == base + i);
  if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
