// The coded entry of an exactly-linear slice of the RD Jacobian (DevPattern::scode, kernels.hip): ONE 32-bit word instead of
// the fp64 value (vA, 8 B) plus the 16-bit column code (cols16, 2 B).  Read by the dot-free Krylov pass (k_cheb) for a slice
// whose entries of A = S + 2 dt N(c) ARE the entries of the static S, bit for bit (the sweep's per-slice flag `lin`).
//
//   bits [15:0]   the column code exactly as cols16 holds it;
//   bits [26:16]  an 11-bit two's-complement offset delta, |delta| <= 1023 (the code -1024 is never written);
//   bits [31:27]  the index of one of the slice's 32 dictionary bases (DevPattern::sdict, 32 x int64 per slice).
//
//   value = bits_as_double(base[index] + delta), a wrapping 64-bit integer add.
//
// The index sits on top so that one logical shift right by 27 yields it, and the delta directly below it so that one signed
// bit-field extract (shift left by 5, arithmetic shift right by 21: v_bfe_i32 on the device) yields the delta; the column code
// needs a mask only.  On a lattice of congruent cells the entries of S of one slice of 64 rows are a handful of numbers up to
// the rounding noise of the cells' determinants (a few hundred units in the last place): the dictionary rule below needs 5 to
// 9 bases for a typical slice, and the decode returns the very 64 bits vS holds.
//
// The dictionary rule (one wave per slice on the device, gl_vc_build_dictionary on the host -- the same greedy clustering):
// over the bit patterns of the slice's real entries, as signed 64-bit integers: take the smallest pattern v no base covers yet,
// make base = v + 1023, which covers [v, v + 2046]; repeat.  A slice that needs more than 32 bases is UNCODED.  Padding entries
// carry value code 0 (index 0, delta 0); the passes mask them by the row's length and never decode them.
// Plain C++ -- host and device share this one definition (tests/value_codes_check.cpp exercises it on the host).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GL_VC_HD __host__ __device__ __forceinline__
#else
#define GL_VC_HD inline
#endif

constexpr int GL_VC_BASES = 32;                            // dictionary entries per slice
constexpr int GL_VC_DELTA_BITS = 11;                       // bits [26:16]
constexpr int GL_VC_DELTA_SHIFT = 16;
constexpr int GL_VC_INDEX_SHIFT = 27;                      // bits [31:27]
constexpr int32_t GL_VC_DELTA_MAX = (1 << (GL_VC_DELTA_BITS - 1)) - 1;   // 1023: a real entry's |delta| is at most this
constexpr int64_t GL_VC_SPAN = 2 * (int64_t)GL_VC_DELTA_MAX;            // a base covers [base - 1023, base + 1023]

GL_VC_HD int64_t gl_vc_bits(double v) {
  int64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}
GL_VC_HD double gl_vc_double(int64_t b) {
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}
// the base that the rule gives the cluster whose smallest pattern is v (wrapping, like the decode's add)
GL_VC_HD int64_t gl_vc_base_for(int64_t v) { return (int64_t)((uint64_t)v + (uint64_t)GL_VC_DELTA_MAX); }
// offset of a value from a base (wrapping 64-bit arithmetic) and whether a word can hold it
GL_VC_HD int64_t gl_vc_delta(int64_t base, double v) { return (int64_t)((uint64_t)gl_vc_bits(v) - (uint64_t)base); }
GL_VC_HD bool gl_vc_fits(int64_t delta) { return delta >= -(int64_t)GL_VC_DELTA_MAX && delta <= (int64_t)GL_VC_DELTA_MAX; }
// the word of a real entry (index < 32, delta must fit) ...
GL_VC_HD uint32_t gl_vc_pack(uint32_t col16, int index, int64_t delta) {
  return (col16 & 0xffffu) | (((uint32_t)(int32_t)delta & ((1u << GL_VC_DELTA_BITS) - 1u)) << GL_VC_DELTA_SHIFT) |
         ((uint32_t)index << GL_VC_INDEX_SHIFT);
}
// ... and of a padding entry: its column code, value code 0
GL_VC_HD uint32_t gl_vc_pack_padding(uint32_t col16) { return col16 & 0xffffu; }

GL_VC_HD uint32_t gl_vc_col(uint32_t word) { return word & 0xffffu; }
GL_VC_HD int gl_vc_index(uint32_t word) { return (int)(word >> GL_VC_INDEX_SHIFT); }
GL_VC_HD int32_t gl_vc_delta_of(uint32_t word) {   // signed bit-field extract of bits [26:16]
  return (int32_t)(word << (32 - GL_VC_INDEX_SHIFT)) >> (32 - GL_VC_DELTA_BITS);
}
GL_VC_HD double gl_vc_value_at(int64_t base, int32_t delta) {
  return gl_vc_double((int64_t)((uint64_t)base + (uint64_t)(int64_t)delta));
}
GL_VC_HD double gl_vc_value(uint32_t word, int64_t base) { return gl_vc_value_at(base, gl_vc_delta_of(word)); }
// Two value codes in one register (the pass keeps them while its gathers are in flight, the column codes are spent by then):
// the upper halves of words a (low half of the pair) and b (high half); `hi` picks one back as a word whose bits [31:16] are set
GL_VC_HD uint32_t gl_vc_pair(uint32_t a, uint32_t b) { return (a >> GL_VC_DELTA_SHIFT) | (b & 0xffff0000u); }
GL_VC_HD uint32_t gl_vc_pair_word(uint32_t pair, int hi) { return hi ? pair : pair << GL_VC_DELTA_SHIFT; }

// The dictionary rule as a plain host function: `bits` = the patterns of a slice's real entries (any order; sorted in place).
// Returns the number of bases the slice needs (written to base[0 .. min(n, 32))); more than GL_VC_BASES = the slice is uncoded.
// The library itself does not call it: the words are built on the device by k_build_value_codes (kernels.hip), which finds
// the same bases with a wave-wide minimum per base instead of a sort.  This statement is what tests/value_codes_check.cpp runs
// on the host; that the device's words decode to the bits of S is what tests/test_gpu_value_codes.py checks, through results.
inline int gl_vc_build_dictionary(int64_t* bits, size_t n, int64_t base[GL_VC_BASES]) {
  std::sort(bits, bits + n);
  int nb = 0;
  size_t i = 0;
  while (i < n) {
    const int64_t v = bits[i];
    if (nb < GL_VC_BASES) base[nb] = gl_vc_base_for(v);
    ++nb;
    while (i < n && (uint64_t)bits[i] - (uint64_t)v <= (uint64_t)GL_VC_SPAN) ++i;
  }
  return nb;
}
