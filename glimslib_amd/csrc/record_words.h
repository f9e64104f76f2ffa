// The compact (row, cell) incidence record of the straight-line assembly sweeps (DevPattern::cr32, kernels.hip): ONE 32-bit
// word instead of the fp64 reaction weight (cw, 8 B) plus the 16-bit slot word (cs16, 2 B).
//
//   bits [14:0]   the slot fields exactly as cs16 holds them: the row's own slot dropped, the slot of the cell's m-th other
//                 vertex in bits [5 (m-1), 5 m), m = 1 .. NV-1 (padding records 0);
//   bits [31:15]  a 17-bit two's-complement offset delta: weight = bits_as_double(base + delta), where `base` is the 64-bit
//                 pattern of the slice's first real record's weight (lowest record index, then lowest lane) and the sum is an
//                 integer one.  The code -2^16 is reserved: it decodes to +0.0 (padding records).
//
// On a mesh of congruent cells with one rho per tissue the weights rho_T |T| d!/(d+3)! of a slice are one number up to the
// rounding noise of the cells' determinants, a few hundred units in the last place: the offsets fit with two decades to spare
// and the decode returns the very 64 bits that cw holds -- no table, no memory access, an integer add on a register.  A slice
// is COMPACT when every real record's offset lies in [-(2^16 - 1), 2^16 - 1]; every other slice is FULL and keeps cw + cs16.
// (A slice of a tissue with rho = 0: base 0, every offset 0.)  Plain C++ -- host and device share this one definition
// (tests/record_words_check.cpp exercises it on the host).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GL_RW_HD __host__ __device__ __forceinline__
#else
#define GL_RW_HD inline
#endif

constexpr int GL_RW_SLOT_BITS = 15;                       // bits [14:0]
constexpr uint32_t GL_RW_SLOT_MASK = (1u << GL_RW_SLOT_BITS) - 1u;
constexpr int32_t GL_RW_DELTA_MAX = (1 << 16) - 1;        // a real record's |delta| is at most this
constexpr int32_t GL_RW_DELTA_ZERO = -(1 << 16);          // the reserved code: weight +0.0

GL_RW_HD int64_t gl_rw_bits(double w) {
  int64_t b;
  memcpy(&b, &w, sizeof(b));
  return b;
}
GL_RW_HD double gl_rw_double(int64_t b) {
  double w;
  memcpy(&w, &b, sizeof(w));
  return w;
}
// offset of a real record's weight from the slice base (wrapping 64-bit arithmetic, as the decode's add)
GL_RW_HD int64_t gl_rw_delta(int64_t base, double w) { return (int64_t)((uint64_t)gl_rw_bits(w) - (uint64_t)base); }
GL_RW_HD bool gl_rw_fits(int64_t delta) { return delta >= -(int64_t)GL_RW_DELTA_MAX && delta <= (int64_t)GL_RW_DELTA_MAX; }
// the record word of a real record (delta must fit) ...
GL_RW_HD uint32_t gl_rw_pack(uint32_t slots15, int64_t delta) {
  return (slots15 & GL_RW_SLOT_MASK) | ((uint32_t)(int32_t)delta << GL_RW_SLOT_BITS);
}
// ... and of a padding record: weight +0.0, slots 0
GL_RW_HD uint32_t gl_rw_pack_zero() { return (uint32_t)GL_RW_DELTA_ZERO << GL_RW_SLOT_BITS; }

GL_RW_HD uint32_t gl_rw_slots(uint32_t word) { return word & GL_RW_SLOT_MASK; }
GL_RW_HD int gl_rw_slot_field(uint32_t word, int m) { return (int)((word >> (5 * (m - 1))) & 31u); }   // m = 1 .. NV-1
GL_RW_HD int32_t gl_rw_delta_of(uint32_t word) { return (int32_t)word >> GL_RW_SLOT_BITS; }               // arithmetic shift
GL_RW_HD double gl_rw_weight(uint32_t word, int64_t base) {
  const int32_t delta = gl_rw_delta_of(word);
  const double w = gl_rw_double((int64_t)((uint64_t)base + (uint64_t)(int64_t)delta));
  return delta == GL_RW_DELTA_ZERO ? 0.0 : w;
}
