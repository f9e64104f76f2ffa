// Which instance of the incidence-list kernels a launch gets (kernels.hip: the assembly sweep k_rd_assemble / k_rd_assemble_s /
// k_rd_assemble_sg and the quadratic-term pass k_rd_quad / k_rd_quad_s): the one statement of that policy.  A key holds the
// template arguments; gl_sweep_key / gl_quad_key make it from what a handle and a call know at run time, and
// gl_sweep_instance / gl_quad_instance say, as constant expressions, which keys have a kernel -- the launchers instantiate
// exactly those.  An instance is added HERE: a value in a ladder or a line in a predicate, then kernels.hip's value lists.
// Plain C++17 -- no device types, no handle -- so that tests/sweep_instances_check.cpp exercises the rules on the host.
#pragma once
#include <cstddef>

enum { GL_AT_F64 = 0, GL_AT_F32 = 1 };                  // the Newton Jacobian's storage (GLIMS_FLAG_FP32_JACOBIAN: fp32)
enum { GL_ST_U32 = 0, GL_ST_U16 = 1, GL_ST_REC32 = 2 };  // the slot stream: cs2, cs16, or the compact records cr32 (record_words.h)

struct GlSweepKey {
  int nv;     // vertices per cell: 3, 4
  int cap;    // the straight-line kernels' compile-time row bound: 16 / 20 / 24 / 32; 0 = the looped kernel
  int rb;     // incidence records in flight per lane and round trip
  int cidx;   // 1: 16-bit column codes
  int at;     // GL_AT_*
  int fg;     // folded guess pass: 0 none, 1 from the guess, 2 from zero
  int mb;     // 1: the mass product from the incidence loop
  int st;     // GL_ST_*
  bool ok;    // an instance exists
};

// The straight-line kernels unroll to a compile-time bound; a class whose longest row has more than 32 entries takes the
// looped kernel.
constexpr int gl_instance_cap(int class_cap) {
  return class_cap <= 16 ? 16 : class_cap <= 20 ? 20 : class_cap <= 24 ? 24 : class_cap <= 32 ? 32 : 0;
}

// Records of the first round trip.  An interior row of a tetrahedral mesh with n entries has 2 n - 6 incidence records: rows
// of at most 16 entries get 26 = 2 x 16 - 6, so such a row needs one round trip; longer bounds, and the looped kernel, 24.
// One fewer where the guess's gather, 32-bit columns and the mass accumulator meet on cs2 -- 170 registers with 26, two waves
// per SIMD instead of three; a row of 16 entries then fetches its last record in a second round trip, the same terms in the
// same order.  With the paired 16-bit slot words (and the compact records) a round trip holds half as many slot registers: 26
// there too.
constexpr int gl_sweep_records(int nv, int cap, int cidx, int fg, int mb, int st) {
  return cap != 16 ? 24 : nv == 4 && cidx == 0 && fg == 1 && mb == 1 && st == GL_ST_U32 ? 25 : 26;
}
// ... of the quadratic-term pass (8 B per record, no Jacobian row to carry)
constexpr int gl_quad_records(int cap) { return cap == 0 ? 24 : cap == 16 ? 28 : 32; }

constexpr bool gl_instance_shape(int nv, int cap, int cidx) {
  return (nv == 3 || nv == 4) && (cap == 0 || cap == 16 || cap == 20 || cap == 24 || cap == 32) && (cidx == 0 || cidx == 1);
}
// The sweep instances.  The looped kernel: plain sweeps on cs2 only.  The guess pass and the mass product: fp64 Jacobian (what
// gl_rd_fusable asks of a handle).  The compact records: fp64 Jacobian with 16-bit column codes -- the int32-column and
// fp32-Jacobian handles keep cw + cs16.
constexpr bool gl_sweep_instance(int nv, int cap, int cidx, int at, int fg, int mb, int st) {
  if (!gl_instance_shape(nv, cap, cidx) || (at != GL_AT_F64 && at != GL_AT_F32) || fg < 0 || fg > 2 || mb < 0 || mb > 1) return false;
  if (cap == 0) return fg == 0 && mb == 0 && st == GL_ST_U32;
  if ((fg != 0 || mb != 0) && at != GL_AT_F64) return false;
  if (st == GL_ST_REC32) return at == GL_AT_F64 && cidx == 1;
  return st == GL_ST_U32 || st == GL_ST_U16;
}
constexpr bool gl_quad_instance(int nv, int cap, int cidx) { return gl_instance_shape(nv, cap, cidx); }

// class_cap: the longest row of the slice class; stream: what the straight-line kernels would read (the looped kernel reads cs2
// whatever the 16-bit words offer; it has no compact lists)
constexpr GlSweepKey gl_sweep_key(int nv, int class_cap, bool idx16, bool jac32, int fg_kind, bool mass, int stream) {
  GlSweepKey k{nv, gl_instance_cap(class_cap), 0, idx16 ? 1 : 0, jac32 ? GL_AT_F32 : GL_AT_F64, fg_kind, mass ? 1 : 0, stream, false};
  if (k.cap == 0 && k.st == GL_ST_U16) k.st = GL_ST_U32;
  k.rb = gl_sweep_records(k.nv, k.cap, k.cidx, k.fg, k.mb, k.st);
  k.ok = class_cap >= 1 && gl_sweep_instance(k.nv, k.cap, k.cidx, k.at, k.fg, k.mb, k.st);
  return k;
}
constexpr GlSweepKey gl_quad_key(int nv, int class_cap, bool idx16) {
  GlSweepKey k{nv, gl_instance_cap(class_cap), 0, idx16 ? 1 : 0, GL_AT_F64, 0, 0, GL_ST_U32, false};
  k.rb = gl_quad_records(k.cap);
  k.ok = class_cap >= 1 && gl_quad_instance(k.nv, k.cap, k.cidx);
  return k;
}

// Dynamic LDS of a launch, sized by the class's own longest row (64 lanes): the sweep keeps the Jacobian row and N(c)'s row in
// fp64, the quadratic pass one float2 per entry.
constexpr size_t gl_sweep_lds(int class_cap) { return (size_t)2 * class_cap * 64 * 8; }
constexpr size_t gl_quad_lds(int class_cap) { return (size_t)class_cap * 64 * 8; }
