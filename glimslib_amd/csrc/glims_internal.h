// Internal declarations of libglimship.so (gfx950 only; no CPU fallback, no portability layer).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>
#include <stdexcept>
#include "../../include/glims_hip.h"
#include "step_policy.h"
#include "mech_policy.h"

#define GL_WAVE 64                 // wavefront width of CDNA4; SELL slice height
#define GL_SIGMA 256               // sigma window (rows) of the SELL-C-sigma row sort (tools/sigma_sweep.py: on an
                                   // unstructured mesh 256 beats 4096 by 1.7x in SpMV time despite +17 % padding)
#define GL_MAX_LABELS 256
// 16-bit column codes: the columns of one 64-row slice fall into a few compact ranges of the Morton numbering (the
// neighbouring 4x4x4 blocks), so a code = (window id, offset) against a per-slice table of GL_N_WIN window bases
// covers every slice of the BASELINE meshes and of 1 M-point Delaunay meshes (tools/pattern_stats.cpp); the SpMV then
// streams 2 B instead of 4 B of index per entry.  Slices that need more windows fall back to the 32-bit stream.
#define GL_WIN_BITS 11
#define GL_N_WIN 32
// multigrid, partitioned runs with glims_set_mg_frame: the auxiliary grids are replicated on every rank; the operator of
// the first one (stencil entries x block entries x 4 B per node: 27 x 9 x 4 B for elasticity on a lattice mesh = 4 M
// nodes, 125 x 9 x 4 B on a general mesh = 0.9 M nodes) may take at most this many bytes -- beyond it the grid spacing
// is widened until it fits
#define GL_MG_GLOBAL_BYTES (4ll << 30)
// Blocks are dealt to the 8 XCDs in chunks of this many consecutive logical blocks: neighbouring slices (overlapping x
// gathers) share one L2 while the XCDs together still walk the matrix front to back (measured: time of the plain
// mapping, fabric reads 2.21 -> 1.97 GB per SpMV at 10 M rows; contiguous eighths are 1-5 % slower).
// glims_options.stream_policy = AUTO: Krylov working sets up to this many bytes stream the operator with the default cache policy
// (measured, profiles/r05_ab_rank_sized.txt: at 269 MB -- C4 / 8 -- cached loads win by 6-7 %, at 2.2 GB -- C4 -- the two are equal)
#define GL_STREAM_CACHED_LIMIT (1024ll << 20)
// (chunks of 128-512 blocks change the in-step kernel times by <= 2 %: profiles/r04_ab_xcd_chunk.txt)
#define GL_XCD_CHUNK 64
// ... and a bit above it in the straight-line sweeps' `remap` argument: store every slice of vA (GLIMS_FLAG_STORE_LINEAR_SLICES)
#define GL_SWEEP_STORE_ALL (1 << 16)

struct glims_error : std::runtime_error {
  int code;
  glims_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define GL_HIP(expr)                                                                            \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      throw glims_error(GLIMS_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + \
                                         __FILE__ + ":" + std::to_string(__LINE__) + ")");      \
  } while (0)

#define GL_NCCL(expr)                                                                              \
  do {                                                                                             \
    ncclResult_t _r = (expr);                                                                      \
    if (_r != ncclSuccess)                                                                         \
      throw glims_error(GLIMS_E_RCCL, std::string(#expr) + ": " + ncclGetErrorString(_r) + " (" + \
                                          __FILE__ + ":" + std::to_string(__LINE__) + ")");        \
  } while (0)

#define GL_REQUIRE(cond, msg)                                  \
  do {                                                         \
    if (!(cond)) throw glims_error(GLIMS_E_USAGE, (msg));      \
  } while (0)

// Device array with explicit lifetime (no implicit copies).
template <class T>
struct dvec {
  T* p = nullptr;
  size_t n = 0;
  dvec() = default;
  dvec(const dvec&) = delete;
  dvec& operator=(const dvec&) = delete;
  ~dvec() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count) {
    if (count == n && p) return;
    release();
    if (count) GL_HIP(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
  }
  void alloc_zero(size_t count, hipStream_t s) {
    alloc(count);
    if (count) GL_HIP(hipMemsetAsync(p, 0, count * sizeof(T), s));
  }
  void upload(const T* h, size_t count, hipStream_t s) {
    alloc(count);
    if (count) GL_HIP(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void upload(const std::vector<T>& h, hipStream_t s) { upload(h.data(), h.size(), s); }
};

// blocks of bs threads that cover n items (at least one)
inline unsigned grid_of(int64_t n, int bs = 256) { return (unsigned)std::max<int64_t>(1, (n + bs - 1) / bs); }

// Host-side result of the symbolic phase (setup_host.cpp).
struct HostPattern {
  int dim = 0, nv = 0;
  int64_t n_nodes = 0, n_own = 0, n_cells = 0;
  std::vector<int32_t> old2new, new2old;   // node renumbering (ghosts keep their place)
  int32_t n_slices = 0;                    // ceil(n_own / 64)
  std::vector<int64_t> slice_ptr;          // [n_slices+1] offsets into cols (multiples of 64)
  std::vector<int32_t> cols;               // SELL-64 column indices (new numbering), padded with the row itself
  // compressed column stream: cols16 = (window << GL_WIN_BITS) | offset, column = win_base[slice][window] + offset;
  // slices whose columns need more than GL_N_WIN windows keep win_ok = 0 and are read through `cols`
  std::vector<uint16_t> cols16;
  std::vector<int32_t> win_base;           // [n_slices * GL_N_WIN]
  std::vector<uint8_t> win_ok;             // [n_slices]
  int64_t n_compressed = 0;                // slices with win_ok
  std::vector<uint8_t> diag_k;             // [n_slices*64] slot of the diagonal in each row
  std::vector<uint8_t> rlen;               // [n_slices*64] stored entries of each row (0 on the padding rows of the last slice)
  std::vector<int64_t> cslice_ptr;         // [n_slices+1] offsets into the (row, cell) incidence arrays
  std::vector<uint32_t> cslots;            // 4 x uint8: slot (within the row) of each vertex of the cell
  std::vector<int32_t> celem;              // cell id, -1 = padding
  std::vector<int32_t> interior_slices, boundary_slices;   // boundary = references a ghost column
  // slices grouped by row-length class (LDS footprint of the assembly sweep): bucket b holds the slices with
  // bucket_cap[b-1] < len <= bucket_cap[b]
  std::vector<int> bucket_cap;
  std::vector<std::vector<int32_t>> bucket_slices;
  std::vector<int32_t> bucket_interior;      // leading entries of bucket_slices[b] that are interior slices
  int max_len = 0, max_clen = 0;
  int64_t nnz = 0, n_corners = 0;
};

struct glims_ctx;
// symbolic.hip: the same phase on the device (the default; the host version above stays as its cross-check)
// cells_p (out): the connectivity in the internal cell order (caller's vertex indices), for the per-cell geometry
void gl_build_pattern_device(glims_ctx* h, const double* d_xyz, const int32_t* d_cells, dvec<int32_t>& cells_p);
int gl_host_threads();   // OpenMP team the host phases may use (affinity mask, cgroup quota, ranks per host)
void build_host_pattern(HostPattern& hp, int dim, int64_t n_nodes, int64_t n_own, int64_t n_cells,
                        const double* xyz, const int32_t* cells);

// Everything a wave of the incidence-list kernels needs to know about its slice, in ONE 40-byte scalar load (the chain
// slice list -> slice offsets -> incidence offsets -> window flag was four dependent memory round trips before a wave could
// issue its first useful load)
struct SliceDesc {
  int64_t base, cbase;     // first entry / first incidence record of the slice
  int32_t s;               // slice
  int32_t len, clen;       // entries / incidence records per lane
  int32_t ok;              // the slice has 16-bit column codes
  int64_t wbase;           // compact record words (record_words.h): the bit pattern the slice's weight offsets count from
};

// Slices of similar length that the incidence-list kernels launch together (kernels.hip, ensure_classes)
struct SliceClass {
  int cap = 0;                 // longest slice of the class, entries per lane (= LDS columns of its launches)
  int n = 0, n_interior = 0;   // slices; the interior ones (no ghost column) come first
  dvec<SliceDesc> desc;        // ... as descriptors (straight-line kernels)
  dvec<int32_t> list;          // ... as plain slice ids (looped kernels, classes of more than 32 entries per row)
  std::vector<int32_t> host_list;   // ... the same on the host
  // the same slices split by record stream (straight-line classes; rebuilt when the weights change, kernels.hip): compact
  // interior, compact boundary, full interior, full boundary -- each in the order of `desc`
  dvec<SliceDesc> rdesc;
  int n_compact[2] = {0, 0}, n_full[2] = {0, 0};   // [interior, boundary]
};

// Device-resident SELL-64 sparsity + incidence lists.
struct DevPattern {
  int32_t n_slices = 0;
  int max_len = 0, max_clen = 0;
  dvec<int64_t> slice_ptr;
  dvec<int32_t> cols;
  dvec<uint16_t> cols16;
  dvec<int32_t> win_base;
  dvec<uint8_t> win_ok;
  dvec<uint8_t> diag_k;
  dvec<uint8_t> rlen;                      // entries of each row: the SpMV's lanes stop there (slots beyond are padding)
  dvec<int64_t> cslice_ptr;
  dvec<uint32_t> cslots;
  dvec<int32_t> celem;
  dvec<double> cw;                         // per-incidence reaction weight rho_T |T| d!/(d+3)!
  dvec<uint32_t> cs2;                      // slot word re-ordered for the hot kernels: byte 0 = the row's own (diagonal) slot, then the cell's other vertices
  dvec<uint32_t> cs16;                     // the straight-line sweeps' 16-bit slot words (own slot dropped, 5 bits per other vertex), two records of a lane per element (k_corner_weights); empty = not valid, the sweeps read cs2
  dvec<uint32_t> cr32;                     // the straight-line sweeps' compact records (record_words.h): slot fields of cs16 + the weight's offset from the slice base, 4 B instead of cw + cs16's 10; empty = none (no cs16), the sweeps read cw + cs16 / cs2
  dvec<int64_t> rec_base;                  // ... per slice: the base (bit pattern of its first real record's weight)
  dvec<uint8_t> rec_ok;                    // ... per slice: 1 = compact (straight-line slice whose every offset fits), 0 = full
  std::vector<uint8_t> rec_ok_host;        // ... the same on the host (k_corner_weights ran: the classes' record lists are stale)
  bool rec_lists_stale = true;
  // the coded entries of S for the dot-free pass (value_codes.h; built after every k_assemble_static, kernels.hip): empty = none
  dvec<uint32_t> scode;                    // per padded entry, SELL layout of vS: column code + value code (dictionary index, delta)
  dvec<int64_t> sdict;                     // ... per slice: its 32 dictionary bases (bit patterns)
  dvec<uint8_t> scoded;                    // ... per slice: 1 = every real entry has a code (at most 32 bases), 0 = uncoded
  dvec<uint32_t> cq;                       // [incidence][2] = (re-ordered slot word, weight as float bits): the quadratic-term pass's 8-byte records
  // the mass product from the sweep's incidence loop (k_corner_weights, rd_assemble_s_slice with MB = 1)
  dvec<double> mass_q;                     // per padded row: (d+3) / rho where every cell of the row has the same rho > 0, else 0
  dvec<int32_t> mass_fb_slices;            // slices with an owned row of mass_q = 0: these keep the mass SpMV (fallback rows)
  int32_t n_mass_fb = 0;                   // ... their number
  int64_t mass_fb_rows = 0;                // owned rows with mass_q = 0
  dvec<int32_t> interior_slices, boundary_slices;
  int32_t n_interior = 0, n_boundary = 0;
  std::vector<int> bucket_cap;
  std::vector<int32_t> bucket_count;
  std::vector<int32_t> bucket_interior;
  std::vector<dvec<int32_t>*> bucket_slices;   // owned; released in ~DevPattern
  std::vector<SliceClass*> classes;            // launch classes of the incidence-list kernels (built on first use, kernels.hip)
  ~DevPattern() {
    for (auto* b : bucket_slices) delete b;
    for (auto* c : classes) delete c;
  }
  int64_t total_entries = 0, total_corners = 0;
};

// Node-local all-reduce through a mailbox in host shared memory that every rank's GPU maps (fine-grained): slot
// [parity][rank] = {seq, v[0..3]} (64 B).  Fused into the final block of the reduction kernels: no extra launch and
// a few microseconds of PCIe latency instead of an RCCL kernel per Krylov iteration.  `seq` lives on the device and
// only advances when the kernel really runs (kernels skipped by the `done` word must not consume a number).
struct NodeMail {
  double* slots = nullptr;             // device address of the mapping; nullptr = not in use
  unsigned long long* seq = nullptr;   // device counter
  int* err = nullptr;                  // device flag: a peer did not arrive in time
  int rank = 0, world = 1;
  long long timeout_ticks = 60ll * 100000000ll;   // wall_clock64 runs at 100 MHz
};

// ---- elasticity multigrid (mg.hip) --------------------------------------------------------------------------
// Auxiliary-grid geometric multigrid for K_el: level 0 is the mesh itself (SELL-64 blocks, single-precision copy),
// level 1 a Cartesian grid of width H ~ 2h laid over the mesh (d-linear interpolation onto the mesh nodes), levels
// 2.. its 2:1 coarsenings.  Coarse operators are Galerkin products stored as dense stencils: no column indices on
// any coarse level, every stream unit-stride over the grid nodes.
struct MgGrid {
  int n[3] = {1, 1, 1};                    // nodes per axis (n[2] = 1 in 2-D)
  int64_t nn = 1;
};
struct MgLevel {                           // one Cartesian level
  MgGrid g;
  int f[3] = {1, 1, 1};                    // coarsening factor per axis towards the next level (1 | 2)
  int o[3] = {0, 0, 0};                    // global index of this box's node 0 (partitioned runs; 0 otherwise)
  int ng[3] = {1, 1, 1};                   // nodes per axis of the level's GLOBAL grid
  bool global = false;                     // replicated on every rank (box = whole grid), residual all-reduced per cycle
  // storage box of the OPERATOR planes (A / A16): lo[3], n[3]; sb_nn = 0: the whole grid.  Box-limited partitioned runs keep
  // the first grid's operator rows for the rank's work box only (vectors, dinv and sc stay whole-grid arrays)
  int sb[6] = {0, 0, 0, 0, 0, 0};
  long long sb_nn = 0;
  dvec<float> A;                           // [S][bs*bs][rows] stencil-major planes (rows = sb_nn or nn)
  bool half = false;                       // smoothed in symmetrically scaled variables with the half-precision copy A16
  dvec<uint16_t> A16;                      // [S][bs*bs][nn] _Float16 planes of S A S, S = diag(1 / sqrt(a_ii))   (half only)
  dvec<double> sc;                         // [bs][nn] the scale factors s; dinv then holds (S A S)_ii^-1       (half only)
  dvec<double> dinv;                       // [bs*bs][nn] inverse diagonal blocks
  dvec<double> x, x2, r, d, res;           // [bs][nn] (component-major)
  double lam = 1.0;                        // estimate of lambda_max(Dinv A)
};
// Neighbour exchange that replaces the all-reduce of the first grid's restricted residual in a box-limited partitioned
// cycle: rank p needs the sum on its work box only, and rank q's partial sums are nonzero only on q's core, so p receives
// (box_p n core_q) from q and sends (box_q n core_p) -- boxes every rank derives from the all-gathered cores.
struct GridRegion {
  int lo[3], n[3];
  int rank;              // the peer this region comes from / goes to
  long long off;         // first node of the region in the message buffers (nodes, not doubles)
};
struct GridExchange {
  bool ready = false;
  int deg = 0;                               // smoother degree the boxes were sized for (a larger one falls back to the all-reduce)
  std::vector<int32_t> peers;                // ascending rank
  std::vector<int64_t> send_ptr, recv_ptr;   // per peer, in nodes
  int n_send_reg = 0, n_recv_reg = 0;
  long long n_send = 0, n_recv = 0;          // nodes
  dvec<GridRegion> send_reg, recv_reg;       // ascending peer rank
  dvec<double> sendbuf, recvbuf;             // [node][bs]
  void reset() {
    ready = false;
    peers.clear();
    send_ptr.clear();
    recv_ptr.clear();
    n_send_reg = n_recv_reg = 0;
    n_send = n_recv = 0;
  }
};
struct MgHierarchy {
  bool ready = false;
  // The operator this hierarchy preconditions (set by the caller of gl_mg_setup; borrowed pointers that must stay valid
  // while `ready`): K_el with bs = dim (elasticity), or the static part S of the RD Jacobian with bs = 1.
  int bs = 0;                              // dofs per mesh node
  const double* op_vals = nullptr;         // fp64 SELL-64 planes [entry][bs * bs][64]
  const uint8_t* op_fixed = nullptr;       // constrained dofs [n_nodes * bs], nullptr = none
  const double* op_dinv = nullptr;         // fp64 inverse diagonal blocks of the constrained operator [n_own][bs * bs]
  dvec<double> own_dinv;                   // ... kept here when nobody else owns them (RD hierarchy)
  dvec<uint16_t> v16;                      // level 0: half-precision copy of S A S (bit pattern of _Float16)
  bool lattice = false;
  int n_levels = 0;                        // incl. the mesh itself
  int64_t cycles = 0;
  double complexity = 0.0, ms_setup = 0.0;
  int R = 1, S = 27;                       // stencil radius / entries of the Cartesian levels
  double lo[3] = {0, 0, 0}, H[3] = {1, 1, 1};
  dvec<int32_t> cell0;                     // [n_own] lower-corner grid node of the level-1 cell that holds a mesh node
  dvec<double> wgt;                        // [n_own][dim] interpolation weight towards the upper node, per axis
  dvec<int32_t> cell_ptr, cell_nodes;      // mesh nodes sorted by level-1 cell (children lists of the grid nodes)
  // restriction mesh -> grid as an explicit operator, SELL-64 over the grid nodes: (child, weight) pairs
  dvec<int64_t> pt_ptr;                    // [ceil(nn / 64) + 1]
  dvec<int32_t> pt_idx;
  dvec<float> pt_w;
  dvec<double> x, x2, d, res;              // level-0 work vectors [n_nodes*bs] (ghost slots stay zero)
  double lam0 = 1.0;
  double cheb_ratio = 30.0;                // the smoothers' interval is [lambda_max / cheb_ratio, lambda_max]
  double default_ratio = 30.0;             // ... its default for this mesh (mg_setup_t), used when glims_options.mg_cheb_ratio = 0
  double dropped_fraction = 0.0;           // mesh edges whose parents lie more than two grid cells apart (not in the coarse operators)
  bool half_smoother = true;               // level-0 smoother streams the half-precision copy of K_el
  bool x32 = false;                        // level-0 cycle vectors in single precision (XNode<BS, float> layout)
  bool exact_level0 = false;               // partitioned run with a global frame: level-0 passes see the ghosts (halo exchange)
  // partitioned run with a global frame, replicated first grid: each rank smooths only its work box of that grid
  bool boxed = false;
  int core[6] = {0, 0, 0, 0, 0, 0};        // this rank's core on the first grid: lo[3], hi[3] (inclusive) of the nodes its own mesh nodes interpolate from
  dvec<int> cores;                         // every rank's core [world][6] (owner rule of the first-grid -> second-grid restriction)
  double box_fraction = 1.0;               // work box / first grid at the set-up's smoother degree
  GridExchange gx;                         // first-grid residual: neighbour exchange instead of the all-reduce (boxed only)
  dvec<double> sc;                         // level-0 scaling s = 1 / sqrt(diag K_el) per dof (1 on constrained dofs)
  dvec<float> dinv0;                       // inverse diagonal blocks of the scaled operator S K S, single precision
  dvec<float> vK32s;                       // single-precision scaled copy (GLIMS_FLAG_MG_FP32_SMOOTHER only)
  dvec<double> rs;                         // scaled residual r~ = S r of the current cycle
  std::vector<MgLevel*> lv;                // owned
  dvec<double> coarse_inv;                 // dense inverse of the coarsest operator [nc][nc], nc = lv.back()->g.nn * bs
  int64_t entries = 0;                     // stored operator entries of the coarse levels (scalars)
  void clear() {
    for (auto* l : lv) delete l;
    lv.clear();
    ready = false;
  }
  ~MgHierarchy() { clear(); }
};
// what glims_create keeps of the mesh geometry for the multigrid set-up
struct MeshMetrics {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  double h_lattice[3] = {0, 0, 0};         // lattice constant per axis if the nodes form a lattice
  bool lattice = false;
  double mean_edge = 0.0;
};

// halo payload of one owned row, written by the kernel that has just produced the row's value(s)
struct PackMap {
  const int32_t* ref = nullptr;    // [n_own]: -1 or index into ptr; nullptr = no fused packing
  const int32_t* ptr = nullptr;
  const int32_t* slot = nullptr;
  double* sendbuf = nullptr;
};

#ifdef __HIPCC__
// Node-local all-reduce of red[0..nq) (see NodeMail): called by every thread of the (single) final reduction block.
// Sums in rank order on every rank -> the same bits everywhere, hence identical decisions.
static __device__ __forceinline__ void node_allreduce(double* __restrict__ red, int nq, const NodeMail nm) {
  __syncthreads();   // red[] written by threads < nq
  if (threadIdx.x >= GL_WAVE) return;
  const int lane = threadIdx.x;
  unsigned long long seq = 0;
  if (lane == 0) {
    seq = *nm.seq + 1ull;
    *nm.seq = seq;
  }
  seq = __shfl(seq, 0, GL_WAVE);
  double* bank = nm.slots + (size_t)(seq & 1ull) * nm.world * 8;
  if (lane == 0) {
    double* mine = bank + (size_t)nm.rank * 8;
    for (int q = 0; q < nq; ++q) __hip_atomic_store(mine + 1 + q, red[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(mine), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  bool ok = true;
  if (lane < nm.world) {
    const unsigned long long* f = reinterpret_cast<const unsigned long long*>(bank + (size_t)lane * 8);
    const long long t0 = wall_clock64();   // 100 MHz
    while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != seq) {
      __builtin_amdgcn_s_sleep(4);
      if (wall_clock64() - t0 > nm.timeout_ticks) {   // default: a peer that is a minute late is not coming
        ok = false;
        break;
      }
    }
  }
  ok = __all(ok);
  __threadfence_system();
  if (lane < nq) {
    double t = 0.0;
    if (ok)
      for (int r = 0; r < nm.world; ++r)
        t += __hip_atomic_load(bank + (size_t)r * 8 + 1 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else
      t = __builtin_nan("");
    red[lane] = t;
  }
  if (!ok && lane == 0) *nm.err = 1;
}

template <int BS>
static __device__ __forceinline__ void pack_row(const PackMap& pm, int64_t row, const double* vals /*[BS]*/) {
  const int32_t r = pm.ref[row];
  if (r < 0) return;
  for (int32_t q = pm.ptr[r]; q < pm.ptr[r + 1]; ++q) {
    const int64_t k = pm.slot[q];
#pragma unroll
    for (int a = 0; a < BS; ++a) pm.sendbuf[k * BS + a] = vals[a];
  }
}

static __device__ __forceinline__ int xcd_chunk_remap(int b, int nb, int G) {
  // Hardware deals block b to XCD b % 8.  Give every XCD chunks of G consecutive logical blocks, chunk after chunk
  // round-robin over the XCDs: neighbouring slices (overlapping x gathers) share one L2, while the eight XCDs
  // together still walk the matrix front to back (one shared, moving x window in the Infinity Cache; DRAM pages are
  // visited nearly sequentially).  The blocks beyond the last full group of 8*G form one more group with chunks of
  // (what is left) / 8; the last < 8 blocks keep their index -> bijective.
  const int full = (nb / (8 * G)) * (8 * G);
  if (b < full) {
    const int q = b >> 3, xcd = b & 7;
    return ((q / G) * 8 + xcd) * G + (q % G);
  }
  const int g2 = (nb - full) >> 3;
  const int t = b - full;
  if (t >= 8 * g2) return b;
  return full + (t & 7) * g2 + (t >> 3);
}

// Level-0 cycle vectors of the elasticity multigrid.  XT = double: [node][BS] doubles.  XT = float (default): the
// ITERATE lives in node records of 16 B (BS = 3: x, y, z, pad) / 8 B (BS = 2), so that a neighbour's value is ONE
// aligned load in the smoother's gather instead of three 8-byte ones; residual / direction vectors are packed
// [node * BS] floats.  In units of doubles a record is GL_XREC(BS) = 2 / 1 long, which is what the halo exchange of a
// partitioned run is told.
template <int BS, class XT> struct XNode;
template <int BS> struct XNode<BS, double> {
  static __device__ __forceinline__ void load(const double* __restrict__ x, int64_t j, double* o) {
#pragma unroll
    for (int a = 0; a < BS; ++a) o[a] = x[j * BS + a];
  }
  static __device__ __forceinline__ void store(double* __restrict__ x, int64_t j, const double* v) {
#pragma unroll
    for (int a = 0; a < BS; ++a) x[j * BS + a] = v[a];
  }
};
template <> struct XNode<3, float> {
  static __device__ __forceinline__ void load(const float* __restrict__ x, int64_t j, double* o) {
    const float4 v = reinterpret_cast<const float4*>(x)[j];
    o[0] = (double)v.x;
    o[1] = (double)v.y;
    o[2] = (double)v.z;
  }
  static __device__ __forceinline__ void store(float* __restrict__ x, int64_t j, const double* v) {
    reinterpret_cast<float4*>(x)[j] = make_float4((float)v[0], (float)v[1], (float)v[2], 0.0f);
  }
};
template <> struct XNode<1, float> {
  static __device__ __forceinline__ void load(const float* __restrict__ x, int64_t j, double* o) { o[0] = (double)x[j]; }
  static __device__ __forceinline__ void store(float* __restrict__ x, int64_t j, const double* v) { x[j] = (float)v[0]; }
};
template <> struct XNode<2, float> {
  static __device__ __forceinline__ void load(const float* __restrict__ x, int64_t j, double* o) {
    const float2 v = reinterpret_cast<const float2*>(x)[j];
    o[0] = (double)v.x;
    o[1] = (double)v.y;
  }
  static __device__ __forceinline__ void store(float* __restrict__ x, int64_t j, const double* v) {
    reinterpret_cast<float2*>(x)[j] = make_float2((float)v[0], (float)v[1]);
  }
};

#endif
// (bs = 1 with single-precision vectors has no whole-double record: such a hierarchy keeps double vectors whenever its
// level-0 passes exchange halos, see mg_setup_t)
inline int gl_xrec_doubles(int bs, bool x32) { return x32 ? (bs == 3 ? 2 : 1) : bs; }

// scalar slots of the Krylov recurrence (device array `scal`)
enum { SC_ALPHA = 0, SC_BETA, SC_GAMMA, SC_IT, SC_COUNT = 8 };
#define GL_CG_HIST 64   // PCG iterations whose recurrence coefficients are recorded (Ritz values: spectral interval of the dot-free solves)

// Recorded trajectory of the discrete adjoint (adjoint.hip, glims_adjoint_record / glims_adjoint_gradient)
struct AdjointState {
  bool recording = false;                  // gl_step appends c_n after every converged step
  bool valid = false;                      // traj[0..] is a trajectory of the current operators
  std::string why;                         // why it is not (message of GLIMS_E_USAGE)
  std::vector<std::unique_ptr<dvec<double>>> traj;   // c_0, c_1, ... (internal numbering)
  bool had_fixed = false;                  // the concentration's Dirichlet node set when recording started
  std::vector<uint8_t> fixed0;
  dvec<int32_t> cell_nodes;                // [n_cells][nv]: internal node of every cell vertex (built by the first gradient)
  dvec<uint8_t> counted;                   // partitioned handles: [n_cells] 1 = this rank adds the cell to the per-label sums
  int64_t gradients = 0, steps = 0, pcg_its = 0, mech_solves = 0, mech_its = 0;   // glims_adjoint_stats
  double ms_backward = 0.0;
  void clear() { traj.clear(); }
  void invalidate(const char* m) {
    if (!recording && traj.empty()) return;
    clear();
    valid = false;
    why = m;
  }
};

// Tangent fields of the diffusion tensor (glims_set_diffusion_tensor_tangents; DESIGN.md section 17, "Tangent fields") and the
// per-label sums that every backward sweep adds up for them (k_sens_tangent in adjoint.hip).  All of it is the handle's own
// memory, allocated by the set call: no entry of an adjoint call's buffer table.
struct GlTensorTangents {
  int K = 0;                               // stored fields, 0 = none (no launch, no gather)
  dvec<double> planes;                     // [K][n_cells][dim (dim + 1) / 2], INTERNAL cell order, packed as diffusion_tensor.h
  dvec<double> part;                       // [GL_ADJ_BLOCKS][GL_ADJ_LT * K]: block partials of one launch
  dvec<double> sums;                       // [K][GL_MAX_LABELS]: zeroed when a sweep starts, accumulated over its steps
  dvec<double> gather;                     // partitioned handles: [world][K * n_labels], the rows of the ranks
  std::vector<double> grad;                // [K][n_labels]: -dt D_t sums of the last completed sweep (every rank: the same bits)
  int grad_labels = 0;
  bool have = false;                       // grad is of a sweep that completed after the fields were set
  std::string why = "no tangent fields are stored";   // why not (message of GLIMS_E_USAGE)
};

struct GlSampler;   // sample.hip

// One stored image-space misfit term (glims_adjoint_image_terms; kernels in sample.hip).  target holds NaN at every point that
// is not observed (outside the mesh, NaN in the caller's array, q_p = 0): the misfit kernels test that alone.
struct GlImageTerm {
  int64_t step = 0, sampler = -1, n = 0, n_obs = 0;
  int kind = 0;
  double level = 0.0, smooth = 1.0, weight = 1.0;
  dvec<double> target, pweight;             // [n]; pweight empty = 1
};

// One stored displacement-image misfit term (glims_adjoint_displacement_image_terms; kernels in sample.hip).  target is kept
// as component planes [dim][n] so that the point-parallel kernels read it coalesced; plane 0 holds NaN at every point that is
// not observed (outside the mesh, q_p = 0, NaN in a component with kappa_a != 0) -- the misfit kernels test that alone -- and
// the planes of the components with kappa_a = 0 hold 0 at the observed points (they enter no arithmetic).
struct GlDisplacementImageTerm {
  int64_t step = 0, sampler = -1, n = 0, n_obs = 0;
  double weight = 1.0, scale = 1.0;
  double cweight[3] = {1.0, 1.0, 1.0};
  dvec<double> target, pweight;             // [dim][n]; [n], empty = 1
};

// One stored image term of the DEFORMED configuration (glims_adjoint_deformed_image_terms; kernels in sample.hip).  Its points
// are located anew, in the mesh at X + scale u_k, at every evaluation: the term owns its point set and a scratch sampler.
// target holds NaN where the caller's array does or where q_p = 0; whether a point is found is decided per evaluation.
struct GlDeformedImageTerm {
  int64_t step = 0, n = 0;
  int kind = 0;
  double level = 0.0, smooth = 1.0, weight = 1.0, scale = 1.0;
  bool is_grid = true;
  double origin[3] = {0.0, 0.0, 0.0}, spacing[3] = {1.0, 1.0, 1.0};
  int64_t size[3] = {1, 1, 1};
  std::vector<double> xyz;                  // point set [n][dim] (the binning of the location reads it on the host)
  dvec<double> target, pweight;             // [n]; pweight empty = 1
  GlSampler* scratch = nullptr;             // owned (sample.hip): the location of the last evaluation
  dvec<double> y, S;                        // deformed coordinates [n_nodes][dim]; S [n][dim]
  dvec<unsigned long long> cnt;             // [1] observed points of the evaluation
  int64_t n_found = -1, n_obs = -1, n_folded = -1;   // of the LAST evaluation (-1 before the first)
  double min_ratio = 1.0;
};

// Derived fields of a recorded step (derive.hip, glims_derive): the last result, the scratch of the two passes, the one-entry
// cache of the projected stress, and which snapshot's displacement the handle's U holds
struct DeriveState {
  dvec<double> res;                        // last result, planes [ncomp][n_nodes], internal numbering (tensors: symmetric components)
  dvec<double> res_il;                     // ... interleaved [n_nodes][ncomp] for the samplers (ncomp > 1; filled on first use)
  bool res_il_valid = false;
  int ncomp = 0;                           // ncomp = 0: nothing derived yet
  dvec<double> cellv;                      // cell pass output, planes [ncomp | nv][n_cells]
  dvec<double> rhs;                        // gathered right-hand sides, planes [ncomp][n_nodes]
  dvec<double> sc, su;                     // GLIMS_DERIVE_HOST: c [n_nodes] and u [n_nodes][dim], internal numbering
  dvec<double> p1;                         // first-stage P1 field of the growth-induced Jacobian [n_nodes]
  dvec<double> out_stage;                  // the caller's [n_nodes][ncomp | d*d] before the copy to the host
  dvec<double> stress;                     // cached projected stress, planes [d(d+1)/2][n_nodes]
  bool stress_valid = false;
  int64_t stress_src = 0;                  // ... of this source (snapshot id or GLIMS_DERIVE_CURRENT)
  uint64_t stress_gen = 0;                 // ... and this displacement generation
  double stress_rtol = 0.0;                // ... solved to this tolerance (reused by calls that ask for no tighter one)
  uint64_t u_gen = 1;                      // advances whenever U, the materials or the elastic operator may have changed
  int64_t u_snapshot = -1;                 // snapshot whose displacement U holds, -1 = none
  std::vector<uint8_t> label_used;         // [GL_MAX_LABELS] 1 = some cell carries the label (empty: not yet read)
  int64_t n_cell_passes = 0, n_mass_solves = 0, n_elastic_solves = 0, n_cache_hits = 0;   // glims_derive_info
  void forget_u() {
    u_snapshot = -1;
    ++u_gen;
  }
};

// Observables of recorded steps (observe.hip, glims_observe): which labels the cells carry, the per-wave tables of the cell pass
// and the call's result before it goes to the host
struct ObserveState {
  std::vector<int32_t> slot_label;         // compact slot -> label, ascending (empty: the labels were not read yet)
  dvec<int32_t> label_slot;                // [GL_MAX_LABELS] label -> compact slot, -1 = no cell carries it
  dvec<int32_t> d_slot_label;              // slot_label on the device
  dvec<double> part;                       // per-wave tables [waves][slots][n_q][1 + dim]
  dvec<double> res;                        // [n_src][n_q][n_labels][1 + dim]
  dvec<double> sc, su;                     // GLIMS_DERIVE_HOST: c [n_nodes] and u [n_nodes][dim], internal numbering
  int64_t n_cell_passes = 0, n_elastic_solves = 0, n_sources = 0;   // glims_observe_info
};

// One stored volume misfit term (glims_adjoint_observable_terms; kernels in observe.hip): J = 1/2 weight (V - target)^2 with V the
// measure of the query over the cells of the counted labels, in the reference configuration or (deformed) at X + scale u_k
struct GlObservableTerm {
  int64_t step = 0;
  int kind = 0;
  double level = 0.0, smooth = 1.0, weight = 1.0, target = 0.0;
  std::vector<uint8_t> mask;               // [n_labels of the call that stored it]: non-zero = counted; empty = every label
  int64_t n_counted = 0;                   // cells of the counted labels
  int64_t n_cut = -1;                      // SHARP: cells the level set cut at the LAST evaluation (-1 before the first)
  double V = NAN;                          // the measure of the LAST evaluation (NaN before the first)
  int deformed = 0;                        // the cells are measured at y = X + scale u_k; the gradient goes through u_k too
  double scale = 1.0;
  int64_t n_folded = -1;                   // deformed: counted cells with vol(y) / vol(X) not > 0 at the LAST evaluation
  double min_ratio = NAN;                  // deformed: the smallest vol(y) / vol(X) over the counted cells, LAST evaluation
  // a centre-of-mass term (glims_adjoint_observable_terms3, moment = 1): J = 1/2 weight |M / V - target_x|^2; `target` is unused
  int moment = 0;
  double target_x[3] = {0.0, 0.0, 0.0};
  double com[3] = {NAN, NAN, NAN};         // M / V of the LAST evaluation (NaN before the first and when the measure was empty)
  int empty = 0;                           // the LAST evaluation found V not > 0: the term contributed nothing
};

// The stored volume terms and the scratch of their passes (observe.hip): per batch of up to GLIMS_OBSERVE_MAX_QUERIES terms that
// observe one step, the vertex partials as planes [term][vertex][cell], the per-wave sums and the reduced values
struct ObsTermState {
  std::vector<GlObservableTerm> terms;
  std::vector<int64_t> label_cells;        // [GL_MAX_LABELS] cells per label (empty: the labels were not read yet)
  dvec<double> planes;                     // d V_T / d c_a            [terms of the batch][dim + 1][n_cells]
  dvec<double> planes2;                    // (H_T dc_j)_a, one direction at a time (second order), same layout
  dvec<double> part;                       // per-wave sums [waves][terms of the batch]
  dvec<unsigned int> cut_part;             // per-wave counts of cut cells, same layout
  dvec<double> vals;                       // [3][MAX_QUERIES]: V, coef = weight (V - target), weight g^T dc_j
  dvec<long long> cuts;                    // [MAX_QUERIES]
  // a list with a deformed term (k_observe_grad_cells<D, 1>, k_observe_def_load_cells): b0 per term and cell, the combined
  // u-load per vertex, component and cell, the per-wave folded counts and smallest ratios, and their reduced values
  dvec<double> b0_planes;                  // [terms of the batch][n_cells]
  dvec<double> load_planes;                // [dim + 1][dim][n_cells]
  dvec<unsigned int> fold_part;            // [waves][MAX_QUERIES]
  dvec<double> ratio_part;                 // [waves][MAX_QUERIES]
  dvec<long long> folds;                   // [MAX_QUERIES]
  dvec<double> ratios;                     // [MAX_QUERIES]
  // a list with a centre-of-mass term (k_observe_mom_cells, k_observe_mom_sum): the per-wave sums of V and M and, per term of
  // the batch, GL_OBS_MOM doubles (V, M, X, alpha, J, empty) that stay on the device between the passes; with a DEFORMED
  // centre-of-mass term also sigma vol(y) b[1 + m] per term, vertex and cell (the second part of its u-load)
  dvec<double> mom_part;                   // [waves][MAX_QUERIES][4]
  dvec<double> mom_vals;                   // [MAX_QUERIES][GL_OBS_MOM]
  dvec<double> b1_planes;                  // [terms of the batch][dim + 1][n_cells]
  int64_t n_mom_passes = 0;                // cumulative moments passes
  int64_t n_def_passes = 0;                // cumulative cell passes with DEF = 1
  int64_t n_cell_passes = 0, n_gathers = 0;   // cumulative (tools/observable_term_cost.py reads the timing lines instead)
};

// What gl_solve_mechanics remembers from one solve to the next.  The history of solved elasticity problems (right-hand side,
// free-dof solution): the operator is linear and time independent, so the least-squares fit of a new right-hand side by the
// stored ones gives the initial guess (mech_policy.h).  The history belongs to ONE elastic operator -- whatever changes K_el or
// the set of constrained dofs calls forget_operator() --, and with the iteration hint to one run: glims_setup and
// glims_set_state call forget_run(), so that a restarted run takes the iteration path of a fresh handle.  (The hint only sizes the
// first batch of cg_solve's launches, so forget_operator() leaves it alone.)  The device arrays stay allocated either way.
struct MechMemory {
  MechRing ring;
  dvec<double> rhs[GL_MHIST], x[GL_MHIST], w[GL_MHIST];   // right-hand sides, solutions, K_el x (= rhs - final residual)
  double G[GL_MHIST][GL_MHIST] = {{0.0}};  // Gram matrix (rhs_k, rhs_l) of the stored right-hand sides (host copy)
  int hint = 0;                            // PCG iterations of the last fp64 solve
  void forget_operator() { ring.restart(); }
  void forget_run() {
    ring.restart();
    hint = 0;
  }
};

struct glims_ctx {
  int dim = 0, nv = 0, device = 0;
  int n_labels = 0;                        // of the last glims_set_materials
  int64_t n_nodes = 0, n_own = 0, n_cells = 0;
  hipStream_t st = nullptr, st_comm = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_pack = nullptr, ev_halo = nullptr;

  std::vector<int32_t> old2new, new2old;
  dvec<int32_t> d_old2new;
  dvec<double> xyz_new;                     // coordinates in the internal numbering [n_nodes][dim] (device-side symbolic phase)
  DevPattern pat;
  int64_t nnz = 0, n_corners = 0;

  dvec<uint8_t> label;                     // per cell, INTERNAL cell order (= celem's indices)
  dvec<int32_t> cell_new2old;              // internal cell index -> caller's (device-side symbolic phase: cells sorted by first owner; empty = identity)
  dvec<double> egeo;                       // per cell: |T|, grad(lambda_a) [nv][dim]
  dvec<double> evol;                       // per cell: |T| once more, compact (the per-incidence weights read 8 B, not a 104-B record)
  dvec<double> dten;                       // per cell, INTERNAL cell order: the packed diffusion tensor (diffusion_tensor.h), dim (dim + 1) / 2
                                           // doubles; empty = none (the isotropic kernels).  glims_set_diffusion_tensor
  double dten_ratio = 1.0;                 // largest lambda_max / lambda_min over the cells of dten
  GlTensorTangents dtan;                   // tangent fields dTT/dtheta_k and the sums of the last backward sweep
  dvec<double> mat;                        // [5][GL_MAX_LABELS]: D, rho, gamma, mu, lambda
  std::vector<double> mat_host;            // host copy of mat, then E [GL_MAX_LABELS] and nu [GL_MAX_LABELS] (adjoint E / nu)
  bool have_materials = false, is_setup = false, have_mech = false, have_state = false;

  glims_options opt;
  glims_stats stats;
  bool use_idx16 = true;                   // columns as 16-bit (window, offset) codes where a slice has them
                                           // (off with GLIMS_FLAG_INT32_COLUMNS: the int32 stream everywhere)
  int64_t stats_defer_miss = 0;
  int64_t nnz_idx16_avail = 0;             // stored entries of slices that have 16-bit codes
  // glims_options.time_kernels: event pairs around the hot kernels of glims_step (bench.py's in-step roofline figures)
  enum { TK_SPMV = 0, TK_SWEEP = 1, TK_UPDATE = 2, TK_MGFINE = 3, TK_SPMVB = 4, TK_QUAD = 5, TK_CHEB = 6, TK_COUNT = 7 };
  std::vector<hipEvent_t> tev;
  std::vector<uint8_t> tev_cat;             // category of pair q = events 2q, 2q+1
  size_t tev_used = 0;
  // time_kernels = 1: the Krylov SpMV only (two event records per launch cost ~2 us each -- too much for the other two
  // kernels inside a timed region at 1 M rows); 2: all three categories
  // 3: the two dominant kernels of the elasticity solve instead (level-0 multigrid pass, block SpMV; eager launches)
  bool timing(int cat) const {
    const bool on = (cat == TK_MGFINE || cat == TK_SPMVB)
                        ? opt.time_kernels == 3
                        : (opt.time_kernels == 2 || (opt.time_kernels == 1 && (cat == TK_SPMV || cat == TK_CHEB)));
    return on && tev_used + 2 <= tev.size();
  }
  void timing_begin();                      // allocates the event pool on first use
  void timing_collect();                    // elapsed times of the recorded pairs -> stats (sums, counts, medians)
  void tick(int cat) {                      // first call opens a pair of category `cat`, the second closes it
    if ((tev_used & 1) == 0) tev_cat[tev_used / 2] = (uint8_t)cat;
    (void)hipEventRecord(tev[tev_used++], st);
  }
  // partitioned runs with time_kernels != 0: event pairs around every halo exchange on the communication stream (cev) and
  // around the compute stream's wait for it (wev) -> stats.ms_exchange / ms_exchange_exposed
  std::vector<hipEvent_t> cev, wev;
  size_t cev_used = 0, wev_used = 0;
  hipEvent_t* comm_pair() {
    if (!opt.time_kernels || cev_used + 2 > cev.size()) return nullptr;
    cev_used += 2;
    return &cev[cev_used - 2];
  }
  hipEvent_t* wait_pair() {
    if (!opt.time_kernels || wev_used + 2 > wev.size()) return nullptr;
    wev_used += 2;
    return &wev[wev_used - 2];
  }
  hipEvent_t* pair(int cat) {               // a pair to be attached to one dispatch (hipExtLaunchKernelGGL)
    tev_cat[tev_used / 2] = (uint8_t)cat;
    tev_used += 2;
    return &tev[tev_used - 2];
  }

  // scalar operator planes (SELL-64 layout) and block planes
  dvec<double> vM, vS, vA, vKel, vG;
  // per slice: non-zero = the MEMORY of vA's slice holds the bits of vS (A = S + 2 dt N(c) with fl(..) = S there): 1 = stored by
  // the latest sweep, 2 = found linear again by it and not stored (rd_assemble_s_slice).  Written by EVERY kernel that writes
  // the slice of vA (the straight-line sweeps test, every other writer stores 0; a copy of vS into vA is followed by cleared
  // flags, build_value_codes): the flag cannot outlive the values it describes.  Empty = the handle streams no value codes
  // (gl_value_codes_wanted), no kernel writes or reads it and every sweep stores every slice.
  dvec<uint8_t> lin;                       // [n_slices] flags, then [GL_VC_HIT_RING] one byte per launch of the dot-free pass
                                           // that was given the coded stream: set by the launch if a wave read a coded slice
  int vc_launches = 0;                     // ... bytes of the ring handed out since it was last emptied
  dvec<float> vA32;                        // Newton Jacobian in single precision (GLIMS_FLAG_FP32_JACOBIAN only)
  bool jac32 = false;
  int spmv_unroll = 8;                     // entries in flight per lane of the scalar SpMV: 8 on lattice meshes, 16 on general ones
  int stream_nt = 1;                       // value / column-code streams of the Krylov operator pass non-temporal (1) or with the
                                           // default cache policy (0): glims_options.stream_policy, resolved at glims_setup
  RunMemory run;                           // what the time stepper remembers within one run (step_policy.h)
  double cheb_test_hi = 1.0;               // TEST HOOK GLIMS_CHEB_TEST_SCALE_HI (read by glims_create): factor on the measured upper end
  dvec<double> cg_hist;                    // [2 * GL_CG_HIST] (alpha_k, beta_k) of the running PCG solve
  dvec<double> cheb_delta;                 // the correction the last Chebyshev solve added to the iterate [n_nodes] (take-back)
  dvec<double> cheb_delta2;                // the same of a step's SECOND solve: kept across the step boundary, it is the next step's guess (run.have_d2)
  dvec<double> d2_prev;                    // the second correction of the step before that one (linear extrapolation of the guess)
  dvec<int> cheb_plan;                     // [1] iteration count computed on the device (a step's first, warm-started solve)
  dvec<float> vKel32;                      // single-precision copy of K_el (inner solves of the elasticity solver)
  // vectors (internal numbering; length n_nodes unless noted)
  dvec<double> c, c_old, b, load_rd, dinv;
  bool swept = false;                      // an assembly sweep has written dinv since the vectors were allocated (glims_apply 12)
  dvec<double> cg_p, cg_s, cg_u, cg_w, cg_r, cg_r2, b2;     // scalar CG work vectors; r2/b2: speculative next step
  // Newton residuals from the quadratic structure (k_rd_quad): the step's first iterate c_0 (whose Jacobian the solves
  // use), the iterate before the last solve, and the two staged vectors a = c_new + c_k - 2 c_0, delta = c_new - c_k
  dvec<double> nq_c0, nq_ck;
  dvec<float> nq_ad;                                          // (a, delta) pairs, single precision (see k_rd_quad)
  MechMemory mech;                         // what the elasticity solve remembers from one solve to the next
  dvec<double> ws_du;                                         // the increment of the step before the last (warm start, k_ws_delta; run.ws_depth)
  PreparedStep prepared;                                      // the next step, where the last sweep already assembled it
  dvec<double> fg_part;                                       // a fused guess pass's sums of |b - A u|^2 per slice (reduced with the sweep's norms)
  dvec<double> ws_c_old_next, ws_du_next;                     // what k_ws_delta would have committed (exchanged with c_old / ws_du)
  dvec<double> U, mload, m_rhs, m_p, m_s, m_u, m_w, m_r, m_dinv, m_uD;   // mechanics, [n_nodes*dim]
  dvec<uint8_t> fixed_c, fixed_u;
  bool have_fixed_c = false, have_fixed_u = false, have_load_rd = false, have_mload = false;
  MgHierarchy mg;                           // elasticity: K_el, 3 x 3 (2 x 2) blocks
  MgHierarchy mg_rd;                        // RD Jacobian: built on its static part S = (1 - dt rho) M + dt K_D, scalar
  int rd_precond_active = 0;                // what the RD solves use: GLIMS_RD_PRECOND_JACOBI | _MULTIGRID (decided at glims_setup)
  double rd_stiffness_ratio = 0.0;          // mean over the rows of S_ii / M_ii (the quantity `auto` decides on)
  double rd_break_even = 1e300;             // Jacobi-PCG iterations per Newton solve above which the hierarchy pays
  std::vector<uint8_t> fixed_c_host;        // host copy of the concentration's Dirichlet mask (did the SET of nodes change?)
  bool mg_frame_set = false;               // glims_set_mg_frame: global bounding box of a partitioned mesh
  double mg_frame_lo[3] = {0, 0, 0}, mg_frame_hi[3] = {0, 0, 0};
  MeshMetrics mm;
  dvec<double> fixed_c_val;                 // Dirichlet values of the concentration [n_nodes] (internal numbering)
  bool dirichlet_c_dirty = false;           // values not yet written into the iterate (done by the next step)
  // partitioned runs: SOME rank may have new Dirichlet values on nodes this rank holds as ghosts -- set by every
  // glims_set_dirichlet_c / glims_set_state (collective calls: every rank makes them, with n = 0 where it owns no constrained
  // node), so that the next step's halo exchange of the iterate happens on all ranks or on none
  bool dirichlet_c_exchange = false;
  std::vector<dvec<double>*> snapshots;     // device-resident recorded concentrations (owned)
  dvec<double> stage;                      // staging for host<->device permuted transfers [n_nodes*dim]

  dvec<double> partials, partials2;        // per-block partial sums (stage 1 / stage 2 of the reduction)
  dvec<double> partials_v;                 // (r.u, r.r) pairs per block of the PCG vector kernels
  dvec<double> partials_rr;                // (-, r.r) pairs of the vector update when the preconditioner is a V-cycle
  dvec<double> red;                        // [4] reduced sums ([3]: the early convergence check's |r|^2)
  dvec<double> scal;                       // [SC_COUNT] recurrence scalars
  dvec<int> done;                          // [1] 0 running, 1 converged, 2 non-finite, 3 breakdown
  double* h_pinned = nullptr;              // pinned, device-mapped mailbox [seq | red[4] | info[2] | done] (32 doubles)
  double* mail_dev = nullptr;              // its device address
  unsigned long long mail_seq = 0;

  // multi-GPU
  int rank = 0, world = 1;
  ncclComm_t comm_halo = nullptr, comm_red = nullptr;
  int n_peers = 0;
  std::vector<int32_t> peer_rank;
  std::vector<int64_t> send_ptr, recv_ptr;
  dvec<int32_t> send_idx;
  // row -> send slots (the vector-update kernel packs the halo payload itself): send_ref[row] = -1 or r with the
  // slots send_slot[send_slot_ptr[r] .. send_slot_ptr[r+1])
  dvec<int32_t> send_ref, send_slot_ptr, send_slot;
  dvec<double> sendbuf;
  int64_t n_send = 0;
  NodeMail nm;                              // active when nm.slots != nullptr
  void* nm_host = nullptr;                  // the mmap'ed segment
  size_t nm_bytes = 0;
  dvec<unsigned long long> nm_seq;
  dvec<int> nm_err;
  glims_halo_fn tr_halo = nullptr;          // host-provided transport (tests / MPI hosts); RCCL when null
  glims_allreduce_fn tr_allreduce = nullptr;
  void* tr_user = nullptr;

  AdjointState adj;
  std::vector<GlSampler*> samplers;         // owned (sample.hip); a destroyed sampler leaves a nullptr so that ids stay valid
  std::vector<GlImageTerm*> img_terms;      // owned (sample.hip): the stored image-space misfit terms of the adjoint calls
  std::vector<GlDeformedImageTerm*> dimg_terms;   // owned (sample.hip): the stored deformed-configuration image terms
  std::vector<GlDisplacementImageTerm*> uimg_terms;   // owned (sample.hip): the stored displacement-image terms
  DeriveState derive;
  ObserveState observe;
  ObsTermState obs_terms;                   // the stored volume misfit terms of the adjoint calls (observe.hip)

  std::string err;
};

// kernels.hip ---------------------------------------------------------------------------------------
void gl_compute_egeo(glims_ctx* h, const double* d_xyz, const int32_t* d_cells);
void gl_gather_u8(glims_ctx* h, int64_t n, const int32_t* idx, const uint8_t* in, uint8_t* out);   // out[i] = in[idx[i]]
void gl_translate_cells(glims_ctx* h, int64_t n, const int32_t* celem, const int32_t* new2old, int32_t* out);
void gl_assemble_static(glims_ctx* h, int with_mechanics);
int gl_rd_grid(const glims_ctx* h);
void gl_rd_quad(glims_ctx* h, const float* ad /*[n_nodes][2] = (a, delta)*/, double* r, double* partials /*[gl_rd_grid][2]*/,
                int part = 0 /*GL_PART_ALL*/);
int gl_spmv_grid(int n_launch);
enum { GL_PART_ALL = 0, GL_PART_INTERIOR = 1, GL_PART_BOUNDARY = 2 };   // slices without / with ghost columns
// The first pass of the dot-free solve that follows a sweep, folded into the sweep (kernels.hip, k_rd_assemble_sg)
struct GlFusedSweep {
  int kind = 0;               // 1: from the guess u (y1 = u + c2 Dinv (res - A u), part = sums of |res - A u|^2 per slice); 2: from zero
  const double* u = nullptr;
  double* y1 = nullptr;
  double* part = nullptr;     // [gl_rd_grid]
  double c2 = 0.0;            // 1 / theta of the solve's interval
};
// The mass product b = M c + load formed by the sweep itself (MB = 1): the sweep DEFINES the right-hand side it is about to
// use -- b2 in a sweep with two right-hand sides, b otherwise -- from its incidence records, row by row where
// DevPattern::mass_q is not 0, and writes it to `bw` (that buffer: it is the next step's b); the rows with mass_q = 0 read
// what the mass SpMV over DevPattern::mass_fb_slices has left there.
struct GlMassSweep {
  const double* load = nullptr;   // added to the product (may be null)
  double* bw = nullptr;           // the buffer behind b2 (or b)
};
bool gl_value_codes_wanted(const glims_ctx* h);   // the dot-free passes of this handle may stream coded slices (value_codes.h)
constexpr int GL_VC_HIT_RING = 1024;
void gl_value_code_counts(const glims_ctx* h, int64_t* lin_slices, int64_t* kept_slices, int64_t* ring_passes);   // (synchronises the stream)
void gl_harvest_coded_passes(glims_ctx* h);
bool gl_rd_fusable(glims_ctx* h);   // every slice class has a straight-line sweep kernel, fp64 Jacobian
bool gl_rd_mass_in_sweep(glims_ctx* h);   // the stepping path forms M c in the sweep (single rank, gl_rd_fusable, flag not set)
void gl_rd_assemble(glims_ctx* h, const double* c, const double* b, const double* b2, double* r_out, double* r2_out,
                    double* partials /*[gl_rd_grid][2]*/, int part = GL_PART_ALL, const GlFusedSweep* fused = nullptr,
                    const GlMassSweep* mass = nullptr);
void gl_spmv_scalar(glims_ctx* h, const double* vals, const double* x, double* y, bool masked);
void gl_apply_G(glims_ctx* h, const double* c, double* y);
void gl_rd_matfree(glims_ctx* h, const double* c, const double* x, double* y);
void gl_spmv_block(glims_ctx* h, const double* x, double* y, bool masked);
void gl_launch_spmv(glims_ctx* h, hipStream_t st, int n_launch, const int32_t* slice_list, const double* vals,
                    const double* x, double* y, const uint8_t* fixed, const double* addv, const double* r,
                    double* partials, int partial_off, const int* done, const float* vals32 = nullptr,
                    hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
void gl_launch_cheb(glims_ctx* h, hipStream_t st, int n_launch, const int32_t* slice_list, const double* vals,
                    const float* vals32, const double* y_in, double* y_out, double* b, const double* dinv, const double* y_prev,
                    double* ylast, double* x, const uint8_t* fixed, double c1, double c2, int k, int m_host, const int* plan,
                    int want_res, const PackMap& pm, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int shift = 0,
                    double* nrm = nullptr);
// y = A x for 1..8 columns stored interleaved [node][P] (k_spmm, on h->st); partials (optional): [gl_spmm_blocks][P] of x.y
void gl_launch_spmm(glims_ctx* h, int P, const double* vals, const double* x, double* y, const uint8_t* fixed,
                    double* partials);
int gl_spmm_blocks(glims_ctx* h);
void gl_launch_spmv_block(glims_ctx* h, hipStream_t st, int n_launch, const int32_t* slice_list, const double* x,
                          double* y, const uint8_t* fixed, const double* r, double* partials, int partial_off,
                          const int* done, bool single_precision_operator = false);

// solver.hip ----------------------------------------------------------------------------------------
int gl_step(glims_ctx* h, int n_steps);
int gl_solve_mechanics(glims_ctx* h, const double* c_dev = nullptr);   // c_dev: concentration to use (default: state)
void gl_halo_exchange(glims_ctx* h, double* vec, int bs);   // blocking w.r.t. h->st (no overlap)
// the same through the caller's send buffer of n_send x bs doubles (the handle's own holds n_send x dim: bs <= dim only)
void gl_halo_exchange_buf(glims_ctx* h, double* vec, int bs, double* sendbuf);
void gl_comm_destroy(glims_ctx* h);
int gl_comm_selftest(glims_ctx* h);
int gl_mailbox_selftest(glims_ctx* h);
int gl_project(glims_ctx* h, double* rhs_dev /*[n_nodes], overwritten*/, double* x_dev /*[n_nodes]*/, double rtol);
double gl_dot(glims_ctx* h, const double* a, const double* b, int64_t n, bool global = true);   // deterministic; host value
void gl_allreduce_bulk(glims_ctx* h, double* dev, size_t n);   // in-place sum over ranks of a device vector (RCCL / transport)
void gl_pair_of(glims_ctx* h, const double* u, float* ad /*[n_nodes][2]*/);   // (a, delta) = (u, u)
// (a, delta) = (c_new + c_k - 2 c_0, c_new - c_k) over all local nodes, as the stepper prepares the pass (k_quad_prep)
void gl_quad_prep(glims_ctx* h, const double* c_new, const double* c_k, const double* c_0, float* ad /*[n_nodes][2]*/);
void gl_apply_dirichlet_c(glims_ctx* h);                                     // c[fixed] = stored values (+ halo)
void gl_block_dinv(glims_ctx* h);                                            // m_dinv of the constrained K_el
bool gl_mech_precondition(glims_ctx* h);   // the elasticity solves' preconditioner, ready to use; returns: it is the multigrid

// PCG with caller-owned vectors (the time stepper's work vectors stay untouched): on entry r = residual of x.  vals = scalar
// operator plane (bs = 1, Jacobi `dinv`) or nullptr (K_el blocks, bs = dim, block-Jacobi `dinv`); mg: V-cycle instead
int gl_pcg(glims_ctx* h, double* x, double* r, double* u, double* w, double* p, double* s, const double* dinv,
           const double* vals, const uint8_t* fixed, int bs, MgHierarchy* mg, int mg_degree, double tol_abs, int maxit,
           int64_t* its, double* res);
// adjoint.hip ---------------------------------------------------------------------------------------
void gl_adjoint_after_step(glims_ctx* h, int status);   // gl_step: record c_n of a converged step / invalidate
void gl_adjoint_start(glims_ctx* h);                    // clear, store c_0 (the current state)
int gl_adjoint_gradient(glims_ctx* h, int n_terms, const glims_misfit* terms, double* J, double* dD, double* drho,
                        double* dgamma, double* dc0, double* dE, double* dnu);
int gl_adjoint_hessian(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                       const double* dir_rho, const double* dir_gamma, const double* dir_c0, double* J, double* dD,
                       double* drho, double* dgamma, double* dc0, double* hv_D, double* hv_rho, double* hv_gamma,
                       double* hv_c0, double* stats);
// glims_adjoint_hessian_spmd: the same call on world <= 1, collective on partitioned handles
int gl_adjoint_hessian_spmd(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                            const double* dir_rho, const double* dir_gamma, const double* dir_c0, double* J, double* dD,
                            double* drho, double* dgamma, double* dc0, double* hv_D, double* hv_rho, double* hv_gamma,
                            double* hv_c0, double* stats);
// glims_adjoint_hessian_full: directions and products in E / nu too (one GPU)
int gl_adjoint_hessian_full(glims_ctx* h, int n_terms, const glims_misfit* terms, int n_dir, const double* dir_D,
                            const double* dir_rho, const double* dir_gamma, const double* dir_c0, const double* dir_E,
                            const double* dir_nu, double* J, double* dD, double* drho, double* dgamma, double* dc0, double* dE,
                            double* dnu, double* hv_D, double* hv_rho, double* hv_gamma, double* hv_c0, double* hv_E,
                            double* hv_nu, double* stats);
// AdjointState::cell_nodes ([n_cells][nv], internal cell order, the caller's vertex order), built on first use: the gradients
// and the samplers share ONE builder
const int32_t* gl_ensure_cell_nodes(glims_ctx* h);

// sample.hip ----------------------------------------------------------------------------------------
int64_t gl_sampler_create(glims_ctx* h, int64_t n, const double* xyz, const double* origin, const double* spacing,
                          const int64_t* size);   // xyz != nullptr: point set; else the grid
// the same points located in the mesh displaced by scale u (u_source: snapshot id, GLIMS_DERIVE_CURRENT or _HOST); returns the
// elastic solve's status
int gl_sampler_create_deformed(glims_ctx* h, int64_t n, const double* xyz, const double* origin, const double* spacing,
                               const int64_t* size, int64_t u_source, const double* u_host, double scale, int64_t* id);
void gl_sampler_deformation_info(glims_ctx* h, int64_t id, int64_t out[2], double* min_ratio);
void gl_sampler_warp(glims_ctx* h, int64_t id, const double* image, const double* origin, const double* spacing,
                     const int64_t* size, int ncomp, int order, double fill, double* out);
void gl_sampler_info(glims_ctx* h, int64_t id, int64_t* n_points, int64_t* n_found);
void gl_sampler_get(glims_ctx* h, int64_t id, int32_t* cell, double* w);
void gl_sampler_apply(glims_ctx* h, int64_t id, int field, int64_t snapshot, const double* nodal, int ncomp, double fill,
                      double* out);
void gl_sampler_apply_t(glims_ctx* h, int64_t id, const double* r, int ncomp, double* g);
void gl_sampler_resolve(glims_ctx* h, int64_t id, const int64_t* cell_gid);   // collective on partitioned handles
void gl_sampler_get_counted(glims_ctx* h, int64_t id, uint8_t* counted);
void gl_sampler_destroy(glims_ctx* h, int64_t id);
void gl_sampler_destroy_all(glims_ctx* h);   // (and the stored image terms of both lists)
// g[row * ld_row + a * ld_comp] (internal numbering, owned rows) = or += (P^T r)[row][a]; r [n_points][ncomp] on the device
void gl_sampler_transpose_dev(glims_ctx* h, int64_t id, const double* r_dev, int ncomp, double* g_int_dev, int64_t ld_row,
                              int64_t ld_comp, bool accumulate);
void gl_image_terms_set(glims_ctx* h, int n, const glims_image_misfit* terms);
void gl_image_term_info(glims_ctx* h, int k, int64_t out[3]);
// g += P^T r of stored term t at the state c (internal numbering); returns sum_p q_p (h(v_p) - t_p)^2 (fixed order)
double gl_image_misfit_grad(glims_ctx* h, const GlImageTerm& t, const double* c, double* g);
// dg[j * ld + row] += (P^T r2_j)[row] for the P directions dc[j * ld + .]
void gl_image_misfit_second(glims_ctx* h, const GlImageTerm& t, const double* c, const double* dc, int P, int64_t ld,
                            double* dg);
void gl_displacement_image_terms_set(glims_ctx* h, int n, const glims_displacement_image_misfit* terms);
void gl_displacement_image_term_info(glims_ctx* h, int k, int64_t out[3]);
// murhs[row * dim + a] += (P^T R)[row][a] of stored term t at the displacement u ([n_nodes][dim], internal numbering); returns
// sum_p q_p sum_a kappa_a (s (P u)_p,a - d_p,a)^2 (fixed order)
double gl_displacement_image_misfit_grad(glims_ctx* h, const GlDisplacementImageTerm& t, const double* u, double* murhs);
// dmurhs[j * ld + row * dim + a] += (P^T R2_j)[row][a] for the P tangents du[j * ld + .] ([n_nodes][dim] each)
void gl_displacement_image_misfit_second(glims_ctx* h, const GlDisplacementImageTerm& t, const double* du, int P, int64_t ld,
                                         double* dmurhs);
void gl_deformed_image_terms_set(glims_ctx* h, int n, const glims_deformed_image_misfit* terms);
void gl_deformed_image_term_info(glims_ctx* h, int k, int64_t out[4], double* min_ratio);
// Stored deformed term t at the state c and displacement u (both internal numbering): locates its points in the mesh at
// X + scale u, g += P^T r, murhs[row * dim + a] += (P^T S)[row][a]; returns sum_p q_p (h(v_p) - t_p)^2 (fixed order)
double gl_deformed_image_misfit_grad(glims_ctx* h, GlDeformedImageTerm& t, const double* c, const double* u, double* g,
                                     double* murhs);

// api.hip: caller's node order -> internal, through h->stage (synchronises h->st)
void gl_to_device_perm(glims_ctx* h, const double* host, double* dst, int bs);
// derive.hip ----------------------------------------------------------------------------------------
int gl_derive(glims_ctx* h, int kind, int64_t snapshot, const double* c_host, const double* u_host, double rtol, double* out);
// the last result as the samplers read a nodal field ([n_nodes][ncomp], internal numbering); refuses when there is none
const double* gl_derive_sampled(glims_ctx* h, int ncomp);
// observe.hip ---------------------------------------------------------------------------------------
int gl_observe(glims_ctx* h, int n_src, const int64_t* src, const double* c_host, const double* u_host, int deformed,
               double scale, int n_q, const glims_observable* q, double* out);
// (terms2 == nullptr: the old entry point's structs, stored with deformed = 0)
void gl_observable_terms_set(glims_ctx* h, int n, const glims_observable_misfit* terms,
                             const glims_observable_misfit2* terms2 = nullptr, const glims_observable_misfit3* terms3 = nullptr);
void gl_observable_term_info(glims_ctx* h, int k, int64_t out[2], double* V);
void gl_observable_term_info2(glims_ctx* h, int k, int64_t out[4], double* V, double* min_ratio);
void gl_observable_term_info3(glims_ctx* h, int k, int64_t out[4], double* V, double* min_ratio, double com[3]);
// whether a stored volume term is deformed / whether one observes `step` (the sweep solves u_k for that step then)
bool gl_observable_terms_any_deformed(const glims_ctx* h);
bool gl_observable_terms_need_u(const glims_ctx* h, int step);
// the checks a gradient / Hessian call makes of the stored volume terms (GLIMS_E_USAGE): steps within 0..N, mask lengths = n_labels,
// a deformed term only on a handle with mechanics, and with second_order no SHARP and no deformed term
void gl_observable_terms_check(glims_ctx* h, int64_t N, const std::string& who, bool second_order);
// The stored volume terms that observe `step`, in list order (c, g, dc, dg in the internal numbering): J += 1/2 w (V - t)^2,
// g += w (V - t) grad V; with P > 0 also dg[j * ld + .] += w (grad V (grad V^T dc_j) + (V - t) H dc_j).  No such term: no launch.
// A deformed term of the step reads uk (u_k [n_nodes][dim], solved by the caller) and adds dJ/du_k to murhs [n_nodes][dim].
void gl_observable_terms_of_step(glims_ctx* h, int step, const double* c, double* g, double* J, int P, const double* dc,
                                 int64_t ld, double* dg, const double* uk = nullptr, double* murhs = nullptr);

// mg.hip --------------------------------------------------------------------------------------------
void gl_mesh_metrics(glims_ctx* h, const HostPattern& hp, const double* xyz_old);
void gl_mg_setup(glims_ctx* h, MgHierarchy& mg);   // mg.bs / op_vals / op_fixed / op_dinv set by the caller
void gl_make_smoother_copy(glims_ctx* h, MgHierarchy& mg, bool half, bool exchange_scale);
// u = V-cycle(r) with Chebyshev smoothers of the given degree; r zero on constrained dofs
// pv (optional): the cycle's last kernel also leaves the per-block partial sums of (r, u) and (r, r), gl_spmv_grid(n_slices)
// pairs -- what the single-reduction PCG wants next
void gl_mg_apply(glims_ctx* h, MgHierarchy& mg, int degree, const double* r, double* u, const int* done = nullptr,
                 double* pv = nullptr);
void gl_make_kel32(glims_ctx* h);
// level-0 operator pass of the multigrid (kernels.hip): mode 0 out = r - A x, 1 Chebyshev step, 2 out = Dinv A x
void gl_launch_mg_fine(glims_ctx* h, MgHierarchy& mg, int mode, const double* xin, const double* r, double* d,
                       double* xout, double c1, double c2, const int* done = nullptr, double* uout = nullptr,
                       const double* r_full = nullptr, double* pv = nullptr, int part = 0);
int gl_mg_fine_blocks(glims_ctx* h, bool split);
bool gl_mg_split_level0(const glims_ctx* h, const MgHierarchy& mg);   // level-0 passes in two launches around the halo exchange
// generic grouped exchange with the handle's transport: per peer p, sendbuf[send_ptr[p] .. send_ptr[p+1]) * bs doubles go
// to peers[p] and recvbuf[recv_ptr[p] .. recv_ptr[p+1]) * bs come from it (empty directions are skipped on both sides)
void gl_exchange(glims_ctx* h, const std::vector<int32_t>& peers, const std::vector<int64_t>& send_ptr,
                 const std::vector<int64_t>& recv_ptr, const double* sendbuf, double* recvbuf, int bs);
void gl_halo_start(glims_ctx* h, double* vec, int bs);
void gl_halo_finish(glims_ctx* h);
// symbolic.hip: device sort helpers (rocPRIM)
void gl_sort_pairs_u32(glims_ctx* h, uint32_t* k_in, uint32_t* k_out, int32_t* v_in, int32_t* v_out, size_t n, int end_bit);
void gl_offsets_of_sorted_keys(glims_ctx* h, const uint32_t* keys_sorted, int64_t n, int64_t n_keys, int32_t* ptr);
// solver.hip: the two hierarchies
void gl_mg_setup_mech(glims_ctx* h);
void gl_mg_setup_rd(glims_ctx* h);
void gl_rd_choose_precond(glims_ctx* h);    // glims_options.rd_precond -> rd_precond_active (collective in partitioned runs)
