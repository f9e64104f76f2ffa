// Samplers: a fixed set of query points -- a voxel grid or a point set -- located once in the handle's
// simplex mesh, kept as (cell, nodes, barycentric weights) per point, and applied to nodal fields:  P f (gather) and P^T r.
//
// Location is CELL-parallel "claiming": every cell visits the query points inside its (slightly padded) bounding box and, when
// it accepts a point (min lambda >= -GLIMS_SAMPLE_EPS), does an integer atomicMin of its CALLER index into cell[p].  Integer
// min does not depend on the order of arrival, so the winner -- the smallest caller index among the accepting cells -- is
// bitwise reproducible.  A grid's points under a box are an index range (no coordinates exist in memory); a point set is
// binned once into a uniform grid over its own bounding box (radix sort by bin), and a cell walks the bin rows under its box,
// each row one contiguous range of the sorted points.  Cells whose box holds more than GL_SAMPLE_BIG candidates (a coarse mesh
// under a fine grid) are queued and get a block each.  One pass over the points then computes the winner's weights.
//
// P^T r without float atomics, store-then-sum: the found points are sorted by winning cell (stable: point order inside a
// cell), cut into chunks of at most GL_SAMPLE_CHUNK points that never straddle two cells; pass 1 writes per chunk
// q[chunk][a] = sum_p w[p][a] r[p] in list order, pass 2 is row-owned -- every node walks its incidence list and adds, cell by
// cell and chunk by chunk, the entries of its own vertex slot.
//
// Partitioned handles: glims_sampler_resolve (collective, once per sampler) keeps on every rank only the points whose local
// winner is the GLOBAL winner -- the smallest global cell id over the ranks -- and marks each point COUNTED on the smallest
// rank that keeps it.  The transpose's lists are then built from the kept points and P^T runs as on one GPU: an owned row has
// all its cells local, so its incidence list sees every kept point of every one of its cells and no exchange is needed.
//
// Deformed samplers (single-rank handles): the same claim and weight kernels run on a transient coordinate array
// y = fl(X + fl(scale u)) instead of the mesh's own, so a point x_p is located in the DISPLACED mesh; with its cell, nodes and
// weights P f is f at the material point X(x_p) that sits at x_p, and P applied to the reference coordinates is the back map
// X(x_p) itself.  glims_sampler_warp evaluates a voxel image at X(x_p) without materialising X.
#include "glims_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>

#include <rocprim/device/device_scan.hpp>

#define GL_SAMPLE_BIG 256      // candidates under one cell's box above which the cell gets a block of its own
#define GL_SAMPLE_CHUNK 256    // points per chunk of a cell's list in the transpose
#define GL_RESOLVE_BYTES ((size_t)64 << 20)   // bound of the [world][chunk] key buffer of glims_sampler_resolve
#define GL_RESOLVE_NONE 9007199254740992.0    // 2^53: key of a point this rank did not find (global cell ids lie below)

struct GlSampler {
  int64_t n = 0, n_found = 0;
  bool is_grid = false;
  dvec<int32_t> cell;          // [n] caller's cell index, -1 = outside the mesh
  dvec<int32_t> node;          // [n][nv] internal node of the winner's vertices (caller's vertex order; 0 when outside)
  dvec<double> w;              // [n][nv]
  // partitioned handles: after glims_sampler_resolve the arrays above hold the KEPT points only (the others cell -1, w 0)
  bool resolved = false;
  dvec<uint8_t> counted;       // [n] resolved samplers: 1 = this rank adds the point to J and to the observed count
  // transpose (built at creation on single-rank handles, by glims_sampler_resolve on partitioned ones)
  bool have_t = false;
  int64_t n_chunks = 0;
  dvec<int32_t> order;         // [n] points sorted by winning internal cell, the n_found found (kept) ones first
  dvec<int32_t> cptr;          // [n_cells + 1] a cell's points in `order`
  dvec<int32_t> chunk_ptr;     // [n_cells + 1] a cell's chunks
  dvec<int32_t> chunk_cell;    // [n_chunks]
  // staging, grown on demand
  dvec<double> f_ext, f_int, out, q, g_int;
  dvec<double> part;           // image misfit: per-block partial sums, then the total
  // deformed samplers (glims_sampler_create_*_deformed): located in the mesh at X + scale u, frozen from then on
  bool deformed = false;
  int64_t n_inverted = 0;      // cells whose det(E_deformed) / det(E_reference) is not > 0
  double min_ratio = 1.0;      // the smallest such ratio
  dvec<double> img;            // glims_sampler_warp: the source image of the call
};

namespace {

#define GL_CHECK_LAUNCH() GL_HIP(hipGetLastError())

struct GridSpec {
  double o[3], s[3];
  long long n[3];
};
struct BinSpec {
  double lo[3], hi[3], inv_h[3];
  int nb[3];
};

// One cell's vertices and the rows of its inverse edge matrix: lambda_a = r[a-1] . (x - x0), a = 1..D, lambda_0 = 1 - sum.
template <int D>
struct CellGeo {
  double x0[D], r[D][D], lo[D], hi[D];
  bool ok;
};

template <int D>
__device__ __forceinline__ void load_cell(const double* __restrict__ xyz, const int32_t* __restrict__ nd, CellGeo<D>& g) {
  double x[D + 1][D];
#pragma unroll
  for (int m = 0; m <= D; ++m)
#pragma unroll
    for (int a = 0; a < D; ++a) x[m][a] = xyz[(int64_t)nd[m] * D + a];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    g.x0[a] = x[0][a];
    double lo = x[0][a], hi = x[0][a];
#pragma unroll
    for (int m = 1; m <= D; ++m) {
      lo = fmin(lo, x[m][a]);
      hi = fmax(hi, x[m][a]);
    }
    g.lo[a] = lo;
    g.hi[a] = hi;
  }
  double e[D][D];   // e[k] = x_{k+1} - x_0
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int a = 0; a < D; ++a) e[k][a] = x[k + 1][a] - x[0][a];
  double det;
  if constexpr (D == 2) {
    det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    g.r[0][0] = e[1][1] / det;
    g.r[0][1] = -e[1][0] / det;
    g.r[1][0] = -e[0][1] / det;
    g.r[1][1] = e[0][0] / det;
  } else {
    double c[3][3];   // c[k] = e[k+1] x e[k+2]
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double* p = e[(k + 1) % 3];
      const double* q = e[(k + 2) % 3];
      c[k][0] = p[1] * q[2] - p[2] * q[1];
      c[k][1] = p[2] * q[0] - p[0] * q[2];
      c[k][2] = p[0] * q[1] - p[1] * q[0];
    }
    det = e[0][0] * c[0][0] + e[0][1] * c[0][1] + e[0][2] * c[0][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) g.r[k][a] = c[k][a] / det;
  }
  g.ok = det != 0.0 && isfinite(det);   // a cell this rank does not hold has all-zero vertices: never accepts
}

template <int D>
__device__ __forceinline__ void bary(const CellGeo<D>& g, const double* x, double* lam /*[D+1]*/) {
  double d[D];
#pragma unroll
  for (int a = 0; a < D; ++a) d[a] = x[a] - g.x0[a];
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double t = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) t += g.r[k][a] * d[a];
    lam[k + 1] = t;
    s += t;
  }
  lam[0] = 1.0 - s;
}

template <int D>
__device__ __forceinline__ bool accepts(const CellGeo<D>& g, const double* x) {
  double lam[D + 1];
  bary<D>(g, x, lam);
  double m = lam[0];
#pragma unroll
  for (int k = 1; k <= D; ++k) m = fmin(m, lam[k]);   // fmin drops a NaN, the comparison below must not: test each
  bool fin = true;
#pragma unroll
  for (int k = 0; k <= D; ++k) fin = fin && (lam[k] == lam[k]);
  return fin && m >= -GLIMS_SAMPLE_EPS;
}

// What the bounding-box prefilter may miss is only what the cell would not accept: a point accepted with lambda >= -eps lies
// within eps x (cell extent) of the cell; the pad is ten times that plus the rounding of the index arithmetic.
template <int D>
__device__ __forceinline__ double box_pad(const CellGeo<D>& g, int a, double extra) {
  double ext = 0.0;
#pragma unroll
  for (int b = 0; b < D; ++b) ext += g.hi[b] - g.lo[b];
  return 1e-9 * ext + 1e-12 * (fabs(g.lo[a]) + fabs(g.hi[a]) + extra);
}

// the coordinate numpy computes as origin + index * spacing: two roundings, no contraction into one fused operation
__device__ __forceinline__ double grid_coord(const GridSpec& g, int a, long long i) {
  return __dadd_rn(g.o[a], __dmul_rn((double)i, g.s[a]));
}

// index range [i0, i1] of the grid points inside the padded box along axis a; false = none (also for non-finite input)
template <int D>
__device__ __forceinline__ bool grid_range(const CellGeo<D>& g, const GridSpec& gs, int a, long long& i0, long long& i1) {
  const double pad = box_pad<D>(g, a, fabs(gs.o[a]));
  const double t0 = (g.lo[a] - pad - gs.o[a]) / gs.s[a];
  const double t1 = (g.hi[a] + pad - gs.o[a]) / gs.s[a];
  const double nmax = (double)(gs.n[a] - 1);
  if (!(t0 <= nmax) || !(t1 >= 0.0)) return false;
  i0 = t0 > 0.0 ? (long long)ceil(t0) : 0;
  i1 = t1 < nmax ? (long long)floor(t1) : gs.n[a] - 1;
  return i0 <= i1;
}

__device__ __forceinline__ int bin_of(const BinSpec& b, int a, double x) {   // clamped; monotone in x
  const double t = (x - b.lo[a]) * b.inv_h[a];
  if (!(t > 0.0)) return 0;
  return t >= (double)(b.nb[a] - 1) ? b.nb[a] - 1 : (int)t;
}

template <int D>
__device__ __forceinline__ bool bin_range(const CellGeo<D>& g, const BinSpec& b, int a, int& b0, int& b1) {
  const double pad = box_pad<D>(g, a, 0.0);
  const double lo = g.lo[a] - pad, hi = g.hi[a] + pad;
  if (!(lo <= b.hi[a]) || !(hi >= b.lo[a])) return false;   // the box misses the point set (or is not finite)
  b0 = bin_of(b, a, lo);
  b1 = bin_of(b, a, hi);
  return b0 <= b1;
}

// ---- grid ----------------------------------------------------------------------------------------------------------------
// One thread per cell; boxes with more than GL_SAMPLE_BIG grid points are queued for k_claim_grid_big.
template <int D>
__global__ __launch_bounds__(256) void k_claim_grid(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                    const double* __restrict__ xyz, const int32_t* __restrict__ new2old,
                                                    GridSpec gs, int* __restrict__ cell, int32_t* __restrict__ big,
                                                    int* __restrict__ n_big) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_cells) return;
  CellGeo<D> g;
  load_cell<D>(xyz, cell_nodes + e * (D + 1), g);
  if (!g.ok) return;
  long long i0[3] = {0, 0, 0}, i1[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < D; ++a)
    if (!grid_range<D>(g, gs, a, i0[a], i1[a])) return;
  const long long cnt = (i1[0] - i0[0] + 1) * (i1[1] - i0[1] + 1) * (i1[2] - i0[2] + 1);
  if (cnt > GL_SAMPLE_BIG) {
    big[atomicAdd(n_big, 1)] = (int32_t)e;
    return;
  }
  const int id = new2old ? new2old[e] : (int)e;
  double x[3];
  for (long long k = i0[2]; k <= i1[2]; ++k) {
    if (D == 3) x[2] = grid_coord(gs, 2, k);
    for (long long j = i0[1]; j <= i1[1]; ++j) {
      x[1] = grid_coord(gs, 1, j);
      for (long long i = i0[0]; i <= i1[0]; ++i) {
        x[0] = grid_coord(gs, 0, i);
        if (accepts<D>(g, x)) atomicMin(cell + ((k * gs.n[1] + j) * gs.n[0] + i), id);
      }
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_claim_grid_big(int n_big, const int32_t* __restrict__ big,
                                                        const int32_t* __restrict__ cell_nodes,
                                                        const double* __restrict__ xyz, const int32_t* __restrict__ new2old,
                                                        GridSpec gs, int* __restrict__ cell) {
  if ((int)blockIdx.x >= n_big) return;
  const int64_t e = big[blockIdx.x];
  CellGeo<D> g;
  load_cell<D>(xyz, cell_nodes + e * (D + 1), g);
  long long i0[3] = {0, 0, 0}, i1[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < D; ++a)
    if (!grid_range<D>(g, gs, a, i0[a], i1[a])) return;
  const long long nx = i1[0] - i0[0] + 1, ny = i1[1] - i0[1] + 1, nz = i1[2] - i0[2] + 1;
  const int id = new2old ? new2old[e] : (int)e;
  for (long long t = threadIdx.x; t < nx * ny * nz; t += blockDim.x) {
    const long long i = i0[0] + t % nx, j = i0[1] + (t / nx) % ny, k = i0[2] + t / (nx * ny);
    double x[3];
    x[0] = grid_coord(gs, 0, i);
    x[1] = grid_coord(gs, 1, j);
    if (D == 3) x[2] = grid_coord(gs, 2, k);
    if (accepts<D>(g, x)) atomicMin(cell + ((k * gs.n[1] + j) * gs.n[0] + i), id);
  }
}

// ---- point sets ------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void k_point_bins(int64_t n, const double* __restrict__ xyz, BinSpec b, uint32_t trash, uint32_t* __restrict__ key,
                             int32_t* __restrict__ val) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint32_t k = 0;
  bool ok = true;
#pragma unroll
  for (int a = D - 1; a >= 0; --a) {
    const double x = xyz[p * D + a];
    ok = ok && x >= b.lo[a] && x <= b.hi[a];   // false for NaN
    k = k * (uint32_t)b.nb[a] + (uint32_t)bin_of(b, a, x);
  }
  key[p] = ok ? k : trash;
  val[p] = (int32_t)p;
}

template <int D>
__global__ void k_gather_points(int64_t n, const int32_t* __restrict__ idx, const double* __restrict__ xyz,
                                double* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int64_t p = idx[q];
#pragma unroll
  for (int a = 0; a < D; ++a) out[q * D + a] = xyz[p * D + a];
}

// sorted points of bin row (j, k), bins b0 .. b1 along x: one contiguous range
__device__ __forceinline__ void row_range(const BinSpec& b, const int32_t* __restrict__ bin_ptr, int b0, int b1, int j, int k,
                                          int& lo, int& hi) {
  const int64_t row = ((int64_t)k * b.nb[1] + j) * b.nb[0];
  lo = bin_ptr[row + b0];
  hi = bin_ptr[row + b1 + 1];
}

template <int D>
__global__ __launch_bounds__(256) void k_claim_points(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                      const double* __restrict__ xyz, const int32_t* __restrict__ new2old,
                                                      BinSpec bs, const int32_t* __restrict__ bin_ptr,
                                                      const double* __restrict__ pts /*sorted*/, const int32_t* __restrict__ pid,
                                                      int* __restrict__ cell, int32_t* __restrict__ big, int* __restrict__ n_big) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_cells) return;
  CellGeo<D> g;
  load_cell<D>(xyz, cell_nodes + e * (D + 1), g);
  if (!g.ok) return;
  int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < D; ++a)
    if (!bin_range<D>(g, bs, a, b0[a], b1[a])) return;
  long long cnt = 0;
  for (int k = b0[2]; k <= b1[2]; ++k)
    for (int j = b0[1]; j <= b1[1]; ++j) {
      int lo, hi;
      row_range(bs, bin_ptr, b0[0], b1[0], j, k, lo, hi);
      cnt += hi - lo;
    }
  if (cnt == 0) return;
  if (cnt > GL_SAMPLE_BIG) {
    big[atomicAdd(n_big, 1)] = (int32_t)e;
    return;
  }
  const int id = new2old ? new2old[e] : (int)e;
  for (int k = b0[2]; k <= b1[2]; ++k)
    for (int j = b0[1]; j <= b1[1]; ++j) {
      int lo, hi;
      row_range(bs, bin_ptr, b0[0], b1[0], j, k, lo, hi);
      for (int q = lo; q < hi; ++q) {
        double x[D];
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = pts[(int64_t)q * D + a];
        if (accepts<D>(g, x)) atomicMin(cell + pid[q], id);
      }
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_claim_points_big(int n_big, const int32_t* __restrict__ big,
                                                          const int32_t* __restrict__ cell_nodes,
                                                          const double* __restrict__ xyz, const int32_t* __restrict__ new2old,
                                                          BinSpec bs, const int32_t* __restrict__ bin_ptr,
                                                          const double* __restrict__ pts, const int32_t* __restrict__ pid,
                                                          int* __restrict__ cell) {
  if ((int)blockIdx.x >= n_big) return;
  const int64_t e = big[blockIdx.x];
  CellGeo<D> g;
  load_cell<D>(xyz, cell_nodes + e * (D + 1), g);
  int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < D; ++a)
    if (!bin_range<D>(g, bs, a, b0[a], b1[a])) return;
  const int id = new2old ? new2old[e] : (int)e;
  for (int k = b0[2]; k <= b1[2]; ++k)
    for (int j = b0[1]; j <= b1[1]; ++j) {
      int lo, hi;
      row_range(bs, bin_ptr, b0[0], b1[0], j, k, lo, hi);
      for (int q = lo + (int)threadIdx.x; q < hi; q += blockDim.x) {
        double x[D];
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = pts[(int64_t)q * D + a];
        if (accepts<D>(g, x)) atomicMin(cell + pid[q], id);
      }
    }
}

// ---- the winner's weights ------------------------------------------------------------------------------------------------
__global__ void k_fill_i32(int64_t n, int v, int* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = v;
}
__global__ void k_invert_cells(int64_t n, const int32_t* __restrict__ fwd, int32_t* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) inv[fwd[i]] = (int32_t)i;
}

// cell[p]: INT_MAX (nobody claimed) -> -1.  key / val (optional): the sort input of the transpose, key = internal cell of the
// winner, n_cells for the points outside.
template <int D>
__global__ __launch_bounds__(256) void k_weights(int64_t n, int64_t n_cells, const double* __restrict__ pts /*or null: grid*/,
                                                 GridSpec gs, const int32_t* __restrict__ cell_nodes,
                                                 const double* __restrict__ xyz, const int32_t* __restrict__ old2new,
                                                 int* __restrict__ cell, int32_t* __restrict__ node, double* __restrict__ w,
                                                 uint32_t* __restrict__ key, int32_t* __restrict__ val,
                                                 unsigned long long* __restrict__ n_found) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int c = p < n ? cell[p] : -1;
  const bool found = c >= 0 && c < n_cells;
  // one counter update per block: a per-thread atomicAdd on ONE address serialises 140 k wave-level adds at 9 M points
  const int found_here = __syncthreads_count(found);
  if (threadIdx.x == 0 && found_here) atomicAdd(n_found, (unsigned long long)found_here);
  if (p >= n) return;
  int64_t e = n_cells;
  double lam[D + 1];
  int32_t nd[D + 1];
#pragma unroll
  for (int m = 0; m <= D; ++m) {
    lam[m] = 0.0;
    nd[m] = 0;
  }
  if (found) {
    e = old2new ? old2new[c] : c;
    double x[3];
    if (pts) {
#pragma unroll
      for (int a = 0; a < D; ++a) x[a] = pts[p * D + a];
    } else {
      const long long i = p % gs.n[0], j = (p / gs.n[0]) % gs.n[1], k = p / (gs.n[0] * gs.n[1]);
      x[0] = grid_coord(gs, 0, i);
      x[1] = grid_coord(gs, 1, j);
      if (D == 3) x[2] = grid_coord(gs, 2, k);
    }
#pragma unroll
    for (int m = 0; m <= D; ++m) nd[m] = cell_nodes[e * (D + 1) + m];
    CellGeo<D> g;
    load_cell<D>(xyz, nd, g);
    bary<D>(g, x, lam);
  } else {
    cell[p] = -1;
  }
#pragma unroll
  for (int m = 0; m <= D; ++m) {
    node[p * (D + 1) + m] = nd[m];
    w[p * (D + 1) + m] = lam[m];
  }
  if (key) {
    key[p] = (uint32_t)e;
    val[p] = (int32_t)p;
  }
}

// ---- P f -------------------------------------------------------------------------------------------------------------------
// One thread per point: NV x (4 B node + 8 B weight) + 8 BS B out, the nodal field gathered through the caches.  BS = 0: any
// component count by looping.
template <int NV, int BS>
__global__ __launch_bounds__(256) void k_sample(int64_t n, int ncomp, const int32_t* __restrict__ cell,
                                                const int32_t* __restrict__ node, const double* __restrict__ w,
                                                const double* __restrict__ f, double fill, double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int nc = BS ? BS : ncomp;
  if (cell[p] < 0) {
    for (int a = 0; a < nc; ++a) out[p * nc + a] = fill;
    return;
  }
  int32_t nd[NV];
  double wt[NV];
#pragma unroll
  for (int m = 0; m < NV; ++m) {
    nd[m] = node[p * NV + m];
    wt[m] = w[p * NV + m];
  }
  if constexpr (BS > 0) {
    double acc[BS];
#pragma unroll
    for (int a = 0; a < BS; ++a) acc[a] = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m)
#pragma unroll
      for (int a = 0; a < BS; ++a) acc[a] += wt[m] * f[(int64_t)nd[m] * BS + a];
#pragma unroll
    for (int a = 0; a < BS; ++a) out[p * BS + a] = acc[a];
  } else {
    for (int a = 0; a < nc; ++a) {
      double acc = 0.0;
#pragma unroll
      for (int m = 0; m < NV; ++m) acc += wt[m] * f[(int64_t)nd[m] * nc + a];
      out[p * nc + a] = acc;
    }
  }
}

// caller's node order <-> internal
__global__ void k_nodal_in(int64_t n, int bs, const int32_t* __restrict__ old2new, const double* __restrict__ ext,
                           double* __restrict__ in) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * bs) return;
  const int64_t o = i / bs;
  in[(int64_t)old2new[o] * bs + (i - o * bs)] = ext[i];
}
__global__ void k_nodal_out(int64_t n, int bs, const int32_t* __restrict__ old2new, const double* __restrict__ in,
                            double* __restrict__ ext) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * bs) return;
  const int64_t o = i / bs;
  ext[i] = in[(int64_t)old2new[o] * bs + (i - o * bs)];
}

// ---- P^T r -----------------------------------------------------------------------------------------------------------------
__global__ void k_chunk_count(int64_t n_cells, const int32_t* __restrict__ cptr, int32_t* __restrict__ cnt) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > n_cells) return;
  cnt[e] = e < n_cells ? (cptr[e + 1] - cptr[e] + GL_SAMPLE_CHUNK - 1) / GL_SAMPLE_CHUNK : 0;
}
__global__ void k_chunk_cells(int64_t n_cells, const int32_t* __restrict__ chunk_ptr, int32_t* __restrict__ chunk_cell) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_cells) return;
  for (int c = chunk_ptr[e]; c < chunk_ptr[e + 1]; ++c) chunk_cell[c] = (int32_t)e;
}

// pass 1, one thread per chunk: q[chunk][a][comp] = sum over the chunk's points, in list order, of w[p][a] r[p][comp]
template <int NV>
__global__ __launch_bounds__(256) void k_sample_t_cells(int64_t n_chunks, int ncomp, const int32_t* __restrict__ chunk_cell,
                                                        const int32_t* __restrict__ chunk_ptr, const int32_t* __restrict__ cptr,
                                                        const int32_t* __restrict__ order, const double* __restrict__ w,
                                                        const double* __restrict__ r, double* __restrict__ q) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_chunks) return;
  const int e = chunk_cell[c];
  const int lo = cptr[e] + (int)(c - chunk_ptr[e]) * GL_SAMPLE_CHUNK;
  const int hi = min(lo + GL_SAMPLE_CHUNK, cptr[e + 1]);
  for (int a = 0; a < ncomp; ++a) {
    double acc[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) acc[m] = 0.0;
    for (int k = lo; k < hi; ++k) {
      const int64_t p = order[k];
      const double rv = r[p * ncomp + a];
#pragma unroll
      for (int m = 0; m < NV; ++m) acc[m] += w[p * NV + m] * rv;
    }
#pragma unroll
    for (int m = 0; m < NV; ++m) q[(c * NV + m) * ncomp + a] = acc[m];
  }
}

// pass 2, one thread per node (row-owned, like the assembly): the node's cells in the order of its incidence list, each
// cell's chunks in chunk order, the entry of the node's own vertex slot.  Component a of row goes to g[row ld_row + a ld_comp].
template <int NV>
__global__ __launch_bounds__(256) void k_sample_t(int64_t n_own, int ncomp, const int64_t* __restrict__ cslice_ptr,
                                                  const uint32_t* __restrict__ cslots, const int32_t* __restrict__ celem,
                                                  const uint8_t* __restrict__ diag_k, const int32_t* __restrict__ chunk_ptr,
                                                  const double* __restrict__ q, double* __restrict__ g, int64_t ld_row,
                                                  int64_t ld_comp, int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_own) return;
  const int64_t s = row >> 6, lane = row & 63;
  const int64_t cbase = cslice_ptr[s];
  const int clen = (int)((cslice_ptr[s + 1] - cbase) >> 6);
  const uint32_t dk = diag_k[row];
  double acc[GLIMS_SAMPLE_MAX_COMP];
#pragma unroll
  for (int a = 0; a < GLIMS_SAMPLE_MAX_COMP; ++a) acc[a] = 0.0;
  for (int k = 0; k < clen; ++k) {
    const int64_t ci = cbase + (int64_t)k * GL_WAVE + lane;
    const int32_t e = celem[ci];
    if (e < 0) continue;
    const int c0 = chunk_ptr[e], c1 = chunk_ptr[e + 1];
    if (c0 == c1) continue;
    const uint32_t sl = cslots[ci];
    int own = 0;
#pragma unroll
    for (int m = 0; m < NV; ++m)
      if (((sl >> (8 * m)) & 255u) == dk) own = m;
    for (int64_t c = c0; c < c1; ++c)
#pragma unroll
      for (int a = 0; a < GLIMS_SAMPLE_MAX_COMP; ++a)
        if (a < ncomp) acc[a] += q[(c * NV + own) * ncomp + a];
  }
  // (accumulate: the row's own thread adds to what g holds -- two misfit terms on one step must add)
#pragma unroll
  for (int a = 0; a < GLIMS_SAMPLE_MAX_COMP; ++a)
    if (a < ncomp) {
      const int64_t o = row * ld_row + a * ld_comp;
      g[o] = accumulate ? g[o] + acc[a] : acc[a];
    }
}

// ---- image-space misfit terms (glims_hip.h, "image-space misfit terms") --------------------------------
// once per stored term: t[p] = NaN where the point is not observed (outside the mesh, q_p = 0); counts the observed ones.
// counted (resolved samplers, else null): only the counted points enter n_obs -- a kept point that another rank counts keeps
// its target, P^T r needs its r here.
__global__ __launch_bounds__(256) void k_img_prepare(int64_t n, const int32_t* __restrict__ cell, const double* __restrict__ q,
                                                     const uint8_t* __restrict__ counted, double* __restrict__ t,
                                                     unsigned long long* __restrict__ n_obs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool obs = false;
  if (p < n) {
    const double tv = t[p];
    obs = cell[p] >= 0 && tv == tv && (!q || q[p] != 0.0);
    if (!obs) t[p] = __longlong_as_double(0x7ff8000000000000LL);
    if (counted && !counted[p]) obs = false;
  }
  const int here = __syncthreads_count(obs);
  if (threadIdx.x == 0 && here) atomicAdd(n_obs, (unsigned long long)here);   // (integer: order-independent)
}

// h(v) - t is formed by the callers; h, h', h'' of a term kind
__device__ __forceinline__ void img_h(int kind, double level, double smooth, double v, double& hv, double& hp, double& h2) {
  if (kind == GLIMS_MISFIT_IMG_THRESH) {
    const double th = tanh((v - level) / smooth);
    hv = 0.5 * (th + 1.0);
    hp = 0.5 * (1.0 - th * th) / smooth;
    h2 = -th * (1.0 - th * th) / (smooth * smooth);
  } else {
    hv = v;
    hp = 1.0;
    h2 = 0.0;
  }
}

__device__ __forceinline__ double img_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// One thread per point: v = sum_a w c[node] gathered from the recorded state (internal numbering), r[p] = weight q h'(v)
// (h(v) - t) for an observed point (t not NaN), else 0 -- a NaN target enters no arithmetic.  part[block] = the block's sum of
// q (h(v) - t)^2: the wave's butterfly, then the four wave sums in a fixed order.  counted (resolved samplers, else null): r
// is written for every kept observed point, the square enters the sum only where this rank counts the point.
// Bytes per point: NV (4 + 8) node ids and weights + 8 (t) + 8 (q, if present) + 1 (counted, if present) + 8 (r); c is
// gathered through the caches.
template <int NV>
__global__ __launch_bounds__(256) void k_img_misfit(int64_t n, int kind, double level, double smooth, double weight,
                                                    const int32_t* __restrict__ node, const double* __restrict__ w,
                                                    const double* __restrict__ c, const double* __restrict__ t,
                                                    const double* __restrict__ q, const uint8_t* __restrict__ counted,
                                                    double* __restrict__ r, double* __restrict__ part) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double sq = 0.0;
  if (p < n) {
    const double tv = t[p];
    double rv = 0.0;
    if (tv == tv) {
      double v = 0.0;
#pragma unroll
      for (int m = 0; m < NV; ++m) v += w[p * NV + m] * c[node[p * NV + m]];
      double hv, hp, h2;
      img_h(kind, level, smooth, v, hv, hp, h2);
      const double qv = q ? q[p] : 1.0;
      const double e = hv - tv;
      rv = weight * qv * hp * e;
      sq = qv * e * e;
      if (counted && !counted[p]) sq = 0.0;
    }
    r[p] = rv;
  }
  __shared__ double sm[4];
  const double ws = img_wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// second stage, ONE block: thread i adds the partials i, i + 1024, ... in block order, then the wave's butterfly and the 16
// wave sums in order -- the same order on every call.  out[0] = the total.
__global__ __launch_bounds__(1024) void k_img_sum(int64_t n_blocks, const double* __restrict__ part, double* __restrict__ out) {
  double s = 0.0;
  for (int64_t b = threadIdx.x; b < n_blocks; b += 1024) s += part[b];
  __shared__ double sm[16];
  s = img_wave_sum(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tsum = 0.0;
    for (int k = 0; k < 16; ++k) tsum += sm[k];
    out[0] = tsum;
  }
}

// Second order, one thread per point, all P columns of a call: r2[p][j] = weight q (h'(v)^2 + h''(v) (h(v) - t)) (P dc_j)_p
// (0 for a point that is not observed).  Column j runs the same arithmetic whatever P is.
// Bytes per point: NV (4 + 8) + 8 (t) + 8 (q, if present) + 8 P (r2); c and the P columns of dc are gathered through the caches.
template <int NV>
__global__ __launch_bounds__(256) void k_img_misfit_dir(int64_t n, int P, int64_t ld, int kind, double level, double smooth,
                                                        double weight, const int32_t* __restrict__ node,
                                                        const double* __restrict__ w, const double* __restrict__ c,
                                                        const double* __restrict__ dc, const double* __restrict__ t,
                                                        const double* __restrict__ q, double* __restrict__ r2) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const double tv = t[p];
  if (!(tv == tv)) {
    for (int j = 0; j < P; ++j) r2[p * P + j] = 0.0;
    return;
  }
  int32_t nd[NV];
  double wt[NV];
  double v = 0.0;
#pragma unroll
  for (int m = 0; m < NV; ++m) {
    nd[m] = node[p * NV + m];
    wt[m] = w[p * NV + m];
    v += wt[m] * c[nd[m]];
  }
  double hv, hp, h2;
  img_h(kind, level, smooth, v, hv, hp, h2);
  const double qv = q ? q[p] : 1.0;
  const double coef = weight * qv * (hp * hp + h2 * (hv - tv));
  for (int j = 0; j < P; ++j) {
    const double* d = dc + (size_t)j * ld;
    double dv = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) dv += wt[m] * d[nd[m]];
    r2[p * P + j] = coef * dv;
  }
}

// ---- displacement-image misfit terms (glims_hip.h, "displacement-image misfit terms") ------------------
// The target d is kept as component planes d[a * n + p]: a wave reads 64 consecutive doubles of a plane (512 B), where the
// caller's [n][D] rows would put the D loads of a lane 8 D bytes apart.  R / R2 must be [n][D] rows for P^T (k_sample_t_cells
// reads r[p * ncomp + a]); the block's 256 D values go through LDS and leave as consecutive doubles.
struct UimgKappa {
  double k[3];
};

// once per stored term: d[0 * n + p] = NaN where the point is not observed (outside the mesh, q_p = 0, NaN in a component with
// kappa_a != 0), and at an observed point the components with kappa_a = 0 become 0; counts the observed points.
template <int D>
__global__ __launch_bounds__(256) void k_uimg_prepare(int64_t n, const int32_t* __restrict__ cell, const double* __restrict__ q,
                                                      UimgKappa kap, double* __restrict__ d,
                                                      unsigned long long* __restrict__ n_obs) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool obs = false;
  if (p < n) {
    obs = cell[p] >= 0 && (!q || q[p] != 0.0);
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const double dv = d[(int64_t)a * n + p];
      if (kap.k[a] != 0.0 && !(dv == dv)) obs = false;
    }
    if (!obs) {
      d[p] = __longlong_as_double(0x7ff8000000000000LL);
    } else {
#pragma unroll
      for (int a = 0; a < D; ++a)
        if (kap.k[a] == 0.0) d[(int64_t)a * n + p] = 0.0;
    }
  }
  const int here = __syncthreads_count(obs);
  if (threadIdx.x == 0 && here) atomicAdd(n_obs, (unsigned long long)here);   // (integer: order-independent)
}

// the block's rows sr[256][D] to out[(first point of the block) * D ...], consecutive doubles; after a __syncthreads of its own
template <int D>
__device__ __forceinline__ void uimg_store_rows(int64_t n, const double* sr, double* __restrict__ out) {
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * 256 * D, end = n * D;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const int64_t i = base + k * 256 + threadIdx.x;
    if (i < end) out[i] = sr[k * 256 + threadIdx.x];
  }
}

// One thread per point: (P u)_p,a = sum_m w u[node_m][a] gathered from u_k ([node][D], internal numbering),
// e_a = s (P u)_p,a - d_p,a, R[p][a] = weight q kappa_a s e_a for an observed point (plane 0 of d not NaN) and a component
// with kappa_a != 0, else 0 -- the others enter no arithmetic.  part[block] = the block's sum of q sum_a kappa_a e_a^2: the
// wave's butterfly, then the four wave sums in a fixed order.
// Bytes per point: (D + 1) (4 + 8) node ids and weights + 8 D (d) + 8 (q, if present) + 8 D (R); u is gathered through the
// caches (D consecutive doubles per node).  2-D: 76 B, 3-D: 104 B with q.
template <int D>
__global__ __launch_bounds__(256) void k_uimg_misfit(int64_t n, double weight, double scale, UimgKappa kap,
                                                     const int32_t* __restrict__ node, const double* __restrict__ w,
                                                     const double* __restrict__ u, const double* __restrict__ d,
                                                     const double* __restrict__ q, double* __restrict__ R,
                                                     double* __restrict__ part) {
  constexpr int NV = D + 1;
  __shared__ double sr[256 * D];
  __shared__ double sm[4];
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double sq = 0.0, rv[D];
#pragma unroll
  for (int a = 0; a < D; ++a) rv[a] = 0.0;
  if (p < n) {
    const double d0 = d[p];
    if (d0 == d0) {
      int32_t nd[NV];
      double wt[NV];
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        nd[m] = node[p * NV + m];
        wt[m] = w[p * NV + m];
      }
      const double qv = q ? q[p] : 1.0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        if (kap.k[a] == 0.0) continue;
        double v = 0.0;
#pragma unroll
        for (int m = 0; m < NV; ++m) v += wt[m] * u[(int64_t)nd[m] * D + a];
        const double e = scale * v - (a == 0 ? d0 : d[(int64_t)a * n + p]);
        rv[a] = weight * qv * kap.k[a] * scale * e;
        sq += kap.k[a] * e * e;
      }
      sq *= qv;
    }
  }
#pragma unroll
  for (int a = 0; a < D; ++a) sr[threadIdx.x * D + a] = rv[a];
  const double ws = img_wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = ws;
  uimg_store_rows<D>(n, sr, R);
  if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// Second order, one thread per point, all P columns of a call: R2[j][p][a] = weight q kappa_a s^2 (P du_j)_p,a (0 for a point
// that is not observed or a component with kappa_a = 0); column j is a contiguous [n][D] block, what P^T reads, and runs the
// same arithmetic whatever P is.
// Bytes per point: (D + 1) (4 + 8) + 8 (plane 0 of d) + 8 (q, if present) + 8 D P (R2); the P tangents are gathered through
// the caches.
template <int D>
__global__ __launch_bounds__(256) void k_uimg_misfit_dir(int64_t n, int P, int64_t ld, double weight, double scale,
                                                         UimgKappa kap, const int32_t* __restrict__ node,
                                                         const double* __restrict__ w, const double* __restrict__ du,
                                                         const double* __restrict__ d, const double* __restrict__ q,
                                                         double* __restrict__ R2) {
  constexpr int NV = D + 1;
  __shared__ double sr[256 * D];
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t nd[NV];
  double wt[NV], coef[D];
#pragma unroll
  for (int m = 0; m < NV; ++m) {
    nd[m] = 0;
    wt[m] = 0.0;
  }
#pragma unroll
  for (int a = 0; a < D; ++a) coef[a] = 0.0;
  bool obs = false;
  if (p < n) {
    const double d0 = d[p];
    obs = d0 == d0;
  }
  if (obs) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      nd[m] = node[p * NV + m];
      wt[m] = w[p * NV + m];
    }
    const double qv = q ? q[p] : 1.0;
#pragma unroll
    for (int a = 0; a < D; ++a) coef[a] = weight * qv * kap.k[a] * scale * scale;
  }
  for (int j = 0; j < P; ++j) {
    const double* dj = du + (size_t)j * ld;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      double r = 0.0;
      if (obs && kap.k[a] != 0.0) {
        double v = 0.0;
#pragma unroll
        for (int m = 0; m < NV; ++m) v += wt[m] * dj[(int64_t)nd[m] * D + a];
        r = coef[a] * v;
      }
      sr[threadIdx.x * D + a] = r;
    }
    uimg_store_rows<D>(n, sr, R2 + (size_t)j * n * D);
    __syncthreads();   // sr is rewritten by the next column
  }
}

// ---- glims_sampler_resolve ---------------------------------------------------------------------------------------------------
// keys: row `rank` of buf[world][m] (zero elsewhere) = the global id of the local winner of point p0 + i, as a double, or
// GL_RESOLVE_NONE.  8 B written per point (+ 4 B cell, 8 B cell_gid gathered).
__global__ __launch_bounds__(256) void k_resolve_keys(int64_t m, int64_t p0, const int32_t* __restrict__ cell,
                                                      const int64_t* __restrict__ cell_gid, double* __restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int c = cell[p0 + i];
  row[i] = c >= 0 ? (double)cell_gid[c] : GL_RESOLVE_NONE;
}

// pick, after the gather: per point the minimum over the rows and the smallest rank that attains it.  This rank KEEPS the point
// iff its own key is that minimum (and a cell), and COUNTS it iff it is that smallest rank; a dropped point loses its cell,
// nodes and weights.  key / val: the transpose's sort input (internal cell of a kept point, n_cells for the others).
// Bytes per point: 8 world (keys) + 4 (cell) + 1 (counted) + 8 (key, val); NV 12 more for a dropped point.
template <int NV>
__global__ __launch_bounds__(256) void k_resolve_pick(int64_t m, int64_t p0, int world, int rank, int64_t n_cells,
                                                      const double* __restrict__ buf, const int32_t* __restrict__ old2new,
                                                      int32_t* __restrict__ cell, int32_t* __restrict__ node,
                                                      double* __restrict__ w, uint8_t* __restrict__ counted,
                                                      uint32_t* __restrict__ key, int32_t* __restrict__ val,
                                                      unsigned long long* __restrict__ n_kept) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (i < m) {
    const int64_t p = p0 + i;
    double best = GL_RESOLVE_NONE;
    int first = -1;
    for (int r = 0; r < world; ++r) {
      const double k = buf[(int64_t)r * m + i];
      if (k < best) {
        best = k;
        first = r;
      }
    }
    const int c = cell[p];
    keep = c >= 0 && buf[(int64_t)rank * m + i] == best;
    counted[p] = keep && first == rank ? 1 : 0;
    if (!keep) {
      cell[p] = -1;
#pragma unroll
      for (int a = 0; a < NV; ++a) {
        node[p * NV + a] = 0;
        w[p * NV + a] = 0.0;
      }
    }
    key[p] = keep ? (uint32_t)(old2new ? old2new[c] : c) : (uint32_t)n_cells;
    val[p] = (int32_t)p;
  }
  const int here = __syncthreads_count(keep);
  if (threadIdx.x == 0 && here) atomicAdd(n_kept, (unsigned long long)here);   // (integer: order-independent)
}

// ---- deformed samplers -------------------------------------------------------------------------------------------------------
// One thread per node: y = fl(X + fl(scale u)), two roundings, never contracted (numpy's points + scale * u).
// Bytes per node: 16 D in (X, u), 8 D out.
template <int D>
__global__ __launch_bounds__(256) void k_deform_xyz(int64_t n, const double* __restrict__ X, const double* __restrict__ u,
                                                    double scale, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int a = 0; a < D; ++a) y[i * D + a] = __dadd_rn(X[i * D + a], __dmul_rn(scale, u[i * D + a]));
}

template <int D>
__device__ __forceinline__ double edge_det(const double* __restrict__ xyz, const int32_t* nd) {
  double e[D][D];
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int a = 0; a < D; ++a) e[k][a] = xyz[(int64_t)nd[k + 1] * D + a] - xyz[(int64_t)nd[0] * D + a];
  if constexpr (D == 2) {
    return e[0][0] * e[1][1] - e[0][1] * e[1][0];
  } else {
    return e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
           e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
  }
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o, 64));
  return v;
}

// One thread per cell: ratio = det(E_deformed) / det(E_reference) = det(I + scale grad u_h) on the cell.  n_bad counts the
// cells whose ratio is not > 0 (folded, flat or non-finite; an integer atomic per block), part[block] = the block's smallest
// ratio (fmin drops a NaN; min does not depend on the order, so the result is the same on every call).
// Bytes per cell: 4 (D + 1) node ids + 8 per block; 2 D (D + 1) coordinates gathered through the caches.
template <int D>
__global__ __launch_bounds__(256) void k_deform_cells(int64_t n_cells, const int32_t* __restrict__ cell_nodes,
                                                      const double* __restrict__ X, const double* __restrict__ y,
                                                      double* __restrict__ part, unsigned long long* __restrict__ n_bad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double ratio = __longlong_as_double(0x7ff0000000000000LL);   // +inf: neutral for min
  bool bad = false;
  if (e < n_cells) {
    int32_t nd[D + 1];
#pragma unroll
    for (int m = 0; m <= D; ++m) nd[m] = cell_nodes[e * (D + 1) + m];
    ratio = edge_det<D>(y, nd) / edge_det<D>(X, nd);
    bad = !(ratio > 0.0) || !isfinite(ratio);
  }
  const int bad_here = __syncthreads_count(bad);
  if (threadIdx.x == 0 && bad_here) atomicAdd(n_bad, (unsigned long long)bad_here);
  __shared__ double sm[4];
  const double wm = wave_min(ratio);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = wm;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmin(fmin(sm[0], sm[1]), fmin(sm[2], sm[3]));
}

// second stage, ONE block over the per-block minima
__global__ __launch_bounds__(1024) void k_deform_min(int64_t n_blocks, const double* __restrict__ part, double* __restrict__ out) {
  double m = __longlong_as_double(0x7ff0000000000000LL);
  for (int64_t b = threadIdx.x; b < n_blocks; b += 1024) m = fmin(m, part[b]);
  __shared__ double sm[16];
  m = wave_min(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = sm[0];
    for (int k = 1; k < 16; ++k) t = fmin(t, sm[k]);
    out[0] = t;
  }
}

// Image term of the deformed configuration (glims_hip.h, "image terms in the deformed configuration"),
// one thread per point of a sampler located in the mesh at y = X + scale u_k.  v, h, r[p] and the block's partial sum of
// q (h(v) - t)^2 are formed exactly as in k_img_misfit (same expressions, same order: with scale = 0 the two agree bit for
// bit); on top of them the location's load  S[p][.] = -scale r_p grad_y c_k|T(p),  grad_y c = sum_k (c_{k+1} - c_0) R_k with
// R the rows of the winner's inverse edge matrix in the DEFORMED coordinates (load_cell).  A winner whose ratio
// det(E_deformed) / det(E_reference) is not > 0 or not finite gets S = 0.  A point is observed iff it was found (cell >= 0)
// and its target is not NaN (q_p = 0 was turned into a NaN target when the term was stored); n_obs counts them (integer).
// The gradient is formed per POINT, not once per cell: a per-cell pass would write 8 D B per cell and save the points the
// 16 D NV B of gathered coordinates, which the caches serve -- the choice is by bytes and unmeasured.
// Bytes per point: 4 (cell) + NV (4 + 8) node ids and weights + 8 (t) + 8 (q, if present) + 8 (r) + 8 D (S); c and the
// 2 D NV coordinates (y and X) are gathered through the caches.
template <int NV>
__global__ __launch_bounds__(256) void k_img_misfit_deformed(int64_t n, int kind, double level, double smooth, double weight,
                                                             double scale, const int32_t* __restrict__ cell,
                                                             const int32_t* __restrict__ node, const double* __restrict__ w,
                                                             const double* __restrict__ c, const double* __restrict__ X,
                                                             const double* __restrict__ y, const double* __restrict__ t,
                                                             const double* __restrict__ q, double* __restrict__ r,
                                                             double* __restrict__ S, double* __restrict__ part,
                                                             unsigned long long* __restrict__ n_obs) {
  constexpr int D = NV - 1;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double sq = 0.0;
  bool obs = false;
  if (p < n) {
    const double tv = t[p];
    double rv = 0.0;
    double sv[D];
#pragma unroll
    for (int a = 0; a < D; ++a) sv[a] = 0.0;
    if (tv == tv && cell[p] >= 0) {
      obs = true;
      double v = 0.0;
#pragma unroll
      for (int m = 0; m < NV; ++m) v += w[p * NV + m] * c[node[p * NV + m]];
      double hv, hp, h2;
      img_h(kind, level, smooth, v, hv, hp, h2);
      const double qv = q ? q[p] : 1.0;
      const double e = hv - tv;
      rv = weight * qv * hp * e;
      sq = qv * e * e;
      int32_t nd[NV];
#pragma unroll
      for (int m = 0; m < NV; ++m) nd[m] = node[p * NV + m];
      CellGeo<D> g;
      load_cell<D>(y, nd, g);
      const double ratio = edge_det<D>(y, nd) / edge_det<D>(X, nd);
      if (g.ok && ratio > 0.0 && isfinite(ratio)) {
        const double c0 = c[nd[0]];
        double grad[D];
#pragma unroll
        for (int a = 0; a < D; ++a) grad[a] = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double dk = c[nd[k + 1]] - c0;
#pragma unroll
          for (int a = 0; a < D; ++a) grad[a] += dk * g.r[k][a];
        }
#pragma unroll
        for (int a = 0; a < D; ++a) sv[a] = -scale * rv * grad[a];
      }
    }
    r[p] = rv;
#pragma unroll
    for (int a = 0; a < D; ++a) S[p * D + a] = sv[a];
  }
  const int here = __syncthreads_count(obs);
  if (threadIdx.x == 0 && here) atomicAdd(n_obs, (unsigned long long)here);   // (integer: order-independent)
  __shared__ double sm[4];
  const double ws = img_wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = ws;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// glims_sampler_warp, one thread per point: out[p][.] = image(X(x_p)), X = sum_m w[p][m] X_node(m) the back-mapped position
// (formed in registers, never stored).  Per axis t = (X - o) / s.
//   ORDER 1 (d-linear): inside iff 0 <= t <= n - 1; i0 = min(floor(t), n - 2) (n = 1: i0 = 0, f = 0), f = t - i0; the value is
//           the sum over the 2^D corners (z outermost, x innermost) of (product of f or 1 - f) * voxel -- plain IEEE arithmetic,
//           a NaN voxel of the stencil propagates even where its weight is 0.
//   ORDER 0 (nearest): inside iff -0.5 <= t < n - 0.5; index floor(t + 0.5) (kept <= n - 1 where t + 0.5 rounds up to n).
// A point outside the mesh or outside the source image gets `fill`.
// Bytes per found point: NV (4 + 8) node ids and weights + 4 (cell) read, 8 ncomp written; the NV D reference coordinates and the
// 2^D (or 1) x ncomp voxels are gathered through the caches.
template <int NV, int D, int ORDER>
__global__ __launch_bounds__(256) void k_warp(int64_t n, int ncomp, const int32_t* __restrict__ cell,
                                              const int32_t* __restrict__ node, const double* __restrict__ w,
                                              const double* __restrict__ xyz, GridSpec gs, const double* __restrict__ img,
                                              double fill, double* __restrict__ out) {
  static_assert(NV == D + 1, "simplices");
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  bool inside = cell[p] >= 0;
  int64_t base = 0;          // voxel (i0, j0, k0)
  double f[D];
  if (inside) {
    double X[D];
#pragma unroll
    for (int a = 0; a < D; ++a) X[a] = 0.0;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int64_t nd = node[p * NV + m];
      const double wt = w[p * NV + m];
#pragma unroll
      for (int a = 0; a < D; ++a) X[a] += wt * xyz[nd * D + a];
    }
    int64_t stride = 1;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const double t = (X[a] - gs.o[a]) / gs.s[a];
      const long long na = gs.n[a];
      long long i0;
      if constexpr (ORDER == 1) {
        inside = inside && t >= 0.0 && t <= (double)(na - 1);   // (false for a NaN)
        const double fl = floor(t);
        i0 = na > 1 ? (fl < (double)(na - 2) ? (long long)fl : na - 2) : 0;
        f[a] = na > 1 ? t - (double)i0 : 0.0;
      } else {
        inside = inside && t >= -0.5 && t < (double)na - 0.5;
        const double fl = floor(t + 0.5);
        i0 = fl < (double)(na - 1) ? (long long)fl : na - 1;
        f[a] = 0.0;
      }
      if (!inside) i0 = 0;   // (never an index from a value that failed the test)
      base += (int64_t)i0 * stride;
      stride *= na;
    }
  }
  if (!inside) {
    for (int c = 0; c < ncomp; ++c) out[p * ncomp + c] = fill;
    return;
  }
  if constexpr (ORDER == 0) {
    for (int c = 0; c < ncomp; ++c) out[p * ncomp + c] = img[base * ncomp + c];
  } else {
    constexpr int NC = 1 << D;
    double cw[NC];
    int64_t off[NC];
    // an axis of one voxel has no second corner: its stencil offset is 0 and f = 0, the corner enters twice with weights 1, 0
    const int64_t sx = gs.n[0] > 1 ? 1 : 0;
    const int64_t sy = gs.n[1] > 1 ? gs.n[0] : 0;
    const int64_t sz = D == 3 && gs.n[2] > 1 ? gs.n[0] * gs.n[1] : 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1;
      double wt = by ? f[1] : 1.0 - f[1];
      if constexpr (D == 3) wt = (bz ? f[2] : 1.0 - f[2]) * wt;
      cw[k] = wt * (bx ? f[0] : 1.0 - f[0]);
      off[k] = base + bx * sx + by * sy + bz * sz;
    }
    for (int c = 0; c < ncomp; ++c) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) acc += cw[k] * img[off[k] * ncomp + c];
      out[p * ncomp + c] = acc;
    }
  }
}

GlSampler& sampler_of(glims_ctx* h, int64_t id, const char* who) {
  if (id < 0 || id >= (int64_t)h->samplers.size() || !h->samplers[(size_t)id])
    throw glims_error(GLIMS_E_USAGE, std::string(who) + ": unknown sampler id " + std::to_string(id));
  return *h->samplers[(size_t)id];
}

void need_memory(const char* who, size_t need) {
  size_t fr = 0, tot = 0;
  GL_HIP(hipMemGetInfo(&fr, &tot));
  if (need > fr)
    throw glims_error(GLIMS_E_HIP, std::string(who) + ": needs about " + std::to_string(need >> 20) +
                                       " MiB of device memory, " + std::to_string(fr >> 20) + " MiB are free");
}

// The transpose's lists from its sort input (key[p] = internal cell of the point's winner, n_cells for a point that enters no
// sum; val[p] = p): the stable sort, a cell's points and chunks.  Creation (single-rank handles) and glims_sampler_resolve.
void build_transpose(glims_ctx* h, GlSampler& s, dvec<uint32_t>& k_in, dvec<int32_t>& v_in) {
  const int64_t n = s.n, ne = h->n_cells;
  hipStream_t st = h->st;
  dvec<uint32_t> k_out;
  k_out.alloc((size_t)n);
  s.order.alloc((size_t)n);
  int bits = 1;
  while (((int64_t)1 << bits) <= ne) ++bits;
  gl_sort_pairs_u32(h, k_in.p, k_out.p, v_in.p, s.order.p, (size_t)n, bits);   // stable: point order inside a cell
  s.cptr.alloc((size_t)ne + 1);
  gl_offsets_of_sorted_keys(h, k_out.p, n, ne, s.cptr.p);
  dvec<int32_t> cnt;
  cnt.alloc((size_t)ne + 1);
  s.chunk_ptr.alloc((size_t)ne + 1);
  hipLaunchKernelGGL(k_chunk_count, dim3(grid_of(ne + 1)), dim3(256), 0, st, ne, s.cptr.p, cnt.p);
  GL_CHECK_LAUNCH();
  {
    size_t bytes = 0;
    GL_HIP(rocprim::exclusive_scan(nullptr, bytes, cnt.p, s.chunk_ptr.p, (int32_t)0, (size_t)ne + 1, rocprim::plus<int32_t>(), st));
    dvec<unsigned char> tmp;
    tmp.alloc(std::max<size_t>(bytes, 16));
    GL_HIP(rocprim::exclusive_scan(tmp.p, bytes, cnt.p, s.chunk_ptr.p, (int32_t)0, (size_t)ne + 1, rocprim::plus<int32_t>(), st));
    int32_t nch = 0;
    GL_HIP(hipMemcpyAsync(&nch, s.chunk_ptr.p + ne, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GL_HIP(hipStreamSynchronize(st));
    s.n_chunks = nch;
  }
  s.chunk_cell.alloc((size_t)std::max<int64_t>(1, s.n_chunks));
  if (ne > 0) {
    hipLaunchKernelGGL(k_chunk_cells, dim3(grid_of(ne)), dim3(256), 0, st, ne, s.chunk_ptr.p, s.chunk_cell.p);
    GL_CHECK_LAUNCH();
  }
  GL_HIP(hipStreamSynchronize(st));
  s.have_t = true;
}

template <int D>
// coords: the [n_nodes][D] node coordinates (internal numbering) the points are located in -- the mesh's own, or a deformed
// sampler's transient x = X + scale u
void create_t(glims_ctx* h, GlSampler& s, const double* xyz_host, const GridSpec& gs, const double* coords) {
  constexpr int NV = D + 1;
  const int64_t n = s.n, ne = h->n_cells;
  hipStream_t st = h->st;
  const bool want_t = h->world <= 1;
  // the sampler itself: 4 + NV (4 + 8) B per point (+ 4 B of order and ~8 B per cell for the transpose); transient: the claim
  // queue, the inverse cell permutation, the sort's keys / values twice, a point set's coordinates twice and its bins
  const size_t keep = (size_t)n * (4 + NV * 12 + (want_t ? 4 : 0)) + (want_t ? (size_t)ne * 12 : 0);
  const size_t temp = (size_t)ne * 8 + (size_t)n * (16 + (s.is_grid ? 0 : 16 * D + 8)) + (64u << 20);
  need_memory("glims_sampler_create", keep + temp);

  const int32_t* cell_nodes = gl_ensure_cell_nodes(h);
  const int32_t* new2old = h->cell_new2old.p;   // nullptr = identity (host symbolic phase)
  s.cell.alloc((size_t)std::max<int64_t>(1, n));
  s.node.alloc((size_t)std::max<int64_t>(1, n) * NV);
  s.w.alloc((size_t)std::max<int64_t>(1, n) * NV);
  dvec<int32_t> big;
  dvec<int> n_big;
  dvec<unsigned long long> d_found;
  big.alloc((size_t)std::max<int64_t>(1, ne));
  n_big.alloc_zero(1, st);
  d_found.alloc_zero(1, st);
  dvec<double> d_pts;
  if (n > 0 && ne > 0) {
    hipLaunchKernelGGL(k_fill_i32, dim3(grid_of(n)), dim3(256), 0, st, n, INT_MAX, s.cell.p);
    GL_CHECK_LAUNCH();
    int nb_host = 0;
    if (s.is_grid) {
      hipLaunchKernelGGL(k_claim_grid<D>, dim3(grid_of(ne)), dim3(256), 0, st, ne, cell_nodes, coords, new2old, gs,
                         s.cell.p, big.p, n_big.p);
      GL_CHECK_LAUNCH();
      GL_HIP(hipMemcpyAsync(&nb_host, n_big.p, sizeof(int), hipMemcpyDeviceToHost, st));
      GL_HIP(hipStreamSynchronize(st));
      if (nb_host > 0) {
        hipLaunchKernelGGL(k_claim_grid_big<D>, dim3(nb_host), dim3(256), 0, st, nb_host, big.p, cell_nodes, coords,
                           new2old, gs, s.cell.p);
        GL_CHECK_LAUNCH();
      }
    } else {
      // bins over the bounding box of the (finite) query points: about two points per bin, not more bins than cells
      BinSpec bs;
      for (int a = 0; a < 3; ++a) {
        bs.lo[a] = std::numeric_limits<double>::infinity();
        bs.hi[a] = -std::numeric_limits<double>::infinity();
        bs.inv_h[a] = 0.0;
        bs.nb[a] = 1;
      }
      for (int64_t p = 0; p < n; ++p) {
        bool fin = true;
        for (int a = 0; a < D; ++a) fin = fin && std::isfinite(xyz_host[p * D + a]);
        if (!fin) continue;
        for (int a = 0; a < D; ++a) {
          bs.lo[a] = std::min(bs.lo[a], xyz_host[p * D + a]);
          bs.hi[a] = std::max(bs.hi[a], xyz_host[p * D + a]);
        }
      }
      if (bs.lo[0] <= bs.hi[0]) {   // at least one finite point
        double vol = 1.0;
        int live = 0;
        for (int a = 0; a < D; ++a)
          if (bs.hi[a] > bs.lo[a]) {
            vol *= bs.hi[a] - bs.lo[a];
            ++live;
          }
        const double want = (double)std::max<int64_t>(1, std::min<int64_t>({n / 2, ne, (int64_t)1 << 27}));
        const double hb = live ? std::pow(vol / want, 1.0 / live) : 1.0;
        int64_t total = 1;
        for (int a = 0; a < D; ++a) {
          const double ext = bs.hi[a] - bs.lo[a];
          if (ext > 0.0 && hb > 0.0) {
            bs.nb[a] = (int)std::min(1024.0, std::max(1.0, std::floor(ext / hb)));
            bs.inv_h[a] = bs.nb[a] / ext;
          }
          total *= bs.nb[a];
        }
        d_pts.upload(xyz_host, (size_t)n * D, st);
        dvec<uint32_t> k_in, k_out;
        dvec<int32_t> v_in, pid, bin_ptr;
        dvec<double> pts_sorted;
        k_in.alloc((size_t)n);
        k_out.alloc((size_t)n);
        v_in.alloc((size_t)n);
        pid.alloc((size_t)n);
        pts_sorted.alloc((size_t)n * D);
        bin_ptr.alloc((size_t)total + 2);
        hipLaunchKernelGGL(k_point_bins<D>, dim3(grid_of(n)), dim3(256), 0, st, n, d_pts.p, bs, (uint32_t)total, k_in.p,
                           v_in.p);
        GL_CHECK_LAUNCH();
        int bits = 1;
        while (((int64_t)1 << bits) <= total) ++bits;
        gl_sort_pairs_u32(h, k_in.p, k_out.p, v_in.p, pid.p, (size_t)n, bits);
        gl_offsets_of_sorted_keys(h, k_out.p, n, total + 1, bin_ptr.p);   // bin_ptr[total]: where the points outside start
        hipLaunchKernelGGL(k_gather_points<D>, dim3(grid_of(n)), dim3(256), 0, st, n, pid.p, d_pts.p, pts_sorted.p);
        GL_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_claim_points<D>, dim3(grid_of(ne)), dim3(256), 0, st, ne, cell_nodes, coords, new2old, bs,
                           bin_ptr.p, pts_sorted.p, pid.p, s.cell.p, big.p, n_big.p);
        GL_CHECK_LAUNCH();
        GL_HIP(hipMemcpyAsync(&nb_host, n_big.p, sizeof(int), hipMemcpyDeviceToHost, st));
        GL_HIP(hipStreamSynchronize(st));
        if (nb_host > 0) {
          hipLaunchKernelGGL(k_claim_points_big<D>, dim3(nb_host), dim3(256), 0, st, nb_host, big.p, cell_nodes,
                             coords, new2old, bs, bin_ptr.p, pts_sorted.p, pid.p, s.cell.p);
          GL_CHECK_LAUNCH();
        }
        GL_HIP(hipStreamSynchronize(st));   // the sort buffers go out of scope
      }
    }
  }
  big.release();
  if (n == 0) return;
  if (ne == 0) {
    hipLaunchKernelGGL(k_fill_i32, dim3(grid_of(n)), dim3(256), 0, st, n, INT_MAX, s.cell.p);
    GL_CHECK_LAUNCH();
  }
  if (!s.is_grid && !d_pts.p) d_pts.upload(xyz_host, (size_t)n * D, st);

  // the winner's weights (and the transpose's sort input)
  dvec<int32_t> c_old2new;
  if (new2old && ne > 0) {
    c_old2new.alloc((size_t)ne);
    hipLaunchKernelGGL(k_invert_cells, dim3(grid_of(ne)), dim3(256), 0, st, ne, new2old, c_old2new.p);
    GL_CHECK_LAUNCH();
  }
  dvec<uint32_t> k_in;
  dvec<int32_t> v_in;
  if (want_t) {
    k_in.alloc((size_t)n);
    v_in.alloc((size_t)n);
  }
  hipLaunchKernelGGL(k_weights<D>, dim3(grid_of(n)), dim3(256), 0, st, n, ne, s.is_grid ? nullptr : d_pts.p, gs, cell_nodes,
                     coords, c_old2new.p, s.cell.p, s.node.p, s.w.p, k_in.p, v_in.p, d_found.p);
  GL_CHECK_LAUNCH();
  unsigned long long nf = 0;
  GL_HIP(hipMemcpyAsync(&nf, d_found.p, sizeof(nf), hipMemcpyDeviceToHost, st));
  GL_HIP(hipStreamSynchronize(st));
  s.n_found = (int64_t)nf;
  if (!want_t) return;

  build_transpose(h, s, k_in, v_in);
}

template <int NV>
void launch_sample(glims_ctx* h, GlSampler& s, int ncomp, const double* f, double fill, double* out) {
  const dim3 g(grid_of(s.n)), b(256);
#define GL_SAMPLE_CASE(BS)                                                                                              \
  hipLaunchKernelGGL((k_sample<NV, BS>), g, b, 0, h->st, s.n, ncomp, s.cell.p, s.node.p, s.w.p, f, fill, out)
  switch (ncomp) {
    case 1: GL_SAMPLE_CASE(1); break;
    case 2: GL_SAMPLE_CASE(2); break;
    case 3: GL_SAMPLE_CASE(3); break;
    default: GL_SAMPLE_CASE(0); break;
  }
#undef GL_SAMPLE_CASE
  GL_CHECK_LAUNCH();
}

}  // namespace

namespace {
// The creators' checks of their points (every creator refuses the same things, before anything is allocated); returns n.
int64_t check_points(glims_ctx* h, int64_t n, const double* xyz, const double* origin, const double* spacing,
                     const int64_t* size, GridSpec& gs) {
  const int D = h->dim;
  for (int a = 0; a < 3; ++a) {
    gs.o[a] = 0.0;
    gs.s[a] = 1.0;
    gs.n[a] = 1;
  }
  if (!xyz) {
    n = 1;
    for (int a = 0; a < D; ++a) {
      GL_REQUIRE(size[a] > 0, "glims_sampler_create_grid: size[" + std::to_string(a) + "] = " + std::to_string(size[a]) +
                                  " is not positive");
      GL_REQUIRE(spacing[a] > 0.0 && std::isfinite(spacing[a]),
                 "glims_sampler_create_grid: spacing[" + std::to_string(a) + "] is not positive");
      GL_REQUIRE(std::isfinite(origin[a]), "glims_sampler_create_grid: origin is not finite");
      gs.o[a] = origin[a];
      gs.s[a] = spacing[a];
      gs.n[a] = size[a];
      GL_REQUIRE(size[a] < INT_MAX / n, "glims_sampler_create_grid: more than 2^31 - 1 points");
      n *= size[a];
    }
  }
  GL_REQUIRE(n < INT_MAX, "glims_sampler_create: more than 2^31 - 2 points");
  GL_REQUIRE(h->xyz_new.n == (size_t)h->n_nodes * D, "mesh coordinates missing");
  GL_REQUIRE(h->world > 1 || h->n_own == h->n_nodes,
             "glims_sampler_create: a handle with ghost nodes needs its halo plan and transport first");
  return n;
}

// locates the points in the mesh whose nodes sit at `coords`; the caller owns the sampler until it enters h->samplers
GlSampler* create_on(glims_ctx* h, int64_t n, const double* xyz, const GridSpec& gs, const double* coords) {
  auto* s = new GlSampler();
  try {
    s->n = n;
    s->is_grid = !xyz;
    if (h->dim == 2) create_t<2>(h, *s, xyz, gs, coords);
    else create_t<3>(h, *s, xyz, gs, coords);
  } catch (...) {
    (void)hipStreamSynchronize(h->st);
    delete s;
    throw;
  }
  return s;
}

// n_inverted and min_ratio of a deformed sampler: one pass over the cells, then one block over the per-block minima
template <int D>
void deformation_stats(glims_ctx* h, GlSampler& s, const double* y) {
  const int64_t ne = h->n_cells;
  if (ne == 0) return;
  const unsigned nb = grid_of(ne);
  dvec<double> part;
  dvec<unsigned long long> d_bad;
  part.alloc((size_t)nb + 1);
  d_bad.alloc_zero(1, h->st);
  hipLaunchKernelGGL(k_deform_cells<D>, dim3(nb), dim3(256), 0, h->st, ne, gl_ensure_cell_nodes(h), h->xyz_new.p, y, part.p,
                     d_bad.p);
  GL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_deform_min, dim3(1), dim3(1024), 0, h->st, (int64_t)nb, part.p, part.p + nb);
  GL_CHECK_LAUNCH();
  unsigned long long bad = 0;
  double mn = 1.0;
  GL_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(bad), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipMemcpyAsync(&mn, part.p + nb, sizeof(mn), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  s.n_inverted = (int64_t)bad;
  s.min_ratio = mn;
}
}  // namespace

int64_t gl_sampler_create(glims_ctx* h, int64_t n, const double* xyz, const double* origin, const double* spacing,
                          const int64_t* size) {
  GridSpec gs;
  n = check_points(h, n, xyz, origin, spacing, size, gs);
  h->samplers.push_back(create_on(h, n, xyz, gs, h->xyz_new.p));
  return (int64_t)h->samplers.size() - 1;
}

int gl_sampler_create_deformed(glims_ctx* h, int64_t n, const double* xyz, const double* origin, const double* spacing,
                               const int64_t* size, int64_t u_source, const double* u_host, double scale, int64_t* id) {
  const char* who = "glims_sampler_create_deformed";
  // ---- refusals: nothing is allocated or changed before the last of them ----
  GL_REQUIRE(h->world <= 1, std::string(who) + ": not available on a partitioned handle (world > 1)");
  GL_REQUIRE(std::isfinite(scale), std::string(who) + ": scale is not finite");
  if (u_source == GLIMS_DERIVE_HOST) {
    GL_REQUIRE(u_host, std::string(who) + ": GLIMS_DERIVE_HOST needs u_host (null pointer)");
  } else {
    GL_REQUIRE(h->is_setup && h->have_mech && h->U.p,
               std::string(who) + ": a snapshot or GLIMS_DERIVE_CURRENT source needs the displacement: "
                                  "glims_setup(with_mechanics=1) first");
    if (u_source == GLIMS_DERIVE_CURRENT) {
      GL_REQUIRE(h->have_state, std::string(who) + ": GLIMS_DERIVE_CURRENT before glims_set_state");
    } else {
      GL_REQUIRE(u_source >= 0 && u_source < (int64_t)h->snapshots.size() && h->snapshots[(size_t)u_source],
                 std::string(who) + ": unknown snapshot id " + std::to_string(u_source));
      GL_REQUIRE(h->have_state, std::string(who) + ": a snapshot source before glims_set_state");
    }
  }
  GridSpec gs;
  n = check_points(h, n, xyz, origin, spacing, size, gs);
  const int D = h->dim;
  const int64_t nn = h->n_nodes;
  need_memory(who, (size_t)nn * D * sizeof(double) * (u_source == GLIMS_DERIVE_HOST ? 2 : 1) + (1u << 20));
  // ---- the displacement ----
  int status = GLIMS_OK;
  dvec<double> u_up;
  const double* u = h->U.p;
  if (u_source == GLIMS_DERIVE_HOST) {
    u_up.alloc((size_t)std::max<int64_t>(1, nn * D));
    gl_to_device_perm(h, u_host, u_up.p, D);   // the permuting upload: neither c nor U is touched
    u = u_up.p;
  } else if (u_source != GLIMS_DERIVE_CURRENT && h->derive.u_snapshot != u_source) {
    // as glims_snapshot_mechanics solves it; glims_derive of the same snapshot finds U in place and the other way round
    h->derive.forget_u();
    status = gl_solve_mechanics(h, h->snapshots[(size_t)u_source]->p);
    h->derive.n_elastic_solves++;
    if (status == GLIMS_OK) h->derive.u_snapshot = u_source;
    if (status == GLIMS_NAN) return status;
  }
  // ---- y = X + scale u, its cells' determinants, the location ----
  dvec<double> y;
  y.alloc((size_t)std::max<int64_t>(1, nn * D));
  if (nn > 0) {
    if (D == 2) hipLaunchKernelGGL(k_deform_xyz<2>, dim3(grid_of(nn)), dim3(256), 0, h->st, nn, h->xyz_new.p, u, scale, y.p);
    else hipLaunchKernelGGL(k_deform_xyz<3>, dim3(grid_of(nn)), dim3(256), 0, h->st, nn, h->xyz_new.p, u, scale, y.p);
    GL_CHECK_LAUNCH();
  }
  GlSampler* s = create_on(h, n, xyz, gs, y.p);
  try {
    s->deformed = true;
    if (D == 2) deformation_stats<2>(h, *s, y.p);
    else deformation_stats<3>(h, *s, y.p);
  } catch (...) {
    (void)hipStreamSynchronize(h->st);
    delete s;
    throw;
  }
  GL_HIP(hipStreamSynchronize(h->st));   // y and the uploaded u go out of scope
  h->samplers.push_back(s);
  *id = (int64_t)h->samplers.size() - 1;
  return status;
}

void gl_sampler_deformation_info(glims_ctx* h, int64_t id, int64_t out[2], double* min_ratio) {
  GlSampler& s = sampler_of(h, id, "glims_sampler_deformation_info");
  if (out) {
    out[0] = s.deformed ? 1 : 0;
    out[1] = s.deformed ? s.n_inverted : 0;
  }
  if (min_ratio) *min_ratio = s.deformed ? s.min_ratio : 1.0;
}

void gl_sampler_warp(glims_ctx* h, int64_t id, const double* image, const double* origin, const double* spacing,
                     const int64_t* size, int ncomp, int order, double fill, double* out) {
  const char* who = "glims_sampler_warp";
  GlSampler& s = sampler_of(h, id, who);
  GL_REQUIRE(h->world <= 1, std::string(who) + ": not available on a partitioned handle (world > 1)");
  GL_REQUIRE(order == 0 || order == 1, std::string(who) + ": order = " + std::to_string(order) + " is neither 0 (nearest) nor 1 (linear)");
  GL_REQUIRE(ncomp >= 1 && ncomp <= GLIMS_SAMPLE_MAX_COMP, std::string(who) + ": ncomp = " + std::to_string(ncomp) + " outside 1 .. 8");
  GL_REQUIRE(image, std::string(who) + ": null image");
  GL_REQUIRE(origin && spacing && size, std::string(who) + ": null origin, spacing or size");
  GL_REQUIRE(out || s.n == 0, std::string(who) + ": null output");
  const int D = h->dim;
  GridSpec gs;
  for (int a = 0; a < 3; ++a) {
    gs.o[a] = 0.0;
    gs.s[a] = 1.0;
    gs.n[a] = 1;
  }
  double nvox_d = 1.0;
  size_t nvox = 1;
  for (int a = 0; a < D; ++a) {
    GL_REQUIRE(size[a] > 0, std::string(who) + ": size[" + std::to_string(a) + "] = " + std::to_string(size[a]) + " is not positive");
    GL_REQUIRE(spacing[a] > 0.0 && std::isfinite(spacing[a]), std::string(who) + ": spacing[" + std::to_string(a) + "] is not positive");
    GL_REQUIRE(std::isfinite(origin[a]), std::string(who) + ": origin is not finite");
    gs.o[a] = origin[a];
    gs.s[a] = spacing[a];
    gs.n[a] = size[a];
    nvox_d *= (double)size[a];
    GL_REQUIRE(nvox_d < 1099511627776.0, std::string(who) + ": more than 2^40 voxels");
    nvox *= (size_t)size[a];
  }
  if (s.n == 0) return;
  const size_t ni = nvox * (size_t)ncomp, no = (size_t)s.n * ncomp;
  if (s.img.n < ni || s.out.n < no) {
    need_memory(who, ((s.img.n < ni ? ni : 0) + (s.out.n < no ? no : 0)) * sizeof(double));
    if (s.img.n < ni) s.img.alloc(ni);
    if (s.out.n < no) s.out.alloc(no);
  }
  GL_HIP(hipMemcpyAsync(s.img.p, image, ni * sizeof(double), hipMemcpyHostToDevice, h->st));
  const dim3 g(grid_of(s.n)), b(256);
#define GL_WARP_CASE(NV, DD, ORD)                                                                                       \
  hipLaunchKernelGGL((k_warp<NV, DD, ORD>), g, b, 0, h->st, s.n, ncomp, s.cell.p, s.node.p, s.w.p, h->xyz_new.p, gs, \
                     s.img.p, fill, s.out.p)
  if (D == 2) {
    if (order == 1) GL_WARP_CASE(3, 2, 1);
    else GL_WARP_CASE(3, 2, 0);
  } else {
    if (order == 1) GL_WARP_CASE(4, 3, 1);
    else GL_WARP_CASE(4, 3, 0);
  }
#undef GL_WARP_CASE
  GL_CHECK_LAUNCH();
  GL_HIP(hipMemcpyAsync(out, s.out.p, no * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
}

void gl_sampler_info(glims_ctx* h, int64_t id, int64_t* n_points, int64_t* n_found) {
  GlSampler& s = sampler_of(h, id, "glims_sampler_info");
  if (n_points) *n_points = s.n;
  if (n_found) *n_found = s.n_found;
}

void gl_sampler_get(glims_ctx* h, int64_t id, int32_t* cell, double* w) {
  GlSampler& s = sampler_of(h, id, "glims_sampler_get");
  if (s.n == 0) return;
  if (cell) GL_HIP(hipMemcpyAsync(cell, s.cell.p, (size_t)s.n * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
  if (w) GL_HIP(hipMemcpyAsync(w, s.w.p, (size_t)s.n * h->nv * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
}

void gl_sampler_apply(glims_ctx* h, int64_t id, int field, int64_t snapshot, const double* nodal, int ncomp, double fill,
                      double* out) {
  GlSampler& s = sampler_of(h, id, "glims_sampler_apply");
  GL_REQUIRE(ncomp >= 1 && ncomp <= GLIMS_SAMPLE_MAX_COMP,
             "glims_sampler_apply: ncomp = " + std::to_string(ncomp) + " outside 1 .. 8");
  GL_REQUIRE(out || s.n == 0, "glims_sampler_apply: null output");
  const double* f = nullptr;
  switch (field) {
    case GLIMS_FIELD_C:
      GL_REQUIRE(h->have_state, "glims_sampler_apply: GLIMS_FIELD_C before glims_set_state");
      GL_REQUIRE(ncomp == 1, "glims_sampler_apply: GLIMS_FIELD_C has 1 component");
      f = h->c.p;
      break;
    case GLIMS_FIELD_U:
      GL_REQUIRE(h->have_mech && h->U.p, "glims_sampler_apply: GLIMS_FIELD_U needs glims_setup(with_mechanics=1)");
      GL_REQUIRE(ncomp == h->dim, "glims_sampler_apply: GLIMS_FIELD_U has dim components");
      f = h->U.p;
      break;
    case GLIMS_FIELD_SNAPSHOT_C:
      GL_REQUIRE(snapshot >= 0 && snapshot < (int64_t)h->snapshots.size() && h->snapshots[(size_t)snapshot],
                 "glims_sampler_apply: unknown snapshot id " + std::to_string(snapshot));
      GL_REQUIRE(ncomp == 1, "glims_sampler_apply: GLIMS_FIELD_SNAPSHOT_C has 1 component");
      f = h->snapshots[(size_t)snapshot]->p;
      break;
    case GLIMS_FIELD_HOST: {
      GL_REQUIRE(nodal, "glims_sampler_apply: GLIMS_FIELD_HOST needs the nodal array");
      const size_t nn = (size_t)h->n_nodes * ncomp;
      if (s.f_ext.n < nn) {
        need_memory("glims_sampler_apply", 2 * nn * sizeof(double));
        s.f_ext.alloc(nn);
        s.f_int.alloc(nn);
      }
      GL_HIP(hipMemcpyAsync(s.f_ext.p, nodal, nn * sizeof(double), hipMemcpyHostToDevice, h->st));
      hipLaunchKernelGGL(k_nodal_in, dim3(grid_of((int64_t)nn)), dim3(256), 0, h->st, h->n_nodes, ncomp, h->d_old2new.p,
                         s.f_ext.p, s.f_int.p);
      GL_CHECK_LAUNCH();
      f = s.f_int.p;
      break;
    }
    case GLIMS_FIELD_DERIVED:
      f = gl_derive_sampled(h, ncomp);
      break;
    case GLIMS_FIELD_XYZ:   // the REFERENCE coordinates: on a deformed sampler the back map X(x_p)
      GL_REQUIRE(ncomp == h->dim, "glims_sampler_apply: GLIMS_FIELD_XYZ has dim components");
      f = h->xyz_new.p;
      break;
    default:
      GL_REQUIRE(false, "glims_sampler_apply: unknown field " + std::to_string(field));
  }
  if (s.n == 0) return;
  const size_t no = (size_t)s.n * ncomp;
  if (s.out.n < no) {
    need_memory("glims_sampler_apply", no * sizeof(double));
    s.out.alloc(no);
  }
  if (h->nv == 3) launch_sample<3>(h, s, ncomp, f, fill, s.out.p);
  else launch_sample<4>(h, s, ncomp, f, fill, s.out.p);
  GL_HIP(hipMemcpyAsync(out, s.out.p, no * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
}

// The two launches of P^T on device pointers: pass 1 into the sampler's chunk buffer, pass 2 row-owned into g (internal
// numbering; overwritten, or added to with `accumulate`).  Without `accumulate` g is [n_nodes][ncomp] contiguous and is zeroed
// first on a partitioned handle: pass 2 writes the owned rows, the ghost rows hold 0.
namespace {
void transpose_on(glims_ctx* h, GlSampler& s, const double* r_dev, int ncomp, double* g_int_dev, int64_t ld_row,
                  int64_t ld_comp, bool accumulate) {
  GL_REQUIRE(h->world <= 1 || s.resolved,
             "glims_sampler_apply_t: not available on a partitioned handle before glims_sampler_resolve (the per-cell sums "
             "need the globally winning cell on every rank that holds it)");
  GL_REQUIRE(ncomp >= 1 && ncomp <= GLIMS_SAMPLE_MAX_COMP,
             "glims_sampler_apply_t: ncomp = " + std::to_string(ncomp) + " outside 1 .. 8");
  if (!(s.n > 0 && s.have_t && s.n_chunks > 0)) {
    if (!accumulate) GL_HIP(hipMemsetAsync(g_int_dev, 0, (size_t)h->n_nodes * ncomp * sizeof(double), h->st));
    return;
  }
  const size_t nq = (size_t)s.n_chunks * h->nv * ncomp;
  if (s.q.n < nq) {
    need_memory("glims_sampler_apply_t", nq * sizeof(double));
    s.q.alloc(nq);
  }
  if (!accumulate && h->n_own < h->n_nodes)
    GL_HIP(hipMemsetAsync(g_int_dev, 0, (size_t)h->n_nodes * ncomp * sizeof(double), h->st));
  if (h->nv == 3)
    hipLaunchKernelGGL(k_sample_t_cells<3>, dim3(grid_of(s.n_chunks)), dim3(256), 0, h->st, s.n_chunks, ncomp,
                       s.chunk_cell.p, s.chunk_ptr.p, s.cptr.p, s.order.p, s.w.p, r_dev, s.q.p);
  else
    hipLaunchKernelGGL(k_sample_t_cells<4>, dim3(grid_of(s.n_chunks)), dim3(256), 0, h->st, s.n_chunks, ncomp,
                       s.chunk_cell.p, s.chunk_ptr.p, s.cptr.p, s.order.p, s.w.p, r_dev, s.q.p);
  GL_CHECK_LAUNCH();
  const DevPattern& pt = h->pat;
  if (h->nv == 3)
    hipLaunchKernelGGL(k_sample_t<3>, dim3(grid_of(h->n_own)), dim3(256), 0, h->st, h->n_own, ncomp, pt.cslice_ptr.p,
                       pt.cslots.p, pt.celem.p, pt.diag_k.p, s.chunk_ptr.p, s.q.p, g_int_dev, ld_row, ld_comp,
                       accumulate ? 1 : 0);
  else
    hipLaunchKernelGGL(k_sample_t<4>, dim3(grid_of(h->n_own)), dim3(256), 0, h->st, h->n_own, ncomp, pt.cslice_ptr.p,
                       pt.cslots.p, pt.celem.p, pt.diag_k.p, s.chunk_ptr.p, s.q.p, g_int_dev, ld_row, ld_comp,
                       accumulate ? 1 : 0);
  GL_CHECK_LAUNCH();
}
}  // namespace

void gl_sampler_transpose_dev(glims_ctx* h, int64_t id, const double* r_dev, int ncomp, double* g_int_dev, int64_t ld_row,
                              int64_t ld_comp, bool accumulate) {
  transpose_on(h, sampler_of(h, id, "glims_sampler_apply_t"), r_dev, ncomp, g_int_dev, ld_row, ld_comp, accumulate);
}

void gl_sampler_apply_t(glims_ctx* h, int64_t id, const double* r, int ncomp, double* g) {
  GlSampler& s = sampler_of(h, id, "glims_sampler_apply_t");
  GL_REQUIRE(h->world <= 1 || s.resolved,
             "glims_sampler_apply_t: not available on a partitioned handle before glims_sampler_resolve (the per-cell sums "
             "need the globally winning cell on every rank that holds it)");
  GL_REQUIRE(ncomp >= 1 && ncomp <= GLIMS_SAMPLE_MAX_COMP,
             "glims_sampler_apply_t: ncomp = " + std::to_string(ncomp) + " outside 1 .. 8");
  GL_REQUIRE(g && (r || s.n == 0), "glims_sampler_apply_t: null argument");
  const int64_t nn = h->n_nodes;
  const size_t ng = (size_t)nn * ncomp, nr = (size_t)std::max<int64_t>(1, s.n) * ncomp;
  const size_t nq = (size_t)std::max<int64_t>(1, s.n_chunks) * h->nv * ncomp;
  if (s.g_int.n < ng || s.f_ext.n < ng || s.out.n < nr || s.q.n < nq) {
    need_memory("glims_sampler_apply_t", (2 * ng + nr + nq) * sizeof(double));
    if (s.g_int.n < ng) s.g_int.alloc(ng);
    if (s.f_ext.n < ng) {
      s.f_ext.alloc(ng);
      s.f_int.alloc(ng);
    }
    if (s.out.n < nr) s.out.alloc(nr);
    if (s.q.n < nq) s.q.alloc(nq);
  }
  if (s.n > 0 && s.have_t && s.n_chunks > 0)
    GL_HIP(hipMemcpyAsync(s.out.p, r, (size_t)s.n * ncomp * sizeof(double), hipMemcpyHostToDevice, h->st));
  gl_sampler_transpose_dev(h, id, s.out.p, ncomp, s.g_int.p, ncomp, 1, false);
  hipLaunchKernelGGL(k_nodal_out, dim3(grid_of((int64_t)ng)), dim3(256), 0, h->st, nn, ncomp, h->d_old2new.p, s.g_int.p,
                     s.f_ext.p);
  GL_CHECK_LAUNCH();
  GL_HIP(hipMemcpyAsync(g, s.f_ext.p, ng * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
}

// ---- glims_sampler_resolve: the globally winning cell on every rank that holds it ------------------------------------------------
namespace {
// One rank's verdict (GLIMS_E_USAGE with the reason); returns the sampler
GlSampler& check_resolve(glims_ctx* h, int64_t id, const int64_t* cell_gid) {
  const char* who = "glims_sampler_resolve";
  GlSampler& s = sampler_of(h, id, who);
  // (a stored term's sampler is resolved already: the call is refused, not taken for a repeated resolve)
  for (size_t k = 0; k < h->img_terms.size(); ++k)
    GL_REQUIRE(h->img_terms[k]->sampler != id, std::string(who) + ": sampler " + std::to_string(id) +
                                                   " is used by stored image term " + std::to_string(k));
  if (s.resolved) return s;
  GL_REQUIRE(cell_gid || h->n_cells == 0, std::string(who) + ": null cell_gid");
  for (int64_t e = 0; e < h->n_cells; ++e) {
    GL_REQUIRE(cell_gid[e] >= 0 && (double)cell_gid[e] < GL_RESOLVE_NONE,
               std::string(who) + ": cell_gid[" + std::to_string(e) + "] is negative or not below 2^53");
    GL_REQUIRE(e == 0 || cell_gid[e] > cell_gid[e - 1],
               std::string(who) + ": cell_gid is not strictly increasing at " + std::to_string(e));
  }
  return s;
}

template <int NV>
void resolve_t(glims_ctx* h, GlSampler& s, const int64_t* cell_gid) {
  const int64_t n = s.n, ne = h->n_cells;
  const int world = h->world;
  hipStream_t st = h->st;
  // the key buffer [world][m] stays bounded: the points go through it in chunks of m
  const int64_t m_max = std::max<int64_t>(1, (int64_t)(GL_RESOLVE_BYTES / (sizeof(double) * (size_t)world)));
  const int64_t m_buf = std::min<int64_t>(n, m_max);
  // kept: counted, order and the per-cell lists; transient: the key buffer, the cell ids, the inverse cell permutation and the
  // sort's keys / values twice
  need_memory("glims_sampler_resolve", (size_t)n * 5 + (size_t)ne * 12 + (size_t)m_buf * world * sizeof(double) +
                                           (size_t)ne * 12 + (size_t)n * 16 + (16u << 20));
  dvec<int64_t> d_gid;
  d_gid.upload(cell_gid, (size_t)ne, st);
  dvec<int32_t> c_old2new;
  if (h->cell_new2old.p && ne > 0) {
    c_old2new.alloc((size_t)ne);
    hipLaunchKernelGGL(k_invert_cells, dim3(grid_of(ne)), dim3(256), 0, st, ne, h->cell_new2old.p, c_old2new.p);
    GL_CHECK_LAUNCH();
  }
  dvec<double> buf;
  dvec<uint32_t> k_in;
  dvec<int32_t> v_in;
  dvec<unsigned long long> d_kept;
  buf.alloc((size_t)m_buf * world);
  k_in.alloc((size_t)n);
  v_in.alloc((size_t)n);
  d_kept.alloc_zero(1, st);
  s.counted.alloc((size_t)n);
  for (int64_t p0 = 0; p0 < n; p0 += m_buf) {
    const int64_t m = std::min<int64_t>(m_buf, n - p0);
    GL_HIP(hipMemsetAsync(buf.p, 0, (size_t)m * world * sizeof(double), st));
    hipLaunchKernelGGL(k_resolve_keys, dim3(grid_of(m)), dim3(256), 0, st, m, p0, s.cell.p, d_gid.p,
                       buf.p + (size_t)h->rank * m);
    GL_CHECK_LAUNCH();
    gl_allreduce_bulk(h, buf.p, (size_t)m * world);   // x + 0 is exact: every rank receives every row bit for bit
    hipLaunchKernelGGL(k_resolve_pick<NV>, dim3(grid_of(m)), dim3(256), 0, st, m, p0, world, h->rank, ne, buf.p, c_old2new.p,
                       s.cell.p, s.node.p, s.w.p, s.counted.p, k_in.p, v_in.p, d_kept.p);
    GL_CHECK_LAUNCH();
  }
  unsigned long long nk = 0;
  GL_HIP(hipMemcpyAsync(&nk, d_kept.p, sizeof(nk), hipMemcpyDeviceToHost, st));
  GL_HIP(hipStreamSynchronize(st));
  s.n_found = (int64_t)nk;
  build_transpose(h, s, k_in, v_in);
}
}  // namespace

void gl_sampler_resolve(glims_ctx* h, int64_t id, const int64_t* cell_gid) {
  if (h->world <= 1) {
    (void)sampler_of(h, id, "glims_sampler_resolve");   // the sampler is global already
    return;
  }
  // Collective: a rank that refused alone would leave the others waiting in the gather.  Every rank's verdict, point count and
  // state go through one all-reduce ([3][world], zeros outside the own column) before any other collective.
  GlSampler* s = nullptr;
  std::string why;
  try {
    s = &check_resolve(h, id, cell_gid);
  } catch (const glims_error& e) {
    if (e.code != GLIMS_E_USAGE) throw;
    why = e.what();
  }
  const size_t W = (size_t)h->world;
  std::vector<double> flag(3 * W, 0.0);
  flag[(size_t)h->rank] = why.empty() ? 0.0 : 1.0;
  flag[W + (size_t)h->rank] = s ? (double)s->n : 0.0;
  flag[2 * W + (size_t)h->rank] = s && s->resolved ? 1.0 : 0.0;
  dvec<double> d_flag;
  d_flag.upload(flag, h->st);
  gl_allreduce_bulk(h, d_flag.p, flag.size());
  GL_HIP(hipMemcpyAsync(flag.data(), d_flag.p, flag.size() * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  std::string refused;
  for (size_t r = 0; r < W; ++r)
    if (flag[r] != 0.0) refused += (refused.empty() ? "" : ", ") + std::to_string(r);
  if (!why.empty()) throw glims_error(GLIMS_E_USAGE, why + " (ranks that refused: " + refused + ")");
  if (!refused.empty())
    throw glims_error(GLIMS_E_USAGE, "glims_sampler_resolve: refused on rank(s) " + refused + " (see their messages)");
  for (size_t r = 1; r < W; ++r) {
    GL_REQUIRE(flag[W + r] == flag[W], "glims_sampler_resolve: the ranks disagree on n_points (rank 0: " +
                                           std::to_string((long long)flag[W]) + ", rank " + std::to_string(r) + ": " +
                                           std::to_string((long long)flag[W + r]) + ")");
    GL_REQUIRE(flag[2 * W + r] == flag[2 * W], "glims_sampler_resolve: the sampler is resolved on some ranks only");
  }
  if (s->resolved) return;
  if (s->n > 0) {
    if (h->nv == 3) resolve_t<3>(h, *s, cell_gid);
    else resolve_t<4>(h, *s, cell_gid);
  }
  s->resolved = true;
}

void gl_sampler_get_counted(glims_ctx* h, int64_t id, uint8_t* counted) {
  GlSampler& s = sampler_of(h, id, "glims_sampler_get_counted");
  if (s.n == 0) return;
  GL_REQUIRE(counted, "glims_sampler_get_counted: null output");
  if (s.resolved) {
    GL_HIP(hipMemcpyAsync(counted, s.counted.p, (size_t)s.n, hipMemcpyDeviceToHost, h->st));
    GL_HIP(hipStreamSynchronize(h->st));
    return;
  }
  std::vector<int32_t> cell((size_t)s.n);
  GL_HIP(hipMemcpyAsync(cell.data(), s.cell.p, (size_t)s.n * sizeof(int32_t), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  for (int64_t p = 0; p < s.n; ++p) counted[p] = cell[(size_t)p] >= 0 ? 1 : 0;
}

// ---- stored image terms ----------------------------------------------------------------------------------------------------
void gl_image_terms_set(glims_ctx* h, int n, const glims_image_misfit* terms) {
  const char* who = "glims_adjoint_image_terms";
  GL_REQUIRE(n >= 0 && (n == 0 || terms), std::string(who) + ": bad term list");
  // every check before anything is allocated or the old list is touched
  size_t need = 0;
  for (int k = 0; k < n; ++k) {
    const glims_image_misfit& t = terms[k];
    const std::string tk = std::string(who) + ": term " + std::to_string(k);
    GlSampler& s = sampler_of(h, t.sampler, who);
    GL_REQUIRE(h->world <= 1 || s.resolved, tk + ": not available on a partitioned handle before glims_sampler_resolve of its "
                                                 "sampler (glims_sampler_apply_t, the transpose the gradient needs, is "
                                                 "refused until then)");
    GL_REQUIRE(!s.deformed, tk + ": its sampler is a deformed one: its points move with the state through u, the derivative of "
                               "the location is not built and a frozen-location gradient would be inexact");
    GL_REQUIRE(t.kind == GLIMS_MISFIT_IMG_L2 || t.kind == GLIMS_MISFIT_IMG_THRESH, tk + ": unknown kind");
    GL_REQUIRE(t.kind != GLIMS_MISFIT_IMG_THRESH || (t.smooth > 0.0 && std::isfinite(t.smooth) && std::isfinite(t.level)),
               tk + ": a threshold term needs smooth > 0 and a finite level");
    GL_REQUIRE(std::isfinite(t.weight), tk + ": non-finite weight");
    GL_REQUIRE(t.target, tk + ": null target");
    GL_REQUIRE(t.step >= 0, tk + ": negative step");
    if (t.pweight)
      for (int64_t p = 0; p < s.n; ++p)
        GL_REQUIRE(t.pweight[p] >= 0.0 && std::isfinite(t.pweight[p]),
                   tk + ": pweight[" + std::to_string(p) + "] is negative or not finite");
    need += (size_t)s.n * (t.pweight ? 16 : 8);
  }
  if (n > 0) need_memory(who, need + (1u << 20));
  std::vector<GlImageTerm*> fresh;
  try {
    dvec<unsigned long long> d_obs;
    for (int k = 0; k < n; ++k) {
      const glims_image_misfit& t = terms[k];
      GlSampler& s = sampler_of(h, t.sampler, who);
      auto* g = new GlImageTerm();
      fresh.push_back(g);
      g->step = t.step;
      g->sampler = t.sampler;
      g->kind = t.kind;
      g->level = t.level;
      g->smooth = t.smooth;
      g->weight = t.weight;
      g->n = s.n;
      if (s.n == 0) continue;
      g->target.upload(t.target, (size_t)s.n, h->st);
      if (t.pweight) g->pweight.upload(t.pweight, (size_t)s.n, h->st);
      d_obs.alloc_zero(1, h->st);
      hipLaunchKernelGGL(k_img_prepare, dim3(grid_of(s.n)), dim3(256), 0, h->st, s.n, s.cell.p, g->pweight.p,
                         s.resolved ? s.counted.p : nullptr, g->target.p, d_obs.p);
      GL_CHECK_LAUNCH();
      unsigned long long no = 0;
      GL_HIP(hipMemcpyAsync(&no, d_obs.p, sizeof(no), hipMemcpyDeviceToHost, h->st));
      GL_HIP(hipStreamSynchronize(h->st));   // (the caller's arrays are free again)
      g->n_obs = (int64_t)no;
    }
  } catch (...) {
    (void)hipStreamSynchronize(h->st);
    for (auto* g : fresh) delete g;
    throw;
  }
  for (auto* g : h->img_terms) delete g;
  h->img_terms.swap(fresh);
}

void gl_image_term_info(glims_ctx* h, int k, int64_t out[3]) {
  GL_REQUIRE(out, "glims_adjoint_image_info: null output");
  GL_REQUIRE(k >= 0 && k < (int)h->img_terms.size(), "glims_adjoint_image_info: no stored term " + std::to_string(k));
  const GlImageTerm& t = *h->img_terms[(size_t)k];
  out[0] = t.sampler;
  out[1] = t.n;
  out[2] = t.n_obs;
}

namespace {
// r / r2 live in the sampler's point staging, the partials in its own buffer
void image_staging(glims_ctx* h, GlSampler& s, int ncomp) {
  const size_t nr = (size_t)s.n * ncomp, np = (size_t)grid_of(s.n) + 1;
  if (s.out.n < nr || s.part.n < np) {
    need_memory("glims_adjoint_gradient (image terms)", (nr + np) * sizeof(double));
    if (s.out.n < nr) s.out.alloc(nr);
    if (s.part.n < np) s.part.alloc(np);
  }
}
}  // namespace

double gl_image_misfit_grad(glims_ctx* h, const GlImageTerm& t, const double* c, double* g) {
  GlSampler& s = sampler_of(h, t.sampler, "glims_adjoint_gradient");
  if (s.n == 0) return 0.0;
  image_staging(h, s, 1);
  const unsigned nb = grid_of(s.n);
  const uint8_t* counted = s.resolved ? s.counted.p : nullptr;   // (partitioned handles: this rank's share of the sum)
  if (h->nv == 3)
    hipLaunchKernelGGL(k_img_misfit<3>, dim3(nb), dim3(256), 0, h->st, s.n, t.kind, t.level, t.smooth, t.weight, s.node.p,
                       s.w.p, c, t.target.p, t.pweight.p, counted, s.out.p, s.part.p);
  else
    hipLaunchKernelGGL(k_img_misfit<4>, dim3(nb), dim3(256), 0, h->st, s.n, t.kind, t.level, t.smooth, t.weight, s.node.p,
                       s.w.p, c, t.target.p, t.pweight.p, counted, s.out.p, s.part.p);
  GL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_img_sum, dim3(1), dim3(1024), 0, h->st, (int64_t)nb, s.part.p, s.part.p + nb);
  GL_CHECK_LAUNCH();
  gl_sampler_transpose_dev(h, t.sampler, s.out.p, 1, g, 1, 0, true);
  double sum = 0.0;
  GL_HIP(hipMemcpyAsync(&sum, s.part.p + nb, sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  return sum;
}

void gl_image_misfit_second(glims_ctx* h, const GlImageTerm& t, const double* c, const double* dc, int P, int64_t ld,
                            double* dg) {
  GlSampler& s = sampler_of(h, t.sampler, "glims_adjoint_hessian");
  if (s.n == 0) return;
  image_staging(h, s, P);
  if (h->nv == 3)
    hipLaunchKernelGGL(k_img_misfit_dir<3>, dim3(grid_of(s.n)), dim3(256), 0, h->st, s.n, P, ld, t.kind, t.level, t.smooth,
                       t.weight, s.node.p, s.w.p, c, dc, t.target.p, t.pweight.p, s.out.p);
  else
    hipLaunchKernelGGL(k_img_misfit_dir<4>, dim3(grid_of(s.n)), dim3(256), 0, h->st, s.n, P, ld, t.kind, t.level, t.smooth,
                       t.weight, s.node.p, s.w.p, c, dc, t.target.p, t.pweight.p, s.out.p);
  GL_CHECK_LAUNCH();
  gl_sampler_transpose_dev(h, t.sampler, s.out.p, P, dg, 1, ld, true);
}

// ---- stored displacement-image terms -------------------------------------------------------------------------------------------
void gl_displacement_image_terms_set(glims_ctx* h, int n, const glims_displacement_image_misfit* terms) {
  const char* who = "glims_adjoint_displacement_image_terms";
  GL_REQUIRE(n >= 0 && (n == 0 || terms), std::string(who) + ": bad term list");
  const int D = h->dim;
  // every check before anything is allocated or the old list is touched
  if (n > 0) {
    GL_REQUIRE(h->world <= 1, std::string(who) + ": not available on partitioned handles (world > 1)");
    GL_REQUIRE(h->is_setup && h->have_mech, std::string(who) + ": a displacement image term needs glims_setup(with_mechanics=1)");
  }
  size_t need = 0;
  for (int k = 0; k < n; ++k) {
    const glims_displacement_image_misfit& t = terms[k];
    const std::string tk = std::string(who) + ": term " + std::to_string(k);
    GlSampler& s = sampler_of(h, t.sampler, who);
    GL_REQUIRE(!s.deformed, tk + ": its sampler is a deformed one: the term compares u at reference points (a warp field on "
                               "the deformed grid is not built)");
    GL_REQUIRE(std::isfinite(t.weight), tk + ": non-finite weight");
    GL_REQUIRE(std::isfinite(t.scale), tk + ": non-finite scale");
    bool any = false;
    for (int a = 0; a < D; ++a) {
      GL_REQUIRE(t.cweight[a] >= 0.0 && std::isfinite(t.cweight[a]),
                 tk + ": cweight[" + std::to_string(a) + "] is negative or not finite");
      any = any || t.cweight[a] != 0.0;
    }
    GL_REQUIRE(any, tk + ": every cweight is 0: the term observes nothing");
    GL_REQUIRE(t.target, tk + ": null target");
    GL_REQUIRE(t.step >= 0, tk + ": negative step");
    if (t.pweight)
      for (int64_t p = 0; p < s.n; ++p)
        GL_REQUIRE(t.pweight[p] >= 0.0 && std::isfinite(t.pweight[p]),
                   tk + ": pweight[" + std::to_string(p) + "] is negative or not finite");
    need += (size_t)s.n * 8 * (D + (t.pweight ? 1 : 0));
  }
  if (n > 0) need_memory(who, need + (1u << 20));
  std::vector<GlDisplacementImageTerm*> fresh;
  try {
    dvec<unsigned long long> d_obs;
    std::vector<double> planes;
    for (int k = 0; k < n; ++k) {
      const glims_displacement_image_misfit& t = terms[k];
      GlSampler& s = sampler_of(h, t.sampler, who);
      auto* g = new GlDisplacementImageTerm();
      fresh.push_back(g);
      g->step = t.step;
      g->sampler = t.sampler;
      g->weight = t.weight;
      g->scale = t.scale;
      UimgKappa kap = {{0.0, 0.0, 0.0}};
      for (int a = 0; a < D; ++a) kap.k[a] = g->cweight[a] = t.cweight[a];
      for (int a = D; a < 3; ++a) g->cweight[a] = 0.0;
      g->n = s.n;
      if (s.n == 0) continue;
      planes.resize((size_t)s.n * D);   // the caller's rows [n][D] -> planes [D][n]
      for (int64_t p = 0; p < s.n; ++p)
        for (int a = 0; a < D; ++a) planes[(size_t)a * s.n + p] = t.target[(size_t)p * D + a];
      g->target.upload(planes.data(), planes.size(), h->st);
      if (t.pweight) g->pweight.upload(t.pweight, (size_t)s.n, h->st);
      d_obs.alloc_zero(1, h->st);
      if (D == 2)
        hipLaunchKernelGGL(k_uimg_prepare<2>, dim3(grid_of(s.n)), dim3(256), 0, h->st, s.n, s.cell.p, g->pweight.p, kap,
                           g->target.p, d_obs.p);
      else
        hipLaunchKernelGGL(k_uimg_prepare<3>, dim3(grid_of(s.n)), dim3(256), 0, h->st, s.n, s.cell.p, g->pweight.p, kap,
                           g->target.p, d_obs.p);
      GL_CHECK_LAUNCH();
      unsigned long long no = 0;
      GL_HIP(hipMemcpyAsync(&no, d_obs.p, sizeof(no), hipMemcpyDeviceToHost, h->st));
      GL_HIP(hipStreamSynchronize(h->st));   // (the caller's arrays and `planes` are free again)
      g->n_obs = (int64_t)no;
    }
  } catch (...) {
    (void)hipStreamSynchronize(h->st);
    for (auto* g : fresh) delete g;
    throw;
  }
  for (auto* g : h->uimg_terms) delete g;
  h->uimg_terms.swap(fresh);
}

void gl_displacement_image_term_info(glims_ctx* h, int k, int64_t out[3]) {
  const char* who = "glims_adjoint_displacement_image_info";
  GL_REQUIRE(out, std::string(who) + ": null output");
  GL_REQUIRE(k >= 0 && k < (int)h->uimg_terms.size(), std::string(who) + ": no stored term " + std::to_string(k));
  const GlDisplacementImageTerm& t = *h->uimg_terms[(size_t)k];
  out[0] = t.sampler;
  out[1] = t.n;
  out[2] = t.n_obs;
}

double gl_displacement_image_misfit_grad(glims_ctx* h, const GlDisplacementImageTerm& t, const double* u, double* murhs) {
  GlSampler& s = sampler_of(h, t.sampler, "glims_adjoint_gradient");
  if (s.n == 0) return 0.0;
  const int D = h->dim;
  image_staging(h, s, D);
  const unsigned nb = grid_of(s.n);
  const UimgKappa kap = {{t.cweight[0], t.cweight[1], t.cweight[2]}};
  // GLIMS_UIMG_TIMING: an event pair around the misfit kernel with its sum and one around the transpose, one line per term
  const bool timed = getenv("GLIMS_UIMG_TIMING") != nullptr;
  float ms_misfit = 0.f, ms_t = 0.f;
  if (timed) GL_HIP(hipEventRecord(h->ev_a, h->st));
  if (D == 2)
    hipLaunchKernelGGL(k_uimg_misfit<2>, dim3(nb), dim3(256), 0, h->st, s.n, t.weight, t.scale, kap, s.node.p, s.w.p, u,
                       t.target.p, t.pweight.p, s.out.p, s.part.p);
  else
    hipLaunchKernelGGL(k_uimg_misfit<3>, dim3(nb), dim3(256), 0, h->st, s.n, t.weight, t.scale, kap, s.node.p, s.w.p, u,
                       t.target.p, t.pweight.p, s.out.p, s.part.p);
  GL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_img_sum, dim3(1), dim3(1024), 0, h->st, (int64_t)nb, s.part.p, s.part.p + nb);
  GL_CHECK_LAUNCH();
  if (timed) {
    GL_HIP(hipEventRecord(h->ev_b, h->st));
    GL_HIP(hipEventSynchronize(h->ev_b));
    GL_HIP(hipEventElapsedTime(&ms_misfit, h->ev_a, h->ev_b));
    GL_HIP(hipEventRecord(h->ev_a, h->st));
  }
  transpose_on(h, s, s.out.p, D, murhs, D, 1, true);
  if (timed) {
    GL_HIP(hipEventRecord(h->ev_b, h->st));
    GL_HIP(hipEventSynchronize(h->ev_b));
    GL_HIP(hipEventElapsedTime(&ms_t, h->ev_a, h->ev_b));
    fprintf(stderr, "glims displacement image terms: step %lld  points %lld  misfit %.4f ms  transpose %.4f ms\n",
            (long long)t.step, (long long)s.n, ms_misfit, ms_t);
  }
  double sum = 0.0;
  GL_HIP(hipMemcpyAsync(&sum, s.part.p + nb, sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  return sum;
}

void gl_displacement_image_misfit_second(glims_ctx* h, const GlDisplacementImageTerm& t, const double* du, int P, int64_t ld,
                                         double* dmurhs) {
  GlSampler& s = sampler_of(h, t.sampler, "glims_adjoint_hessian");
  if (s.n == 0) return;
  const int D = h->dim;
  image_staging(h, s, D * P);
  const UimgKappa kap = {{t.cweight[0], t.cweight[1], t.cweight[2]}};
  if (D == 2)
    hipLaunchKernelGGL(k_uimg_misfit_dir<2>, dim3(grid_of(s.n)), dim3(256), 0, h->st, s.n, P, ld, t.weight, t.scale, kap,
                       s.node.p, s.w.p, du, t.target.p, t.pweight.p, s.out.p);
  else
    hipLaunchKernelGGL(k_uimg_misfit_dir<3>, dim3(grid_of(s.n)), dim3(256), 0, h->st, s.n, P, ld, t.weight, t.scale, kap,
                       s.node.p, s.w.p, du, t.target.p, t.pweight.p, s.out.p);
  GL_CHECK_LAUNCH();
  for (int j = 0; j < P; ++j)
    transpose_on(h, s, s.out.p + (size_t)j * s.n * D, D, dmurhs + (size_t)j * ld, D, 1, true);
}

// ---- stored image terms of the deformed configuration ------------------------------------------------------------------------
namespace {
void delete_deformed_term(GlDeformedImageTerm* t) {
  if (!t) return;
  delete t->scratch;
  delete t;
}
}  // namespace

void gl_deformed_image_terms_set(glims_ctx* h, int n, const glims_deformed_image_misfit* terms) {
  const char* who = "glims_adjoint_deformed_image_terms";
  GL_REQUIRE(n >= 0 && (n == 0 || terms), std::string(who) + ": bad term list");
  // every check before anything is allocated or the old list is touched
  if (n > 0) {
    GL_REQUIRE(h->world <= 1, std::string(who) + ": not available on a partitioned handle (world > 1)");
    GL_REQUIRE(h->is_setup && h->have_mech,
               std::string(who) + ": the terms move with the displacement: glims_setup(with_mechanics=1) first");
  }
  const int D = h->dim;
  size_t need = 0;
  std::vector<int64_t> np((size_t)std::max(1, n), 0);
  for (int k = 0; k < n; ++k) {
    const glims_deformed_image_misfit& t = terms[k];
    const std::string tk = std::string(who) + ": term " + std::to_string(k);
    GL_REQUIRE(t.kind == GLIMS_MISFIT_IMG_L2 || t.kind == GLIMS_MISFIT_IMG_THRESH, tk + ": unknown kind");
    GL_REQUIRE(t.kind != GLIMS_MISFIT_IMG_THRESH || (t.smooth > 0.0 && std::isfinite(t.smooth) && std::isfinite(t.level)),
               tk + ": a threshold term needs smooth > 0 and a finite level");
    GL_REQUIRE(std::isfinite(t.weight), tk + ": non-finite weight");
    GL_REQUIRE(std::isfinite(t.scale), tk + ": non-finite scale");
    GL_REQUIRE(t.target, tk + ": null target");
    GL_REQUIRE(t.step >= 0, tk + ": negative step");
    GL_REQUIRE(!t.xyz || t.n_points >= 0, tk + ": negative n_points");
    GridSpec gs;
    const int64_t np_k = check_points(h, t.n_points, t.xyz, t.origin, t.spacing, t.size, gs);
    np[(size_t)k] = np_k;
    if (t.pweight)
      for (int64_t p = 0; p < np_k; ++p)
        GL_REQUIRE(t.pweight[p] >= 0.0 && std::isfinite(t.pweight[p]),
                   tk + ": pweight[" + std::to_string(p) + "] is negative or not finite");
    // the copies (target, pweight), S and r, the scratch sampler with its transpose, the deformed coordinates; the location's
    // transient buffers are checked again by every evaluation
    need += (size_t)np_k * ((t.pweight ? 16 : 8) + 8 * (D + 1) + 4 + (D + 1) * 12 + 4) + (size_t)h->n_cells * 12 +
            (size_t)h->n_nodes * D * 8;
  }
  if (n > 0) need_memory(who, need + (1u << 20));
  std::vector<GlDeformedImageTerm*> fresh;
  try {
    for (int k = 0; k < n; ++k) {
      const glims_deformed_image_misfit& t = terms[k];
      const int64_t np_k = np[(size_t)k];
      auto* g = new GlDeformedImageTerm();
      fresh.push_back(g);
      g->step = t.step;
      g->kind = t.kind;
      g->level = t.level;
      g->smooth = t.smooth;
      g->weight = t.weight;
      g->scale = t.scale;
      g->n = np_k;
      g->is_grid = !t.xyz;
      if (t.xyz) {
        g->xyz.assign(t.xyz, t.xyz + (size_t)np_k * D);
      } else {
        for (int a = 0; a < D; ++a) {
          g->origin[a] = t.origin[a];
          g->spacing[a] = t.spacing[a];
          g->size[a] = t.size[a];
        }
      }
      if (np_k == 0) continue;
      // q_p = 0 is "not observed" whatever the location says: a NaN target, as the fixed terms keep it
      std::vector<double> tg(t.target, t.target + (size_t)np_k);
      if (t.pweight)
        for (int64_t p = 0; p < np_k; ++p)
          if (t.pweight[p] == 0.0) tg[(size_t)p] = std::numeric_limits<double>::quiet_NaN();
      g->target.upload(tg, h->st);
      if (t.pweight) g->pweight.upload(t.pweight, (size_t)np_k, h->st);
      GL_HIP(hipStreamSynchronize(h->st));   // (tg and the caller's arrays are free again)
    }
  } catch (...) {
    (void)hipStreamSynchronize(h->st);
    for (auto* g : fresh) delete_deformed_term(g);
    throw;
  }
  GL_HIP(hipStreamSynchronize(h->st));
  for (auto* g : h->dimg_terms) delete_deformed_term(g);
  h->dimg_terms.swap(fresh);
}

void gl_deformed_image_term_info(glims_ctx* h, int k, int64_t out[4], double* min_ratio) {
  const char* who = "glims_adjoint_deformed_image_info";
  GL_REQUIRE(out, std::string(who) + ": null output");
  GL_REQUIRE(k >= 0 && k < (int)h->dimg_terms.size(), std::string(who) + ": no stored term " + std::to_string(k));
  const GlDeformedImageTerm& t = *h->dimg_terms[(size_t)k];
  out[0] = t.n;
  out[1] = t.n_found;
  out[2] = t.n_obs;
  out[3] = t.n_folded;
  if (min_ratio) *min_ratio = t.min_ratio;
}

double gl_deformed_image_misfit_grad(glims_ctx* h, GlDeformedImageTerm& t, const double* c, const double* u, double* g,
                                     double* murhs) {
  const char* who = "glims_adjoint_gradient (deformed image terms)";
  const int D = h->dim;
  const int64_t nn = h->n_nodes;
  if (t.n == 0) {
    t.n_found = t.n_obs = t.n_folded = 0;
    t.min_ratio = 1.0;
    return 0.0;
  }
  const size_t ny = (size_t)std::max<int64_t>(1, nn * D), ns = (size_t)t.n * D;
  if (t.y.n != ny || t.S.n != ns) {
    need_memory(who, (ny + ns) * sizeof(double));
    t.y.alloc(ny);
    t.S.alloc(ns);
  }
  t.cnt.alloc_zero(1, h->st);
  // y = X + scale u_k, the location in it (cell, nodes, weights and the transpose's lists), the cells' determinant ratios
  if (nn > 0) {
    if (D == 2) hipLaunchKernelGGL(k_deform_xyz<2>, dim3(grid_of(nn)), dim3(256), 0, h->st, nn, h->xyz_new.p, u, t.scale, t.y.p);
    else hipLaunchKernelGGL(k_deform_xyz<3>, dim3(grid_of(nn)), dim3(256), 0, h->st, nn, h->xyz_new.p, u, t.scale, t.y.p);
    GL_CHECK_LAUNCH();
  }
  GridSpec gs;
  for (int a = 0; a < 3; ++a) {
    gs.o[a] = t.origin[a];
    gs.s[a] = t.spacing[a];
    gs.n[a] = t.size[a];
  }
  if (!t.scratch) t.scratch = new GlSampler();
  GlSampler& s = *t.scratch;
  s.n = t.n;
  s.is_grid = t.is_grid;
  s.deformed = true;
  s.have_t = false;
  s.n_chunks = 0;
  const double* xyz_host = t.is_grid ? nullptr : t.xyz.data();
  if (D == 2) {
    create_t<2>(h, s, xyz_host, gs, t.y.p);
    deformation_stats<2>(h, s, t.y.p);
  } else {
    create_t<3>(h, s, xyz_host, gs, t.y.p);
    deformation_stats<3>(h, s, t.y.p);
  }
  image_staging(h, s, 1);
  const size_t nq = (size_t)std::max<int64_t>(1, s.n_chunks) * h->nv * D;   // (both transposes below fit)
  if (s.q.n < nq) {
    need_memory(who, nq * sizeof(double));
    s.q.alloc(nq);
  }
  const unsigned nb = grid_of(s.n);
  if (h->nv == 3)
    hipLaunchKernelGGL(k_img_misfit_deformed<3>, dim3(nb), dim3(256), 0, h->st, s.n, t.kind, t.level, t.smooth, t.weight,
                       t.scale, s.cell.p, s.node.p, s.w.p, c, h->xyz_new.p, t.y.p, t.target.p, t.pweight.p, s.out.p, t.S.p,
                       s.part.p, t.cnt.p);
  else
    hipLaunchKernelGGL(k_img_misfit_deformed<4>, dim3(nb), dim3(256), 0, h->st, s.n, t.kind, t.level, t.smooth, t.weight,
                       t.scale, s.cell.p, s.node.p, s.w.p, c, h->xyz_new.p, t.y.p, t.target.p, t.pweight.p, s.out.p, t.S.p,
                       s.part.p, t.cnt.p);
  GL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_img_sum, dim3(1), dim3(1024), 0, h->st, (int64_t)nb, s.part.p, s.part.p + nb);
  GL_CHECK_LAUNCH();
  transpose_on(h, s, s.out.p, 1, g, 1, 0, true);       // dJ/dc_k += P^T r
  transpose_on(h, s, t.S.p, D, murhs, D, 1, true);     // dJ/du_k += P^T S
  double sum = 0.0;
  unsigned long long no = 0;
  GL_HIP(hipMemcpyAsync(&sum, s.part.p + nb, sizeof(double), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipMemcpyAsync(&no, t.cnt.p, sizeof(no), hipMemcpyDeviceToHost, h->st));
  GL_HIP(hipStreamSynchronize(h->st));
  t.n_found = s.n_found;
  t.n_obs = (int64_t)no;
  t.n_folded = s.n_inverted;
  t.min_ratio = s.min_ratio;
  return sum;
}

void gl_sampler_destroy(glims_ctx* h, int64_t id) {
  (void)sampler_of(h, id, "glims_sampler_destroy");
  for (size_t k = 0; k < h->img_terms.size(); ++k)
    GL_REQUIRE(h->img_terms[k]->sampler != id, "glims_sampler_destroy: sampler " + std::to_string(id) +
                                                   " is used by stored image term " + std::to_string(k) +
                                                   " (glims_adjoint_image_terms)");
  for (size_t k = 0; k < h->uimg_terms.size(); ++k)
    GL_REQUIRE(h->uimg_terms[k]->sampler != id, "glims_sampler_destroy: sampler " + std::to_string(id) +
                                                    " is used by stored displacement image term " + std::to_string(k) +
                                                    " (glims_adjoint_displacement_image_terms)");
  GL_HIP(hipStreamSynchronize(h->st));
  delete h->samplers[(size_t)id];
  h->samplers[(size_t)id] = nullptr;
}

void gl_sampler_destroy_all(glims_ctx* h) {
  for (auto* t : h->img_terms) delete t;
  h->img_terms.clear();
  for (auto* t : h->dimg_terms) delete_deformed_term(t);
  h->dimg_terms.clear();
  for (auto* t : h->uimg_terms) delete t;
  h->uimg_terms.clear();
  for (auto* s : h->samplers) delete s;
  h->samplers.clear();
}
