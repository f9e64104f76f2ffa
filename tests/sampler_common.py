"""Numpy statement of the sampler contract (include/glims_hip.h, "samplers") -- the reference of the
sampler tests, independent of the code under test.

P: barycentric coordinates lambda_a(x) of a point in a cell from the cell's vertex coordinates (fp64 solve of the d x d edge
system, lambda_0 = 1 - sum); a cell ACCEPTS x iff min_a lambda_a >= -EPS; among the accepting cells the smallest cell index
wins; no accepting cell: cell -1, weights 0, value = fill.  P^T is the scatter-add of w[p][a] r[p] into the winner's nodes.

`locate` also returns, per point, the decision margin min_T |min_a lambda_a(T) + EPS| over the candidate cells: a comparison
of cell indices with another implementation means something only where no accept / reject decision sits on the rounding
edge, so tests assert margin >= EPS / 2 for all their points BEFORE they compare (`assert_decisive`)."""
import numpy as np

EPS = 1e-10            # GLIMS_SAMPLE_EPS
KAPPA_MAX = 1e4        # meshes the helper admits: rounding of lambda ~ kappa 2^-52 <= 2.2e-12, twenty times below EPS / 2


def edge_matrices(points, cells):
    X = np.asarray(points, dtype=np.float64)[np.asarray(cells)]
    return np.swapaxes(X[:, 1:] - X[:, :1], 1, 2)          # [M, d, d], column a = x_{a+1} - x_0


def kappa(points, cells):
    """2-norm condition number of every cell's edge matrix."""
    return np.linalg.cond(edge_matrices(points, cells))


def assert_mesh_ok(points, cells):
    k = kappa(points, cells)
    assert np.isfinite(k).all() and k.max() < KAPPA_MAX, "cell edge matrices up to kappa = %.3g" % k.max()
    return k


def barycentric(points, cells, cell_ids, x):
    """lambda [n, d+1] of the points x [n, d] in the cells cell_ids [n] (vertex order of the `cells` rows)."""
    E = edge_matrices(points, np.asarray(cells)[cell_ids])
    x0 = np.asarray(points, dtype=np.float64)[np.asarray(cells)[cell_ids, 0]]
    lam = np.linalg.solve(E, (x - x0)[..., None])[..., 0]
    return np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)


def grid_points(origin, spacing, size):
    """Points of a grid, x fastest: p = (k * size[1] + j) * size[0] + i  ->  origin + (i, j, k) * spacing."""
    d = len(size)
    ax = [np.asarray(origin, dtype=np.float64)[a] + np.arange(size[a], dtype=np.float64) * np.asarray(spacing, dtype=np.float64)[a]
          for a in range(d)]
    mesh = np.meshgrid(*ax[::-1], indexing='ij')           # slowest axis first
    return np.stack([m.reshape(-1) for m in mesh[::-1]], axis=1)


def locate(points, cells, x, chunk=256):
    """Returns (cell [n] int32, weights [n, d+1], margin [n], n_accept [n]).  margin is +inf for a point without a candidate."""
    P = np.asarray(points, dtype=np.float64)
    C = np.asarray(cells)
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    X = P[C]
    lo, hi = X.min(axis=1), X.max(axis=1)
    pad = 1e-6 * (hi - lo).sum(axis=1, keepdims=True) + 1e-9 * np.abs(P).max()    # bounding-box prefilter, generous
    lo, hi = lo - pad, hi + pad
    cell = np.full(n, -1, dtype=np.int32)
    w = np.zeros((n, d + 1))
    margin = np.full(n, np.inf)
    n_acc = np.zeros(n, dtype=np.int64)
    if n == 0 or len(C) == 0:
        return cell, w, margin, n_acc
    # points in a spatially coherent order, so that a chunk's bounding box selects few cells
    span = np.maximum(P.max(axis=0) - P.min(axis=0), 1e-300)
    key = np.clip(((x - P.min(axis=0)) / span * 16).astype(np.int64), 0, 15)
    order = np.lexsort(tuple(key[:, a] for a in range(d)))
    for s in range(0, n, chunk):
        ids = order[s:s + chunk]
        xs = x[ids]
        sel = np.flatnonzero(((hi >= xs.min(axis=0)) & (lo <= xs.max(axis=0))).all(axis=1))
        if len(sel) == 0:
            continue
        inside = ((xs[:, None, :] >= lo[None, sel, :]) & (xs[:, None, :] <= hi[None, sel, :])).all(axis=2)
        pi, ci = np.nonzero(inside)                        # candidate (point, cell) pairs; ci ascending per point
        if len(pi) == 0:
            continue
        lam = barycentric(P, C, sel[ci], xs[pi])
        lmin = lam.min(axis=1)
        np.minimum.at(margin, ids[pi], np.abs(lmin + EPS))
        acc = lmin >= -EPS
        np.add.at(n_acc, ids[pi], acc.astype(np.int64))
        win = np.full(len(ids), np.iinfo(np.int64).max)
        np.minimum.at(win, pi[acc], sel[ci[acc]])
        found = win < np.iinfo(np.int64).max
        cell[ids[found]] = win[found]
    f = cell >= 0
    if f.any():
        w[f] = barycentric(P, C, cell[f], x[f])
    return cell, w, margin, n_acc


def assert_decisive(margin):
    """No accept / reject decision of these points sits on the rounding edge."""
    m = margin.min() if len(margin) else np.inf
    assert m >= EPS / 2, "smallest decision margin %.3e < EPS / 2" % m
    return m


def apply(cells, cell, w, f, fill=np.nan):
    """P f: f [n_nodes] or [n_nodes, k]."""
    f = np.asarray(f, dtype=np.float64)
    f2 = f.reshape(len(f), -1)
    out = np.full((len(cell), f2.shape[1]), fill, dtype=np.float64)
    ok = cell >= 0
    nodes = np.asarray(cells)[cell[ok]]
    out[ok] = (w[ok][:, :, None] * f2[nodes]).sum(axis=1)
    return out[:, 0] if f.ndim == 1 else out


def apply_t(cells, cell, w, r, n_nodes):
    """P^T r by scatter-add: r [n] or [n, k]."""
    r = np.asarray(r, dtype=np.float64)
    r2 = r.reshape(len(r), -1)
    g = np.zeros((n_nodes, r2.shape[1]))
    ok = cell >= 0
    nodes = np.asarray(cells)[cell[ok]]
    for a in range(nodes.shape[1]):
        np.add.at(g, nodes[:, a], w[ok][:, a:a + 1] * r2[ok])
    return g[:, 0] if r.ndim == 1 else g


# ---- the meshes and grids of the tests ----------------------------------------------------------------------------------------
def jittered_delaunay_2d(nx, ny, lo=(0.0, 0.0), hi=(2.0, 1.0), jitter=0.25, seed=0):
    """Delaunay triangulation of a jittered lattice on a rectangle (boundary nodes move along the boundary only): unstructured,
    and without the slivers of a random-point mesh."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    idx = np.stack(np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing='ij'), axis=-1).reshape(-1, 2)
    m = np.array([nx, ny])
    free = (idx > 0) & (idx < m[None, :])
    h = (np.asarray(hi) - np.asarray(lo)) / m
    pts = (idx + (rng.random(idx.shape) - 0.5) * 2.0 * jitter * free) * h + np.asarray(lo)
    cells = Delaunay(pts).simplices.astype(np.int32)
    X = pts[cells]
    area = 0.5 * np.abs(np.linalg.det(X[:, 1:] - X[:, :1]))
    return np.ascontiguousarray(pts), np.ascontiguousarray(cells[area > 1e-9 * h.prod()])


def overhanging_grid(points, size, overhang=0.05, shift=0.3819660112501051):
    """(origin, spacing) of a grid of `size` points per axis that overhangs the mesh's bounding box by `overhang` of its extent
    on every side and is shifted by an irrational-looking fraction of a voxel."""
    lo, hi = points.min(axis=0), points.max(axis=0)
    ext = hi - lo
    size = np.asarray(size)
    spacing = ext * (1.0 + 2.0 * overhang) / (size - 1)
    origin = lo - overhang * ext + shift * spacing * 0.1
    return origin, spacing


def half_spacing_grid(lo, hi, n):
    """The nodes and edge midpoints of a box mesh with n[a] cells per axis as a grid: (origin, spacing, size)."""
    lo, hi, n = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), np.asarray(n)
    return lo, (hi - lo) / n / 2.0, 2 * n + 1
