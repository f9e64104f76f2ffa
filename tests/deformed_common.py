"""Numpy statement of the deformed-sampler and warp contract (include/glims_hip.h, "deformed-configuration samplers and image
warping") -- the reference of tests/test_deformed_cpu.py and tests/test_gpu_deformed_sampler.py,
independent of the code under test.

A deformed sampler locates its points in the mesh whose nodes sit at  points + scale * u  with the rules of
tests/sampler_common.py (`locate`); the back map is P applied to the reference coordinates; `resample` evaluates a voxel image
at arbitrary positions by the header's order-1 / order-0 rules and returns, next to the values, the decision margin of every
position: how far its inside / outside decision (order 1: t from 0 and n - 1; order 0: t + 0.5 from the nearest integer, which
covers both the inside test and the choice of the voxel) is from flipping.  Tests assert margin >= 1e-9 BEFORE they compare."""
import numpy as np

import sampler_common as sc

RESAMPLE_MARGIN = 1e-9     # positions come from a d x d fp64 solve and a d+1 term sum: rounding ~ 1e-13 of a voxel at most


def smooth_displacement(points, amp):
    """u_a = amp ext_a sin(pi t_{a+1}) cos(pi/2 t_a) + 0.03 ext_a, t the position in the bounding box scaled to [0, 1]^d,
    a + 1 cyclic over the axes, ext_a the box extent along axis a."""
    P = np.asarray(points, dtype=np.float64)
    lo, hi = P.min(axis=0), P.max(axis=0)
    ext = hi - lo
    t = (P - lo) / ext
    d = P.shape[1]
    u = np.empty_like(P)
    for a in range(d):
        u[:, a] = amp * ext[a] * np.sin(np.pi * t[:, (a + 1) % d]) * np.cos(0.5 * np.pi * t[:, a]) + 0.03 * ext[a]
    return u


def deformed_points(points, u, scale=1.0):
    return np.asarray(points, dtype=np.float64) + scale * np.asarray(u, dtype=np.float64).reshape(np.shape(points))


def locate(points, cells, u, scale, x):
    """sampler_common.locate in the displaced mesh: (cell, weights, margin, n_accept)."""
    return sc.locate(deformed_points(points, u, scale), cells, x)


def cell_ratios(points, cells, u, scale=1.0):
    """det(E_deformed) / det(E_reference) per cell = det(I + scale grad u_h)."""
    return (np.linalg.det(sc.edge_matrices(deformed_points(points, u, scale), cells)) /
            np.linalg.det(sc.edge_matrices(points, cells)))


def n_inverted(ratios):
    return int((~(ratios > 0) | ~np.isfinite(ratios)).sum())


def back_map(points, cells, cell, w, fill=np.nan):
    """X(x_p): P applied to the reference coordinates."""
    return sc.apply(cells, cell, w, np.asarray(points, dtype=np.float64), fill=fill)


def resample(image, origin, spacing, X, order, fill=np.nan):
    """image: array [z,] y, x [, k] with voxel centres origin + index * spacing; X [n, d] positions (NaN rows: outside).
    Returns (values [n] or [n, k], margin [n]); margin is +inf for a NaN position."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    a = np.asarray(image, dtype=np.float64)
    flat = a.ndim == d
    a = a.reshape(a.shape[:d] + (-1,))
    size = np.array(a.shape[:d][::-1])                          # points per axis, x first
    k = a.shape[-1]
    ok = np.isfinite(X).all(axis=1)
    t = (X - np.asarray(origin, dtype=np.float64)) / np.asarray(spacing, dtype=np.float64)
    t = np.where(ok[:, None], t, 0.0)
    out = np.full((n, k), fill, dtype=np.float64)
    margin = np.full(n, np.inf)
    if order == 1:
        inside = ok & ((t >= 0) & (t <= size - 1)).all(axis=1)
        m = np.minimum(np.abs(t), np.abs(t - (size - 1))).min(axis=1)
        i0 = np.where(size > 1, np.minimum(np.floor(t), size - 2), 0).astype(np.int64)
        f = np.where(size > 1, t - i0, 0.0)
        acc = np.zeros((n, k))
        for corner in range(1 << d):
            bits = [(corner >> b) & 1 for b in range(d)]
            wgt = np.ones(n)
            for b in reversed(range(d)):                        # z outermost, x innermost
                wgt = wgt * (f[:, b] if bits[b] else 1.0 - f[:, b])
            idx = [np.clip(i0[:, b] + bits[b] * (size[b] > 1), 0, size[b] - 1) for b in range(d)]
            acc += wgt[:, None] * a[tuple(idx[::-1])]           # plain arithmetic: 0 * NaN = NaN propagates
        out[inside] = acc[inside]
    elif order == 0:
        inside = ok & ((t >= -0.5) & (t < size - 0.5)).all(axis=1)
        s = t + 0.5
        m = np.abs(s - np.rint(s)).min(axis=1)
        idx = [np.clip(np.floor(s[:, b]).astype(np.int64), 0, size[b] - 1) for b in range(d)]
        out[inside] = a[tuple(idx[::-1])][inside]
    else:
        raise ValueError("order must be 0 or 1")
    margin[ok] = m[ok]
    return (out[:, 0] if flat else out), margin


def assert_resample_decisive(margin):
    m = margin.min() if len(margin) else np.inf
    assert m >= RESAMPLE_MARGIN, "smallest resample margin %.3e < %.1e" % (m, RESAMPLE_MARGIN)
    return m
