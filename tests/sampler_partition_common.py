"""Numpy statement of the RESOLVED sampler of a partitioned run (include/glims_hip.h, glims_sampler_resolve; DESIGN.md section
14, "Partitioned handles") -- the reference of the partitioned sampler / image-term tests, independent of the code under test.

Every rank locates the same points in the cells of its own part (sampler_common.locate on partition_mesh's sub-mesh).  Then
  - the global winner of a point is the smallest GLOBAL cell id over the ranks' local winners;
  - a rank KEEPS a point iff its local winner is the global winner;
  - a point is COUNTED on the smallest rank that keeps it;
  - P^T r runs on every rank over its kept points, and only the rows of the nodes a rank OWNS are taken from it;
  - J adds, on every rank, the squares of the points the rank counts.
"""
import numpy as np

import sampler_common as sc
from glimslib_amd.partition import partition_mesh

BIG = np.iinfo(np.int64).max


def locate_on_parts(points, cells, world, x):
    """(parts, loc): partition_mesh's part of every rank and sampler_common.locate of x in it (cell = LOCAL cell index)."""
    parts = [partition_mesh(points, cells, world, r) for r in range(world)]
    loc = []
    for p in parts:
        cell, w, margin, _ = sc.locate(p.points, p.cells, x)
        sc.assert_decisive(margin)
        loc.append((cell, w))
    return parts, loc


def resolve(parts, loc):
    """(win [n] global cell id or -1, keep [world, n], counted [world, n]) by the rule above."""
    keys = np.stack([np.where(cell >= 0, np.asarray(p.cell_ids, dtype=np.int64)[np.maximum(cell, 0)], BIG)
                     for p, (cell, _) in zip(parts, loc)])
    best = keys.min(axis=0)
    keep = (keys == best[None]) & (best < BIG)[None]
    first = keep.argmax(axis=0)
    counted = keep & (np.arange(len(parts))[:, None] == first[None])
    return np.where(best < BIG, best, -1), keep, counted


def kept(loc_r, keep_r):
    """A rank's (cell, w) with the dropped points cleared, as the resolved device sampler holds them."""
    cell, w = loc_r
    return np.where(keep_r, cell, -1).astype(np.int32), np.where(keep_r[:, None], w, 0.0)


def apply_t_by_owned_rows(parts, loc, keep, r, n_nodes):
    """P^T r assembled from every rank's owned rows (global node order)."""
    r = np.asarray(r, dtype=np.float64)
    out = np.zeros((n_nodes,) + r.shape[1:])
    seen = np.zeros(n_nodes, dtype=np.int64)
    for p, lr, kr in zip(parts, loc, keep):
        cell, w = kept(lr, kr)
        g = sc.apply_t(p.cells, cell, w, r, len(p.points))
        own = np.asarray(p.global_ids)[:p.n_own]
        out[own] = g[:p.n_own]
        seen[own] += 1
    assert (seen == 1).all()                      # every node is owned by exactly one rank
    return out


def counted_sums(parts, loc, counted, f, t, q=None):
    """Per rank: sum over the points it counts of q (P f - t)^2, f a nodal field in the global order (NaN t = not observed)."""
    sums = []
    for p, (cell, w), cr in zip(parts, loc, counted):
        v = sc.apply(p.cells, cell, w, np.asarray(f)[p.global_ids], fill=0.0)
        ok = cr & ~np.isnan(t)
        qq = np.ones(len(t)) if q is None else q
        sums.append(float(np.sum(qq[ok] * (v[ok] - t[ok]) ** 2)))
    return sums


def vertex_and_overhanging_points(points, size):
    """The mesh's own vertices (every one a tie of all the cells around it) followed by an overhanging, non-aligned grid."""
    origin, spacing = sc.overhanging_grid(points, size)
    return np.concatenate([np.asarray(points, dtype=np.float64), sc.grid_points(origin, spacing, size)])
