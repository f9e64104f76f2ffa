"""
The slot words of the assembly sweeps' (row, cell) incidence records, stated in numpy (kernels.hip, k_corner_weights).

A row's entries sit in slots 0 .. len-1 (its columns in ascending order, the row's own node among them).  An incidence record
of row i and cell T names the slots of T's vertices in row i:

  cs2  (32 bits)  byte 0 = the row's own slot, bytes 1 .. NV-1 = the other vertices of T in cell order;
  cs16 (16 bits)  the own slot dropped (the sweep has it from diag_k); bits [5 (m-1), 5 m) = byte m of cs2, m = 1 .. NV-1.

Padding records are 0 in both.  A slot of a row of at most 32 entries fits 5 bits; the straight-line sweeps (rows of at most
32 entries) read cs16, everything else cs2.
"""
import numpy as np


def row_slots(cells, n):
    """(ptr, cols): CSR of the node adjacency with the diagonal, columns ascending -- slot of column j in row i is its position."""
    nv = cells.shape[1]
    i = np.repeat(cells, nv, axis=1).ravel()
    j = np.tile(cells, (1, nv)).ravel()
    key = np.unique(i.astype(np.int64) * n + j)
    rows, cols = key // n, key % n
    ptr = np.searchsorted(rows, np.arange(n + 1))
    return ptr, cols


def incidence_words(cells, n):
    """(row, word32) for every (row, cell) incidence: the re-ordered 32-bit slot word."""
    ptr, cols = row_slots(cells, n)
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr)) * n + cols      # ascending
    nv = cells.shape[1]
    rows, words = [], []
    for a in range(nv):                       # the incidences of the cells' a-th vertex
        r = cells[:, a].astype(np.int64)
        slot = np.stack([np.searchsorted(keys, r * n + cells[:, m]) - ptr[r] for m in range(nv)], axis=1)
        others = np.delete(slot, a, axis=1)   # cell order, own vertex left out
        w = slot[:, a].copy()
        for m in range(nv - 1):
            w |= others[:, m] << (8 * (m + 1))
        rows.append(r)
        words.append(w)
    return np.concatenate(rows), np.concatenate(words).astype(np.uint32)


def pack16(word32, nv):
    """cs2 word -> (cs16 word, fits): fits is False where a slot needs more than 5 bits (the field is then saturated)."""
    w = np.asarray(word32, dtype=np.uint32)
    out = np.zeros(w.shape, dtype=np.uint32)
    ok = np.ones(w.shape, dtype=bool)
    for m in range(1, nv):
        k = (w >> np.uint32(8 * m)) & np.uint32(255)
        ok &= k < 32
        out |= np.minimum(k, 31).astype(np.uint32) << np.uint32(5 * (m - 1))
    return out.astype(np.uint16), ok


def unpack16(word16, nv):
    """cs16 word -> the slots of the cell's other vertices, [.., NV-1]."""
    w = np.asarray(word16, dtype=np.uint32)
    return np.stack([(w >> np.uint32(5 * (m - 1))) & np.uint32(31) for m in range(1, nv)], axis=-1)
