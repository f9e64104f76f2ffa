"""
The compact (row, cell) incidence records of the straight-line assembly sweeps, stated in numpy (glimslib_amd/csrc/record_words.h,
k_corner_weights in kernels.hip).

One 32-bit word per record instead of the fp64 reaction weight (8 B) and the 16-bit slot word (2 B):

  bits [14:0]   the slot fields of cs16 (tests/slot_words16_common.py): own slot dropped, 5 bits per other vertex of the cell;
  bits [31:15]  a 17-bit two's-complement offset delta, weight = as_double(as_int64(base) + delta); base = the bit pattern of
                the slice's first real record's weight (lowest record index in its row, then lowest lane); the code -2^16 is
                reserved and decodes to +0.0 (padding records).

A slice (64 consecutive rows) is COMPACT when it belongs to a straight-line class (rows of at most 32 entries) and every real
record's offset lies in [-(2^16 - 1), 2^16 - 1]; every other slice is FULL and keeps today's streams.
"""
import numpy as np

from slot_words16_common import incidence_words, pack16, row_slots

WAVE = 64
SLOT_BITS = 15
SLOT_MASK = np.uint32((1 << SLOT_BITS) - 1)
DELTA_MAX = (1 << 16) - 1
DELTA_ZERO = -(1 << 16)
WORD_ZERO = np.uint32((DELTA_ZERO << SLOT_BITS) & 0xFFFFFFFF)      # a padding record: weight +0.0, slots 0


def cell_volumes(points, cells):
    """|T| in the expression order of k_egeo, every product and sum rounded on its own (no fused multiply-add)."""
    X = np.asarray(points, dtype=np.float64)[np.asarray(cells)]
    if X.shape[2] == 2:
        a, b = X[:, 1, 0] - X[:, 0, 0], X[:, 1, 1] - X[:, 0, 1]
        c, d = X[:, 2, 0] - X[:, 0, 0], X[:, 2, 1] - X[:, 0, 1]
        return np.abs(a * d - b * c) * 0.5
    r = X[:, 1:, :] - X[:, :1, :]
    c12 = [r[:, 1, 1] * r[:, 2, 2] - r[:, 1, 2] * r[:, 2, 1], r[:, 1, 2] * r[:, 2, 0] - r[:, 1, 0] * r[:, 2, 2],
           r[:, 1, 0] * r[:, 2, 1] - r[:, 1, 1] * r[:, 2, 0]]
    det = r[:, 0, 0] * c12[0] + r[:, 0, 1] * c12[1] + r[:, 0, 2] * c12[2]
    return np.abs(det) * (1.0 / 6.0)


def record_weights(points, cells, rho_cell):
    """rho_T |T| d!/(d+3)! per cell, as k_corner_weights forms it: (rho * |T|) * fact."""
    fact = 1.0 / 60.0 if np.asarray(cells).shape[1] == 3 else 1.0 / 120.0
    return np.asarray(rho_cell, dtype=np.float64) * cell_volumes(points, cells) * fact


def bits(w):
    return np.asarray(w, dtype=np.float64).view(np.int64)


def pack(slots15, weight, base):
    """(word, fits) of REAL records: slot fields + the weight's offset from the int64 `base`."""
    with np.errstate(over='ignore'):
        delta = (bits(weight).view(np.uint64) - np.uint64(np.int64(base).view(np.uint64))).view(np.int64)
    fits = (delta >= -DELTA_MAX) & (delta <= DELTA_MAX)
    d = np.where(fits, delta, 0)
    word = (np.asarray(slots15, dtype=np.uint32) & SLOT_MASK) | ((d & 0x1FFFF).astype(np.uint32) << np.uint32(SLOT_BITS))
    return word, fits


def unpack(word, base):
    """(slot fields as one 15-bit number, weight): the sweep's decode."""
    w = np.asarray(word, dtype=np.uint32)
    delta = w.view(np.int32) >> SLOT_BITS                               # arithmetic shift
    with np.errstate(over='ignore'):
        pattern = (np.uint64(np.int64(base).view(np.uint64)) + delta.astype(np.int64).view(np.uint64)).view(np.int64)
    weight = np.where(delta == DELTA_ZERO, 0.0, pattern.view(np.float64))
    return w & SLOT_MASK, weight


def slice_rule(rows, weight, short_row, fits16, n):
    """
    The set-up rule per slice of 64 consecutive rows.  rows / weight / fits16: per real record, the records of a row in the
    order given; short_row: per row, at most 32 entries.  Returns (slice of every record, base per slice, compact per slice).
    """
    rows = np.asarray(rows)
    order = np.argsort(rows, kind='stable')
    q = np.empty(len(rows), dtype=np.int64)                               # index of the record in its row
    start = np.searchsorted(rows[order], np.arange(n))
    q[order] = np.arange(len(rows)) - start[rows[order]]
    sl, lane = rows // WAVE, rows % WAVE
    n_slices = (n + WAVE - 1) // WAVE
    key = q * WAVE + lane                                                 # lowest record index, then lowest lane
    first = np.full(n_slices, -1, dtype=np.int64)
    o = np.lexsort((key, sl))
    s_sorted = sl[o]
    head = np.r_[True, s_sorted[1:] != s_sorted[:-1]]
    first[s_sorted[head]] = o[head]
    base = np.where(first >= 0, bits(weight)[np.maximum(first, 0)], 0)
    _, fits = pack(np.zeros(len(rows), dtype=np.uint32), weight, base[sl])
    bad = np.zeros(n_slices, dtype=bool)
    np.logical_or.at(bad, sl, ~(fits & np.asarray(fits16)))
    straight = np.ones(n_slices, dtype=bool)
    np.logical_and.at(straight, np.arange(n) // WAVE, np.asarray(short_row))
    return sl, base, straight & ~bad


def mesh_records(points, cells, rho_cell):
    """Everything the rule reads from a mesh: (rows, 16-bit slot words, fits16, weights, short_row)."""
    cells = np.asarray(cells)
    n, nv = len(points), cells.shape[1]
    ptr, _ = row_slots(cells, n)
    rows, w32 = incidence_words(cells, n)
    w16, fits16 = pack16(w32, nv)
    weight = np.tile(record_weights(points, cells, rho_cell), nv)       # incidence_words: vertex a of every cell, a = 0 .. NV-1
    return rows, w16, fits16, weight, np.diff(ptr) <= 32
