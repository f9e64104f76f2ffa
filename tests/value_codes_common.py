"""
The coded entries of the static RD operator S that the dot-free Krylov pass streams for exactly-linear slices, stated in numpy
(glimslib_amd/csrc/value_codes.h, k_build_value_codes in kernels.hip).

One 32-bit word per stored entry instead of the fp64 value (8 B) and the 16-bit column code (2 B):

  bits [15:0]   the column code as cols16 holds it;
  bits [26:16]  an 11-bit two's-complement offset delta, |delta| <= 1023;
  bits [31:27]  the index of one of the slice's 32 dictionary bases;      value = as_double(base[index] + delta).

The dictionary of a slice (64 consecutive rows) by greedy clustering of the bit patterns of its real entries, as signed 64-bit
integers: the smallest pattern v that no base covers yet gives base = v + 1023, which covers [v, v + 2046]; repeat.  A slice that
needs more than 32 bases is UNCODED and keeps the 10-byte stream.
"""
import numpy as np

WAVE = 64
BASES = 32
DELTA_MAX = 1023
SPAN = 2 * DELTA_MAX
DELTA_SHIFT, INDEX_SHIFT = 16, 27


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def dictionary(patterns):
    """The greedy rule on the int64 patterns of one slice: every base it needs, in increasing order (any number of them)."""
    v = np.sort(np.asarray(patterns, dtype=np.int64))
    base = []
    i = 0
    while i < len(v):
        base.append(int(v[i]) + DELTA_MAX)
        i = int(np.searchsorted(v, int(v[i]) + SPAN, side='right'))
    return np.array(base, dtype=np.int64)


def pack(col16, patterns, base):
    """(word, fits) of real entries against a slice's bases (at most 32 of them)."""
    p = np.asarray(patterns, dtype=np.int64)
    base = np.asarray(base, dtype=np.int64)
    idx = np.clip(np.searchsorted(base, p - DELTA_MAX, side='left'), 0, max(len(base) - 1, 0))   # the first base >= p - 1023
    delta = p - base[idx] if len(base) else np.full(len(p), SPAN, dtype=np.int64)
    fits = (np.abs(delta) <= DELTA_MAX) & (idx < BASES)
    d = np.where(fits, delta, 0)
    word = ((np.asarray(col16, dtype=np.uint32) & np.uint32(0xFFFF)) | ((d & 0x7FF).astype(np.uint32) << np.uint32(DELTA_SHIFT)) |
            (np.where(fits, idx, 0).astype(np.uint32) << np.uint32(INDEX_SHIFT)))
    return word, fits


def unpack(word, base):
    """(column code, value): the pass's decode."""
    w = np.asarray(word, dtype=np.uint32)
    idx = (w >> np.uint32(INDEX_SHIFT)).astype(np.int64)
    delta = ((w << np.uint32(32 - INDEX_SHIFT)).view(np.int32) >> (32 - 11)).astype(np.int64)    # arithmetic shift
    return w & np.uint32(0xFFFF), (np.asarray(base, dtype=np.int64)[idx] + delta).view(np.float64)


def slice_entries(S, order, s):
    """Bit patterns and columns of the stored entries of slice s of the CSR matrix S with its rows taken in `order`."""
    rows = order[s * WAVE:(s + 1) * WAVE]
    ptr = S.indptr
    idx = np.concatenate([np.arange(ptr[r], ptr[r + 1]) for r in rows])
    return bits(S.data[idx]), S.indices[idx]


def survey(S, order, step=1):
    """Bases needed by every step-th slice: (slice ids, number of bases each)."""
    n_slices = (S.shape[0] + WAVE - 1) // WAVE
    ids = np.arange(0, n_slices, step)
    return ids, np.array([len(dictionary(slice_entries(S, order, s)[0])) for s in ids])
