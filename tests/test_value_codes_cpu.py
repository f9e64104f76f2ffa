"""
The coded entries of S that the dot-free Krylov pass streams for exactly-linear slices (DevPattern::scode,
glimslib_amd/csrc/value_codes.h), checked in numpy on the oracle's S: the rule of tests/value_codes_common.py codes nearly every
slice of the flagship lattice with a handful of bases and returns the exact 64 bits of every entry it codes; meshes whose cells
all differ have no coded slice (their passes then read today's streams); the limits of the offset and of the dictionary sit
where the header says.  tests/value_codes_check.cpp asserts the same rules on the header itself, compiled with the host compiler
alone.

The oracle assembles S in another summation order than the library, and its rows are taken in Morton order, not in the library's
numbering: the shares here say what the RULE gives on such an operator; the device reports its own (glims_stats.rd_scode_slices).

Reference counterpart: none (a storage format of this implementation; the reference assembles through UFL forms).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from glimslib_amd import partition, workloads

from oracle import glims_oracle as go

import value_codes_common as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _static_operator(w):
    o = go.OracleTumorGrowth(w.mesh.points, np.asarray(w.mesh.cells), w.per_cell('D'), w.per_cell('rho'), w.per_cell('gamma'),
                             w.per_cell('E'), w.per_cell('nu'), w.dt)
    order = np.argsort(partition.morton_keys(w.mesh.points), kind='stable')
    return o.S, order


def _check_round_trip(S, order, ids, nb):
    """Every coded slice of `ids`: each entry has exactly one word, and the word decodes to the entry's very bits."""
    for s, n in zip(ids, nb):
        if n > vc.BASES:
            continue
        p, cols = vc.slice_entries(S, order, s)
        base = vc.dictionary(p)
        word, fits = vc.pack(cols & 0xFFFF, p, base)
        assert fits.all()
        c, back = vc.unpack(word, base)
        assert np.array_equal(vc.bits(back), p)
        assert np.array_equal(c, (cols & 0xFFFF).astype(np.uint32))


def test_the_flagship_lattice_is_coded():
    """C4's box at n = 47 (its two tissues, its dt), every fourth slice: at least 0.95 of them need at most 32 bases."""
    S, order = _static_operator(workloads.config_c4(47))
    ids, nb = vc.survey(S, order, step=4)
    share = float((nb <= vc.BASES).mean())
    print("C4 box n = 47: %d slices sampled, %.3f coded, median %d bases, most %d" % (len(ids), share, np.median(nb), nb.max()))
    assert share >= 0.95
    _check_round_trip(S, order, ids, nb)


# Every cell of these meshes has its own shape, so the 64 diagonal entries of a slice alone are 64 numbers that differ in their
# leading digits: far more than 32 clusters of 2047 consecutive bit patterns.
@pytest.mark.parametrize("name,points,jitter", [("jittered lattice", 2000, 0.3), ("random 1000", 1000, None)])
def test_meshes_of_unlike_cells_are_not_coded(name, points, jitter):
    S, order = _static_operator(workloads.config_unstructured(points, jitter=jitter, seed=0))
    ids, nb = vc.survey(S, order)
    full = ids[(ids + 1) * vc.WAVE <= S.shape[0]]            # (the last slice may hold a few rows only)
    coded_full = int((nb[:len(full)] <= vc.BASES).sum())
    print("%s: %d slices, %d coded (%d of the %d whole ones), fewest bases %d" %
          (name, len(ids), int((nb <= vc.BASES).sum()), coded_full, len(full), nb.min()))
    assert coded_full == 0
    _check_round_trip(S, order, ids, nb)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("width,bases", [(2046, 1), (2047, 2), (2048, 2)])
def test_limit_of_the_offset(width, bases, sign):
    """Two entries `width` ulps apart: one base covers 2047 consecutive patterns."""
    lo = int(vc.bits(np.array([sign * 0.0468]))[0])
    p = np.array([lo + width, lo], dtype=np.int64)
    base = vc.dictionary(p)
    assert len(base) == bases and base[0] == lo + vc.DELTA_MAX
    word, fits = vc.pack(np.array([0x5A5A, 0xFFFF]), p, base)
    assert fits.all()
    cols, back = vc.unpack(word, base)
    assert np.array_equal(vc.bits(back), p) and list(cols) == [0x5A5A, 0xFFFF]
    # against the first base alone the far entry fits only at the limit
    _, fits1 = vc.pack(np.zeros(2, dtype=np.uint32), p, base[:1])
    assert bool(fits1.all()) == (bases == 1)


@pytest.mark.parametrize("n,coded", [(32, True), (33, False)])
def test_limit_of_the_dictionary(n, coded):
    lo = int(vc.bits(np.array([0.731]))[0])
    p = (lo + 100000 * np.arange(n, dtype=np.int64)[:, None] + np.array([0, 900, 2046], dtype=np.int64)[None, :]).ravel()
    base = vc.dictionary(p)
    assert len(base) == n and (len(base) <= vc.BASES) == coded
    word, fits = vc.pack(np.zeros(len(p), dtype=np.uint32), p, base)
    assert bool(fits.all()) == coded
    if coded:
        assert np.array_equal(vc.bits(vc.unpack(word, base)[1]), p)
        assert (word >> np.uint32(vc.INDEX_SHIFT)).max() == 31


def test_both_signs_and_zero_in_one_slice():
    p = np.concatenate([vc.bits(np.array([-0.0468, 0.731, 0.0])), vc.bits(np.array([-0.0468]))[:1] + 5])
    base = vc.dictionary(p)
    assert len(base) == 3 and base[0] < 0 and base[1] == vc.DELTA_MAX
    word, fits = vc.pack(np.arange(4), p, base)
    assert fits.all() and np.array_equal(vc.bits(vc.unpack(word, base)[1]), p)


def test_header_rules_hold_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "value_codes_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "value_codes_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
