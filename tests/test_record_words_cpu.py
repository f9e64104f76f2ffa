"""
The compact incidence records of the straight-line assembly sweeps (DevPattern::cr32, glimslib_amd/csrc/record_words.h), checked
in numpy: the rule of tests/record_words_common.py returns the slot fields of cs16 and the exact 64 bits of every weight of every
slice it calls compact; the reserved code is +0.0; the limit of the 17-bit offset sits where the header says; a lattice with one
rho is all compact and meshes with cells of different volumes have no compact slice (what their sweeps then read is today's
streams).  tests/record_words_check.cpp asserts the same rule on the header itself, compiled with the host compiler alone.

Reference counterpart: none (a storage format of this implementation; the reference assembles through UFL forms).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from glimslib_amd import workloads
from glimslib_amd.mesh import RectangleMesh

import record_words_common as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c3():
    w = workloads.config_c3(8)
    return w.mesh, w.per_cell('rho')


def _rectangle():
    mesh = RectangleMesh((-5.0, -5.0), (5.0, 5.0), 12, 12)
    return mesh, np.full(len(mesh.cells), 0.1)


def _unstructured(points, jitter):
    w = workloads.config_unstructured(points, jitter=jitter, seed=0)
    return w.mesh, w.per_cell('rho')


# name -> (mesh and rho per cell, expected: 'all' compact / 'none')
MESHES = {
    "c3(8)": (_c3, 'all'),
    "rectangle 12x12": (_rectangle, 'all'),
    "jittered lattice": (lambda: _unstructured(2000, 0.3), 'none'),
    "random 1000": (lambda: _unstructured(1000, None), 'none'),
}


@pytest.mark.parametrize("name", list(MESHES))
def test_packing_rule(name):
    make, expect = MESHES[name]
    mesh, rho = make()
    cells = np.asarray(mesh.cells)
    n, nv = len(mesh.points), cells.shape[1]
    assert np.all(rho > 0.0) and (expect != 'all' or len(np.unique(rho)) == 1)
    rows, w16, fits16, weight, short_row = rw.mesh_records(mesh.points, cells, rho)
    assert short_row.all() and fits16.all()          # every mesh here has straight-line classes only
    sl, base, compact = rw.slice_rule(rows, weight, short_row, fits16, n)
    spread = np.ptp(rw.bits(weight))
    print("%s: %d rows, %d slices, %d compact; %d distinct weights over %d ulps" %
          (name, n, len(compact), compact.sum(), len(np.unique(weight)), spread))
    if expect == 'all':
        assert compact.all() and spread <= rw.DELTA_MAX
    else:
        assert not compact.any()
    # every record of a compact slice: the fields of cs16 and the very bits of the weight
    rec = compact[sl]
    word, fits = rw.pack(w16[rec], weight[rec], base[sl][rec])
    assert fits.all()
    slots, back = rw.unpack(word, base[sl][rec])
    assert np.array_equal(slots, w16[rec].astype(np.uint32))
    assert np.array_equal(rw.bits(back), rw.bits(weight[rec]))
    assert np.all(slots >> np.uint32(5 * (nv - 1)) == 0)


def test_reserved_code_is_plus_zero():
    for base in (0, int(rw.bits(np.float64(1.25e-3))), int(rw.bits(np.float64(-3.0)))):
        slots, w = rw.unpack(np.array([rw.WORD_ZERO]), base)
        assert slots[0] == 0 and w[0] == 0.0 and not np.signbit(w[0])
    # ... and no real record's word carries it
    word, fits = rw.pack(np.array([0x7FFF, 0], dtype=np.uint32), np.array([1.0, 1.0]), rw.bits(np.float64(1.0)))
    assert fits.all() and np.all(word.view(np.int32) >> rw.SLOT_BITS != rw.DELTA_ZERO)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("off,compact", [(2 ** 16 - 1, True), (2 ** 16, False), (2 ** 16 + 1, False)])
def test_limit_of_the_offset(off, compact, sign):
    """A slice of 64 one-record rows whose weights lie exactly `off` ulps apart."""
    b = int(rw.bits(np.float64(0.05 * 1.0 / 6.0 / 120.0)))
    pattern = np.full(64, b, dtype=np.int64)
    pattern[17] = b + sign * off
    weight = pattern.view(np.float64)
    rows = np.arange(64)
    sl, base, ok = rw.slice_rule(rows, weight, np.ones(64, dtype=bool), np.ones(64, dtype=bool), 64)
    assert base[0] == b and bool(ok[0]) == compact
    word, fits = rw.pack(np.full(64, 0x5A5A, dtype=np.uint32), weight, b)
    assert bool(fits.all()) == compact
    if compact:
        slots, back = rw.unpack(word, b)
        assert np.array_equal(rw.bits(back), pattern) and np.all(slots == 0x5A5A)


def test_a_slice_of_zero_weights_is_compact():
    mesh, _ = _c3()
    cells = np.asarray(mesh.cells)
    rows, w16, fits16, weight, short_row = rw.mesh_records(mesh.points, cells, np.zeros(len(cells)))
    sl, base, compact = rw.slice_rule(rows, weight, short_row, fits16, len(mesh.points))
    assert compact.all() and np.all(base == 0)
    word, fits = rw.pack(w16, weight, base[sl])
    assert fits.all() and np.all(word >> np.uint32(rw.SLOT_BITS) == 0)
    assert np.all(rw.bits(rw.unpack(word, base[sl])[1]) == 0)


def test_a_long_row_makes_its_slice_full():
    rows = np.arange(64)
    short = np.ones(64, dtype=bool)
    short[5] = False
    _, _, ok = rw.slice_rule(rows, np.ones(64), short, np.ones(64, dtype=bool), 64)
    assert not ok[0]


def test_header_rules_hold_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "record_words_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "record_words_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
