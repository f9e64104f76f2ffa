"""
The 16-bit slot words of the straight-line assembly sweeps (DevPattern::cs16, k_corner_weights), checked in numpy on the
meshes of tests/test_gpu_slot_words16.py: the packing rule of tests/slot_words16_common.py loses nothing for a row of at most
32 entries -- every slot is below 32, a record has NV-1 fields, and unpacking returns bytes 1 .. NV-1 of the 32-bit word.

Reference counterpart: none (a storage format of this implementation; the reference assembles through UFL forms).
"""
import numpy as np
import pytest

from glimslib_amd import workloads
from glimslib_amd.mesh import RectangleMesh

from slot_words16_common import incidence_words, pack16, row_slots, unpack16


def _rectangle():
    return RectangleMesh((-5.0, -5.0), (5.0, 5.0), 12, 12)


# name -> (mesh factory, longest row or None)
MESHES = {
    "c3(8)": (lambda: workloads.config_c3(8).mesh, None),
    "rectangle 12x12": (_rectangle, None),
    "jittered lattice seed 0": (lambda: workloads.config_unstructured(2000, jitter=0.3, seed=0).mesh, 25),
    "jittered lattice seed 1": (lambda: workloads.config_unstructured(2000, jitter=0.3, seed=1).mesh, 24),
    "random 800 seed 3": (lambda: workloads.config_unstructured(800, seed=3).mesh, 32),
    "random 1000 seed 0": (lambda: workloads.config_unstructured(1000, seed=0).mesh, 32),
    "random 3000 seed 0": (lambda: workloads.config_unstructured(3000, seed=0).mesh, 36),
}


@pytest.mark.parametrize("name", list(MESHES))
def test_packing_rule(name):
    make, longest = MESHES[name]
    mesh = make()
    cells = np.asarray(mesh.cells)
    n, nv = len(mesh.points), cells.shape[1]
    ptr, _ = row_slots(cells, n)
    rlen = np.diff(ptr)
    if longest is not None:
        assert rlen.max() == longest
    rows, w32 = incidence_words(cells, n)
    assert len(rows) == nv * len(cells)
    short = rlen[rows] <= 32
    assert short.any()
    # every slot of a record is a slot of its row; the own slot is none of the others
    fields32 = np.stack([(w32 >> np.uint32(8 * m)) & np.uint32(255) for m in range(nv)], axis=-1)
    assert np.all(fields32 < rlen[rows][:, None])
    assert np.all(fields32[:, 1:] != fields32[:, :1])
    if nv < 4:
        assert np.all(w32 >> np.uint32(8 * nv) == 0)
    w16, fits = pack16(w32, nv)
    # rows of at most 32 entries: every slot below 32, and nothing is lost
    assert np.all(fields32[short] < 32) and np.all(fits[short])
    assert np.array_equal(unpack16(w16[short], nv), fields32[short][:, 1:])
    assert unpack16(w16, nv).shape[-1] == nv - 1
    assert np.all((w16.astype(np.uint32) >> np.uint32(5 * (nv - 1))) == 0)      # NV-1 fields, nothing above them
    top = int(fields32[short][:, 1:].max())
    print("%s: %d rows of %d..%d entries, %d incidences (%d of rows <= 32 entries), largest slot there %d" %
          (name, n, rlen.min(), rlen.max(), len(rows), short.sum(), top))
    if longest == 32:
        assert int(fields32[short].max()) == 31      # slot 31 occurs (as an own slot or in a field, by the numbering)
    if longest is not None and longest > 32:
        assert not fits.all()                  # a looped class: its records keep the 32-bit words


def test_padding_records_are_zero():
    w16, fits = pack16(np.zeros(3, dtype=np.uint32), 4)
    assert np.all(w16 == 0) and fits.all()
