"""
The straight-line assembly sweeps read the slots of an incidence record from a 16-bit word (DevPattern::cs16: the row's own
slot dropped, 5 bits per other vertex of the cell, two records of a lane per 32-bit element) instead of the 32-bit word with a
byte per vertex (cs2).  The slots are the same, so every result must be: each case runs default flags against
GLIMS_FLAG_SLOT_WORDS32 through the C-ABI handle and asks for the same bits of the concentration after a few steps, the same
solver counts, and the same bits from the hooks the sweep feeds directly -- glims_apply(8) (the sweep at c = x), glims_apply(10)
(the right-hand side the sweep forms, where the handle has that mode) and glims_rd_residual.  The packing rule itself is
checked on the same meshes in tests/test_slot_words16_cpu.py.

Shapes, the smallest that reach each branch: a 3-D lattice of 729 rows (CAP 16; 24^3 for stepping, where both folded solves
occur), a 2-D mesh (NV = 3: two fields), jittered lattices with rows of 5..25 / 5..24 entries (classes of 16, 20, 32 and 24
entries; slots up to 24 need the fifth bit), random-point meshes whose longest row has exactly 32 entries (slot 31, all classes
straight-line), and one with a row of 36 entries (a class of the looped kernel, which keeps cs2 whatever the flag says).

Reference counterpart: none (a storage format of this implementation); the sweep stands in for the assembly of
'F == 0' (simulation_tumor_growth.py), and how it reads its records must not show in any result.
"""
import numpy as np
import pytest

from glimslib_amd import workloads
from glimslib_amd.mesh import RectangleMesh

pytestmark = pytest.mark.gpu

COUNTS = ('newton_its', 'rd_assemblies', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks', 'cheb_fused_passes',
          'rd_mass_in_sweep')


def _c3_reduced(n):
    w = workloads.config_c3(n)
    hx = 240.0 / n
    w.c0 = np.exp(-((w.mesh.points - np.array([118.0, -109.0, 72.0])) ** 2).sum(axis=1) / (2.0 * (2.5 * hx) ** 2))
    return w


def _three_tissues(n):
    w = _c3_reduced(n)
    mid = w.mesh.cell_midpoints()
    w.cell_label = np.where(mid[:, 0] < 70.0, workloads.CSF, w.cell_label).astype(np.int32)
    w.tables = {k: list(v) for k, v in w.tables.items()}
    w.tables['D'][workloads.WM] = 2.0
    return w


def _rectangle():
    mesh = RectangleMesh((-5.0, -5.0), (5.0, 5.0), 12, 12)
    label = np.where(mesh.cell_midpoints()[:, 0] > 0.0, 1, 2).astype(np.int32)
    tables = dict(D=[0.0, 0.1, 0.05], rho=[0.0, 0.1, 0.1], gamma=[0.0, 0.2, 0.1], E=[1.0, 1e-3, 1e-3], nu=[0.3, 0.4, 0.4])
    c0 = np.exp(-((mesh.points - np.array([1.0, 1.0])) ** 2).sum(axis=1))
    return workloads.Workload("2-D 12x12", mesh, label, tables, c0, 1.0, 10, False)


def _longest_row(w):
    nbr = [set() for _ in range(len(w.mesh.points))]
    for cell in w.mesh.cells:
        for v in cell:
            nbr[v].update(cell)
    return max(len(s) for s in nbr)


def _open(backend, w, flags_or=0, flags_andnot=0, dirichlet=None, load=None, **opts):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    opts.setdefault('dt', w.dt)
    h.set_options(flags=(h.options.flags | flags_or) & ~flags_andnot, **opts)
    if dirichlet is not None:
        h.set_dirichlet_c(dirichlet[0], dirichlet[1])
    if load is not None:
        h.set_rd_load(load)
    h.setup(False)
    h.set_state(w.c0)
    return h


def _one(backend, w, steps, flags_or, mass_hook, **kw):
    h = _open(backend, w, flags_or=flags_or, **kw)
    n = len(w.mesh.points)
    x = np.random.default_rng(5).standard_normal(n)
    hooks = [h.apply(8, x)[0], h.apply(0, x)[0], h.rd_residual(np.abs(x), w.c0)]
    if mass_hook:
        hooks.append(h.apply(10, x)[0])
    h.set_state(w.c0)
    st, prev, most = 0, 0, 0
    for _ in range(steps):      # (one call per step: a step's folded passes can be counted)
        st |= h.step(1)
        now = h.stats()['cheb_fused_passes']
        prev, most = now, max(most, now - prev)
    c = h.get_state(want_u=False)[0]
    s = h.stats()
    s['most_folded_in_a_step'] = most
    h.close()
    assert st == 0
    return c, s, hooks


def _same_bits(backend, w, steps, what, flags_or=0, mass_hook=True, **kw):
    """Default slot words against GLIMS_FLAG_SLOT_WORDS32: field, counts and hooks."""
    a = _one(backend, w, steps, flags_or, mass_hook, **kw)
    b = _one(backend, w, steps, flags_or | backend.FLAG_SLOT_WORDS32, mass_hook, **kw)
    print("%s: %d rows, %d steps: Newton %d, sweeps %d (%d with the mass product), dot-free solves %d, folded passes %d; "
          "largest difference %.3e" % (what, len(w.mesh.points), steps, a[1]['newton_its'], a[1]['rd_assemblies'],
                                       a[1]['rd_mass_in_sweep'], a[1]['cheb_solves'], a[1]['cheb_fused_passes'],
                                       np.abs(a[0] - b[0]).max()))
    # the 16-bit words are really in use in the one run and not in the other (every mesh here has a straight-line class)
    assert a[1]['rd_slot16_sweeps'] > 0 and b[1]['rd_slot16_sweeps'] == 0
    assert np.array_equal(a[0], b[0])
    for k in COUNTS:
        assert a[1][k] == b[1][k], (k, a[1][k], b[1][k])
    assert len(a[2]) == len(b[2])
    for i, (ya, yb) in enumerate(zip(a[2], b[2])):
        assert np.all(np.isfinite(ya)) and np.abs(ya).max() > 0.0, i
        assert np.array_equal(ya, yb), i
    return a


def test_lattice_hooks_on_729_rows(backend):
    w = _c3_reduced(8)
    assert len(w.mesh.points) == 729
    _same_bits(backend, w, 6, "3-D n = 8")


def test_lattice_stepping_with_both_folded_solves(backend):
    w = _c3_reduced(24)
    a = _same_bits(backend, w, 8, "3-D n = 24")
    assert a[1]['most_folded_in_a_step'] == 2       # a step's first and second solve both took their first pass from a sweep
    assert a[1]['rd_mass_in_sweep'] > 0


def test_two_dimensional(backend):
    _same_bits(backend, _rectangle(), 6, "2-D 12 x 12")


@pytest.mark.parametrize("seed,longest", [(0, 25), (1, 24)])
def test_jittered_lattice_classes_16_20_24_32(backend, seed, longest):
    w = workloads.config_unstructured(2000, jitter=0.3, seed=seed)
    assert _longest_row(w) == longest
    a = _same_bits(backend, w, 6, "jittered lattice, seed %d" % seed)
    assert a[1]['rd_mass_in_sweep'] > 0


@pytest.mark.parametrize("points,seed", [(800, 3), (1000, 0)])
def test_longest_row_of_exactly_32_entries(backend, points, seed):
    w = workloads.config_unstructured(points, seed=seed)
    assert _longest_row(w) == 32
    a = _same_bits(backend, w, 6, "random points %d, seed %d" % (points, seed))
    assert a[1]['rd_mass_in_sweep'] > 0       # every class is a straight-line one


def test_looped_class_keeps_the_32_bit_words(backend):
    w = workloads.config_unstructured(3000, seed=0)
    assert _longest_row(w) == 36
    a = _same_bits(backend, w, 6, "random points 3000 (looped class)", mass_hook=False)
    assert a[1]['rd_mass_in_sweep'] == 0


# ---- each option once, on the smallest mesh that has the feature -----------------------------------------------------------

def test_int32_columns(backend):
    w = workloads.config_unstructured(2000, jitter=0.3, seed=0)
    _same_bits(backend, w, 6, "int32 columns", flags_or=backend.FLAG_INT32_COLUMNS)


def test_fp32_jacobian(backend):
    _same_bits(backend, _c3_reduced(8), 6, "fp32 Jacobian", flags_or=backend.FLAG_FP32_JACOBIAN, mass_hook=False)


def test_dirichlet_rows(backend):
    w = _c3_reduced(8)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    a = _same_bits(backend, w, 6, "Dirichlet rows", dirichlet=(bn, np.full(len(bn), 0.01)))
    assert np.all(a[0][bn] == 0.01)


def test_three_tissues_have_mass_fallback_rows(backend):
    a = _same_bits(backend, _three_tissues(8), 6, "three tissues")
    assert a[1]['rd_mass_fallback_rows'] > 0


def test_rd_load(backend):
    w = _c3_reduced(8)
    load = 1e-3 * np.exp(-((w.mesh.points - np.array([100.0, -100.0, 70.0])) ** 2).sum(axis=1) / 4000.0)
    _same_bits(backend, w, 6, "RD load", load=load)


def test_without_the_fused_guess_pass(backend):
    a = _same_bits(backend, _c3_reduced(8), 6, "no fused guess", flags_or=backend.FLAG_NO_FUSED_GUESS)
    assert a[1]['cheb_fused_passes'] == 0


def test_without_the_mass_product_in_the_sweep(backend):
    a = _same_bits(backend, _c3_reduced(8), 6, "no fused mass", flags_or=backend.FLAG_NO_FUSED_MASS, mass_hook=False)
    assert a[1]['rd_mass_in_sweep'] == 0
