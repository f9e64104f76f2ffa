"""
The straight-line assembly sweeps read the records of a COMPACT slice from one 32-bit word each (DevPattern::cr32,
glimslib_amd/csrc/record_words.h): the 16-bit slot fields of cs16 and, in the upper 17 bits, the offset of the fp64 reaction
weight's bit pattern from a per-slice base -- instead of the weight (cw, 8 B) and the slot word (cs16, 2 B).  The decode returns
the 64 bits cw holds, so every result must be the same: each case runs default flags against GLIMS_FLAG_RECORD_WORDS_FULL
through the C-ABI handle and asks for the same bits of the concentration after 6-8 steps, the same solver counts, and the same
bits from the hooks the sweep feeds directly -- glims_apply(8) (the sweep at c = x), glims_apply(10) (the right-hand side the
sweep forms, where the handle has that mode), glims_apply(0) and glims_rd_residual.  glims_stats says which slices are compact
(rd_rec_compact_slices / rd_rec_full_slices) and whether a sweep read cr32 (rd_rec32_sweeps).  The packing rule itself is
checked on the host in tests/test_record_words_cpu.py.

Shapes, the smallest that reach each branch: a 3-D lattice of 729 rows (all compact; 24^3 for stepping, where both folded solves
and the mass product occur: FG = 1, FG = 2 and MB = 1), a 2-D mesh (NV = 3: two fields), the three-tissue lattice with rho = 0
for x < 70 at n = 12 (2197 rows: 8 compact and 27 full slices in one class -- the smallest of 8 / 12 / 16 with both kinds; at n = 8 all
12 slices touch both a cell with rho = 0 and one without and are full), a jittered lattice
and random points with a longest row of 32 (cell volumes differ: no compact slice, the sweeps launch what they launched before),
and random points with a row of 36 entries (a class of the looped kernel).  fp64 Jacobian with 16-bit column codes only:
GLIMS_FLAG_INT32_COLUMNS, GLIMS_FLAG_FP32_JACOBIAN and GLIMS_FLAG_SLOT_WORDS32 (the compact word embeds the 16-bit fields)
keep today's streams, asserted through the stats.

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
MIXED_N = 12


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
    assert w.tables['rho'][workloads.CSF] == 0.0
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


def _open(backend, w, flags_or=0, dirichlet=None, load=None, **opts):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    opts.setdefault('dt', w.dt)
    h.set_options(flags=h.options.flags | flags_or, **opts)
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


def _same_bits(backend, w, steps, what, flags_or=0, mass_hook=True, compact='all', **kw):
    """
    Default record streams against GLIMS_FLAG_RECORD_WORDS_FULL: field, counts and hooks.
    compact: what the default run's stats must say -- 'all' / 'none' / 'mixed' slices of the straight-line classes compact and
    read from cr32, or 'off' (the slices may be compact, the handle's sweeps keep today's streams).
    """
    a = _one(backend, w, steps, flags_or, mass_hook, **kw)
    b = _one(backend, w, steps, flags_or | backend.FLAG_RECORD_WORDS_FULL, mass_hook, **kw)
    nc, nf = a[1]['rd_rec_compact_slices'], a[1]['rd_rec_full_slices']
    print("%s: %d rows, %d steps: Newton %d, sweeps %d (%d with the mass product, %d reading compact records), dot-free solves "
          "%d, folded passes %d; straight-line slices %d compact, %d full; largest difference %.3e" %
          (what, len(w.mesh.points), steps, a[1]['newton_its'], a[1]['rd_assemblies'], a[1]['rd_mass_in_sweep'],
           a[1]['rd_rec32_sweeps'], a[1]['cheb_solves'], a[1]['cheb_fused_passes'], nc, nf, np.abs(a[0] - b[0]).max()))
    # which slices are compact is a property of the set-up, not of the flag; no sweep reads cr32 under the flag
    assert (b[1]['rd_rec_compact_slices'], b[1]['rd_rec_full_slices']) == (nc, nf)
    assert b[1]['rd_rec32_sweeps'] == 0
    if compact == 'all':
        assert nc > 0 and nf == 0 and a[1]['rd_rec32_sweeps'] > 0
    elif compact == 'mixed':
        assert nc > 0 and nf > 0 and a[1]['rd_rec32_sweeps'] > 0
    elif compact == 'none':
        assert nc == 0 and a[1]['rd_rec32_sweeps'] == 0
    else:
        assert compact == 'off' and a[1]['rd_rec32_sweeps'] == 0
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
    a = _same_bits(backend, w, 6, "3-D n = 8")
    assert a[1]['rd_rec_compact_slices'] == 12       # 729 rows: every slice


def test_lattice_stepping_with_both_folded_solves(backend):
    w = _c3_reduced(24)
    a = _same_bits(backend, w, 8, "3-D n = 24")
    assert a[1]['most_folded_in_a_step'] == 2       # a step's first and second solve both took their first pass from a sweep
    assert a[1]['rd_mass_in_sweep'] > 0
    assert a[1]['rd_rec32_sweeps'] == a[1]['rd_slot16_sweeps']      # every sweep of the run


def test_two_dimensional(backend):
    _same_bits(backend, _rectangle(), 6, "2-D 12 x 12")


def test_one_class_with_a_compact_and_a_full_list(backend):
    w = _three_tissues(MIXED_N)
    a = _same_bits(backend, w, 6, "three tissues, n = %d" % MIXED_N, compact='mixed')
    assert a[1]['rd_mass_fallback_rows'] > 0


def test_jittered_lattice_has_no_compact_slice(backend):
    w = workloads.config_unstructured(2000, jitter=0.3, seed=0)
    a = _same_bits(backend, w, 6, "jittered lattice", compact='none')
    assert a[1]['rd_mass_in_sweep'] > 0 and a[1]['rd_slot16_sweeps'] > 0


def test_random_points_longest_row_32_have_no_compact_slice(backend):
    w = workloads.config_unstructured(1000, seed=0)
    assert _longest_row(w) == 32
    a = _same_bits(backend, w, 6, "random points 1000", compact='none')
    assert a[1]['rd_mass_in_sweep'] > 0 and a[1]['rd_slot16_sweeps'] > 0


def test_looped_class_is_untouched(backend):
    w = workloads.config_unstructured(3000, seed=0)
    assert _longest_row(w) == 36
    a = _same_bits(backend, w, 6, "random points 3000 (looped class)", mass_hook=False, compact='none')
    assert a[1]['rd_mass_in_sweep'] == 0


# ---- each option once, on 729 rows -------------------------------------------------------------------------------------------

def test_dirichlet_rows(backend):
    w = _c3_reduced(8)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    a = _same_bits(backend, w, 6, "Dirichlet rows", dirichlet=(bn, np.full(len(bn), 0.01)))
    assert np.all(a[0][bn] == 0.01)


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


def test_slot_words32_switches_the_compact_records_off(backend):
    a = _same_bits(backend, _c3_reduced(8), 6, "32-bit slot words", flags_or=backend.FLAG_SLOT_WORDS32, compact='off')
    assert a[1]['rd_slot16_sweeps'] == 0 and a[1]['rd_rec_compact_slices'] == 12


def test_int32_columns_keep_todays_streams(backend):
    a = _same_bits(backend, _c3_reduced(8), 6, "int32 columns", flags_or=backend.FLAG_INT32_COLUMNS, compact='off')
    assert a[1]['rd_slot16_sweeps'] > 0 and a[1]['rd_rec_compact_slices'] == 12


def test_fp32_jacobian_keeps_todays_streams(backend):
    a = _same_bits(backend, _c3_reduced(8), 6, "fp32 Jacobian", flags_or=backend.FLAG_FP32_JACOBIAN, mass_hook=False,
                   compact='off')
    assert a[1]['rd_slot16_sweeps'] > 0 and a[1]['rd_rec_compact_slices'] == 12
