"""
The dot-free Krylov pass (k_cheb) reads an EXACTLY LINEAR slice of the RD Jacobian -- one whose stored values of
A = S + 2 dt N(c) are the values of the static S bit for bit, which the assembly sweep flags per slice and per sweep -- from one
32-bit word per entry (DevPattern::scode, glimslib_amd/csrc/value_codes.h): the 16-bit column code, a 5-bit index into the
slice's dictionary of 32 bit patterns and an 11-bit offset, instead of the value (8 B) and the column code (2 B).  The decode
returns the 64 bits vA holds, so every result must be the same: each case runs default flags against GLIMS_FLAG_NO_VALUE_CODES
through the C-ABI handle and asks for the same bits of the concentration after 6-8 steps and the same solver counts.
glims_stats says how many slices of S have codes (rd_scode_slices / rd_scode_uncoded_slices), how many slices the latest sweep
found exactly linear (rd_lin_slices) and in how many launches of the pass a wave read a slice from the words
(cheb_coded_passes, counted on the device: it proves the branch was reached).  The dictionary rule itself is checked on the
host in tests/test_value_codes_cpu.py.

Shapes, the smallest that reach each branch.  Both kinds of slice in every step: a long thin box at the flagship's mesh width
(240 / 215 per cell) seeded four cells from one end -- 4 x 4 x 120 cells of one tissue (3025 rows, 48 slices) and 4 x 4 x 160
cells of two tissues split at mid-length (4025 rows, 63 slices); the far end stays exactly linear while the seeded end does not
(a cubic box will not do: the consistent-mass solve's tails reach the walls after one step).  No linear slice: the cube at
n = 8.  Other shapes: a 2-D strip (NV = 3, rows of 7), a jittered lattice and random points (no coded slice), random points
with a row of 36 entries (a class of the looped sweep, which stores lin = 0).  Dirichlet rows, a tissue with rho = 0, a state
set anew in mid-run and a sweep at another state between steps (flags cannot go stale), and the handles that keep the 10-byte
stream: fp32 Jacobian, int32 columns, a partitioned handle, multigrid-preconditioned solves.

Reference counterpart: none (a storage format of this implementation); the pass stands in for the linear solves of
'F == 0' (simulation_tumor_growth.py), and how it reads its operator must not show in any result.
"""
import importlib.util
import os

import numpy as np
import pytest

from glimslib_amd import workloads
from glimslib_amd.mesh import BoxMesh, RectangleMesh

pytestmark = pytest.mark.gpu

COUNTS = ('newton_its', 'rd_assemblies', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks', 'cheb_fused_passes',
          'rd_mass_in_sweep', 'cheb_host_counts', 'rd_rec32_sweeps')
HX = 240.0 / 215.0     # the flagship's mesh width
TABLES = dict(D=[0.0, 0.0, 0.01, 0.05, 0.0], rho=[0.0, 0.0, 0.05, 0.05, 0.0], gamma=[0.0, 0.1, 0.1, 0.1, 0.1],
              E=[1.0, 1000e-6, 3000e-6, 3000e-6, 1000e-6], nu=[0.3, 0.45, 0.45, 0.45, 0.3])


def _seed(points, centre):
    return np.exp(-0.5 * ((points - np.asarray(centre)) ** 2).sum(axis=1))


def _thin_box(nz, two_tissues):
    mesh = BoxMesh((0.0, 0.0, 0.0), (4 * HX, 4 * HX, nz * HX), 4, 4, nz)
    mid = mesh.cell_midpoints()
    label = np.where(two_tissues & (mid[:, 2] > 0.5 * nz * HX), workloads.GM, workloads.WM).astype(np.int32)
    c0 = _seed(mesh.points, (2 * HX, 2 * HX, 4 * HX))
    return workloads.Workload("thin box 4 x 4 x %d" % nz, mesh, label, TABLES, c0, 1.0, 10, False)


def _other_end(w, nz):
    return _seed(w.mesh.points, (2 * HX, 2 * HX, (nz - 4) * HX))


def _strip():
    mesh = RectangleMesh((0.0, 0.0), (4 * HX, 300 * HX), 4, 300)
    label = np.full(len(mesh.cells), workloads.WM, dtype=np.int32)
    c0 = _seed(mesh.points, (2 * HX, 4 * HX))
    return workloads.Workload("2-D strip 4 x 300", mesh, label, TABLES, c0, 1.0, 10, False)


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


def _longest_row(w):
    nbr = [set() for _ in range(len(w.mesh.points))]
    for cell in w.mesh.cells:
        for v in cell:
            nbr[v].update(cell)
    return max(len(s) for s in nbr)


def _open(backend, w, flags_or=0, dirichlet=None, **opts):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    opts.setdefault('dt', w.dt)
    h.set_options(flags=h.options.flags | flags_or, **opts)
    if dirichlet is not None:
        h.set_dirichlet_c(dirichlet[0], dirichlet[1])
    h.setup(False)
    h.set_state(w.c0)
    return h


def _one(backend, w, steps, flags_or, between=None, **kw):
    """`steps` steps, one call each; between(h, step): what happens after step `step`.  Returns the field, the final stats
    and, per step, (rd_lin_slices, cheb_coded_passes) as the handle reports them after it."""
    h = _open(backend, w, flags_or=flags_or, **kw)
    st, per_step = 0, []
    for i in range(steps):
        st |= h.step(1)
        s = h.stats()
        per_step.append((s['rd_lin_slices'], s['cheb_coded_passes']))
        if between is not None:
            between(h, i + 1)
    c = h.get_state(want_u=False)[0]
    s = h.stats()
    h.close()
    assert st == 0
    return c, s, per_step


def _same_bits(backend, w, steps, what, flags_or=0, **kw):
    """Default flags against GLIMS_FLAG_NO_VALUE_CODES: the field's bits and the solver's counts."""
    a = _one(backend, w, steps, flags_or, **kw)
    b = _one(backend, w, steps, flags_or | backend.FLAG_NO_VALUE_CODES, **kw)
    n_slices = (len(w.mesh.points) + 63) // 64
    print("%s: %d rows, %d slices, %d steps: Newton %d, sweeps %d, dot-free solves %d with %d passes, %d of them read codes; "
          "slices of S coded %d, uncoded %d; exactly linear after each step %s; largest difference %.3e" %
          (what, len(w.mesh.points), n_slices, steps, a[1]['newton_its'], a[1]['rd_assemblies'], a[1]['cheb_solves'],
           a[1]['cheb_its'], a[1]['cheb_coded_passes'], a[1]['rd_scode_slices'], a[1]['rd_scode_uncoded_slices'],
           [p[0] for p in a[2]], np.abs(a[0] - b[0]).max()))
    # under the flag: no codes, no flags, no coded pass
    assert b[1]['rd_scode_slices'] == 0 and b[1]['rd_scode_uncoded_slices'] == 0 and b[1]['cheb_coded_passes'] == 0
    assert all(p == (0, 0) for p in b[2])
    assert np.all(np.isfinite(a[0])) and np.array_equal(a[0], b[0])
    for k in COUNTS:
        assert a[1][k] == b[1][k], (k, a[1][k], b[1][k])
    return a, n_slices


# ---- both kinds of slice in every step ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz,two_tissues,rows,slices", [(120, False, 3025, 48), (160, True, 4025, 63)])
def test_thin_box_has_linear_and_nonlinear_slices_in_every_step(backend, nz, two_tissues, rows, slices):
    w = _thin_box(nz, two_tissues)
    assert len(w.mesh.points) == rows
    a, n_slices = _same_bits(backend, w, 8, w.name)
    assert n_slices == slices
    assert a[1]['cheb_solves'] > 0 and a[1]['cheb_coded_passes'] > 0
    # a lattice of congruent cells: every slice of S has its codes, so each exactly-linear slice is read from them
    assert a[1]['rd_scode_slices'] == slices and a[1]['rd_scode_uncoded_slices'] == 0
    for lin, _ in a[2]:
        assert 0 < lin < slices


@pytest.mark.parametrize("seed", ["config's own", "widened"])
def test_cube_without_a_coded_pass_after_the_first_step(backend, seed):
    """config_c3(8): no pass reads a word after step 1.  With the configuration's own seed (1 mm wide on a 30 mm mesh) the
    field is zero to rounding, no solve runs at all and every slice stays flagged; with the seed widened to 2.5 cells the
    solves run and the tails reach every slice by the end of the first step, so no slice is flagged."""
    w = workloads.config_c3(8) if seed == "config's own" else _c3_reduced(8)
    a, n_slices = _same_bits(backend, w, 6, "cube n = 8, seed: " + seed)
    assert a[1]['rd_scode_slices'] + a[1]['rd_scode_uncoded_slices'] == n_slices
    assert all(passes == a[2][0][1] for _, passes in a[2]) and a[1]['cheb_coded_passes'] == a[2][0][1]
    if seed == "widened":
        assert a[1]['cheb_solves'] > 0 and all(lin == 0 for lin, _ in a[2])
    else:
        assert a[1]['cheb_coded_passes'] == 0


# ---- other shapes: whatever the handle reports, and the same bits ---------------------------------------------------------------

def test_two_dimensional_strip(backend):
    w = _strip()
    a, n_slices = _same_bits(backend, w, 6, w.name)
    assert a[1]['rd_scode_slices'] + a[1]['rd_scode_uncoded_slices'] == n_slices
    assert a[1]['rd_scode_slices'] > 0 and a[1]['cheb_coded_passes'] > 0
    assert 0 < a[2][-1][0] < n_slices           # the far end of the strip stays linear


@pytest.mark.parametrize("points,jitter", [(2000, 0.3), (1000, None)])
def test_meshes_of_unlike_cells_have_no_coded_slice(backend, points, jitter):
    w = workloads.config_unstructured(points, jitter=jitter, seed=0)
    a, n_slices = _same_bits(backend, w, 6, w.name)
    # (every cell has its own shape: a slice's 64 diagonal entries alone need more than 32 bases, test_value_codes_cpu.py)
    assert a[1]['rd_scode_slices'] == 0 and a[1]['rd_scode_uncoded_slices'] == n_slices
    # no slice has words, so no pass can read one -- whatever the sweeps flag (the seed is wide here: they flag nothing)
    assert a[1]['cheb_solves'] > 0 and a[1]['cheb_coded_passes'] == 0 and all(p == (0, 0) for p in a[2])


def test_looped_sweep_stores_no_flag(backend):
    w = workloads.config_unstructured(3000, seed=0)
    assert _longest_row(w) == 36
    a, n_slices = _same_bits(backend, w, 6, "random points 3000 (looped class)")
    assert a[1]['rd_scode_slices'] == 0 and a[1]['rd_scode_uncoded_slices'] == n_slices
    assert a[1]['cheb_solves'] > 0 and a[1]['cheb_coded_passes'] == 0
    assert all(p == (0, 0) for p in a[2])


# ---- constraints ----------------------------------------------------------------------------------------------------------------

def test_dirichlet_rows_on_the_thin_box(backend):
    w = _thin_box(120, False)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    bn = bn[w.mesh.points[bn, 2] > 100 * HX]                       # the walls of the far (linear) end
    a, _ = _same_bits(backend, w, 6, "thin box, Dirichlet rows", dirichlet=(bn, np.full(len(bn), 0.01)))
    assert np.all(a[0][bn] == 0.01)
    assert a[1]['cheb_coded_passes'] > 0


def test_three_tissues_with_a_zero_rho(backend):
    w = _three_tissues(12)
    a, n_slices = _same_bits(backend, w, 6, "three tissues, n = 12")
    assert a[1]['rd_mass_fallback_rows'] > 0
    assert a[1]['rd_scode_slices'] + a[1]['rd_scode_uncoded_slices'] == n_slices


# ---- flags cannot go stale ------------------------------------------------------------------------------------------------------

def test_a_new_state_in_mid_run(backend):
    """After three steps the seed moves to the other end: the slices that were linear are not any more, and the reverse."""
    w = _thin_box(120, False)
    other = _other_end(w, 120)

    def between(h, step):
        if step == 3:
            h.set_state(other)

    a, n_slices = _same_bits(backend, w, 7, "thin box, state set anew after step 3", between=between)
    assert all(0 < lin < n_slices for lin, _ in a[2])
    assert a[1]['cheb_coded_passes'] > a[2][2][1]       # coded passes after the change as well


def test_a_sweep_at_another_state_between_steps(backend):
    """glims_apply(8, x) with a random x leaves A(x) != S everywhere (and then puts A(c) back): bits as under the flag."""
    w = _thin_box(120, False)
    x = np.abs(np.random.default_rng(3).standard_normal(len(w.mesh.points)))
    seen = []

    def between(h, step):
        y = h.apply(8, x)[0]
        seen.append(float(np.abs(y).max()))

    a, n_slices = _same_bits(backend, w, 6, "thin box, apply(8) between steps", between=between)
    assert all(v > 0.0 for v in seen)
    assert all(0 < lin < n_slices for lin, _ in a[2])


# ---- the handles that keep the 10-byte stream -----------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", ["FLAG_FP32_JACOBIAN", "FLAG_INT32_COLUMNS"])
def test_other_storage_formats_keep_todays_stream(backend, flag):
    w = _thin_box(120, False)
    a, _ = _same_bits(backend, w, 6, "thin box, " + flag, flags_or=getattr(backend, flag))
    assert a[1]['cheb_solves'] > 0
    assert a[1]['cheb_coded_passes'] == 0 and a[1]['rd_scode_slices'] == 0 and all(p == (0, 0) for p in a[2])


def test_multigrid_preconditioned_solves_keep_todays_stream(backend):
    """A stiff step (D x 300): the RD solves are PCG with the V-cycle, which reads vA."""
    w = _thin_box(120, False)
    w.tables = {k: list(v) for k, v in w.tables.items()}
    w.tables['D'] = [300.0 * v for v in w.tables['D']]
    a, _ = _same_bits(backend, w, 3, "thin box, stiff, V-cycle", rd_precond=backend.RD_PRECOND_MULTIGRID)
    assert a[1]['rd_precond_used'] == backend.RD_PRECOND_MULTIGRID and a[1]['rd_mg_cycles'] > 0
    assert a[1]['cheb_coded_passes'] == 0


def _rehearse():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rehearse_partition", os.path.join(root, "tools", "rehearse_partition.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_partitioned_handle_keeps_todays_stream(backend):
    """Two ranks as threads of this process (parallel.ThreadedTransport): no codes are built, no pass is given any."""
    rp = _rehearse()
    w = _thin_box(120, False)
    import ctypes
    default = backend.Options()
    backend.load_library().glims_options_default(ctypes.byref(default))
    st_a, c_a, _, ss_a = rp.run_partitioned(w, 2, 4, 0)
    st_b, c_b, _, ss_b = rp.run_partitioned(w, 2, 4, 0, flags=default.flags | backend.FLAG_NO_VALUE_CODES)
    assert st_a == 0 and st_b == 0
    for s in ss_a + ss_b:
        assert s['cheb_solves'] > 0
        assert s['cheb_coded_passes'] == 0 and s['rd_scode_slices'] == 0 and s['rd_lin_slices'] == 0
    assert np.array_equal(c_a, c_b)
    for sa, sb in zip(ss_a, ss_b):
        for k in COUNTS:
            assert sa[k] == sb[k], (k, sa[k], sb[k])
