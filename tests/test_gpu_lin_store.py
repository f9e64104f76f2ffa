"""
A straight-line assembly sweep that finds a slice of 64 rows exactly linear (every value of A = S + 2 dt N(c) it has formed has
the bits of its entry of S) where the previous sweep found and left it so does not store the slice's values: the memory of vA
holds those bits already.  glims_stats.rd_lin_kept_slices counts the slices whose store the latest sweep left out; the flag
GLIMS_FLAG_STORE_LINEAR_SLICES makes every sweep store every slice.  Nothing else may change, so every case runs one call
sequence on two handles, default flags against GLIMS_FLAG_STORE_LINEAR_SLICES, and asks for the same bits of
  the concentration,
  glims_apply(0, x) for a fixed random x (k_spmv reads vA itself, never the value codes),
  the residual of a sweep at the state (glims_rd_residual) and the inverse diagonal it leaves (glims_apply(12, 1)),
  every integer of glims_stats but rd_lin_kept_slices, and the solver's last residuals and spectral interval,
at every checkpoint of the sequence.  A stale slice of vA would show in glims_apply(0) at once and in the PCG solves' counts.

Shapes, the smallest that reach each branch: the brain-extent box at n = 12 (2197 rows, 35 slices, two tissues) with a seed of
amplitude 1e-9 next to one corner (see _cube); the thin boxes of tests/test_gpu_value_codes.py (3025 rows, 48 slices: a seeded
end that is not linear and a far end that is), a 2-D strip (NV = 3), a jittered lattice (full records, no value codes), random
points with a row of 36 entries (a class of the looped sweep), and two ranks as threads of one process.  The adjoint call runs
on the smallest misfit set-up of tests/test_gpu_adjoint.py (81 rows, no linear slice) and, with the same terms, on the thin box,
where slices are kept around it.

Reference counterpart: none (a store this implementation leaves out); the sweep stands in for the assembly of 'F == 0'
(simulation_tumor_growth.py), and whether it rewrites bits that are there already must not show in any result.
"""
import importlib.util
import os

import numpy as np
import pytest

from glimslib_amd import workloads
from glimslib_amd.mesh import BoxMesh, RectangleMesh

pytestmark = pytest.mark.gpu

HX = 240.0 / 215.0     # the flagship's mesh width
TABLES = dict(D=[0.0, 0.0, 0.01, 0.05, 0.0], rho=[0.0, 0.0, 0.05, 0.05, 0.0], gamma=[0.0, 0.1, 0.1, 0.1, 0.1],
              E=[1.0, 1000e-6, 3000e-6, 3000e-6, 1000e-6], nu=[0.3, 0.45, 0.45, 0.45, 0.3])
FLOATS = ('last_newton_res', 'last_cg_res', 'cheb_lmin', 'cheb_lmax')


def _seed(points, centre, width=1.0):
    return np.exp(-0.5 * ((points - np.asarray(centre)) ** 2).sum(axis=1) / width ** 2)


def _cube():
    """config C3's box at n = 12 (cells of 20 x 20 x 12.9 mm, WM ellipsoid in a GM shell).  A slice is exactly linear where
    2 dt rho c stays below half an ulp of S, c < ~1e-15, and on cells this large the step is mass-dominated: the discrete
    Green's function of M + dt K falls by ~0.27 per cell.  A seed of amplitude 1e-9, one cell wide, two cells from the corner
    of the box: ~6 decades = ~10 cells of reach, on a box whose far corner is 17 cells away -- both kinds of slice after every
    step."""
    w = workloads.config_c3(12)
    w.c0 = 1e-9 * _seed(w.mesh.points, (40.0, -200.0, 26.0), 20.0)
    return w


def _thin_box(nz=120, two_tissues=False):
    mesh = BoxMesh((0.0, 0.0, 0.0), (4 * HX, 4 * HX, nz * HX), 4, 4, nz)
    mid = mesh.cell_midpoints()
    label = np.where(two_tissues & (mid[:, 2] > 0.5 * nz * HX), workloads.GM, workloads.WM).astype(np.int32)
    c0 = _seed(mesh.points, (2 * HX, 2 * HX, 4 * HX))
    return workloads.Workload("thin box 4 x 4 x %d" % nz, mesh, label, TABLES, c0, 1.0, 10, False)


def _strip():
    mesh = RectangleMesh((0.0, 0.0), (4 * HX, 300 * HX), 4, 300)
    label = np.full(len(mesh.cells), workloads.WM, dtype=np.int32)
    c0 = _seed(mesh.points, (2 * HX, 4 * HX))
    return workloads.Workload("2-D strip 4 x 300", mesh, label, TABLES, c0, 1.0, 10, False)


def _faint_corner_seed(w):
    """The brain-extent meshes of a few thousand points have cells of ~15-20 mm: the seed of _cube, for the same reason."""
    w.c0 = 1e-9 * _seed(w.mesh.points, (40.0, -200.0, 26.0), 20.0)
    return w


def _n_slices(w):
    return (len(w.mesh.points) + 63) // 64


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


def _x(n):
    return np.random.default_rng(11).standard_normal(n)


def _look(h, sweep=True):
    """What a handle shows at a checkpoint.  The products and the counts come first, as the steps left them; then (sweep) the
    residual of one sweep at the state and the inverse diagonal it leaves, and the flags after THAT sweep."""
    n = h.n_nodes
    out = dict(c=h.get_state(want_u=False)[0], Ax=h.apply(0, _x(n))[0])
    s = h.stats()
    out['lin'], out['kept'] = s['rd_lin_slices'], s['rd_lin_kept_slices']
    out['counts'] = {k: v for k, v in s.items()
                     if k != 'rd_lin_kept_slices' and (k in FLOATS or (isinstance(v, (int, np.integer)) and not isinstance(v, bool)))}
    if sweep:
        out['R'] = h.rd_residual(out['c'], out['c'])
        out['dinv'] = h.apply(12, np.ones(n))[0]
        out['Ax2'] = h.apply(0, _x(n))[0]
        s = h.stats()
        out['lin2'], out['kept2'] = s['rd_lin_slices'], s['rd_lin_kept_slices']
    return out


def _same(a, b, what):
    """Checkpoint by checkpoint: default handle `a` against the handle under the flag `b`."""
    assert len(a) == len(b) and len(a) > 0
    for i, (p, q) in enumerate(zip(a, b)):
        for k in ('c', 'Ax', 'R', 'dinv', 'Ax2'):
            if k in p:
                assert np.all(np.isfinite(p[k])), (what, i, k)
                assert np.array_equal(p[k], q[k]), (what, i, k, float(np.abs(p[k] - q[k]).max()))
        for k in ('lin', 'lin2'):
            if k in p:
                assert p[k] == q[k], (what, i, k, p[k], q[k])
        assert sorted(p['counts']) == sorted(q['counts']) and len(p['counts']) > 30
        for k, v in p['counts'].items():
            assert v == q['counts'][k], (what, i, k, v, q['counts'][k])
        for k in ('kept', 'kept2'):
            if k in p:
                assert 0 <= p[k] <= p['lin' + k[4:]], (what, i, k, p[k])
                assert q[k] == 0, (what, i, k, q[k])


def _both(backend, w, script, what, flags_or=0, flags_default=0, **kw):
    """script(h) -> list of _look()s.  Runs it under flags_or | flags_default and under flags_or | STORE_LINEAR_SLICES."""
    runs = []
    for f in (flags_default, backend.FLAG_STORE_LINEAR_SLICES):
        h = _open(backend, w, flags_or=flags_or | f, **kw)
        try:
            runs.append(script(h))
        finally:
            h.close()
    a = runs[0]
    print("%s: %d rows, %d slices; per checkpoint (linear, kept) %s, after one more sweep %s; solves %d dot-free, %d PCG passes" %
          (what, len(w.mesh.points), _n_slices(w), [(p['lin'], p['kept']) for p in a],
           [(p['lin2'], p['kept2']) for p in a if 'lin2' in p], a[-1]['counts']['cheb_solves'], a[-1]['counts']['cg_its']))
    _same(runs[0], runs[1], what)
    return a


def _steps(n, sweep=True):
    """n calls of step(1), a checkpoint after each.  sweep: True = every checkpoint runs the sweep hook (which drops what the
    step's last sweep prepared for the next step's first solve), 'last' = only the final one, False = none."""
    def script(h):
        out = []
        for i in range(n):
            assert h.step(1) == 0
            out.append(_look(h, sweep is True or (sweep == 'last' and i == n - 1)))
        return out
    return script


# ---- 1. lattice, localised tumour ------------------------------------------------------------------------------------------------

def test_cube_with_a_localised_tumour(backend):
    w = _cube()
    assert len(w.mesh.points) == 2197 and len(set(w.cell_label.tolist())) == 2
    n_slices = _n_slices(w)
    a = _both(backend, w, _steps(6, sweep=False), "cube n = 12")
    for i, p in enumerate(a):
        assert 0 < p['lin'] < n_slices, (i, p['lin'])
        assert p['kept'] <= p['lin']
        if i >= 1:
            assert p['kept'] > 0, (i, p['kept'])
    assert a[-1]['counts']['cheb_solves'] + a[-1]['counts']['cg_its'] > 0      # the steps did solve


# ---- 2. a flag's life -------------------------------------------------------------------------------------------------------------

def test_a_flags_life_linear_nonlinear_linear(backend):
    """One sweep at a time (glims_rd_residual at the state is one sweep).  Zero field: every slice is linear; the first sweep
    after glims_setup stores it (flags 1), the next keeps it (flags 2), and so does a step.  A field >= 0.1 everywhere: no
    slice is linear, nothing is kept.  Zero again: the slices hold A(0.1..) != S, so the first sweep must store them."""
    w = _thin_box(120, False)
    n, ns = len(w.mesh.points), _n_slices(w)
    zero = np.zeros(n)
    high = 0.1 + 0.2 * _seed(w.mesh.points, (2 * HX, 2 * HX, 60 * HX), 10.0)
    seen = {}

    def script(h):
        out = []
        key = h.options.flags & backend.FLAG_STORE_LINEAR_SLICES
        log = seen.setdefault(key, [])

        def sweep(c):
            h.rd_residual(c, c)
            s = h.stats()
            log.append((s['rd_lin_slices'], s['rd_lin_kept_slices']))

        h.set_state(zero)
        sweep(zero)
        sweep(zero)
        assert h.step(1) == 0
        out.append(_look(h))
        h.set_state(high)
        sweep(high)
        assert h.step(1) == 0
        out.append(_look(h))
        h.set_state(zero)
        sweep(zero)
        sweep(zero)
        assert h.step(1) == 0
        out.append(_look(h))
        return out

    a = _both(backend, w, script, "thin box, zero / >= 0.1 / zero")
    d, f = seen[0], seen[backend.FLAG_STORE_LINEAR_SLICES]
    assert d == [(ns, 0), (ns, ns), (0, 0), (ns, 0), (ns, ns)], d
    assert f == [(ns, 0), (ns, 0), (0, 0), (ns, 0), (ns, 0)], f
    assert (a[0]['lin'], a[0]['kept']) == (ns, ns) and (a[0]['lin2'], a[0]['kept2']) == (ns, ns)
    assert (a[1]['lin'], a[1]['kept']) == (0, 0) and (a[1]['lin2'], a[1]['kept2']) == (0, 0)
    assert (a[2]['lin'], a[2]['kept']) == (ns, ns)


# ---- 3. other writers of vA -------------------------------------------------------------------------------------------------------

def test_setup_again_on_a_stepped_handle(backend):
    """glims_setup copies S into vA and clears the flags: the first sweep after it stores."""
    w = _thin_box(120, False)
    after = []

    def script(h):
        out = _steps(2)(h)
        c = h.get_state(want_u=False)[0]
        h.setup(False)
        s = h.stats()
        after.append((s['rd_lin_slices'], s['rd_lin_kept_slices']))
        h.set_state(c)
        return out + _steps(2)(h)

    a = _both(backend, w, script, "thin box, setup again after step 2")
    assert after == [(0, 0), (0, 0)]
    assert a[1]['kept2'] > 0 and a[-1]['kept'] > 0


def test_an_adjoint_gradient_between_steps(backend):
    """The adjoint's sweeps write its own buffer and keep no flags (ForwardGuard): the handle's vA and flags are as before."""
    from adjoint_common import Problem
    prob = Problem(2, 8)
    terms = prob.terms(3, with_u=False)
    grads = []

    def run(flag):
        h = backend.Handle(prob.points, prob.cells, prob.labels)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12, flags=h.options.flags | flag)
        h.set_dirichlet_c(prob.dir_c[0], prob.dir_c[1])
        h.set_dirichlet_u(prob.dir_u[0], prob.dir_u[1])
        h.setup(with_mechanics=True)
        h.set_state(prob.c0)
        h.adjoint_record(True)
        try:
            out = _steps(3)(h)
            grads.append(h.adjoint_gradient(terms, 2))
            out.append(_look(h))
            return out + _steps(2)(h)
        finally:
            h.close()

    a, b = run(0), run(backend.FLAG_STORE_LINEAR_SLICES)
    _same(a, b, "adjoint gradient after step 3")
    assert grads[0][0] == grads[1][0] and all(np.array_equal(x, y) for x, y in zip(grads[0][1:], grads[1][1:]))


def test_an_adjoint_gradient_over_kept_slices(backend):
    """The set-up above (c >= 5e-10 everywhere, a Dirichlet value of 0.05) has no linear slice, so nothing is kept around its
    gradient call.  Here the same misfit terms on the thin box, no Dirichlet value on c: the far end is exactly linear, and
    slices ARE kept right before the gradient call, in the sweep right after it and after the steps that follow.  The
    backward sweeps assemble A at the recorded states into the adjoint's own buffer, which no flag describes: had they seen
    the handle's flags they would have left linear slices of that buffer unwritten (a different gradient than under the
    opt-out flag), and had they written the handle's buffer, glims_apply(0) after the call would differ."""
    from adjoint_common import Problem
    w = _thin_box(120, False)
    ns = _n_slices(w)
    t = w.tables
    prob = Problem.from_mesh(w.mesh.points, w.mesh.cells, w.cell_label, t['D'], t['rho'], t['gamma'], t['E'], t['nu'], w.c0,
                             dt=w.dt)
    terms = prob.terms(3, with_u=False)
    grads = []

    def run(flag):
        h = backend.Handle(prob.points, prob.cells, prob.labels)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, flags=h.options.flags | flag)
        h.setup(with_mechanics=False)
        h.set_state(prob.c0)
        h.adjoint_record(True)
        try:
            out = _steps(3)(h)
            grads.append(h.adjoint_gradient(terms, prob.n_labels))
            out.append(_look(h))
            return out + _steps(2)(h)
        finally:
            h.close()

    a, b = run(0), run(backend.FLAG_STORE_LINEAR_SLICES)
    print("thin box, adjoint gradient after step 3: %d slices; per checkpoint (linear, kept) %s, after one more sweep %s" %
          (ns, [(p['lin'], p['kept']) for p in a], [(p['lin2'], p['kept2']) for p in a]))
    _same(a, b, "thin box, adjoint gradient after step 3")
    assert grads[0][0] == grads[1][0] and all(np.array_equal(x, y) for x, y in zip(grads[0][1:], grads[1][1:]))
    assert np.isfinite(grads[0][0]) and all(np.all(np.isfinite(x)) for x in grads[0][1:])
    before, after = a[2], a[3]
    assert 0 < before['lin2'] < ns and before['kept2'] > 0            # the sweep right before the gradient call kept slices
    assert (after['lin'], after['kept']) == (before['lin2'], before['kept2'])   # the call leaves the handle's flags as they were
    assert after['kept2'] > 0 and after['kept2'] == after['lin2'] == before['lin2']   # the same state again: all of them kept
    for p in a[4:]:
        assert p['kept'] > 0 and 0 < p['lin'] < ns


def test_fp32_jacobian_then_fp64_again(backend):
    """Under GLIMS_FLAG_FP32_JACOBIAN the sweeps write vA32 and the handle keeps no flags; glims_setup without the flag starts
    from vA = S and cleared flags."""
    w = _thin_box(120, False)

    def script(h):
        keep = h.options.flags
        h.set_options(flags=keep | backend.FLAG_FP32_JACOBIAN)
        h.setup(False)
        h.set_state(w.c0)
        out = _steps(2)(h)
        assert all(p['lin'] == 0 and p['kept'] == 0 and p['kept2'] == 0 for p in out)
        c = h.get_state(want_u=False)[0]
        h.set_options(flags=keep)
        h.setup(False)
        h.set_state(c)
        return out + _steps(2)(h)

    a = _both(backend, w, script, "thin box, fp32 Jacobian for two steps")
    assert a[-1]['kept'] > 0


@pytest.mark.parametrize("what", ["full Newton", "PCG"])
def test_other_iterations(backend, what):
    """GLIMS_FLAG_FULL_NEWTON (a sweep per Newton iteration) and rd_linear = PCG (every solve streams vA)."""
    w = _thin_box(120, False)
    kw = dict(flags_or=backend.FLAG_FULL_NEWTON) if what == "full Newton" else dict(rd_linear=backend.RD_LINEAR_PCG)
    a = _both(backend, w, _steps(4), "thin box, " + what, **kw)
    assert a[-1]['kept'] > 0 and 0 < a[-1]['lin'] < _n_slices(w)
    if what == "PCG":
        assert a[-1]['counts']['cheb_solves'] == 0 and a[-1]['counts']['cg_its'] > 0


# ---- 4. kernel branches -----------------------------------------------------------------------------------------------------------

def test_two_dimensional_strip(backend):
    w = _strip()
    a = _both(backend, w, _steps(4), w.name)
    assert a[-1]['kept'] > 0 and 0 < a[-1]['lin'] < _n_slices(w)


def test_jittered_lattice_keeps_without_value_codes(backend):
    w = _faint_corner_seed(workloads.config_unstructured(2000, jitter=0.3, seed=0))
    a = _both(backend, w, _steps(4), w.name)
    assert a[-1]['counts']['rd_scode_slices'] == 0 and a[-1]['counts']['cheb_coded_passes'] == 0
    assert a[-1]['kept'] > 0 and 0 < a[-1]['lin'] < _n_slices(w)


def test_looped_class_never_keeps(backend):
    """Random points with a row of 36 entries: the slices of the looped sweep's class store flag 0 in every sweep, so a zero
    field leaves fewer flags than slices; the slices of the straight-line classes are kept."""
    w = workloads.config_unstructured(3000, seed=0)
    ns = _n_slices(w)
    w.c0 = np.zeros(len(w.mesh.points))
    a = _both(backend, w, _steps(2), "random points 3000 (looped class), zero field")
    assert 0 < a[-1]['lin'] < ns and a[-1]['kept'] == a[-1]['lin'] and a[-1]['kept2'] == a[-1]['lin2'] == a[-1]['lin']
    w = _faint_corner_seed(workloads.config_unstructured(3000, seed=0))
    _both(backend, w, _steps(3), "random points 3000 (looped class), faint seed")


def test_dirichlet_rows(backend):
    """Fixed rows in both kinds of slice.  c = 0.01 on the walls beyond z = 100 cells: those slices are not linear, and the
    value spreads towards the middle as the seed does from the other end.  c = 0 on the walls between z = 50 and 70 cells,
    the stretch farthest from both: where any slice is linear these are, so kept slices hold fixed rows (16 of the 25 nodes of
    a layer are on the walls, a slice is 2.6 layers)."""
    w = _thin_box(120, False)
    ns = _n_slices(w)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    z = w.mesh.points[bn, 2]
    far, mid = z > 100 * HX, (z > 50 * HX) & (z < 70 * HX)
    assert far.sum() > 64 and mid.sum() > 64
    val = np.where(far, 0.01, 0.0)[far | mid]
    bn = bn[far | mid]
    a = _both(backend, w, _steps(4), "thin box, Dirichlet rows", dirichlet=(bn, val))
    assert np.array_equal(a[-1]['c'][bn], val)
    for i, p in enumerate(a):
        assert 0 < p['lin'] < ns and 0 < p['lin2'] < ns, (i, p['lin'], p['lin2'])
        assert p['kept2'] > 0, (i, p['kept2'])
        if i >= 1:
            assert p['kept'] > 0, (i, p['kept'])


@pytest.mark.parametrize("flag", ["FLAG_NO_FUSED_GUESS", "FLAG_NO_FUSED_MASS", "FLAG_SLOT_WORDS32", "FLAG_RECORD_WORDS_FULL"])
def test_sweep_instances(backend, flag):
    """FG = 0 against the default's FG = 1 and 2; MB = 0; 32-bit slot words; weight + slot word instead of compact records.
    Eight steps with no hook between them: the folded passes begin once the dot-free solves have their interval."""
    w = _thin_box(160, True)
    a = _both(backend, w, _steps(8, sweep='last'), "thin box, two tissues, " + flag, flags_or=getattr(backend, flag))
    assert a[-1]['kept'] > 0 and 0 < a[-1]['lin'] < _n_slices(w)
    if flag == "FLAG_NO_FUSED_GUESS":
        assert a[-1]['counts']['cheb_fused_passes'] == 0
        d = _both(backend, w, _steps(8, sweep='last'), "thin box, two tissues, default")
        assert d[-1]['counts']['cheb_fused_passes'] > 0 and d[-1]['counts']['cheb_fused_zero_starts'] > 0
        assert d[-1]['counts']['cheb_host_counts'] > 0
        assert np.array_equal(d[-1]['c'], a[-1]['c'])
    elif flag == "FLAG_NO_FUSED_MASS":
        assert a[-1]['counts']['rd_mass_in_sweep'] == 0
    elif flag == "FLAG_SLOT_WORDS32":
        assert a[-1]['counts']['rd_slot16_sweeps'] == 0
    else:
        assert a[-1]['counts']['rd_rec32_sweeps'] == 0


# ---- 5. partitioned handle --------------------------------------------------------------------------------------------------------

def _rehearse():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rehearse_partition", os.path.join(root, "tools", "rehearse_partition.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_partitioned_handle_stores_every_slice(backend):
    """Two ranks as threads of this process: the handles keep no flags, every sweep stores, and the field is the single-rank
    run's to the tolerance of tests/test_gpu_multirank.py (1e-9 in the relative 2-norm)."""
    rp = _rehearse()
    w = _thin_box(120, False)
    st1, c1, _, s1 = rp.run_single(w, 4, 0)
    st, c, _, ss = rp.run_partitioned(w, 2, 4, 0)
    assert st1 == 0 and st == 0
    assert s1['rd_lin_kept_slices'] > 0
    for s in ss:
        assert s['rd_lin_kept_slices'] == 0 and s['rd_lin_slices'] == 0
    assert rp.rel_l2(c, c1) < 1e-9
