"""
The mass product b = M c + load formed by the assembly sweep from its incidence loop (rd_assemble_s_slice with MB = 1) instead
of by a mass SpMV before it.  For a row whose cells share one rho > 0 the sweep's records give (M c)_i = (d+3)/rho sum_T w_T
(s_T + c_i) (tests/test_mass_from_incidences_cpu.py); rows at an interface of two rho, or touching a tissue with rho = 0, are
fallback rows and keep the SpMV, which then runs over their slices only.  The cases: the product itself against the assembled
M (glims_apply which = 10 against which = 2), stepping with and without GLIMS_FLAG_NO_FUSED_MASS, that every b of the stepping
path comes from one formula (chunked and restarted runs give the same bits), and where the mode must stay off.

The hook is which = 10: 8 and 9 are the sweep's and the quadratic-term pass's timing hooks (tests/test_gpu_parity.py).

Reference counterpart: 'u_previous1 * v1 * dx' (simulation_tumor_growth.py:117); how the product is scheduled must not show in
any result beyond the rounding of another summation order.
"""
import numpy as np
import pytest

from glimslib_amd import workloads
from oracle.glims_oracle import rel_l2

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
TOL_FIELD = 1e-12     # the tightest full-size oracle tolerance of the suite; a cap -- the difference is a few eps per step
COUNTS = ('newton_its', 'rd_assemblies', 'rd_quad_updates', 'cheb_solves', 'cheb_fallbacks')


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


def _open(backend, w, flags_or=0, flags_andnot=0, dirichlet=None, load=None, rho=None, **opts):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'] if rho is None else rho, t['gamma'], t['E'], t['nu'])
    opts.setdefault('dt', w.dt)
    h.set_options(flags=(h.options.flags | flags_or) & ~flags_andnot, **opts)
    if dirichlet is not None:
        h.set_dirichlet_c(dirichlet[0], dirichlet[1])
    if load is not None:
        h.set_rd_load(load)
    h.setup(False)
    h.set_state(w.c0)
    return h


def _fallback_rows(w, rho):
    """Rows whose cells do not all carry the same rho > 0 (by value), from the mesh."""
    rho_cell = np.asarray(rho, dtype=float)[w.cell_label]
    n = len(w.mesh.points)
    lo, hi = np.full(n, np.inf), np.full(n, -np.inf)
    for a in range(w.mesh.cells.shape[1]):
        np.minimum.at(lo, w.mesh.cells[:, a], rho_cell)
        np.maximum.at(hi, w.mesh.cells[:, a], rho_cell)
    return (lo != hi) | ~(lo > 0.0)


def _longest_row(w):
    nbr = [set() for _ in range(len(w.mesh.points))]
    for cell in w.mesh.cells:
        for v in cell:
            nbr[v].update(cell)
    return max(len(s) for s in nbr)


def _check_direct(h, w, rho, load=None, what="", bit_equal_fallback=True):
    """apply(10) = M x + load as the stepping path's sweep forms it, against the assembled M: componentwise within
    128 eps (M |x|)_i -- both are sums of a few dozen products with a handful of roundings each -- and the fallback rows, which
    the SpMV itself wrote, bit for bit."""
    n = len(w.mesh.points)
    x = np.random.default_rng(3).standard_normal(n)
    y = h.apply(10, x)[0]
    ref = h.apply(2, x)[0]
    bound = 128.0 * EPS * h.apply(2, np.abs(x))[0]
    if load is not None:
        ref = ref + load
    fb = _fallback_rows(w, rho)
    s = h.stats()
    err = np.abs(y - ref)
    print("%s: %d rows, %d fallback (stat %d); largest error / bound %.3f" %
          (what, n, fb.sum(), s['rd_mass_fallback_rows'], (err / bound).max()))
    assert s['rd_mass_fallback_rows'] == fb.sum()
    assert np.all(err <= bound)
    if bit_equal_fallback and load is None:
        assert np.array_equal(y[fb], ref[fb])
    return int(fb.sum())


# ---- 1. the product itself ------------------------------------------------------------------------------------------------

def test_direct_equal_rho_has_no_fallback_rows(backend):
    w = _c3_reduced(8)
    h = _open(backend, w)
    assert _check_direct(h, w, w.tables['rho'], what="3-D n = 8, equal rho") == 0
    h.close()


def test_direct_three_tissues_fallback_rows_are_the_spmv_bits(backend):
    w = _three_tissues(8)
    h = _open(backend, w)
    assert _check_direct(h, w, w.tables['rho'], what="3-D n = 8, CSF | GM | WM") > 0
    h.close()


def test_direct_two_dimensional(backend):
    from glimslib_amd.mesh import RectangleMesh
    mesh = RectangleMesh((-5.0, -5.0), (5.0, 5.0), 12, 12)
    label = np.where(mesh.cell_midpoints()[:, 0] > 0.0, 1, 2).astype(np.int32)
    tables = dict(D=[0.0, 0.1, 0.05], rho=[0.0, 0.1, 0.1], gamma=[0.0, 0.2, 0.1], E=[1.0, 1e-3, 1e-3], nu=[0.3, 0.4, 0.4])
    c0 = np.exp(-((mesh.points - np.array([1.0, 1.0])) ** 2).sum(axis=1))
    w = workloads.Workload("2-D 12x12", mesh, label, tables, c0, 1.0, 10, False)
    h = _open(backend, w)
    assert _check_direct(h, w, tables['rho'], what="2-D 12 x 12") == 0
    h.close()


def test_direct_int32_columns(backend):
    w = _three_tissues(8)
    h = _open(backend, w, flags_or=backend.FLAG_INT32_COLUMNS)
    assert _check_direct(h, w, w.tables['rho'], what="int32 columns") > 0
    h.close()


def test_direct_with_load(backend):
    """The load is added in the same fused multiply-add (q macc + load); sized like M |x| so that it matters and its own
    rounding (one eps of the sum) stays inside the bound."""
    w = _three_tissues(8)
    vol = 240.0 * 240.0 * 155.0 / len(w.mesh.points)
    load = 0.2 * vol * np.cos(0.05 * w.mesh.points[:, 0]) * np.exp(-((w.mesh.points - np.array([100.0, -100.0, 70.0])) ** 2).sum(axis=1) / 4000.0)
    h = _open(backend, w, load=load)
    _check_direct(h, w, w.tables['rho'], load=load, what="with rd_load")
    h.close()


def test_direct_with_dirichlet_rows(backend):
    """Constrained rows: b is not used there (the residual is 0), but the buffer still holds M x as the SpMV's does."""
    w = _three_tissues(8)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    h = _open(backend, w, dirichlet=(bn, np.full(len(bn), 0.01)))
    _check_direct(h, w, w.tables['rho'], what="Dirichlet rows")
    h.close()


@pytest.mark.parametrize("seed,longest", [(0, 25), (1, 24)])
def test_direct_unstructured_rows_up_to_32_entries(backend, seed, longest):
    """A lattice of 2 560 points jittered by 0.3 h, Delaunay: rows of 6..25 (seed 0) or 6..24 (seed 1) entries -- slice classes
    of the 16-, 20- and 32-entry (seed 0) or 24-entry (seed 1) straight-line instances, none of the looped kernel."""
    w = workloads.config_unstructured(2000, jitter=0.3, seed=seed)
    assert _longest_row(w) == longest and longest <= 32
    h = _open(backend, w)
    assert _check_direct(h, w, w.tables['rho'], what="jittered lattice, seed %d" % seed) == 0
    h.close()


# ---- 2. stepping ----------------------------------------------------------------------------------------------------------

def _run(backend, w, script, **kw):
    h = _open(backend, w, **kw)
    st = script(h)
    c = h.get_state(want_u=False)[0]
    s = h.stats()
    h.close()
    assert st == 0
    return c, s


def _steps(n):
    return lambda h: h.step(n)


def _on_and_off(backend, w, script, flags_or=0, **kw):
    a = _run(backend, w, script, flags_or=flags_or, **kw)
    b = _run(backend, w, script, flags_or=flags_or | backend.FLAG_NO_FUSED_MASS, **kw)
    d = rel_l2(a[0], b[0])
    print("sweeps with the mass product %d (flag: %d), fallback rows %d; Newton %d, sweeps %d; rel-L2 against the flag's run %.3e" %
          (a[1]['rd_mass_in_sweep'], b[1]['rd_mass_in_sweep'], a[1]['rd_mass_fallback_rows'], a[1]['newton_its'],
           a[1]['rd_assemblies'], d))
    assert b[1]['rd_mass_in_sweep'] == 0
    for k in COUNTS:
        assert a[1][k] == b[1][k], (k, a[1][k], b[1][k])
    return a, b, d


@pytest.mark.parametrize("tissues", [2, 3])
def test_eight_steps_against_the_flag(backend, tissues):
    w = _c3_reduced(24) if tissues == 2 else _three_tissues(20)
    a, b, d = _on_and_off(backend, w, _steps(8))
    assert a[1]['rd_mass_in_sweep'] > 0
    assert (a[1]['rd_mass_fallback_rows'] == 0) == (tissues == 2)
    assert d <= TOL_FIELD


def test_int32_columns_on_an_unstructured_mesh(backend):
    """Rows of 16 entries with 32-bit columns, a guess pass and the mass accumulator: the one instance whose first round trip
    takes 25 incidence records instead of 26 (a third wave per SIMD) -- the 26th comes with the second round trip."""
    w = workloads.config_unstructured(2000, jitter=0.3, seed=0)
    a, b, d = _on_and_off(backend, w, _steps(6), flags_or=backend.FLAG_INT32_COLUMNS)
    assert a[1]['rd_mass_in_sweep'] > 0 and a[1]['cheb_fused_passes'] > 0
    assert d <= TOL_FIELD
    c = _run(backend, w, _steps(6), flags_or=backend.FLAG_INT32_COLUMNS | backend.FLAG_NO_FUSED_GUESS)
    assert np.array_equal(a[0], c[0])


# ---- 3. one formula for every b: the same bits however the run is cut --------------------------------------------------------

@pytest.mark.parametrize("dirichlet", [False, True])
def test_chunked_and_restarted_runs_give_the_same_bits(backend, dirichlet):
    """With Dirichlet rows glims_set_state marks the boundary values as to be written into the iterate, so the first b after
    every set_state -- of the restarted run and of the fresh handle alike -- is the SpMV's."""
    w = _three_tissues(20)
    kw = {}
    if dirichlet:
        f = w.mesh.facets()
        bn = np.unique(f['vertices'][f['exterior']])
        kw = dict(dirichlet=(bn, np.full(len(bn), 0.01)))
    c8, s8 = _run(backend, w, _steps(8), **kw)
    assert s8['rd_mass_in_sweep'] > 0

    def one_by_one(h):
        st = 0
        for _ in range(8):
            st |= h.step(1)
        return st
    c1, s1 = _run(backend, w, one_by_one, **kw)
    for k in COUNTS + ('rd_mass_in_sweep',):
        assert s1[k] == s8[k], k
    assert np.array_equal(c1, c8)

    # a run that hands its state back to itself after step 4 (the system the last sweep prepared is dropped: the next step's b
    # comes from the single-right-hand-side sweep) against a fresh handle started from that state
    mid = {}

    def restart(h):
        st = h.step(4)
        mid['c'] = h.get_state(want_u=False)[0]
        h.set_state(mid['c'])
        return st | h.step(4)
    ca, _ = _run(backend, w, restart, **kw)
    w2 = _three_tissues(20)
    w2.c0 = mid['c']
    cb, _ = _run(backend, w2, _steps(4), **kw)
    assert np.array_equal(ca, cb)


def test_fused_guess_pass_still_gives_the_same_bits(backend):
    """Default flags against GLIMS_FLAG_NO_FUSED_GUESS, the mass product in the sweep in both: FG = 0, 1 and 2 instances form
    the same right-hand side."""
    w = _c3_reduced(24)
    a = _run(backend, w, _steps(10))
    b = _run(backend, w, _steps(10), flags_or=backend.FLAG_NO_FUSED_GUESS)
    assert a[1]['cheb_fused_passes'] > 0 and b[1]['cheb_fused_passes'] == 0
    assert a[1]['rd_mass_in_sweep'] > 0 and a[1]['rd_mass_in_sweep'] == b[1]['rd_mass_in_sweep']
    for k in COUNTS + ('cg_its', 'cheb_its'):
        assert a[1][k] == b[1][k], k
    assert np.array_equal(a[0], b[0])


# ---- 4. where the mode stays off ---------------------------------------------------------------------------------------------

def test_off_with_the_fp32_jacobian(backend):
    w = _c3_reduced(20)
    a, b, _ = _on_and_off(backend, w, _steps(6), flags_or=backend.FLAG_FP32_JACOBIAN)
    assert a[1]['rd_mass_in_sweep'] == 0
    assert np.array_equal(a[0], b[0])
    h = _open(backend, w, flags_or=backend.FLAG_FP32_JACOBIAN)
    with pytest.raises(backend.BackendError):
        h.apply(10, w.c0)
    h.close()


def test_off_with_a_looped_slice_class(backend):
    """3 000 random points, Delaunay: rows of up to 36 entries -- a class of the looped sweep kernel, the SpMV everywhere."""
    w = workloads.config_unstructured(3000, seed=0)
    assert _longest_row(w) > 32
    a, b, _ = _on_and_off(backend, w, _steps(6))
    assert a[1]['rd_mass_in_sweep'] == 0
    assert np.array_equal(a[0], b[0])


def test_extrapolated_guess_keeps_the_spmv_for_the_first_b(backend):
    """GLIMS_FLAG_EXTRAPOLATE_GUESS moves the iterate between the mass product and the step's first sweep: that b keeps the
    SpMV on the old state; other sweeps may still form theirs."""
    w = _c3_reduced(20)
    a, b, d = _on_and_off(backend, w, _steps(8), flags_or=backend.FLAG_EXTRAPOLATE_GUESS)
    assert d <= TOL_FIELD


def test_new_dirichlet_values_between_steps(backend):
    """New boundary values enter the iterate after b = M c^n was formed: the step after them forms b with the SpMV, on the old
    state (a sweep at the new iterate would put the new values into b)."""
    w = _c3_reduced(20)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])

    def script(h):
        st = h.step(4)
        h.set_dirichlet_c(bn, np.full(len(bn), 0.02))
        return st | h.step(4)
    a, b, d = _on_and_off(backend, w, script, dirichlet=(bn, np.full(len(bn), 0.01)))
    assert a[1]['rd_mass_in_sweep'] > 0
    assert np.all(a[0][bn] == 0.02)
    assert d <= TOL_FIELD


def test_the_step_after_set_dirichlet_c_assembles_once_more_without_the_product(backend):
    """The SAME boundary values set again after step 4 (every solve from zero, so that the dropped warm start changes nothing):
    the iterate does not move, but the system the last sweep prepared is dropped and the values count as new -- step 5 forms
    b = M c^n with the SpMV and runs one sweep that the continuous run does not: one more assembly, no more sweeps with the
    mass product, the same Newton iterations."""
    w = _c3_reduced(20)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    val = np.full(len(bn), 0.01)

    def again(h):
        st = h.step(4)
        h.set_dirichlet_c(bn, val)
        return st | h.step(4)

    def straight(h):
        return h.step(4) | h.step(4)
    kw = dict(dirichlet=(bn, val), flags_andnot=backend.FLAG_WARM_START)
    a = _run(backend, w, again, **kw)
    c = _run(backend, w, straight, **kw)
    print("values set again: %d sweeps, %d with the mass product, Newton %d; continuous: %d, %d, %d; rel-L2 %.3e" %
          (a[1]['rd_assemblies'], a[1]['rd_mass_in_sweep'], a[1]['newton_its'], c[1]['rd_assemblies'],
           c[1]['rd_mass_in_sweep'], c[1]['newton_its'], rel_l2(a[0], c[0])))
    assert c[1]['rd_mass_in_sweep'] > 0
    assert a[1]['newton_its'] == c[1]['newton_its']
    assert a[1]['rd_assemblies'] == c[1]['rd_assemblies'] + 1
    assert a[1]['rd_mass_in_sweep'] == c[1]['rd_mass_in_sweep']
    assert rel_l2(a[0], c[0]) <= TOL_FIELD


# ---- 5. materials changed between two set-ups --------------------------------------------------------------------------------

def test_materials_changed_between_setups(backend):
    w = _c3_reduced(8)
    t = w.tables
    h = _open(backend, w)
    assert _check_direct(h, w, t['rho'], what="rho equal") == 0
    rho2 = list(t['rho'])
    rho2[workloads.WM] = 0.08
    h.set_materials(t['D'], rho2, t['gamma'], t['E'], t['nu'])
    h.setup(False)
    h.set_state(w.c0)
    n_fb = _check_direct(h, w, rho2, what="rho of white matter changed")
    assert 0 < n_fb < len(w.mesh.points)
    assert h.step(2) == 0 and h.stats()['rd_mass_in_sweep'] > 0
    h.close()
