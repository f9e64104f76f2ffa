"""
The quadratic-term pass (k_rd_quad_s / k_rd_quad: r <- r - dt N(a) delta and the slice sums of |r|^2) as an operator against the
float64 reference of tests/quad_pass_common.py, row by row inside the derived bound
    reps dt (R_i + 3 NV + 5) 2^-24 Q_i + 4 x 2^-53 |y_i|,
through glims_apply(9) (a = delta = x) and glims_apply(11) (a = x + c, delta = x - c, prepared by the stepper's own kernel), with
glims_peek_partials for the slice sums.  The stepper confirms every step with a sweep, so a wrong pass cannot change a result,
only cost iterations: nothing else in the suite would name a wrong slot, a dropped record, a wrong diagonal factor or a slice
sum that counts rows it should not.  tests/test_quad_pass_cpu.py shows that each of those defects leaves the bound.

Every mesh asserts the kernel instances it reaches (the 'glims slice class' lines of GLIMS_VERBOSE) and runs with 16-bit and
with 32-bit columns.  The fan meshes give 2-D rows of 16, 20, 24, 32 and 41 entries: the NV = 3 instances for more than 16
entries, which no rectangle or Delaunay mesh reaches; the second half of the file runs the other incidence-list kernels (the
assembly sweep with its mass product and guess pass, the matrix-free product, the 16-bit slot words) on them against the oracle.

Reference counterpart: the Newton residual of 'F == 0' (simulation_tumor_growth.py:115-120), whose only nonlinear term
'rho * sol1 * (1 - sol1) * v1 * dx' is quadratic -- the form N the pass applies.
"""
import re

import numpy as np
import pytest

from oracle.glims_oracle import OracleTumorGrowth, rel_l2
from quad_pass_common import CASES, FAN_K, LOOPED, U32, case, inputs, pair_of, quad_abs, quad_bound, quad_ref, rho_of
from test_gpu_slot_words16 import _same_bits

pytestmark = pytest.mark.gpu

COUNTS = ('newton_its', 'rd_assemblies', 'rd_quad_updates', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks',
          'cheb_fused_passes', 'rd_mass_in_sweep')
CLASS_LINE = re.compile(r"glims slice class: (\d+) slices \((\d+) interior\) of at most (\d+) entries: (\S+) kernels")
_REF = {}


def _reference(cid, which, k):
    """(ref = N(a) delta, Q, R) of input k of a case, computed once and shared (read only)."""
    key = (cid, k)
    if key not in _REF:
        w = case(cid)
        a, d = pair_of(which, inputs(w)[k][2], w.c0)
        ref = quad_ref(w.mesh.points, w.mesh.cells, rho_of(w), a, d)
        Q, R = quad_abs(w.mesh.points, w.mesh.cells, rho_of(w), a, d)
        for v in (ref, Q, R):
            v.setflags(write=False)
        _REF[key] = (ref, Q, R)
    return _REF[key]


def _exterior(w):
    f = w.mesh.facets()
    return np.unique(f['vertices'][f['exterior']])


def _open(backend, w, int32=False, state=True, dirichlet=None, load=None, flags_or=0):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    h.set_options(dt=w.dt, flags=h.options.flags | flags_or | (backend.FLAG_INT32_COLUMNS if int32 else 0))
    if dirichlet is not None:
        h.set_dirichlet_c(dirichlet, np.full(len(dirichlet), 0.01))
    if load is not None:
        h.set_rd_load(load)
    h.setup(False)
    if state:
        h.set_state(w.c0)
    return h


def _instances(err_text):
    """The kernel instances of the handle's slice classes: the unroll bound (16 / 20 / 24 / 32) of a straight-line class, LOOPED
    otherwise; the printed kind must agree with the class's longest row."""
    out = set()
    found = CLASS_LINE.findall(err_text)
    assert found, "no 'glims slice class' line"
    for _, _, cap, kind in found:
        cap = int(cap)
        assert kind == ("straight-line" if cap <= 32 else "looped"), (cap, kind)
        out.add(next((c for c in (16, 20, 24, 32) if cap <= c), LOOPED))
    return out, sorted(int(c[2]) for c in found)


def _check_slice_sums(h, y):
    """partials[.][0] summed over the slices = sum of y_i^2 over the returned rows (the same non-negative terms in another
    order: the deviation is at most n 2^-53 relative); the second column is written as 0."""
    p = h.peek_partials()
    s = float(np.sum(y * y))
    assert p[1] == 0.0
    assert abs(p[0] - s) <= 1e-12 * s, (p[0], s)


def _check_pass(h, cid, fixed=None):
    """Hooks 9 and 11, reps 1 and 2, row by row against the reference; returns the largest err / (reps dt 2^-24 Q_i)."""
    w = case(cid)
    n, dim = len(w.mesh.points), w.mesh.points.shape[1]
    free = np.ones(n, dtype=bool)
    if fixed is not None:
        free[fixed] = False
    worst = 0.0
    for k, (which, what, x) in enumerate(inputs(w)):
        ref, Q, R = _reference(cid, which, k)
        for reps in (1, 2):       # (the second repetition reads a non-zero r)
            y = h.apply(which, x, reps=reps)[0]
            assert np.all(np.isfinite(y)) and np.abs(y).max() > 0.0
            err = np.abs(y + reps * w.dt * ref)
            bound = quad_bound(dim, reps, w.dt, Q, R, y)
            m = free & (Q > 0.0)
            ratio = (err[m] / (reps * w.dt * U32 * Q[m])).max()
            worst = max(worst, ratio)
            print("%s, which = %d (%s), reps %d: largest err / (reps dt 2^-24 Q_i) = %.3f, smallest bound %.1f" %
                  (w.name, which, what, reps, ratio, (R[m] + 3 * (dim + 1) + 5).min()))
            assert np.all(err[free] <= bound[free]), (which, what, reps, int(np.argmax(np.where(free, err - bound, -np.inf))))
            assert np.all(y[~free] == 0.0)                       # Dirichlet rows: exactly 0
            assert np.all(y[free & (Q == 0.0)] == 0.0)           # rows whose cells all have rho = 0
            _check_slice_sums(h, y)
    return worst


@pytest.mark.parametrize("int32", [False, True], ids=["cols16", "cols32"])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_pass_against_the_reference(backend, monkeypatch, capfd, cid, int32):
    monkeypatch.setenv("GLIMS_VERBOSE", "1")
    w = case(cid)
    h = _open(backend, w, int32)
    worst = _check_pass(h, cid)
    h.close()
    text = capfd.readouterr()
    inst, caps = _instances(text.err)
    print(text.out, end="")
    print("%s (%s columns): classes of at most %s entries -> instances %s; largest err / (reps dt 2^-24 Q_i) = %.3f" %
          (w.name, "32-bit" if int32 else "16-bit", caps, sorted(inst, key=str), worst))
    assert inst == CASES[cid][1], (inst, CASES[cid][1])
    if cid == 'random_1000':
        assert LOOPED not in inst and max(caps) == 32
    if cid == 'random_3000':
        assert max(caps) > 32
    if cid == 'c3_n8':
        assert len(w.mesh.points) % 64 != 0          # ragged last slice


@pytest.mark.parametrize("int32", [False, True], ids=["cols16", "cols32"])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_dirichlet_rows_are_zero_and_not_counted(backend, cid, int32):
    w = case(cid)
    bn = _exterior(w)
    assert 0 < len(bn) < len(w.mesh.points)
    h = _open(backend, w, int32, dirichlet=bn)
    assert np.array_equal(h.get_state(want_u=False)[0], w.c0)      # (the values enter the iterate with the next step)
    _check_pass(h, cid, fixed=bn)
    h.close()


@pytest.mark.parametrize("cid", sorted(CASES))
def test_sweep_slice_sums_without_a_state(backend, cid):
    w = case(cid)
    x = inputs(w)[0][2]
    h = _open(backend, w, state=False)
    y = h.apply(8, x)[0]
    assert np.abs(y).max() > 0.0
    _check_slice_sums(h, y)
    h.close()
    bn = _exterior(w)
    h = _open(backend, w, state=False, dirichlet=bn)
    y = h.apply(8, x)[0]
    assert np.all(y[bn] == 0.0) and np.abs(y).max() > 0.0
    _check_slice_sums(h, y)
    h.close()


@pytest.mark.parametrize("int32", [False, True], ids=["cols16", "cols32"])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_hooks_are_neutral(backend, cid, int32):
    """apply(0) gives the same bits before and after hooks 9 and 11, and three steps after them the same bits and counts as on
    a handle that never ran them."""
    w = case(cid)
    x = inputs(w)[1][2]
    fresh = _open(backend, w, int32)
    assert fresh.step(3) == 0
    c_fresh, s_fresh = fresh.get_state(want_u=False)[0], fresh.stats()
    fresh.close()
    h = _open(backend, w, int32)
    h.rd_residual(w.c0, w.c0)            # assembles A(c)
    before = h.apply(0, x)[0]
    h.apply(9, x, reps=2)
    h.apply(11, x, reps=2)
    assert np.array_equal(h.apply(0, x)[0], before)
    assert np.array_equal(h.get_state(want_u=False)[0], w.c0)
    assert h.step(3) == 0
    c, s = h.get_state(want_u=False)[0], h.stats()
    h.close()
    assert np.array_equal(c, c_fresh)
    for k in COUNTS:
        assert s[k] == s_fresh[k], (k, s[k], s_fresh[k])


def test_misuse(backend):
    w = case('fan15')
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    with pytest.raises(backend.BackendError) as ei:
        h.peek_partials()
    assert ei.value.code == backend.GLIMS_E_USAGE and "glims_setup" in str(ei.value)
    h.close()
    h = _open(backend, w, state=False)
    x = inputs(w)[0][2]
    with pytest.raises(backend.BackendError) as ei:
        h.apply(11, x)
    assert ei.value.code == backend.GLIMS_E_USAGE and "needs the state" in str(ei.value)
    with pytest.raises(backend.BackendError) as ei:
        h.apply(13, x)
    assert ei.value.code == backend.GLIMS_E_USAGE and "unknown operator" in str(ei.value)
    h.apply(9, x)                          # no state needed
    h.set_state(w.c0)
    h.apply(11, x)
    h.close()


# ---- 2-D rows of more than 16 entries through the other incidence-list kernels ---------------------------------------------------

def _oracle(w, load=None):
    return OracleTumorGrowth(w.mesh.points, w.mesh.cells, w.per_cell('D'), w.per_cell('rho'), w.per_cell('gamma'),
                             w.per_cell('E'), w.per_cell('nu'), w.dt, rd_load=load)


@pytest.mark.parametrize("int32", [False, True], ids=["cols16", "cols32"])
@pytest.mark.parametrize("k", FAN_K)
def test_fan_mesh_operators_match_the_oracle(backend, k, int32):
    """1e-13: the suite's tolerance for operators on unstructured meshes (tests/test_gpu_parity.py)."""
    w = case('fan%d' % k)
    n = len(w.mesh.points)
    rng = np.random.default_rng(k)
    x, c, cp = rng.standard_normal(n), rng.random(n), rng.random(n)
    load = 0.05 * np.cos(3.0 * w.mesh.points[:, 0]) * (1.0 + w.mesh.points[:, 1] ** 2)
    o = _oracle(w, load)
    h = _open(backend, w, int32, state=False, load=load)
    assert rel_l2(h.apply(2, x)[0], o.M @ x) < 1e-13
    assert rel_l2(h.apply(1, x)[0], o.S @ x) < 1e-13
    assert rel_l2(h.apply(8, x)[0], -0.5 * ((o.rd_jacobian(x) + o.S) @ x)) < 1e-13
    assert rel_l2(h.rd_residual(c, cp), o.rd_residual(c, cp)) < 1e-13
    h.set_state(c)
    h.rd_residual(c, c)                    # assembles A(c)
    ya = h.apply(0, x)[0]
    assert rel_l2(ya, o.rd_jacobian(c) @ x) < 1e-13
    assert rel_l2(h.apply(7, x)[0], ya) < 1e-14          # (test_matrix_free_product_equals_the_assembled_one's)
    assert rel_l2(h.apply(8, x)[0], -0.5 * ((o.rd_jacobian(x) + o.S) @ x)) < 1e-13
    assert np.array_equal(h.apply(0, x)[0], ya)          # hook 8 has put A(c) back
    if k <= 31:       # every class straight-line: the sweep forms the mass product
        assert rel_l2(h.apply(10, x)[0], o.M @ x + load) < 1e-13
        assert h.stats()['rd_mass_fallback_rows'] > 0    # mixed tissues at the hub
    else:
        with pytest.raises(backend.BackendError):
            h.apply(10, x)
    h.close()


@pytest.mark.parametrize("k", FAN_K)
def test_fan_mesh_slot_words_give_the_same_bits(backend, k):
    w = case('fan%d' % k)
    a = _same_bits(backend, w, 4, w.name, mass_hook=k <= 31)
    if k <= 31:
        assert a[1]['rd_mass_in_sweep'] > 0
    else:             # the looped class keeps the 32-bit words and the mass SpMV; the straight-line class reads cs16
        assert a[1]['rd_mass_in_sweep'] == 0 and a[1]['rd_slot16_sweeps'] > 0
