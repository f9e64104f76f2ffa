"""
The first pass of a dot-free solve folded into the assembly sweep before it (k_rd_assemble_sg): the guess pass of a step's first
and second solve, or the start of a solve from zero, computed on the row of A(c) the sweep has just formed instead of by a
launch that streams the Jacobian again.  The sweep's extra output is speculative -- formed before it is known whether the solve
will want it -- so the cases here are about two things: the folded pass writes the bits the separate launch writes, and a
payload that no longer fits (another interval, another guess, a new state) is dropped.  Each case runs the same build with and
without GLIMS_FLAG_NO_FUSED_GUESS through the C-ABI handle and asks for the same bits and the same counts.

Reference counterpart: none of its own -- the linear solves stand in for the KSP behind `self.solver.solve()`
(simulation_base.py:302); how their first operator pass is scheduled must not show in any result.
"""
import os

import numpy as np
import pytest

from glimslib_amd import workloads
from oracle.glims_oracle import rel_l2

pytestmark = pytest.mark.gpu

TOL_PATHS = 1e-9      # dot-free against PCG (test_gpu_chebyshev.py)
TOL_RANKS = 1e-10     # partitioned against single-rank concentration (test_gpu_multirank.py)
COUNTS = ('newton_its', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks', 'rd_assemblies', 'rd_quad_updates')


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


def _steps(n):
    def script(h):
        return h.step(n)
    return script


def _both(backend, w, script, flags_or=0, **kw):
    """The same script on a handle with default flags and on one with the separate launches: (field, stats) of each."""
    out = []
    for off in (0, backend.FLAG_NO_FUSED_GUESS):
        h = _open(backend, w, flags_or=off | flags_or, **kw)
        st = script(h)
        c = h.get_state(want_u=False)[0]
        s = h.stats()
        h.close()
        assert st == 0
        out.append((c, s))
    return out


def _same(a, b, what=""):
    (c1, s1), (c0, s0) = a, b
    print("%s: folded passes %d (flag: %d), dot-free solves %d, passes %d, Newton %d, sweeps %d; difference %.3e" %
          (what, s1['cheb_fused_passes'], s0['cheb_fused_passes'], s1['cheb_solves'], s1['cheb_its'], s1['newton_its'],
           s1['rd_assemblies'], rel_l2(c1, c0)))
    assert s0['cheb_fused_passes'] == 0
    for k in COUNTS:
        assert s1[k] == s0[k], (k, s1[k], s0[k])
    assert np.array_equal(c1, c0)


def test_sixteen_steps_two_folded_passes_per_steady_step(backend):
    """Default flags, 16 steps: the counter grows, by at most one pass per dot-free solve and by two in a steady step (first
    and second solve), stays 0 under the flag, and sixteen calls of step(1) -- the payload of the next step's first solve
    crosses every call boundary -- give the bits and counts of one call of step(16).  On this box the forcing controller
    turns the midpoint correction on after ten steps (steps start taking a third Newton iteration): it changes the first
    right-hand side after the sweep, so those steps' first solves keep their own guess pass and only the second solve's is
    folded -- the counter grows by one per such step at most."""
    w = _c3_reduced(24)
    a, b = _both(backend, w, _steps(16))
    _same(a, b, "16 steps")
    assert a[1]['cheb_fused_passes'] > 0

    h = _open(backend, w)
    prev, per_step = h.stats(), []
    for _ in range(16):
        assert h.step(1) == 0
        s = h.stats()
        per_step.append((s['cheb_fused_passes'] - prev['cheb_fused_passes'], s['cheb_solves'] - prev['cheb_solves'],
                         s['midpoint_steps'] - prev['midpoint_steps']))
        prev = s
    c = h.get_state(want_u=False)[0]
    h.close()
    print("per step (folded passes, dot-free solves, midpoint correction):", per_step)
    for f, n, mid in per_step:
        assert 0 <= f <= min(n, 2 - mid)     # one first pass per solve at most; none for a corrected first right-hand side
    assert any(f == 2 for f, _, mid in per_step if not mid)
    assert any(f == 1 for f, _, mid in per_step if mid)      # (the second solve's pass is still folded there)
    for k in COUNTS + ('cheb_fused_passes',):
        assert prev[k] == a[1][k], k
    assert np.array_equal(c, a[0])


@pytest.mark.parametrize("mesh", ["brain-like", "2-D"])
def test_ragged_slices_and_several_row_length_classes(backend, mesh):
    """An unstructured mesh (a partly filled last slice, rows of many lengths: several CAP classes of the sweep, padded slots in
    most rows) and a 2-D mesh (NV = 3)."""
    w = workloads.config_brain_like(8000, isolate=True) if mesh == "brain-like" else workloads.config_c1()
    a, b = _both(backend, w, _steps(8))
    _same(a, b, mesh)
    assert a[1]['cheb_solves'] > 0 and a[1]['cheb_fused_passes'] > 0


def test_constrained_rows_keep_their_value(backend):
    """Three tissues (one inert), Dirichlet nodes of c at 0.01 and an RD load: constrained rows get t = 0, Dinv = 1 and
    y_1 = u, as in k_cheb."""
    w = _three_tissues(20)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    load = 1e-3 * np.exp(-((w.mesh.points - np.array([100.0, -100.0, 70.0])) ** 2).sum(axis=1) / 400.0)
    kw = dict(dirichlet=(bn, np.full(len(bn), 0.01)), load=load, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    a, b = _both(backend, w, _steps(8), **kw)
    _same(a, b, "three tissues, Dirichlet + load")
    assert a[1]['cheb_fused_passes'] > 0
    assert np.all(a[0][bn] == 0.01)


def test_column_encodings(backend, monkeypatch):
    """16-bit column codes everywhere, int32 columns (flag, or GLIMS_WIN_LIMIT = 0) and a mix with the per-slice fallback
    (GLIMS_WIN_LIMIT = 2): the folded pass decodes what the sweep decodes."""
    w = workloads.config_brain_like(8000, isolate=True)
    ref = None
    for int32, env in ((False, None), (True, None), (False, "2"), (False, "0")):
        monkeypatch.delenv("GLIMS_WIN_LIMIT", raising=False)
        if env is not None:
            monkeypatch.setenv("GLIMS_WIN_LIMIT", env)
        a, b = _both(backend, w, _steps(6), flags_or=backend.FLAG_INT32_COLUMNS if int32 else 0)
        _same(a, b, "int32 %s, GLIMS_WIN_LIMIT %s" % (int32, env))
        assert a[1]['cheb_fused_passes'] > 0
        if ref is None:
            ref = a
        assert np.array_equal(a[0], ref[0]) and a[1]['cheb_fused_passes'] == ref[1]['cheb_fused_passes']
    monkeypatch.delenv("GLIMS_WIN_LIMIT", raising=False)


def test_payload_is_dropped_at_a_learning_step(backend):
    """36 steps: step 33 re-measures the interval with PCG solves (age 32); the sweep before it carries nothing."""
    w = _c3_reduced(20)
    a, b = _both(backend, w, _steps(36))
    _same(a, b, "36 steps")
    assert a[1]['cheb_fused_passes'] > 0 and a[1]['cheb_learn_solves'] >= 2


def test_payload_is_dropped_at_a_take_back(backend, monkeypatch):
    """TEST HOOK GLIMS_CHEB_TEST_SCALE_HI = 0.45: solves are taken back and repeated with PCG; the run lands on the PCG path's
    field, with and without folded passes, and the two agree in every count."""
    w = _c3_reduced(24)
    h = _open(backend, w, rd_linear=backend.RD_LINEAR_PCG)
    assert h.step(10) == 0
    cp = h.get_state(want_u=False)[0]
    h.close()
    monkeypatch.setenv("GLIMS_CHEB_TEST_SCALE_HI", "0.45")
    a, b = _both(backend, w, _steps(10))
    monkeypatch.delenv("GLIMS_CHEB_TEST_SCALE_HI")
    _same(a, b, "wrong interval")
    assert a[1]['cheb_fallbacks'] >= 1
    assert rel_l2(a[0], cp) < TOL_PATHS


@pytest.mark.parametrize("event", ["dirichlet", "set_state", "dt"])
def test_payload_is_dropped_when_the_problem_changes_between_calls(backend, event):
    """New Dirichlet values, a new state or a new dt between two step calls: what the last sweep prepared for the next step is
    not used."""
    w = _c3_reduced(20)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])

    def script(h):
        st = h.step(8)
        if event == "dirichlet":
            h.set_dirichlet_c(bn, np.full(len(bn), 0.02))
        elif event == "set_state":
            h.set_state(0.5 * w.c0)
        else:
            h.set_options(dt=0.5 * w.dt)
            h.setup(False)
        return st | h.step(6)

    kw = dict(dirichlet=(bn, np.full(len(bn), 0.01))) if event == "dirichlet" else {}
    a, b = _both(backend, w, script, **kw)
    _same(a, b, event)
    assert a[1]['cheb_fused_passes'] > 0


def test_fp32_jacobian_keeps_the_separate_launches(backend):
    w = _c3_reduced(20)
    a, b = _both(backend, w, _steps(8), flags_or=backend.FLAG_FP32_JACOBIAN)
    _same(a, b, "fp32 Jacobian")
    assert a[1]['cheb_solves'] > 0 and a[1]['cheb_fused_passes'] == 0


def test_long_rows_keep_the_separate_launches(backend):
    """config_unstructured(6000, seed=1): if a row has more than 32 entries its class takes the looped sweep kernel, and the
    whole handle keeps today's launches."""
    w = workloads.config_unstructured(6000, seed=1)
    nbr = [set() for _ in range(len(w.mesh.points))]
    for cell in w.mesh.cells:
        for v in cell:
            nbr[v].update(cell)
    longest = max(len(s) for s in nbr)
    a, b = _both(backend, w, _steps(6))
    _same(a, b, "unstructured, longest row %d" % longest)
    if longest > 32:
        assert a[1]['cheb_fused_passes'] == 0


def test_partitioned_handles_keep_the_separate_launches(backend):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rehearse_partition", os.path.join(root, "tools", "rehearse_partition.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    w = _c3_reduced(20)
    s_1, c_1, _, st_1 = rp.run_single(w, 8, 0, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    s, c, _, ss = rp.run_partitioned(w, 2, 8, 0, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    print("2 ranks: folded passes %s (single rank %d); vs single %.2e" %
          ([int(x['cheb_fused_passes']) for x in ss], st_1['cheb_fused_passes'], rel_l2(c, c_1)))
    assert s == 0 and s_1 == 0
    assert st_1['cheb_fused_passes'] > 0 and all(x['cheb_fused_passes'] == 0 and x['cheb_solves'] > 0 for x in ss)
    assert rel_l2(c, c_1) < TOL_RANKS


def test_solves_from_zero_take_their_start_from_the_sweep(backend):
    """GLIMS_FLAG_WARM_START cleared: every solve starts from zero; the sweep's variant without a gather stands in for
    k_cheb_start."""
    w = _c3_reduced(24)
    a, b = _both(backend, w, _steps(10), flags_andnot=backend.FLAG_WARM_START)
    _same(a, b, "from zero")
    assert a[1]['cheb_solves'] > 0 and a[1]['cheb_fused_passes'] > 0
