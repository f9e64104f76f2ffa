"""
The pass count of a folded warm-started dot-free solve comes from the host.  Such a solve's first pass ran in the assembly sweep
before it (k_rd_assemble_sg, FG = 1), so the norm its count follows from, |b - A u|^2, is a per-slice sum of that sweep: it is
reduced in the sweep's own reduce chain, arrives in the same mail as the two residual norms, and the host evaluates the count
expression the device's k_cheb_plan evaluates (gl_cheb_count) -- no second reduction, no plan kernel, no launch that returns at
once.  glims_stats.cheb_host_counts counts these solves.  Every other warm-started solve (unfolded; partitioned handles) keeps
the device-side count.  How the count is obtained must not show: bits and counts equal those of GLIMS_FLAG_NO_FUSED_GUESS,
whose solves all plan on the device, and a run gives the same bits however it is cut into calls.

Reference counterpart: none of its own -- the linear solves stand in for the KSP behind `self.solver.solve()`
(simulation_base.py:302).
"""
import importlib.util
import os

import numpy as np
import pytest

from glimslib_amd import workloads
from oracle.glims_oracle import rel_l2

pytestmark = pytest.mark.gpu

TOL_PATHS = 1e-9      # dot-free against PCG (test_gpu_chebyshev.py)
TOL_RANKS = 1e-10     # partitioned against single-rank concentration (test_gpu_multirank.py)
COUNTS = ('newton_its', 'rd_assemblies', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks', 'rd_mass_in_sweep',
          'rd_quad_updates')


def _c3_reduced(n):
    w = workloads.config_c3(n)
    hx = 240.0 / n
    w.c0 = np.exp(-((w.mesh.points - np.array([118.0, -109.0, 72.0])) ** 2).sum(axis=1) / (2.0 * (2.5 * hx) ** 2))
    return w


def _open(backend, w, flags_or=0, flags_andnot=0, **opts):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    opts.setdefault('dt', w.dt)
    h.set_options(flags=(h.options.flags | flags_or) & ~flags_andnot, **opts)
    h.setup(False)
    h.set_state(w.c0)
    return h


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


@pytest.fixture(scope="module")
def sixteen(backend):
    """_c3_reduced(24), 16 steps in one call: default flags, and with GLIMS_FLAG_NO_FUSED_GUESS.  Shared, never modified."""
    w = _c3_reduced(24)
    return w, _run(backend, w, _steps(16)), _run(backend, w, _steps(16), flags_or=backend.FLAG_NO_FUSED_GUESS)


def test_sixteen_steps_against_the_device_side_counts(backend, sixteen):
    w, a, b = sixteen
    print("default: host counts %d, folded passes %d, dot-free solves %d, passes %d, Newton %d; flag: host counts %d; "
          "difference %.3e" % (a[1]['cheb_host_counts'], a[1]['cheb_fused_passes'], a[1]['cheb_solves'], a[1]['cheb_its'],
                               a[1]['newton_its'], b[1]['cheb_host_counts'], rel_l2(a[0], b[0])))
    assert a[1]['cheb_host_counts'] > 0
    assert b[1]['cheb_host_counts'] == 0 and b[1]['cheb_fused_passes'] == 0
    for k in COUNTS:
        assert a[1][k] == b[1][k], (k, a[1][k], b[1][k])
    assert np.array_equal(a[0], b[0])


def test_host_counts_are_the_folded_passes_of_warm_started_solves(backend, sixteen):
    """Step by step: a folded pass is either a guess pass (the host then chooses the count) or a start from zero (a count the
    host always knew; glims_stats.cheb_fused_zero_starts).  So in every step host counts = folded passes - folded starts from
    zero; in a steady step -- both solves start from a guess -- host counts and folded passes are both 2, and 1 in a step where
    the midpoint correction leaves only the second solve folded; with GLIMS_FLAG_WARM_START cleared every folded pass is a
    start from zero: no host count at all.  Sixteen calls of step(1) give the bits and counts of one call of step(16)."""
    w, a, _ = sixteen
    h = _open(backend, w)
    prev, per_step = h.stats(), []
    for _ in range(16):
        assert h.step(1) == 0
        s = h.stats()
        per_step.append((s['cheb_host_counts'] - prev['cheb_host_counts'], s['cheb_fused_passes'] - prev['cheb_fused_passes'],
                         s['midpoint_steps'] - prev['midpoint_steps'],
                         s['cheb_fused_zero_starts'] - prev['cheb_fused_zero_starts']))
        prev = s
    c = h.get_state(want_u=False)[0]
    h.close()
    print("per step (host counts, folded passes, midpoint correction, folded starts from zero):", per_step)
    assert all(hc >= 0 and z >= 0 and hc == f - z for hc, f, _, z in per_step)
    assert any(hc == 2 == f for hc, f, mid, _ in per_step if not mid)      # a steady step: both solves start from a guess
    assert any(hc == 1 == f for hc, f, mid, _ in per_step if mid)          # ... the second solve's pass is still folded there
    assert any(z > 0 for _, _, _, z in per_step)                            # (and both kinds of folded pass occur in the run)
    for k in COUNTS + ('cheb_fused_passes', 'cheb_host_counts'):
        assert prev[k] == a[1][k], k
    assert np.array_equal(c, a[0])

    cz, sz = _run(backend, w, _steps(10), flags_andnot=backend.FLAG_WARM_START)
    assert sz['cheb_fused_passes'] > 0 and sz['cheb_host_counts'] == 0
    assert sz['cheb_fused_zero_starts'] == sz['cheb_fused_passes']


def test_restarted_run_gives_the_bits_of_a_fresh_handle(backend):
    """A run that hands its state back to itself after step 8 (the payload of the next step's first solve, its norm included,
    is dropped with the system the last sweep prepared) against a fresh handle started from that state.  glims_set_state
    starts the stepper's run memory afresh, so the second half also takes the fresh handle's iteration path: every integer
    counter of glims_stats grows by what the fresh handle's grows by (folded passes and folded starts from zero included:
    they depend on what the previous run's second solves were asked for, if that is not forgotten)."""
    w = _c3_reduced(24)
    mid = {}

    def restart(h):
        st = h.step(8)
        mid['c'] = h.get_state(want_u=False)[0]
        h.set_state(mid['c'])
        mid['s'] = h.stats()            # (glims_set_state starts the count of steps afresh; the other counters go on)
        return st | h.step(8)
    ca, sa = _run(backend, w, restart)
    w2 = _c3_reduced(24)
    w2.c0 = mid['c']

    def fresh(h):
        mid['s0'] = h.stats()
        return h.step(8)
    cb, sb = _run(backend, w2, fresh)
    print("restarted: host counts %d; fresh handle from the state of step 8: %d" % (sa['cheb_host_counts'], sb['cheb_host_counts']))
    assert sa['cheb_host_counts'] > 0
    assert np.array_equal(ca, cb)
    ints = [k for k in sorted(sa) if isinstance(sa[k], (int, np.integer)) and not isinstance(sa[k], bool)]
    second, alone = {k: sa[k] - mid['s'][k] for k in ints}, {k: sb[k] - mid['s0'][k] for k in ints}
    print("second half:", {k: v for k, v in second.items() if v}, "\nfresh handle:", {k: v for k, v in alone.items() if v})
    assert len(ints) > 30 and second['steps'] == 8 and second['newton_its'] > 0
    for k in ints:
        if k == 'rd_precond_used':      # (not a counter: what `auto` settled on, which glims_set_state keeps on purpose)
            assert sa[k] == sb[k]
        else:
            assert second[k] == alone[k], (k, second[k], alone[k])


def test_take_back_then_the_device_plans_again(backend, monkeypatch):
    """TEST HOOK GLIMS_CHEB_TEST_SCALE_HI = 0.45 (tests/test_gpu_chebyshev.py; read when the handle is created): solves are
    taken back, the next step measures the interval again with PCG solves (a learning step), and the step after that has no
    payload from a sweep -- its warm-started first solve is unfolded and plans on the device.  Step by step: the step after a
    take-back adds no host count; neither does the step after a learning step, although it runs dot-free solves (unless it had
    to learn again itself).  The run agrees with the flag's run (whose counts are all the device's) in bits and counts and
    lands on the PCG path's field."""
    w = _c3_reduced(24)
    cp, _ = _run(backend, w, _steps(10), rd_linear=backend.RD_LINEAR_PCG)
    monkeypatch.setenv("GLIMS_CHEB_TEST_SCALE_HI", "0.45")
    per_step = []

    def one_by_one(h):
        st, prev = 0, h.stats()
        for _ in range(10):
            st |= h.step(1)
            s = h.stats()
            per_step.append(tuple(s[k] - prev[k] for k in ('cheb_fallbacks', 'cheb_learn_solves', 'cheb_host_counts', 'cheb_solves')))
            prev = s
        return st
    a = _run(backend, w, one_by_one)
    b = _run(backend, w, _steps(10), flags_or=backend.FLAG_NO_FUSED_GUESS)
    monkeypatch.delenv("GLIMS_CHEB_TEST_SCALE_HI")
    print("wrong interval: take-backs %d, host counts %d, folded passes %d, dot-free solves %d; against PCG %.3e" %
          (a[1]['cheb_fallbacks'], a[1]['cheb_host_counts'], a[1]['cheb_fused_passes'], a[1]['cheb_solves'], rel_l2(a[0], cp)))
    print("per step (take-backs, learning solves, host counts, dot-free solves):", per_step)
    assert a[1]['cheb_fallbacks'] >= 1
    after_take_back = [now for before, now in zip(per_step[:-1], per_step[1:]) if before[0] > 0]
    after_learning = [now for before, now in zip(per_step[:-1], per_step[1:]) if before[1] > 0 and now[1] == 0]
    assert after_take_back and after_learning
    assert all(now[2] == 0 for now in after_take_back)
    assert all(now[2] == 0 and now[3] > 0 for now in after_learning)
    assert b[1]['cheb_host_counts'] == 0
    for k in COUNTS:
        assert a[1][k] == b[1][k], (k, a[1][k], b[1][k])
    assert np.array_equal(a[0], b[0])
    assert rel_l2(a[0], cp) < TOL_PATHS


def test_partitioned_handles_keep_the_device_side_count(backend):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rehearse_partition", os.path.join(root, "tools", "rehearse_partition.py"))
    rp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rp)
    w = _c3_reduced(20)
    s_1, c_1, _, st_1 = rp.run_single(w, 8, 0, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    s, c, _, ss = rp.run_partitioned(w, 2, 8, 0, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    print("2 ranks: host counts %s (single rank %d); vs single %.2e" %
          ([int(x['cheb_host_counts']) for x in ss], st_1['cheb_host_counts'], rel_l2(c, c_1)))
    assert s == 0 and s_1 == 0
    assert st_1['cheb_host_counts'] > 0
    assert all(x['cheb_host_counts'] == 0 and x['cheb_solves'] > 0 for x in ss)
    assert rel_l2(c, c_1) < TOL_RANKS
