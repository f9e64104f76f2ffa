"""
The dot-free Krylov pass without a Dinv stream and without a direction stream (k_cheb): Dinv_row = 1 / A_ii from the diagonal
entry the row has just read, and the previous direction as the difference of the last two iterates, d = y_in - y_prev, where
y_prev is the buffer the pass is about to overwrite -- except in pass 2, where it is the guess the solve started from (or
nothing, for a start from zero).  One case per branch that this adds, each through the C-ABI handle and against the PCG path
of the same build (rd_linear = PCG) at the tolerance of "another iteration path, same field" (test_gpu_chebyshev.py: 1e-9).

Reference counterpart: the KSP behind `self.solver.solve()` (simulation_base.py:302): its sparse LU is exact, so every Krylov
variant must land on the same Newton fixed point.
"""
import os

import numpy as np
import pytest

from glimslib_amd import workloads
from oracle.glims_oracle import rel_l2

pytestmark = pytest.mark.gpu

TOL_PATHS = 1e-9      # dot-free against PCG (test_gpu_chebyshev.py)
TOL_FP32 = 1e-6       # the project's end-to-end tolerance on the concentration
TOL_RANKS = 1e-10     # partitioned against single-rank concentration (test_gpu_multirank.py)


def _c3_reduced(n):
    w = workloads.config_c3(n)
    hx = 240.0 / n
    w.c0 = np.exp(-((w.mesh.points - np.array([118.0, -109.0, 72.0])) ** 2).sum(axis=1) / (2.0 * (2.5 * hx) ** 2))
    return w


def _default_flags(backend, w):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    flags = h.options.flags
    h.close()
    return flags


def _run(backend, w, steps, dirichlet=None, load=None, dt=None, per_step=False, **opts):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    h.set_options(dt=w.dt if dt is None else dt, **opts)
    if dirichlet is not None:
        h.set_dirichlet_c(dirichlet[0], dirichlet[1])
    if load is not None:
        h.set_rd_load(load)
    h.setup(False)
    h.set_state(w.c0)
    trace = []
    if per_step:
        st, prev = 0, h.stats()
        for _ in range(steps):
            st |= h.step(1)
            s = h.stats()
            trace.append({k: s[k] - prev[k] for k in ('newton_its', 'cheb_solves', 'cheb_its', 'cheb_learn_solves')})
            prev = s
    else:
        st = h.step(steps)
    c = h.get_state(want_u=False)[0]
    s = h.stats()
    h.close()
    return (st, c, s, trace) if per_step else (st, c, s)


def test_solves_from_zero_have_no_previous_iterate_in_pass_2(backend):
    """GLIMS_FLAG_WARM_START cleared: every dot-free solve starts from zero, the start kernel writes y_1 only and pass 2 takes
    d_1 = y_1 (y_prev null); from pass 3 on the direction comes from the buffer being overwritten."""
    w = _c3_reduced(24)
    flags = _default_flags(backend, w) & ~backend.FLAG_WARM_START
    s1, c1, st1 = _run(backend, w, 10, flags=flags)
    s2, c2, st2 = _run(backend, w, 10, flags=flags, rd_linear=backend.RD_LINEAR_PCG)
    print("from zero: Chebyshev solves %d, passes %d, fallbacks %d; vs PCG %.2e" %
          (st1['cheb_solves'], st1['cheb_its'], st1['cheb_fallbacks'], rel_l2(c1, c2)))
    assert s1 == 0 and s2 == 0
    assert st1['cheb_solves'] > 0 and st1['cheb_fallbacks'] == 0 and st2['cheb_solves'] == 0
    assert st1['cheb_its'] > 2 * st1['cheb_solves']     # (solves long enough to reach the passes that read y_out back)
    assert rel_l2(c1, c2) < TOL_PATHS


def test_guessed_solves_take_the_guess_as_previous_iterate(backend):
    """Default flags, 16 steps: the first solve of a step starts from the extrapolated increment and the second from the
    extrapolated second correction (both in cg_u: y_prev = warm_u in pass 2).  That the guesses engaged shows in the counts:
    fewer passes than the same run without them."""
    w = _c3_reduced(28)
    flags = _default_flags(backend, w)
    s1, c1, st1 = _run(backend, w, 16)
    s0, c0, st0 = _run(backend, w, 16, flags=flags & ~backend.FLAG_WARM_START)
    s2, c2, st2 = _run(backend, w, 16, rd_linear=backend.RD_LINEAR_PCG)
    print("guesses: Chebyshev solves %d, passes %d (without guesses %d), fallbacks %d; vs PCG %.2e, vs no guesses %.2e" %
          (st1['cheb_solves'], st1['cheb_its'], st0['cheb_its'], st1['cheb_fallbacks'], rel_l2(c1, c2), rel_l2(c1, c0)))
    assert s1 == 0 and s0 == 0 and s2 == 0
    assert st1['cheb_solves'] > 0 and st1['cheb_fallbacks'] == 0
    assert st1['cg_its'] < st0['cg_its']
    assert rel_l2(c1, c2) < TOL_PATHS


def test_a_guessed_solve_of_two_passes_reads_the_guess_in_its_final_pass(backend):
    """A small, mass-dominated step (dt = 0.02: Dinv A within a few per mille of the identity): the device sizes the step's
    first, guessed solve at m = 2, so that pass 2 -- the one that takes y_prev from the guess -- is also the pass that adds the
    correction to the iterate and keeps it in ylast.  The count of that solve alone: the same run up to step 6, then one step
    limited to a single Newton iteration (newton_maxit = 1) -- one dot-free solve, two passes."""
    w = _c3_reduced(20)
    s1, c1, st1, tr = _run(backend, w, 12, dt=0.02, per_step=True)
    s2, c2, st2 = _run(backend, w, 12, dt=0.02, rd_linear=backend.RD_LINEAR_PCG)
    for i, d in enumerate(tr):
        print("step %2d: Newton %d, Chebyshev solves %d, passes %d, learning solves %d" %
              (i + 1, d['newton_its'], d['cheb_solves'], d['cheb_its'], d['cheb_learn_solves']))
    print("two-pass solves: vs PCG %.2e" % rel_l2(c1, c2))
    assert s1 == 0 and s2 == 0
    assert st1['cheb_solves'] > 0 and st1['cheb_fallbacks'] == 0
    assert rel_l2(c1, c2) < TOL_PATHS

    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    h.set_options(dt=0.02)
    h.setup(False)
    h.set_state(w.c0)
    assert h.step(6) == 0
    s_a = h.stats()
    h.set_options(newton_maxit=1)
    h.step(1)                       # (a step of one Newton iteration does not meet the tolerance: the status is not the point)
    s_b = h.stats()
    h.close()
    d = {k: s_b[k] - s_a[k] for k in ('newton_its', 'cheb_solves', 'cheb_its', 'cheb_learn_solves')}
    print("step 7 cut after its first solve: %s" % d)
    assert d['newton_its'] == 1 and d['cheb_learn_solves'] == 0
    assert d['cheb_solves'] == 1 and d['cheb_its'] == 2


def _three_tissues(n):
    """Reduced C3 with a third, inert tissue (CSF: D = rho = 0) on one side and a white matter forty times as diffusive: rows
    whose diagonal is the mass term alone next to rows dominated by diffusion."""
    w = _c3_reduced(n)
    mid = w.mesh.cell_midpoints()
    w.cell_label = np.where(mid[:, 0] < 70.0, workloads.CSF, w.cell_label).astype(np.int32)
    w.tables = {k: list(v) for k, v in w.tables.items()}
    w.tables['D'][workloads.WM] = 2.0
    assert w.tables['D'][workloads.CSF] == 0.0 and w.tables['rho'][workloads.CSF] == 0.0
    return w


def test_constrained_rows_and_a_strongly_varying_diagonal(backend):
    """Dirichlet nodes of c (rows the operator pass masks: their stored diagonal is not what the sweep's Dinv array holds), an
    RD load and three tissues, one inert and one with large D: 1 / A_ii from the streamed diagonal against the PCG path, which
    still reads the array."""
    w = _three_tissues(20)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    load = 1e-3 * np.exp(-((w.mesh.points - np.array([100.0, -100.0, 70.0])) ** 2).sum(axis=1) / 400.0)
    bc = (bn, np.full(len(bn), 0.01))
    s1, c1, st1 = _run(backend, w, 8, dirichlet=bc, load=load, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    s2, c2, st2 = _run(backend, w, 8, dirichlet=bc, load=load, rd_linear=backend.RD_LINEAR_PCG)
    print("three tissues, Dirichlet + load: Chebyshev solves %d, passes %d, fallbacks %d, interval [%.3f, %.3f]; vs PCG %.2e" %
          (st1['cheb_solves'], st1['cheb_its'], st1['cheb_fallbacks'], st1['cheb_lmin'], st1['cheb_lmax'], rel_l2(c1, c2)))
    assert s1 == 0 and s2 == 0
    assert st1['cheb_solves'] > 0 and st2['cheb_solves'] == 0
    assert np.all(np.isfinite(c1)) and np.all(c1[bn] == 0.01)
    assert rel_l2(c1, c2) < TOL_PATHS


def test_fp32_jacobian_still_reads_the_dinv_array(backend):
    """GLIMS_FLAG_FP32_JACOBIAN: the stored diagonal is rounded to single precision while the sweep's Dinv came from the
    double, so k_cheb<.., float> keeps the array; the direction comes from the iterates there too.  Against the default
    (fp64) run at the project's end-to-end tolerance, and against fp32 PCG."""
    w = _c3_reduced(24)
    flags = _default_flags(backend, w) | backend.FLAG_FP32_JACOBIAN
    s1, c1, st1 = _run(backend, w, 10, flags=flags)
    s0, c0, st0 = _run(backend, w, 10)
    s2, c2, st2 = _run(backend, w, 10, flags=flags, rd_linear=backend.RD_LINEAR_PCG)
    print("fp32 Jacobian: Chebyshev solves %d, passes %d, fallbacks %d; vs the fp64 run %.2e, vs fp32 PCG %.2e" %
          (st1['cheb_solves'], st1['cheb_its'], st1['cheb_fallbacks'], rel_l2(c1, c0), rel_l2(c1, c2)))
    assert s1 == 0 and s0 == 0 and s2 == 0
    assert st1['cheb_solves'] > 0 and st0['cheb_solves'] > 0 and st2['cheb_solves'] == 0
    assert rel_l2(c1, c0) < TOL_FP32
    assert rel_l2(c1, c2) < TOL_PATHS


def _rehearse():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rehearse_partition", os.path.join(root, "tools", "rehearse_partition.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_runs_read_their_own_rows_of_the_previous_iterate(backend, world):
    """Ranks as threads of this process (parallel.ThreadedTransport), dot-free: the interior and the boundary launch of a pass
    see the same y_prev, and a lane reads its own row only -- the field equals the single-rank run's, Newton and pass counts
    are the same on every rank, and the run lands on the PCG path."""
    rp = _rehearse()
    w = _c3_reduced(24)
    s_1, c_1, _, st_1 = rp.run_single(w, 10, 0, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    s_p, c_p, _, _ = rp.run_single(w, 10, 0, rd_linear=backend.RD_LINEAR_PCG)
    s, c, _, ss = rp.run_partitioned(w, world, 10, 0, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    print("%d ranks: Newton %s (single rank %d), Chebyshev solves %s, passes %s (%d); vs single %.2e, vs PCG %.2e" %
          (world, [int(x['newton_its']) for x in ss], st_1['newton_its'], [int(x['cheb_solves']) for x in ss],
           [int(x['cheb_its']) for x in ss], st_1['cheb_its'], rel_l2(c, c_1), rel_l2(c, c_p)))
    assert s == 0 and s_1 == 0 and s_p == 0
    assert all(x['cheb_solves'] > 0 and x['cheb_fallbacks'] == 0 for x in ss)
    for k in ('newton_its', 'cheb_its', 'cheb_solves', 'cg_its'):
        assert all(x[k] == ss[0][k] for x in ss), k
    assert rel_l2(c, c_1) < TOL_RANKS
    assert rel_l2(c, c_p) < TOL_PATHS


def test_a_taken_back_solve_still_recovers(backend, monkeypatch):
    """TEST HOOK GLIMS_CHEB_TEST_SCALE_HI = 0.45: the interval's upper end far below the spectrum, the correction is taken
    back (x -= ylast) and the iteration repeated with PCG.  ylast is now also a buffer pass 2 may read its previous iterate
    from; the run still lands on the PCG path's field."""
    w = _c3_reduced(24)
    s2, c2, st2 = _run(backend, w, 10, rd_linear=backend.RD_LINEAR_PCG)
    monkeypatch.setenv("GLIMS_CHEB_TEST_SCALE_HI", "0.45")
    s1, c1, st1 = _run(backend, w, 10)
    monkeypatch.delenv("GLIMS_CHEB_TEST_SCALE_HI")
    print("wrong interval: Chebyshev solves %d, taken back %d, learning solves %d; vs PCG %.2e" %
          (st1['cheb_solves'], st1['cheb_fallbacks'], st1['cheb_learn_solves'], rel_l2(c1, c2)))
    assert s1 == 0 and s2 == 0
    assert st1['cheb_solves'] > 0 and st1['cheb_fallbacks'] >= 1
    assert rel_l2(c1, c2) < TOL_PATHS
