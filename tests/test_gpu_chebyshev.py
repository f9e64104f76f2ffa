"""
The dot-free RD linear solves (glims_options.rd_linear, ABI 6): Chebyshev semi-iteration fused into the operator pass, interval
from the Lanczos coefficients of recorded PCG solves.  Through the C-ABI, against the oracle and against the PCG path.

Reference counterpart: the KSP behind `self.solver.solve()` (simulation_base.py:302; solver parameters
simulation_tumor_growth.py:126-130) -- the reference's sparse LU is exact, so every Krylov variant here must land on the same
Newton fixed point.
"""
import numpy as np
import pytest

from glimslib_amd import workloads
from oracle.glims_oracle import OracleTumorGrowth, rel_l2

pytestmark = pytest.mark.gpu


def _c3_reduced(n):
    w = workloads.config_c3(n)
    hx = 240.0 / n
    w.c0 = np.exp(-((w.mesh.points - np.array([118.0, -109.0, 72.0])) ** 2).sum(axis=1) / (2.0 * (2.5 * hx) ** 2))
    return w


def _run(backend, w, steps, **opts):
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    h.set_options(dt=w.dt, **opts)
    h.setup(False)
    h.set_state(w.c0)
    st = h.step(steps)
    c = h.get_state(want_u=False)[0]
    s = h.stats()
    h.close()
    return st, c, s


def test_chebyshev_solves_land_on_the_oracle_and_on_the_pcg_path(backend):
    """Reduced C3 (dt rho = 0.05), 12 steps: the default (auto = Chebyshev after the learning step) against rd_linear = PCG and
    against the oracle's Newton + LU; the dot-free path really ran, needed no fallback, and no more than ~PCG's passes."""
    w = _c3_reduced(28)
    s1, c1, st1 = _run(backend, w, 12)
    s2, c2, st2 = _run(backend, w, 12, rd_linear=backend.RD_LINEAR_PCG)
    assert s1 == 0 and s2 == 0
    print("default: Newton %d, Krylov passes %d (Chebyshev solves %d / passes %d, learning solves %d, fallbacks %d, interval "
          "[%.3f, %.3f]) | PCG: Newton %d, iterations %d" %
          (st1['newton_its'], st1['cg_its'], st1['cheb_solves'], st1['cheb_its'], st1['cheb_learn_solves'],
           st1['cheb_fallbacks'], st1['cheb_lmin'], st1['cheb_lmax'], st2['newton_its'], st2['cg_its']))
    assert st2['cheb_solves'] == 0 and st2['cheb_learn_solves'] == 0
    assert st1['cheb_solves'] >= 15 and st1['cheb_learn_solves'] >= 2 and st1['cheb_fallbacks'] == 0
    assert 0.3 < st1['cheb_lmin'] < 1.0 < st1['cheb_lmax'] < 3.5
    assert st1['newton_its'] <= st2['newton_its'] + 3
    assert st1['cg_its'] <= 1.25 * st2['cg_its'] + 6
    assert rel_l2(c1, c2) < 1e-9
    o = OracleTumorGrowth(w.mesh.points, w.mesh.cells, w.per_cell('D'), w.per_cell('rho'), w.per_cell('gamma'),
                          w.per_cell('E'), w.per_cell('nu'), w.dt)
    co = w.c0
    for _ in range(12):
        co, _ = o.rd_step(co)
    assert rel_l2(c1, co) < 1e-8


def test_a_wrong_interval_is_taken_back_and_the_step_repeated_with_pcg(backend, monkeypatch):
    """TEST HOOK GLIMS_CHEB_TEST_SCALE_HI = 0.45: the upper end of the interval is set far below the spectrum, the polynomial
    grows on most of the right-hand side, the Newton residual does not contract -> the correction is taken back, the iteration
    repeated with PCG, the interval measured again; the run still lands on the PCG path's field."""
    w = _c3_reduced(24)
    s2, c2, st2 = _run(backend, w, 8, rd_linear=backend.RD_LINEAR_PCG)
    monkeypatch.setenv("GLIMS_CHEB_TEST_SCALE_HI", "0.45")
    s1, c1, st1 = _run(backend, w, 8)
    monkeypatch.delenv("GLIMS_CHEB_TEST_SCALE_HI")
    print("wrong interval: %d Chebyshev solves, %d taken back, %d learning solves; Newton %d vs %d" %
          (st1['cheb_solves'], st1['cheb_fallbacks'], st1['cheb_learn_solves'], st1['newton_its'], st2['newton_its']))
    assert s1 == 0 and s2 == 0
    assert st1['cheb_fallbacks'] >= 1 and st1['cheb_learn_solves'] >= 4
    assert rel_l2(c1, c2) < 1e-9


def test_chebyshev_with_dirichlet_concentration_and_source(backend):
    """Constrained rows (Dirichlet c) and a load vector through the dot-free path: equal to the PCG path."""
    w = _c3_reduced(20)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    res = {}
    for name, lin in (("cheb", backend.RD_LINEAR_CHEBYSHEV), ("pcg", backend.RD_LINEAR_PCG)):
        h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
        t = w.tables
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        h.set_options(dt=w.dt, rd_linear=lin)
        h.set_dirichlet_c(bn, np.full(len(bn), 0.01))
        h.set_rd_load(1e-3 * np.exp(-((w.mesh.points - np.array([100.0, -100.0, 70.0])) ** 2).sum(axis=1) / 400.0))
        h.setup(False)
        h.set_state(w.c0)
        assert h.step(6) == 0
        res[name] = (h.get_state(want_u=False)[0], h.stats())
        h.close()
    assert res["cheb"][1]['cheb_solves'] > 0 and res["cheb"][1]['cheb_fallbacks'] == 0
    assert np.allclose(res["cheb"][0][bn], 0.01)
    assert rel_l2(res["cheb"][0], res["pcg"][0]) < 1e-9


def test_brain_like_mesh_chebyshev_against_pcg(backend):
    """The unstructured brain-like mesh (reduced): true spectrum of Dinv A far wider than what the right-hand sides excite
    (tools/proto_chebyshev.py: [0.17, 3.3] against Ritz [0.66, 2.0]) -- the dot-free path must still land on PCG's field, and
    if a solve is taken back the run recovers."""
    w = workloads.config_brain_like(60000, isolate=True)
    s1, c1, st1 = _run(backend, w, 10)
    s2, c2, st2 = _run(backend, w, 10, rd_linear=backend.RD_LINEAR_PCG)
    print("brain-like 60 k: Chebyshev solves %d, passes %d, fallbacks %d, interval [%.3f, %.3f]; Krylov passes %d vs PCG %d; "
          "Newton %d vs %d" % (st1['cheb_solves'], st1['cheb_its'], st1['cheb_fallbacks'], st1['cheb_lmin'], st1['cheb_lmax'],
                               st1['cg_its'], st2['cg_its'], st1['newton_its'], st2['newton_its']))
    assert s1 == 0 and s2 == 0
    assert st1['cheb_solves'] > 0
    assert rel_l2(c1, c2) < 1e-9
    assert st1['cg_its'] <= 1.3 * st2['cg_its'] + 10


def test_stream_policy_and_explicit_chebyshev_do_not_change_the_bits(backend):
    """The cache policy of the operator streams (glims_options.stream_policy) only changes how loads are issued: cached and
    non-temporal runs are bitwise equal, counters included; rd_linear = CHEBYSHEV differs from AUTO only where AUTO's cost model
    sends a tight solve to PCG -- on this problem nowhere."""
    w = _c3_reduced(24)
    s1, c1, st1 = _run(backend, w, 10, stream_policy=backend.STREAM_CACHED)
    s2, c2, st2 = _run(backend, w, 10, stream_policy=backend.STREAM_NONTEMPORAL)
    s3, c3, st3 = _run(backend, w, 10, rd_linear=backend.RD_LINEAR_CHEBYSHEV)
    assert s1 == 0 and s2 == 0 and s3 == 0
    assert st1['stream_nontemporal'] == 0 and st2['stream_nontemporal'] == 1
    assert np.array_equal(c1, c2)
    for k in ('newton_its', 'cg_its', 'cheb_its', 'cheb_solves', 'rd_assemblies', 'rd_quad_updates'):
        assert st1[k] == st2[k], k
    assert st1['krylov_working_set'] > 0
    assert np.array_equal(c1, c3) or rel_l2(c1, c3) < 1e-10


def test_guesses_of_both_solves_change_the_counts_not_the_fields(backend):
    """Both linear solves of a step start from a guess (GLIMS_FLAG_WARM_START, default): the first from the extrapolated increment,
    the second from the extrapolated second correction of the two steps before (solver.hip: k_d2_guess; on the PCG path applied only
    if it brings the residual down to a fifth).  Reduced C3, 40 steps, on the dot-free path and on the PCG path, each against the
    same run without guesses: the same fields (the Newton tolerance decides what a step returns, not where its solves start),
    fewer Krylov passes, no more Newton iterations than a few."""
    w = _c3_reduced(32)
    out = {}
    for name, opts in (("dot-free", {}), ("pcg", dict(rd_linear=backend.RD_LINEAR_PCG))):
        s_w, c_w, st_w = _run(backend, w, 40, **opts)
        h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
        flags = h.options.flags & ~backend.FLAG_WARM_START   # (the library's defaults, minus the guesses)
        h.close()
        s_c, c_c, st_c = _run(backend, w, 40, flags=flags, **opts)
        assert s_w == 0 and s_c == 0
        print("%s: with guesses Newton %d, Krylov passes %d (take-backs %d) | without Newton %d, passes %d | fields %.1e apart" %
              (name, st_w['newton_its'], st_w['cg_its'], st_w['cheb_fallbacks'], st_c['newton_its'], st_c['cg_its'],
               rel_l2(c_w, c_c)))
        assert rel_l2(c_w, c_c) < 1e-9
        assert st_w['cg_its'] < 0.9 * st_c['cg_its']
        assert st_w['newton_its'] <= st_c['newton_its'] + 4
        out[name] = c_w
    assert rel_l2(out["dot-free"], out["pcg"]) < 1e-9


# ---- where the dot-free path branches -----------------------------------------------------------------------------------------

def _box(nx, ny, nz, extent):
    """A box at the spacing of reduced C3 (D dt / h^2 small: the dot-free path's regime), grey matter with a white-matter
    ellipsoid, C3's tables and a Gaussian seed of width 2.5 h at the centre."""
    from glimslib_amd.mesh import BoxMesh
    ext = np.asarray(extent, dtype=float)
    mesh = BoxMesh((0.0, 0.0, 0.0), tuple(ext), nx, ny, nz)
    mid = mesh.cell_midpoints()
    q = (((mid - 0.5 * ext) / (0.35 * ext)) ** 2).sum(axis=1)
    label = np.where(q < 1.0, workloads.WM, workloads.GM).astype(np.int32)
    w = workloads.config_c3(4)
    hx = ext[0] / nx
    c0 = np.exp(-((mesh.points - 0.5 * ext) ** 2).sum(axis=1) / (2.0 * (2.5 * hx) ** 2))
    return workloads.Workload("box %dx%dx%d" % (nx, ny, nz), mesh, label, w.tables, c0, 1.0, 0, False)


def _oracle_steps(w, steps):
    o = OracleTumorGrowth(w.mesh.points, w.mesh.cells, w.per_cell('D'), w.per_cell('rho'), w.per_cell('gamma'),
                          w.per_cell('E'), w.per_cell('nu'), w.dt)
    co = w.c0
    for _ in range(steps):
        co, _ = o.rd_step(co)
    return co


def _zero_pass_run(backend, w, flags, maxit=None, **opts):
    """Ten steps (dot-free solves under way: cheb_delta / cheb_delta2 hold real corrections), then cg_atol above the residual
    the next step starts from, and more steps: every solve from zero has its tolerance met before it starts."""
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    h.set_options(dt=w.dt, flags=flags, **opts)
    h.setup(False)
    h.set_state(w.c0)
    assert h.step(10) == 0
    c_a = h.get_state(want_u=False)[0]
    s_a = h.stats()
    r0 = np.linalg.norm(h.rd_residual(c_a, c_a))   # |R(c^n; c^n)|: where the next step's first solve starts
    h.set_options(cg_atol=10.0 * r0, **({} if maxit is None else dict(newton_maxit=maxit)))
    st = h.step(3)                                  # (stops at the first step that does not converge)
    c_b = h.get_state(want_u=False)[0]
    s_b = h.stats()
    maxit_used = h.options.newton_maxit
    h.close()
    return st, c_a, c_b, s_a, s_b, maxit_used


@pytest.mark.parametrize("warm", [True, False], ids=["default-flags", "no-warm-start"])
def test_a_solve_whose_tolerance_is_met_leaves_the_state_alone(backend, warm):
    """cg_atol above the Newton residual: a dot-free solve from zero has nothing to do.  It must enqueue no pass, write no
    correction, not be taken back, count no pass -- PCG's zero iterations --, and the step ends as the PCG path's does.
    (Before the fix the solve recorded a correction it never wrote and the take-back subtracted the previous one from c.)
    Default flags: the step's first solve starts from the warm-start guess and runs (its count is chosen on the device); the
    second one starts from zero.  Without GLIMS_FLAG_WARM_START the first solve is already the one from zero."""
    w = _c3_reduced(24)
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    flags = h.options.flags if warm else h.options.flags & ~backend.FLAG_WARM_START
    h.close()
    st, c_a, c_b, s_a, s_b, maxit = _zero_pass_run(backend, w, flags)
    st_p, c_ap, c_bp, s_ap, s_bp, _ = _zero_pass_run(backend, w, flags, rd_linear=backend.RD_LINEAR_PCG)
    d = {k: s_b[k] - s_a[k] for k in ('newton_its', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks', 'steps')}
    print("%s: status %d (PCG %d); over the zero-pass step %s; field moved %.2e (PCG %.2e); dot-free vs PCG %.2e" %
          ("warm" if warm else "cold", st, st_p, d, rel_l2(c_b, c_a), rel_l2(c_bp, c_ap), rel_l2(c_b, c_bp)))
    assert s_a['cheb_solves'] > 0 and s_a['cheb_fallbacks'] == 0 and s_ap['cheb_solves'] == 0
    assert st == st_p == backend.GLIMS_NOT_CONVERGED
    assert np.all(np.isfinite(c_b)) and np.all(np.isfinite(c_bp))
    assert d['cheb_fallbacks'] == 0
    assert d['newton_its'] == maxit == s_bp['newton_its'] - s_ap['newton_its']
    assert rel_l2(c_a, c_ap) < 1e-9
    if not warm:
        # no solve ran at all: not one pass, the field bit for bit where the previous step left it -- on both paths
        assert d['cheb_solves'] == 0 and d['cheb_its'] == 0 and d['cg_its'] == 0
        assert np.array_equal(c_b, c_a) and np.array_equal(c_bp, c_ap)
        assert rel_l2(c_b, c_bp) < 1e-9
    else:
        # only the warm-started first solve ran; the same run stopped right after it (newton_maxit = 1) ends on the same bits
        assert d['cheb_solves'] == 1 and 0 < d['cheb_its'] == d['cg_its']
        st1, _, c_b1, _, s_b1, _ = _zero_pass_run(backend, w, flags, maxit=1)
        assert st1 == backend.GLIMS_NOT_CONVERGED and s_b1['cheb_fallbacks'] == s_a['cheb_fallbacks']
        assert np.array_equal(c_b, c_b1)
        assert rel_l2(c_b, c_a) > 1e-6   # (the first solve moved the field: a take-back would show)
        # (the two paths differ in how far the warm-started solve went -- the guess alone meets the tolerance --, not by a
        #  whole correction)
        assert rel_l2(c_b, c_bp) < 0.05 * rel_l2(c_b, c_a)


def _column_code_runs(backend, w, steps, monkeypatch):
    outs = []
    for int32, env in ((False, None), (True, None), (False, "2"), (False, "0")):
        monkeypatch.delenv("GLIMS_WIN_LIMIT", raising=False)
        if env is not None:
            monkeypatch.setenv("GLIMS_WIN_LIMIT", env)
        h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
        flags = h.options.flags | (backend.FLAG_INT32_COLUMNS if int32 else 0)
        h.close()
        outs.append(_run(backend, w, steps, flags=flags))
    monkeypatch.delenv("GLIMS_WIN_LIMIT", raising=False)
    for s, c, st in outs:
        assert s == 0 and st['cheb_solves'] > 0 and np.all(np.isfinite(c))
    for s, c, st in outs[1:]:
        assert np.array_equal(c, outs[0][1])
        for k in ('newton_its', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks'):
            assert st[k] == outs[0][2][k], k
    return [st for _, _, st in outs]


def test_column_encodings_on_the_dot_free_path_are_bitwise_equivalent(backend, monkeypatch):
    """k_cheb reads a slice's columns as 16-bit (window, offset) codes where the slice's windows fit the table (win_ok) and as
    int32 elsewhere: all codes (default), none (GLIMS_FLAG_INT32_COLUMNS, or the test hook GLIMS_WIN_LIMIT = 0) and a genuine
    mix (GLIMS_WIN_LIMIT = 2) give the same bits and the same counts through whole runs of dot-free solves -- on a box of some
    twenty thousand nodes and a ragged one of a single slice (the UNR = 8 variant of lattice meshes)."""
    big = _box(30, 28, 26, (240.0, 312.0, 192.0))
    sts = _column_code_runs(backend, big, 8, monkeypatch)
    assert sts[0]['nnz_idx16'] == sts[0]['nnz_padded']
    assert sts[1]['nnz_idx16'] == 0 and sts[3]['nnz_idx16'] == 0
    assert 0 < sts[2]['nnz_idx16'] < sts[2]['nnz_padded']   # genuinely mixed
    _column_code_runs(backend, _box(3, 2, 1, (30.0, 20.0, 10.0)), 8, monkeypatch)


def test_column_encodings_on_the_brain_like_mesh_are_bitwise_equivalent(backend, monkeypatch):
    """The same on the unstructured brain-like mesh, whose operator passes take the UNR = 16 variant of k_cheb."""
    w = workloads.config_brain_like(24000, isolate=True)
    sts = _column_code_runs(backend, w, 6, monkeypatch)
    assert sts[0]['nnz_idx16'] > 0
    assert sts[1]['nnz_idx16'] == 0 and sts[3]['nnz_idx16'] == 0
    assert sts[2]['nnz_idx16'] < sts[0]['nnz_idx16']


@pytest.mark.parametrize("mesh", ["lattice", "brain-like"])
def test_fp32_jacobian_through_the_dot_free_path(backend, mesh):
    """GLIMS_FLAG_FP32_JACOBIAN: the Krylov passes read a single-precision copy of the Newton Jacobian (k_cheb<8, *, *, float>;
    products and sums stay fp64).  The Newton residual is evaluated in fp64 by the sweeps, so the fixed point does not move:
    the dot-free run lands on the fp32 PCG run's field and on the oracle's Newton + LU.  The stream policy changes only how the
    loads are issued: bitwise equal."""
    w = _c3_reduced(16) if mesh == "lattice" else workloads.config_brain_like(8000, isolate=True)
    steps = 8 if mesh == "lattice" else 5
    h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    flags = h.options.flags | backend.FLAG_FP32_JACOBIAN
    h.close()
    s1, c1, st1 = _run(backend, w, steps, flags=flags, stream_policy=backend.STREAM_CACHED)
    s2, c2, st2 = _run(backend, w, steps, flags=flags, stream_policy=backend.STREAM_NONTEMPORAL)
    s3, c3, st3 = _run(backend, w, steps, flags=flags, rd_linear=backend.RD_LINEAR_PCG)
    co = _oracle_steps(w, steps)
    print("%s fp32 Jacobian: Chebyshev solves %d, passes %d, fallbacks %d; vs fp32 PCG %.2e, vs oracle %.2e" %
          (mesh, st1['cheb_solves'], st1['cheb_its'], st1['cheb_fallbacks'], rel_l2(c1, c3), rel_l2(c1, co)))
    assert s1 == 0 and s2 == 0 and s3 == 0
    assert st1['cheb_solves'] > 0 and st3['cheb_solves'] == 0
    assert st1['stream_nontemporal'] == 0 and st2['stream_nontemporal'] == 1
    assert np.array_equal(c1, c2)
    for k in ('newton_its', 'cg_its', 'cheb_its', 'cheb_solves', 'cheb_fallbacks'):
        assert st1[k] == st2[k], k
    assert rel_l2(c1, c3) < 1e-8
    assert rel_l2(c1, co) < 1e-8


def _rehearse():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rehearse_partition", os.path.join(root, "tools", "rehearse_partition.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_take_back_in_partitioned_runs(backend, monkeypatch):
    """TEST HOOK GLIMS_CHEB_TEST_SCALE_HI = 0.45 (read when a handle is created) with the ranks as threads of this process
    (parallel.ThreadedTransport): every rank takes its owned rows' correction back (k_sub_inplace), joins the sweep that
    follows and drops the interval -- all on the same Newton iteration, from all-reduced residuals; the run repeats the
    single-rank run with the same hook (same iterations, same take-backs, the field to rounding) and lands on the PCG path."""
    rp = _rehearse()
    w = _c3_reduced(24)
    s_p, c_p, _, _ = rp.run_single(w, 8, 0, rd_linear=backend.RD_LINEAR_PCG)
    monkeypatch.setenv("GLIMS_CHEB_TEST_SCALE_HI", "0.45")
    s_1, c_1, _, st_1 = rp.run_single(w, 8, 0)
    assert s_p == 0 and s_1 == 0 and st_1['cheb_fallbacks'] >= 1
    for world in (2, 4):
        s, c, _, ss = rp.run_partitioned(w, world, 8, 0)
        print("%d ranks: take-backs %s (single rank %d), Newton %s (%d), Chebyshev solves %s; vs single %.2e, vs PCG %.2e" %
              (world, [int(x['cheb_fallbacks']) for x in ss], st_1['cheb_fallbacks'], [int(x['newton_its']) for x in ss],
               st_1['newton_its'], [int(x['cheb_solves']) for x in ss], rel_l2(c, c_1), rel_l2(c, c_p)))
        assert s == 0
        assert ss[0]['cheb_fallbacks'] >= 1 and all(x['cheb_fallbacks'] == ss[0]['cheb_fallbacks'] for x in ss)
        # (the same iterations as the single-rank run, not just the same fixed point: a rank that kept its correction is
        #  repaired by the Newton iteration -- with more iterations, and a field some 1e-11 off instead of at rounding level)
        assert all(x['newton_its'] == st_1['newton_its'] for x in ss)
        assert all(x['cheb_fallbacks'] == st_1['cheb_fallbacks'] for x in ss)
        assert all(x['cheb_solves'] > 0 for x in ss)
        assert rel_l2(c, c_1) < 1e-13 and rel_l2(c, c_p) < 1e-9


def test_take_back_keeps_dirichlet_values_exact(backend, monkeypatch):
    """Constrained rows (Dirichlet c) and an RD load with a deliberately wrong interval (GLIMS_CHEB_TEST_SCALE_HI = 0.45): the
    take-back subtracts the kept correction from every owned row, constrained ones included -- whose correction is zero --, so
    the boundary values stay exact, and the run lands on the PCG path's field."""
    w = _c3_reduced(20)
    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    load = 1e-3 * np.exp(-((w.mesh.points - np.array([100.0, -100.0, 70.0])) ** 2).sum(axis=1) / 400.0)
    res = {}
    for name, lin in (("pcg", backend.RD_LINEAR_PCG), ("cheb", backend.RD_LINEAR_CHEBYSHEV)):
        if name == "cheb":
            monkeypatch.setenv("GLIMS_CHEB_TEST_SCALE_HI", "0.45")
        h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
        t = w.tables
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        h.set_options(dt=w.dt, rd_linear=lin)
        h.set_dirichlet_c(bn, np.full(len(bn), 0.01))
        h.set_rd_load(load)
        h.setup(False)
        h.set_state(w.c0)
        assert h.step(8) == 0
        res[name] = (h.get_state(want_u=False)[0], h.stats())
        h.close()
    c, st = res["cheb"]
    print("Dirichlet + load, wrong interval: %d take-backs, %d Chebyshev solves; vs PCG %.2e" %
          (st['cheb_fallbacks'], st['cheb_solves'], rel_l2(c, res["pcg"][0])))
    assert st['cheb_fallbacks'] >= 1 and st['cheb_solves'] > 0
    assert np.all(c[bn] == 0.01)
    assert rel_l2(c, res["pcg"][0]) < 1e-9
