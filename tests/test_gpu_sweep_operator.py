"""
The assembly sweep (k_rd_assemble, k_rd_assemble_s: A(c) = S + 2 dt N(c) stored in fp64 or fp32, the Newton residual, dinv, the
slice sums, the exactly-linear flags) as an operator against the np.longdouble reference of tests/sweep_common.py, row by row
inside the bounds derived there -- never a norm.  The stepper forms the residual in registers from the row it has just computed,
so Newton lands on the oracle's field with a wrong stored entry, a wrong dinv, a wrong slice sum or a wrong `lin` flag; only
iteration counts would move.  Here every output is read back through the C-ABI handle:

  rd_residual(c, c_prev)  with and without an rd_load           -> R
  glims_apply(8)  at a random x                                 -> -1/2 (A(x) + S) x
  glims_apply(0 | 5) on three probes after a sweep              -> the STORED A (after hook 8: A(x), no state needed; after
                                                                   hook 10: the MB = 1 instances' A; with a state: A(c), and
                                                                   hook 7 agrees with hook 0 to 1e-14)
  glims_apply(12) on ones after each sweep                      -> dinv against 1 / diag A_ref
  glims_peek_partials                                           -> column 0 = sum of the returned rows' squares, column 1 = 0
  stats()['rd_lin_slices'] after rd_residual(c, c) on ball fields -> sweep_common.lin_reference, exactly
one storage axis at a time (16-bit column codes, int32 columns, a genuine mix through GLIMS_WIN_LIMIT, 32-bit slot words, full
record words, fp32 Jacobian), on every mesh of quad_pass_common.CASES, each asserting the kernel instances it reaches.  Dirichlet
rows, ghost rows (two ranks as threads of this process) and the hooks' neutrality have tests of their own.
tests/test_sweep_cpu.py shows that each of six defects leaves the bound of the outputs it corrupts by a factor 10 and no other
(its table): a record dropped, 3 c_i for 4 c_i on the diagonal, a wrong slot -> R, A and dinv here; vA stored with dt for 2 dt
-> only the products with the stored A; dinv from S -> only hook 12; an fp32 handle's residual formed from the rounded entry
-> only R on the fp32 axis, which is held to the fp64 bound.  (Measured once with a library built by hand with the fourth and
fifth defect in rd_assemble_s_slice, never committed: R and hook 8 stayed at 0.02 of their bounds, dinv and the products with
the stored A left theirs by twelve orders of magnitude, on the lattice, the random-point mesh and a fan mesh.)

Out of scope: the folded guess pass (FG = 1, 2) and the second right-hand side -- no hook reaches them; they stay with
tests/test_gpu_fused_guess_pass.py (bit for bit against the separate k_cheb launch, which tests/test_gpu_chebyshev.py and
tests/test_gpu_cheb_streams.py hold to a reference) -- and the interior / boundary slice split of partitioned stepping.

Largest err / bound observed on the MI355X in the run that verified this file (a record, not a threshold; the bound is the
yardstick), over all meshes, per output and storage axis:

    output                          default   cols32  slots32  recfull     fp32   winmix  2 ranks
    R                                 0.024    0.024    0.024    0.024    0.024    0.022        -
    R with a load                     0.092    0.092    0.092    0.092    0.092    0.092        -
    R, Dirichlet rows set             0.023    0.023    0.023    0.023    0.023    0.017        -
    R, owned rows                         -        -        -        -        -        -    0.023
    dinv after hook 10                0.041    0.041    0.041    0.041        -    0.029        -
    dinv after hook 8                 0.033    0.033    0.033    0.033    0.033    0.031        -
    dinv after rd_residual            0.035    0.035    0.035    0.035    0.035    0.027        -
    dinv, Dirichlet rows set          0.033    0.033    0.033    0.033    0.033    0.031        -
    dinv, owned rows                      -        -        -        -        -        -    0.026
    hook 0, owned rows                    -        -        -        -        -        -    0.022
    hook 1, owned rows                    -        -        -        -        -        -    0.019
    hook 10 (M x)                     0.030    0.030    0.030    0.030        -    0.029        -
    hook 2, owned rows                    -        -        -        -        -        -    0.017
    hook 8                            0.026    0.026    0.026    0.026    0.026    0.025        -
    hook 8, Dirichlet rows set        0.026    0.026    0.026    0.026    0.026    0.025        -
    hook 8, owned rows                    -        -        -        -        -        -    0.023
    stored A after hook 10            0.035    0.035    0.035    0.035        -    0.035        -
    stored A after hook 8             0.035    0.035    0.035    0.035    0.853    0.035        -
    stored A with a state             0.035    0.035    0.035    0.035    0.902    0.035        -
    stored A, Dirichlet rows set      0.035    0.035    0.035    0.035    0.770    0.035        -

Reference counterpart: the Jacobian and residual of 'F == 0' (simulation_tumor_growth.py:115-120).
"""
import numpy as np
import pytest

from oracle.glims_oracle import rel_l2
from sweep_common import (CASES, LD, LOOPED, SweepRef, ball_field, case, inside, lin_reference, sums_bound, worst)
from test_gpu_quad_pass import COUNTS, _exterior, _instances, _open

pytestmark = pytest.mark.gpu

_BASE, _AT = {}, {}
STRAIGHT = tuple(c for c in sorted(CASES) if LOOPED not in CASES[c][1])      # every class straight-line: lin flags on all slices
WIN_MIX_CASES = ('random_3000', 'jittered_seed0')
AXES = ('default', 'cols32', 'winmix', 'slots32', 'recfull', 'fp32')
AXIS_CASES = [(cid, a) for cid in sorted(CASES) for a in AXES if a != 'winmix' or cid in WIN_MIX_CASES]


def _base(cid):
    if cid not in _BASE:
        _BASE[cid] = SweepRef(case(cid))
    return _BASE[cid]


def _vectors(cid):
    """The inputs of a case: c (the case's field), c_prev in [0, 1], two iterates x for the hooks, a load, three probes."""
    w = case(cid)
    n = len(w.mesh.points)
    rng = np.random.default_rng(29)
    p = w.mesh.points
    return dict(c=np.asarray(w.c0, dtype=np.float64), c_prev=rng.random(n), x=rng.standard_normal(n), x10=rng.standard_normal(n),
                load=0.05 * np.cos(3.0 * p[:, 0]) * (1.0 + p[:, 1] ** 2),
                probes={'normal': rng.standard_normal(n), 'ones': np.ones(n), 'x': np.asarray(p[:, 0], dtype=np.float64)})


def _at(cid, key):
    """The reference at one of the case's iterates ('c', 'x', 'x10'), built once per process and shared (read only)."""
    if (cid, key) not in _AT:
        _AT[(cid, key)] = _base(cid).at(_vectors(cid)[key])
    return _AT[(cid, key)]


def _flags(backend, axis):
    return {'slots32': backend.FLAG_SLOT_WORDS32, 'recfull': backend.FLAG_RECORD_WORDS_FULL,
            'fp32': backend.FLAG_FP32_JACOBIAN}.get(axis, 0)


def _open_axis(backend, monkeypatch, w, axis, **kw):
    """A handle on one storage axis.  'winmix': the first GLIMS_WIN_LIMIT that leaves some slices with 16-bit codes and some
    without (asserted from the stats)."""
    monkeypatch.delenv("GLIMS_WIN_LIMIT", raising=False)
    if axis != 'winmix':
        return _open(backend, w, int32=axis == 'cols32', flags_or=_flags(backend, axis), **kw)
    seen = []
    for limit in ("2", "3", "4", "6", "1", "8", "12"):
        monkeypatch.setenv("GLIMS_WIN_LIMIT", limit)
        h = _open(backend, w, **kw)
        st = h.stats()
        if 0 < st['nnz_idx16'] < st['nnz_padded']:
            return h
        seen.append((limit, st['nnz_idx16'], st['nnz_padded']))
        h.close()
    raise AssertionError("no GLIMS_WIN_LIMIT gives a genuine mix: %r" % (seen,))


def _held(ratios, what, got, ref, bound, rows=None):
    """Row by row: |got - ref| <= bound on `rows` (all rows by default); notes the largest err / bound."""
    got = np.asarray(got)
    err = np.abs(got.astype(LD) - ref)
    if rows is not None:
        err, bound = err[rows], np.asarray(bound)[rows]
    assert np.all(np.isfinite(got))
    r = worst(err, bound)
    ratios[what] = max(ratios.get(what, 0.0), r)
    assert inside(err, bound), (what, r, int(np.argmax(err - bound)))


def _sums(h, y):
    p = h.peek_partials()
    s = float(np.sum(y * y))
    assert p[1] == 0.0
    assert abs(p[0] - s) <= sums_bound(len(y), s), (p[0], s)


def _dinv(h, ratios, what, at, fixed=None):
    """Hook 12 on ones: dinv itself.  Relative against 1 / diag A_ref; exactly 1 on Dirichlet rows."""
    n = at.base.n
    d = h.apply(12, np.ones(n))[0]
    free = np.ones(n, dtype=bool)
    if fixed is not None:
        free[fixed] = False
        assert np.all(d[fixed] == 1.0)
    _held(ratios, what, d.astype(LD) * at.diag(), 1.0, at.dinv_bound(), rows=free)


def _stored(h, ratios, what, at, probes, fp32, rows=None):
    """Hooks 0 and 5 on the probes: the stored A against A_ref z."""
    for name, z in probes.items():
        ref, bound = at.product(z), at.product_bound(z, fp32)
        for hook in (0, 5):
            _held(ratios, what, h.apply(hook, z)[0], ref, bound, rows)


def _report(w, axis, ratios):
    for what, r in sorted(ratios.items()):
        print("RATIO | %-28s | %-8s | %-40s | %.3f" % (what, axis, w.name, r))


@pytest.mark.parametrize("cid,axis", AXIS_CASES, ids=["%s-%s" % ca for ca in AXIS_CASES])
def test_sweep_outputs_against_the_reference(backend, monkeypatch, capfd, cid, axis):
    monkeypatch.setenv("GLIMS_VERBOSE", "1")
    w, v = case(cid), _vectors(cid)
    base, fp32 = _base(cid), axis == 'fp32'
    at_c, at_x = _at(cid, 'c'), _at(cid, 'x')
    ratios = {}
    h = _open_axis(backend, monkeypatch, w, axis, state=False)
    with pytest.raises(backend.BackendError) as ei:          # no sweep has run
        h.apply(12, v['x'])
    assert ei.value.code == backend.GLIMS_E_USAGE
    # the residual (on an fp32 handle too inside the fp64 bound: it is formed from the unrounded entry)
    R = h.rd_residual(v['c'], v['c_prev'])
    _held(ratios, 'R', R, at_c.residual(v['c_prev']), at_c.residual_bound(v['c_prev']))
    _sums(h, R)
    _dinv(h, ratios, 'dinv after rd_residual', at_c)
    # hook 8 at x, and what it left: A(x) and its diagonal, no state set
    y8 = h.apply(8, v['x'])[0]
    _held(ratios, 'hook 8', -y8, at_x.residual(np.zeros(base.n)), at_x.residual_bound(np.zeros(base.n)))
    _sums(h, y8)
    _dinv(h, ratios, 'dinv after hook 8', at_x)
    _stored(h, ratios, 'stored A after hook 8', at_x, v['probes'], fp32)
    # the MB = 1 instances' stored A: hook 10 at another x
    mass_mode = not fp32 and LOOPED not in CASES[cid][1]
    if mass_mode:
        at_10 = _at(cid, 'x10')
        y10 = h.apply(10, v['x10'])[0]
        _held(ratios, 'hook 10 (M x)', y10, base.m_product(v['x10']), base.m_product_bound(v['x10']))
        _dinv(h, ratios, 'dinv after hook 10', at_10)
        _stored(h, ratios, 'stored A after hook 10', at_10, v['probes'], False)
    else:
        with pytest.raises(backend.BackendError) as ei:
            h.apply(10, v['x10'])
        assert ei.value.code == backend.GLIMS_E_USAGE
    # with a state: A(c) after rd_residual(c, c); the matrix-free product agrees with the stored one
    h.set_state(v['c'])
    Rcc = h.rd_residual(v['c'], v['c'])
    _held(ratios, 'R', Rcc, at_c.residual(v['c']), at_c.residual_bound(v['c']))
    _dinv(h, ratios, 'dinv after rd_residual', at_c)
    _stored(h, ratios, 'stored A with a state', at_c, v['probes'], fp32)
    z = v['probes']['normal']
    y7, y0 = h.apply(7, z)[0], h.apply(0, z)[0]
    if fp32:      # (hook 0 reads the rounded entries, hook 7 forms them afresh: each inside the fp32 bound of the same reference)
        assert inside(np.abs(y7 - y0), 2.0 * at_c.product_bound(z, True))
    else:
        assert rel_l2(y7, y0) < 1e-14
    lin = h.stats()['rd_lin_slices']
    if fp32:
        assert lin == 0
    h.close()
    # ... and with a load
    h = _open_axis(backend, monkeypatch, w, axis, state=False, load=v['load'])
    R = h.rd_residual(v['c'], v['c_prev'])
    _held(ratios, 'R with a load', R, at_c.residual(v['c_prev'], v['load']), at_c.residual_bound(v['c_prev'], v['load']))
    _sums(h, R)
    if mass_mode:
        y10 = h.apply(10, v['x10'])[0]
        _held(ratios, 'hook 10 (M x)', y10, base.m_product(v['x10']) + v['load'].astype(LD), base.m_product_bound(v['x10'], v['load']))
    h.close()
    text = capfd.readouterr()
    inst, caps = _instances(text.err)
    print(text.out, end="")
    _report(w, axis, ratios)
    print("%s (%s): classes of at most %s entries -> instances %s" % (w.name, axis, caps, sorted(inst, key=str)))
    assert inst == CASES[cid][1], (inst, CASES[cid][1])


@pytest.mark.parametrize("cid,axis", AXIS_CASES, ids=["%s-%s" % ca for ca in AXIS_CASES])
def test_dirichlet_rows(backend, monkeypatch, cid, axis):
    """Exterior nodes at 0.01: R and hook 8 exactly 0 there, dinv exactly 1, nothing added to the slice sum; every other row
    inside its bound (the columns of Dirichlet nodes stay in those rows: the sweep eliminates nothing)."""
    w, v = case(cid), _vectors(cid)
    base = _base(cid)
    at_c, at_x = _at(cid, 'c'), _at(cid, 'x')
    bn = _exterior(w)
    assert 0 < len(bn) < base.n
    free = np.ones(base.n, dtype=bool)
    free[bn] = False
    ratios = {}
    h = _open_axis(backend, monkeypatch, w, axis, state=False, dirichlet=bn)
    R = h.rd_residual(v['c'], v['c_prev'])
    assert np.all(R[bn] == 0.0) and np.abs(R).max() > 0.0
    _held(ratios, 'R, Dirichlet rows set', R, at_c.residual(v['c_prev']), at_c.residual_bound(v['c_prev']), rows=free)
    _sums(h, R)
    _dinv(h, ratios, 'dinv, Dirichlet rows set', at_c, fixed=bn)
    y8 = h.apply(8, v['x'])[0]
    assert np.all(y8[bn] == 0.0) and np.abs(y8).max() > 0.0
    _held(ratios, 'hook 8, Dirichlet rows set', -y8, at_x.residual(np.zeros(base.n)), at_x.residual_bound(np.zeros(base.n)),
          rows=free)
    _sums(h, y8)
    _dinv(h, ratios, 'dinv, Dirichlet rows set', at_x, fixed=bn)
    _stored(h, ratios, 'stored A, Dirichlet rows set', at_x, v['probes'], axis == 'fp32', rows=free)
    h.close()
    _report(w, axis, ratios)


@pytest.mark.parametrize("k", [0, 1, 2], ids=["corner", "centre", "opposite"])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_lin_slices(backend, monkeypatch, cid, k):
    """c = 0 outside a ball: the slices whose rows see no cell with rho c > 0 store the bits of S, and are counted -- exactly on
    the meshes whose classes are all straight-line, at most the reference's count where a looped class (which stores 0) exists;
    never on an fp32 handle."""
    w = case(cid)
    base = _base(cid)
    c = ball_field(w, k)
    counts = {}
    for axis in ('default', 'slots32', 'recfull', 'fp32'):
        h = _open_axis(backend, monkeypatch, w, axis, state=False)
        h.rd_residual(c, c)
        counts[axis] = h.stats()['rd_lin_slices']
        numbering = h.numbering()
        h.close()
    flags, ambiguous = lin_reference(w, c, numbering, base)
    assert ambiguous == 0
    want = int(flags.sum())
    print("%s, ball %d: %d of %d slices exactly linear in the reference, on the device %r" % (w.name, k, want, len(flags), counts))
    assert counts['fp32'] == 0
    for axis in ('default', 'slots32', 'recfull'):
        if cid in STRAIGHT:
            assert counts[axis] == want, (axis, counts[axis], want)
        else:
            assert counts[axis] <= want, (axis, counts[axis], want)


@pytest.mark.parametrize("cid", ['c3_n8', 'random_1000'])
def test_ghost_rows(backend, cid):
    """Two ranks as threads of this process: every rank's vectors hold the global values on its nodes, ghosts included; its
    owned rows of hooks 0, 1, 2, 8 and of rd_residual match the GLOBAL reference's rows inside the same bounds, ghost rows come
    back as 0, hook 10 is refused and no `lin` flag is kept.  (No hook communicates on such a handle; both ranks run the same
    calls in the same order all the same.)"""
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import build_local_part, node_owners
    w, v = case(cid), _vectors(cid)
    base = _base(cid)
    at_c, at_x, at_0 = _at(cid, 'c'), _at(cid, 'x'), base.at(np.zeros(base.n))
    pts, cells = w.mesh.points, w.mesh.cells
    world = 2
    owner = node_owners(pts, world, cells)
    parts = [build_local_part(pts, cells, owner, r, world) for r in range(world)]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    z = v['probes']['normal']

    def body(rank, tr):
        part = parts[rank]
        g = part.global_ids
        h = backend.Handle(part.points, part.cells, w.cell_label[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(lo, hi)
        t = w.tables
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        h.set_options(dt=w.dt)
        h.setup(False)
        out = dict(y8=h.apply(8, v['x'][g])[0])
        out['d8'] = h.apply(12, np.ones(len(g)))[0]
        for hook in (0, 1, 2):
            out[hook] = h.apply(hook, z[g])[0]
        out['R'] = h.rd_residual(v['c'][g], v['c_prev'][g])
        out['dR'] = h.apply(12, np.ones(len(g)))[0]
        try:
            h.apply(10, v['x'][g])
            out['refused'] = None
        except backend.BackendError as e:
            out['refused'] = e.code
        out['lin'] = h.stats()['rd_lin_slices']
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return out

    res = run_threaded_ranks(world, body)
    ratios = {}
    n0 = np.zeros(base.n)
    for rank, out in enumerate(res):
        part = parts[rank]
        own = part.global_ids[:part.n_own]
        assert 0 < part.n_own < part.n_local
        for key in ('y8', 'd8', 0, 1, 2, 'R', 'dR'):
            assert np.all(out[key][part.n_own:] == 0.0), key            # ghost rows
        assert out['refused'] == backend.GLIMS_E_USAGE and out['lin'] == 0

        def held(what, got, ref, bound):
            _held(ratios, what, got[:part.n_own], ref[own], np.asarray(bound)[own])
        held('hook 8, owned rows', -out['y8'], at_x.residual(n0), at_x.residual_bound(n0))
        held('hook 0, owned rows', out[0], at_x.product(z), at_x.product_bound(z))
        held('hook 1, owned rows', out[1], at_0.product(z), at_0.product_bound(z))
        held('hook 2, owned rows', out[2], base.m_product(z), base.m_product_bound(z))
        held('R, owned rows', out['R'], at_c.residual(v['c_prev']), at_c.residual_bound(v['c_prev']))
        _held(ratios, 'dinv, owned rows', out['d8'][:part.n_own].astype(LD) * at_x.diag()[own], 1.0, at_x.dinv_bound()[own])
        _held(ratios, 'dinv, owned rows', out['dR'][:part.n_own].astype(LD) * at_c.diag()[own], 1.0, at_c.dinv_bound()[own])
    _report(w, '2 ranks', ratios)


@pytest.mark.parametrize("axis", ['default', 'cols32', 'fp32'])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_hooks_are_neutral(backend, monkeypatch, cid, axis):
    """After every hook of this file on a handle with a state, hook 0 and hook 12 return the bits they returned before, and
    three steps give the bits and the counts of a handle that never ran them."""
    w, v = case(cid), _vectors(cid)
    fresh = _open_axis(backend, monkeypatch, w, axis)
    assert fresh.step(3) == 0
    c_fresh, s_fresh = fresh.get_state(want_u=False)[0], fresh.stats()
    fresh.close()
    h = _open_axis(backend, monkeypatch, w, axis)
    h.rd_residual(w.c0, w.c0)            # assembles A(c)
    x, ones = v['x'], np.ones(len(v['x']))
    before, d_before = h.apply(0, x)[0], h.apply(12, ones)[0]
    h.apply(8, x)
    if axis != 'fp32' and LOOPED not in CASES[cid][1]:
        h.apply(10, v['x10'])
    for hook in (12, 5, 7, 1, 2):
        h.apply(hook, x)
    h.peek_partials()
    assert np.array_equal(h.apply(0, x)[0], before)
    assert np.array_equal(h.apply(12, ones)[0], d_before)
    assert np.array_equal(h.get_state(want_u=False)[0], w.c0)
    assert h.step(3) == 0
    c, s = h.get_state(want_u=False)[0], h.stats()
    h.close()
    assert np.array_equal(c, c_fresh)
    for k in COUNTS:
        assert s[k] == s_fresh[k], (k, s[k], s_fresh[k])
