"""
Tumour volumes and centres of mass per tissue on the device (glims_observe, csrc/observe.hip) against the per-cell loop of
tests/observe_common.py:
  1. host-array mode, all three kinds, reference and deformed configuration, on a rectangle of less than one block of the
     cell pass, a box of more than one block (480 cells, no multiple of 64), the brain-like unstructured mesh, the box with
     labels {0, 7, 255} (gaps, the top label, three labels inside one wave) and the box with 40 labels (per-wave tables in
     global memory instead of LDS);
  2. known answers: c = x_0 clipped between node planes, the same under u = A x, exact zeros, per-label cell volumes;
  3. snapshot mode after a coupled run: many snapshots in one call, the counters of cell passes and elastic solves;
  4. bitwise repeatability, and the bits of the steps that follow;
  5. a folded cell; 6. every refusal; 7. the public API.
Bound of (1): |got - want| <= (2 N_cells 2^-53 + 64 2^-52) sum|T|, times max|x| for the moments -- the worst-case difference of
two fp64 sums of the same terms in different orders plus the per-cell bound of tests/test_observe_cpu.py.

Reference counterpart: compute_from_conc_for_each_time_step, glimslib/optimization_workflow/image_based_optimization.py:1333-1397.
"""
import ctypes as C

import numpy as np
import pytest

from glimslib_amd import fenics_local as fenics

import derive_common as dc
import observe_common as oc

pytestmark = pytest.mark.gpu


def _handle(backend, mesh, lab, n_labels, mechanics=True):
    t = oc.tables(n_labels)
    h = backend.Handle(mesh.points, mesh.cells, lab)
    h.set_materials(*[t[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=1.0)
    if mechanics:
        f = mesh.facets()
        bn = np.unique(f['vertices'][f['exterior']])
        d = mesh.points.shape[1]
        dofs = (bn[:, None] * d + np.arange(d)).ravel()
        h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
    h.setup(mechanics)
    return h


def _xmax(mesh, u=None):
    return np.abs(mesh.points).max() + (0.0 if u is None else np.abs(u).max())


# ---- 1. host mode against the loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "box", "brain", "box_sparse", "box_many"])
def test_host_mode_matches_the_loop(backend, name):
    mesh, lab, n_labels, c, u = oc.problem(name)
    d = mesh.points.shape[1]
    qs = oc.queries(name)
    h = _handle(backend, mesh, lab, n_labels)
    i0 = h.observe_info()
    for deformed in (False, True):
        want, counts, sum_abs = oc.reference(name, deformed)
        for k, q in enumerate(qs):
            if q[0] == "sharp":
                assert counts[k] == set(range(d + 2)), (q, counts[k])        # every in-count occurs
        got = h.observe(qs, c=c, u=u if deformed else None, deformed=deformed)
        assert got.shape == (1, len(qs), n_labels, 1 + d)
        unused = np.setdiff1d(np.arange(n_labels), np.unique(lab))
        assert np.all(got[0][:, unused] == 0.0)                              # a label that no cell carries: exact zeros
        oc.assert_close(got[0], want, len(mesh.cells), sum_abs, _xmax(mesh, u if deformed else None),
                        "%s deformed=%s" % (name, deformed))
    i1 = h.observe_info()
    assert {k: i1[k] - i0[k] for k in i1} == {"cell_passes": 2, "elastic_solves": 0, "sources": 2}
    h.close()


# ---- 2. known answers -----------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_box(backend):
    mesh = oc.box()                                                          # [0, 2] x [0, 1] x [0, 1.5], node planes x_0 = 0.4 k
    lab = oc.half_labels(mesh, cut=1.2)                                      # the label interface is the plane x_0 = 1.2
    vol = np.abs([oc._vol(p) for p in mesh.points[mesh.cells].tolist()])
    assert abs(vol[lab == 1].sum() - 1.2 * 1.5) < 1e-13 and abs(vol[lab == 2].sum() - 0.8 * 1.5) < 1e-13
    h = _handle(backend, mesh, lab, 3)
    X = mesh.points
    n, xmax = len(mesh.cells), np.abs(X).max()
    bv, bm = oc.bound(n, 3.0, xmax)
    # c = x_0, level 0.7: the cut lies between node planes
    t = h.observe([("sharp", 0.7)], c=X[:, 0].copy())[0, 0]
    V = np.array([0.0, (1.2 - 0.7) * 1.5, 0.8 * 1.5])
    com = np.array([[0, 0, 0], [0.95, 0.5, 0.75], [1.6, 0.5, 0.75]])
    assert np.all(t[0] == 0.0)
    assert np.abs(t[:, 0] - V).max() <= bv and np.abs(t[:, 1:] - V[:, None] * com).max() <= bm, t
    tot = t.sum(axis=0)
    assert abs(tot[0] - (2 - 0.7) * 1 * 1.5) <= bv and np.abs(tot[1:] / tot[0] - [1.35, 0.5, 0.75]).max() <= bm
    # the same under u = A x: V scales by det(I + A), the centre of mass maps affinely
    A = 0.01 * (np.arange(9).reshape(3, 3) + 1.0)
    A[0, 0] += 0.03
    F = np.eye(3) + A
    td = h.observe([("sharp", 0.7)], c=X[:, 0].copy(), u=X @ A.T, deformed=True)[0, 0]
    J = np.linalg.det(F)
    bvd, bmd = oc.bound(n, 3.0 * J, np.abs(X @ F.T).max())
    assert np.abs(td[:, 0] - J * V).max() <= bvd
    assert np.abs(td[:, 1:] - (J * V)[:, None] * (com @ F.T)).max() <= bmd
    # scale: x = X + 0.5 u
    th = h.observe([("sharp", 0.7)], c=X[:, 0].copy(), u=X @ A.T, deformed=True, scale=0.5)[0, 0]
    assert np.abs(th[:, 0] - np.linalg.det(np.eye(3) + 0.5 * A) * V).max() <= bvd
    # c = 0 with a level > 0: exact zeros
    assert np.all(h.observe([("sharp", 0.1), ("sharp", 1e-300)], c=np.zeros(len(X))) == 0.0)
    # level <= min c: the cell volumes per label; MASS of c = 1: the same
    c = oc.bump(X)
    cells = np.array([0.0, 1.8, 1.2])
    t = h.observe([("sharp", c.min()), ("sharp", -1.0), ("mass",)], c=c)[0]
    assert np.abs(t[:2, :, 0] - cells).max() <= bv
    t1 = h.observe([("mass",)], c=np.ones(len(X)))[0, 0]
    assert np.abs(t1[:, 0] - cells).max() <= bv
    assert np.abs(t1[:, 1:] - cells[:, None] * np.array([[0, 0, 0], [0.6, 0.5, 0.75], [1.6, 0.5, 0.75]])).max() <= bm
    h.close()


# ---- 3. snapshot mode -----------------------------------------------------------------------------------------------------------
def _coupled_run(backend, name, n_steps=3):
    mesh, lab, n_labels, _, _ = oc.problem(name)
    h = _handle(backend, mesh, lab, n_labels)
    h.set_state(oc.bump(mesh.points, width=0.4))
    ids = []
    for _ in range(n_steps):
        assert h.step(1) == backend.GLIMS_OK
        ids.append(h.snapshot_save())
    return h, mesh, lab, n_labels, ids


EIGHT = [("sharp", 0.12), ("sharp", 0.5), ("mass",), ("smooth", 0.12, 0.05), ("smooth", 0.5, 0.05), ("sharp", 0.3),
         ("smooth", 0.3, 0.02), ("sharp", 0.05)]


@pytest.mark.parametrize("name", ["rect", "box"])
def test_snapshot_mode(backend, name):
    h, mesh, lab, n_labels, ids = _coupled_run(backend, name)
    qs = oc.normalise(EIGHT)
    # 8 queries cost one cell pass per source
    i0 = h.observe_info()
    many = h.observe(EIGHT, snapshots=ids)
    i1 = h.observe_info()
    assert {k: i1[k] - i0[k] for k in i1} == {"cell_passes": len(ids), "elastic_solves": 0, "sources": len(ids)}
    # many snapshots in one call = one call per snapshot, bit for bit; = host mode on the downloaded field, to the bound of (1)
    for k, sid in enumerate(ids):
        assert np.array_equal(h.observe(EIGHT, snapshots=[sid])[0], many[k])
        c = h.snapshot_load(sid)
        assert np.array_equal(h.observe(EIGHT, c=c)[0], many[k])               # (the same pass over the same numbers)
        want, _, sum_abs = oc.observe_mesh(mesh.points, mesh.cells, lab, c, qs, n_labels)
        oc.assert_close(many[k], want, len(mesh.cells), sum_abs, _xmax(mesh), "%s snapshot %d" % (name, sid))
    # more than 8 queries: several calls, the same numbers
    eleven = EIGHT + [("sharp", 0.2), ("mass",), ("sharp", 0.12)]
    t = h.observe(eleven, snapshots=ids[-1:])[0]
    assert np.array_equal(t[:8], many[-1]) and np.array_equal(t[9], many[-1][2]) and np.array_equal(t[10], many[-1][0])
    # deformed: one elastic solve per snapshot, none when U already belongs to it
    i1, m1 = h.observe_info(), h.stats()['mech_solves']
    dm = h.observe(EIGHT, snapshots=ids, deformed=True)
    i2, m2 = h.observe_info(), h.stats()['mech_solves']
    assert h.last_observe_status == backend.GLIMS_OK
    assert i2["elastic_solves"] - i1["elastic_solves"] == len(ids) == m2 - m1
    assert np.array_equal(h.observe(EIGHT, snapshots=ids[-1:], deformed=True)[0], dm[-1])     # U belongs to the last one
    assert h.observe_info()["elastic_solves"] == i2["elastic_solves"]
    u, st = h.snapshot_mechanics(ids[0])                                       # sets the memory
    assert st == backend.GLIMS_OK
    i3 = h.observe_info()
    d0 = h.observe(EIGHT, snapshots=ids[:1], deformed=True)[0]
    assert h.observe_info()["elastic_solves"] == i3["elastic_solves"]
    c = h.snapshot_load(ids[0])
    assert np.array_equal(h.observe(EIGHT, c=c, u=u, deformed=True)[0], d0)
    want, _, sum_abs = oc.observe_mesh(mesh.points, mesh.cells, lab, c, qs, n_labels, u=u.reshape(len(c), -1))
    oc.assert_close(d0, want, len(mesh.cells), sum_abs, _xmax(mesh, u), "%s snapshot %d deformed" % (name, ids[0]))
    assert np.abs(d0 - many[0]).max() > 0.0                                    # (the tumour does displace the tissue)
    # the handle's own state as it stands
    assert h.solve_mechanics() == backend.GLIMS_OK
    c, u = h.get_state()
    assert np.array_equal(h.observe(EIGHT, deformed=True), h.observe(EIGHT, c=c, u=u, deformed=True))
    assert np.array_equal(h.observe(EIGHT), h.observe(EIGHT, c=c))
    h.close()


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "box"])
def test_same_bits_on_every_call_and_in_the_steps_that_follow(backend, name):
    mesh, lab, n_labels, c, u = oc.problem(name)
    h = _handle(backend, mesh, lab, n_labels)
    for deformed in (False, True):
        a = h.observe(EIGHT, c=c, u=u if deformed else None, deformed=deformed)
        for _ in range(3):
            assert np.array_equal(h.observe(EIGHT, c=c, u=u if deformed else None, deformed=deformed), a)
    h.close()
    runs = []
    for observe in (True, False):
        h, _, _, _, ids = _coupled_run(backend, name, n_steps=2)
        if observe:
            h.observe(EIGHT, snapshots=ids)
            h.observe(EIGHT)
        s0 = h.stats()
        assert h.step(1) == backend.GLIMS_OK
        if observe:
            h.observe(EIGHT[:3])                                               # interleaved between the steps
        assert h.step(1) == backend.GLIMS_OK
        s1 = h.stats()
        runs.append((h.get_state(want_u=False)[0],
                     {k: s1[k] - s0[k] for k in ("steps", "newton_its", "cg_its", "cheb_solves", "cheb_its")}))
        h.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1], runs


# ---- 5. a folded cell -------------------------------------------------------------------------------------------------------------
def test_a_folded_cell_counts_negatively(backend):
    mesh, lab, n_labels, c, _ = oc.problem("box")
    X, cells = mesh.points, mesh.cells
    # push vertex 0 of cell 0 through its opposite face: x -> x - 2.5 (x - centroid of the face)
    v = cells[0][0]
    u = np.zeros_like(X)
    u[v] = -2.5 * (X[v] - X[cells[0][1:]].mean(axis=0))
    folded = [e for e in range(len(cells))
              if oc._vol(X[cells[e]].tolist()) * oc._vol((X + u)[cells[e]].tolist()) < 0.0]
    assert 0 in folded
    qs = [("sharp", -1.0, 1.0), ("mass", 0.0, 1.0), ("sharp", 0.3, 1.0)]
    want, _, sum_abs = oc.observe_mesh(X, cells, lab, c, qs, n_labels, u=u)
    signed = sum(oc._vol((X + u)[cl].tolist()) * (1.0 if oc._vol(X[cl].tolist()) >= 0 else -1.0) for cl in cells.tolist())
    assert signed < sum_abs - 1e-6                                             # (the folded cells do count negatively)
    h = _handle(backend, mesh, lab, n_labels)
    got = h.observe(qs, c=c, u=u, deformed=True)[0]
    oc.assert_close(got, want, len(cells), sum_abs, _xmax(mesh, u), "folded")
    bv, _ = oc.bound(len(cells), sum_abs, 1.0)
    assert abs(got[0, :, 0].sum() - signed) <= bv
    h.close()


# ---- 6. misuse --------------------------------------------------------------------------------------------------------------------
def _raw(backend, h, src, c, u, deformed, scale, qs, n_q=None, out=None, null=()):
    """glims_observe through ctypes with every argument in the caller's hands; returns (status, out)."""
    src = np.asarray(src, dtype=np.int64)
    arr = (backend.Observable * max(len(qs), 1))()
    for k, (kind, level, smooth) in enumerate(qs):
        arr[k].kind, arr[k].level, arr[k].smooth = kind, level, smooth
    n_q = len(qs) if n_q is None else n_q
    if out is None:
        out = np.full((max(len(src), 1), 16, h.n_labels or 1, 1 + h.dim), -7.0)
    dp = C.POINTER(C.c_double)
    args = dict(src=src.ctypes.data_as(C.POINTER(C.c_int64)), c=None if c is None else c.ctypes.data_as(dp),
                u=None if u is None else u.ctypes.data_as(dp), q=arr, out=out.ctypes.data_as(dp))
    for k in null:
        args[k] = None
    st = h.lib.glims_observe(h._h, len(src), args["src"], args["c"], args["u"], int(deformed), float(scale), n_q,
                             args["q"], args["out"])
    return st, out


def test_refusals(backend):
    mesh, lab, n_labels, c, u = oc.problem("rect")
    c, u = np.ascontiguousarray(c), np.ascontiguousarray(u).reshape(-1)
    H = backend.DERIVE_HOST
    sharp = [(1, 0.12, 1.0)]

    def refused(h, needle, *a, **kw):
        st, out = _raw(backend, h, *a, **kw)
        msg = (h.lib.glims_last_error(h._h) or b"").decode()
        assert st == backend.GLIMS_E_USAGE, (needle, st, msg)
        assert needle in msg, (needle, msg)
        assert np.all(out == -7.0), needle                                     # nothing written

    h = _handle(backend, mesh, lab, n_labels)
    refused(h, "unknown kind", [H], c, None, 0, 1.0, [(3, 0.1, 1.0)])
    refused(h, "unknown kind", [H], c, None, 0, 1.0, sharp + [(-1, 0.1, 1.0)])
    refused(h, "unknown snapshot", [0], None, None, 0, 1.0, sharp)
    refused(h, "unknown snapshot", [-3], None, None, 0, 1.0, sharp)
    refused(h, "outside 1..8", [H], c, None, 0, 1.0, sharp, n_q=0)
    refused(h, "outside 1..8", [H], c, None, 0, 1.0, sharp * 9)
    st, out = _raw(backend, h, [], c, None, 0, 1.0, sharp)
    assert st == backend.GLIMS_E_USAGE and b"n_src" in h.lib.glims_last_error(h._h) and np.all(out == -7.0)
    refused(h, "n_src = 1", [H, H], c, None, 0, 1.0, sharp)
    refused(h, "n_src = 1", [backend.DERIVE_CURRENT, backend.DERIVE_CURRENT], None, None, 0, 1.0, sharp)
    refused(h, "before glims_set_state", [backend.DERIVE_CURRENT], None, None, 0, 1.0, sharp)
    refused(h, "c_host", [H], None, None, 0, 1.0, sharp)
    refused(h, "u_host", [H], c, None, 1, 1.0, sharp)
    refused(h, "null pointer", [H], c, None, 0, 1.0, sharp, null=("q",))
    refused(h, "null pointer", [H], c, None, 0, 1.0, sharp, null=("src",))
    st, _ = _raw(backend, h, [H], c, None, 0, 1.0, sharp, null=("out",))
    assert st == backend.GLIMS_E_USAGE and b"null pointer" in h.lib.glims_last_error(h._h)
    refused(h, "smooth", [H], c, None, 0, 1.0, [(2, 0.1, 0.0)])
    refused(h, "smooth", [H], c, None, 0, 1.0, [(2, 0.1, -1.0)])
    refused(h, "scale", [H], c, u, 1, np.inf, sharp)
    refused(h, "scale", [H], c, u, 1, np.nan, sharp)
    refused(h, "level", [H], c, None, 0, 1.0, [(1, np.nan, 1.0)])
    refused(h, "level", [H], c, None, 0, 1.0, [(0, np.inf, 1.0)])
    assert h.observe_info() == {"cell_passes": 0, "elastic_solves": 0, "sources": 0}
    want = oc.reference("rect", False)
    got = h.observe(oc.QUERIES, c=c)[0]                                       # ... and the handle works
    oc.assert_close(got, want[0], len(mesh.cells), want[2], _xmax(mesh), "after the refusals")
    # a partitioned handle
    halo = backend.HALO_FN(lambda *a: 0)
    red = backend.ALLREDUCE_FN(lambda *a: 0)
    h.set_transport(0, 2, halo, red)
    refused(h, "partitioned", [H], c, None, 0, 1.0, sharp)
    h.set_transport(0, 1, halo, red)
    assert np.array_equal(h.observe(oc.QUERIES, c=c)[0], got)
    h.close()
    # before glims_setup
    h = backend.Handle(mesh.points, mesh.cells, lab)
    t = oc.tables(n_labels)
    h.set_materials(*[t[k] for k in ("D", "rho", "gamma", "E", "nu")])
    refused(h, "before glims_setup", [H], c, None, 0, 1.0, sharp)
    h.close()
    # deformed on a handle set up without mechanics
    h = _handle(backend, mesh, lab, n_labels, mechanics=False)
    refused(h, "needs the displacement", [H], c, u, 1, 1.0, sharp)
    assert np.array_equal(h.observe(oc.QUERIES, c=c)[0], got)
    h.close()


# ---- 7. public API ----------------------------------------------------------------------------------------------------------------
class _Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def _sim(dim, on_device):
    """A coupled two-tissue run (tissue B inside the disc / ball of derive_common.two_labels, A outside) whose initial tumour
    lies inside B."""
    from glimslib_amd.simulation import TumorGrowth
    mesh = oc.rectangle() if dim == 2 else oc.box()
    sim = TumorGrowth(mesh)
    zero = fenics.Constant(np.zeros(dim))
    sim.setup_global_parameters(subdomains=dc.two_labels(mesh), domain_names={1: 'A', 2: 'B'},
                                boundaries={'boundary_all': _Boundary()},
                                dirichlet_bcs={'clamp': {'bc_value': zero, 'named_boundary': 'boundary_all', 'subspace_id': 0}})
    model = {k: {'A': dc.TABLES[t][1], 'B': dc.TABLES[t][2]} for k, t in
             (('diffusion', 'D'), ('coupling', 'gamma'), ('proliferation', 'rho'), ('E', 'E'), ('poisson', 'nu'))}
    r2 = 'pow(x[0]-0.9,2)+pow(x[1]-0.45,2)' + ('+pow(x[2]-0.675,2)' if dim == 3 else '')
    iv = fenics.Expression('0.8*exp(-30*(%s))' % r2, degree=1)
    sim.setup_model_parameters(iv_expression={0: zero, 1: iv}, sim_time=3, sim_time_step=1, **model)
    sim.run(save_method=None, plot=False, results_on_device=on_device)
    return sim


def test_public_api(backend):
    sim = _sim(2, on_device=True)
    h = sim._backend
    steps = sim.results.get_recording_steps()
    n_cells, sum_abs = len(sim.mesh.cells), 2.0
    i0 = h.observe_info()
    vol = sim.compute_from_conc_for_each_time_step(threshold=0.05, computation='volume')
    i1 = h.observe_info()
    # one pass per step recorded on the device (step 0, the initial condition, is host-resident: numpy)
    n_dev = sum(getattr(sim.results.get_result(s).get_field(), 'snapshot_id', None) is not None for s in steps)
    assert n_dev >= len(steps) - 1 > 0
    assert i1["sources"] - i0["sources"] == n_dev == i1["cell_passes"] - i0["cell_passes"]
    assert list(vol.columns) == ['sim_time_step', 'all', 'a', 'b']
    assert list(vol['sim_time_step']) == list(steps)
    bv, bm = oc.bound(n_cells, sum_abs, _xmax(sim.mesh))
    assert np.abs(vol['all'] - (vol['a'] + vol['b'])).max() <= 4 * oc.EPS * sum_abs
    assert vol['b'][0] > 0.0 and vol['all'].iloc[-1] > 0.0
    com = sim.compute_from_conc_for_each_time_step(threshold=0.4, computation='com')
    assert list(com.columns) == ['sim_time_step', 'all_0', 'all_1', 'a_0', 'a_1', 'b_0', 'b_1']
    v4 = sim.compute_from_conc_for_each_time_step(threshold=0.4)
    assert v4['a'][0] == 0.0 and v4['b'][0] > 0.0
    assert np.isnan(com['a_0'][0]) and np.isnan(com['a_1'][0])                 # no tumour in tissue A at step 0
    assert abs(com['b_0'][0] - 0.9) < 0.1 and abs(com['b_1'][0] - 0.45) < 0.1
    # device=False (numpy on the downloaded fields) agrees with the device to the bound of (1)
    for kw in (dict(kind='sharp'), dict(kind='smooth', smooth=0.05), dict(kind='mass')):
        a = sim.compute_from_conc_for_each_time_step(threshold=0.05, device=None, **kw)
        b = sim.compute_from_conc_for_each_time_step(threshold=0.05, device=False, **kw)
        assert list(a.columns) == list(b.columns)
        err = np.abs(a.values[:, 1:] - b.values[:, 1:]).max()
        print(kw, "%.2e" % err, bv)
        assert err <= bv, (kw, err)
    # deformed: the device solves each step's displacement, numpy takes the results' lazily solved one -- two elastic solves of the
    # same system, each to the solver's tolerance
    dv = sim.compute_from_conc_for_each_time_step(threshold=0.05, deformed=True)
    dn = sim.compute_from_conc_for_each_time_step(threshold=0.05, deformed=True, device=False)
    assert np.abs(dv.values - dn.values).max() <= 1e-6 * sum_abs
    assert np.abs(dv['all'] - vol['all']).max() > 0.0
    # the raw table
    t, st = sim.observe([('sharp', 0.05), ('mass',)], steps=steps[-2:])
    assert t.shape == (2, 2, 3, 3) and st == list(steps[-2:])
    assert np.abs(t[:, 0, :, 0].sum(axis=1) - vol['all'].values[-2:]).max() <= 4 * oc.EPS * sum_abs
    # host-resident results: numpy unless device=True
    sim2 = _sim(2, on_device=False)
    p0 = sim2._backend.observe_info()["cell_passes"]
    a = sim2.compute_from_conc_for_each_time_step(threshold=0.05)
    assert sim2._backend.observe_info()["cell_passes"] == p0
    b = sim2.compute_from_conc_for_each_time_step(threshold=0.05, device=True)
    assert sim2._backend.observe_info()["cell_passes"] == p0 + len(steps)
    assert np.abs(a.values - b.values).max() <= bv and np.abs(a.values - vol.values).max() <= bv
