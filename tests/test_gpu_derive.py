"""
Derived fields on the device (glims_derive, csrc/derive.hip) against the numpy statement of tests/derive_common.py:
host-array mode on three meshes (a rectangle whose last 64-row slice is partial, a box of more than one cell-pass block, the
brain-like unstructured mesh with a curved two-tissue interface), snapshot mode after a coupled run, the counters of the
projected-stress cache, bitwise repeatability and forward bits, sampling of the device-resident result, the public API, and
every refusal.  Every mesh carries two labels that differ in all five materials.

Reference counterpart: the PostProcess classes, glimslib/simulation_helpers/helper_classes.py:1521-1972.
"""
import ctypes as C

import numpy as np
import pytest

from glimslib_amd import fenics_local as fenics
from oracle.glims_oracle import rel_l2

import derive_common as dc

pytestmark = pytest.mark.gpu

MESHES = ("rect", "box", "brain")
_cache = {}


def _problem(name):
    """(mesh, labels, reference, c, u), built once per session and never modified."""
    if name not in _cache:
        if name == "rect":
            mesh = fenics.RectangleMesh((0, 0), (2, 1), 12, 9)        # 130 nodes: three slices, the last partial
        elif name == "box":
            mesh = fenics.BoxMesh((0, 0, 0), (2, 1, 1.5), 5, 4, 4)    # 150 nodes, 480 cells: two blocks of the cell pass
        else:
            from glimslib_amd import workloads
            mesh = workloads.config_brain_like(24000, isolate=True).mesh
        lab = dc.two_labels(mesh)
        assert set(np.unique(lab)) == {1, 2}
        ref = dc.DeriveReference(mesh.points, mesh.cells, lab, dc.TABLES)
        c, u = dc.sample_fields(mesh.points, seed=len(mesh.points))
        _cache[name] = (mesh, lab, ref, c, u)
    return _cache[name]


def _handle(backend, mesh, lab, mechanics=True, tables=dc.TABLES):
    h = backend.Handle(mesh.points, mesh.cells, lab)
    h.set_materials(*[tables[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=1.0)
    if mechanics:
        f = mesh.facets()
        bn = np.unique(f['vertices'][f['exterior']])
        d = mesh.points.shape[1]
        dofs = (bn[:, None] * d + np.arange(d)).ravel()
        h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
    h.setup(mechanics)
    return h


def _host_args(kind, c, u):
    return dict(c=c if kind in dc.NEEDS_C else None, u=u if kind in dc.NEEDS_U else None)


# ---- 1. host mode against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_host_mode_matches_reference(backend, name):
    mesh, lab, ref, c, u = _problem(name)
    h = _handle(backend, mesh, lab)
    worst = {}
    for kind in dc.KINDS:
        got = h.derive(kind, rtol=1e-12, **_host_args(kind, c, u))
        want = ref.field(kind, c=c, u=u)
        assert got.shape == want.shape, kind
        worst[kind] = rel_l2(got, want)
    print(name, {k: "%.2e" % v for k, v in worst.items()})
    h.close()
    assert max(worst.values()) <= 1e-10, worst


@pytest.mark.parametrize("dim", [2, 3])
def test_host_mode_known_answers(backend, dim):
    """u = A x, c = c0 on a one-tissue mesh: every field is a constant that the P1 space holds exactly."""
    mesh = _problem("rect" if dim == 2 else "box")[0]
    h = _handle(backend, mesh, np.ones(len(mesh.cells), dtype=np.int32))
    A = 0.01 * (np.arange(dim * dim).reshape(dim, dim) + 1.0)
    A[0, 0] += 0.03
    c0 = 0.35
    u, c = mesh.points @ A.T, np.full(len(mesh.points), c0)
    E, nu, gamma, rho = (dc.TABLES[k][1] for k in ("E", "nu", "gamma", "rho"))
    eps = 0.5 * (A + A.T)
    mu, lam = E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))
    sig = 2 * mu * eps + lam * np.trace(eps) * np.eye(dim)
    dev = sig - np.trace(sig) / 3.0 * np.eye(dim)
    jt = np.linalg.det(np.eye(dim) + A)
    answers = {"strain_tensor": eps, "stress_tensor": sig, "pressure": np.trace(sig) / 3.0,
               "van_mises_stress": np.sqrt(1.5 * (dev * dev).sum()), "log_growth": rho * c0 * (1 - c0),
               "mech_expansion": gamma * c0, "total_jacobian": jt, "growth_induced_jacobian": (1 + gamma * c0) ** dim,
               "concentration_deformed_config": c0 * (1 + gamma * c0) ** dim / jt}
    for kind, val in answers.items():
        got = h.derive(kind, **_host_args(kind, c, u))
        err = rel_l2(got, np.broadcast_to(val, got.shape))
        print(dim, kind, "%.2e" % err)
        assert err <= 1e-10, (kind, err)
    h.close()


# ---- 2. snapshot mode --------------------------------------------------------------------------------------------------------
def _coupled_run(backend, name, n_steps=3):
    mesh, lab, ref, _, _ = _problem(name)
    h = _handle(backend, mesh, lab)
    X = mesh.points
    ctr = X.min(axis=0) + 0.45 * (X.max(axis=0) - X.min(axis=0))
    h.set_state(0.8 * np.exp(-4.0 * ((X - ctr) ** 2).sum(axis=1)))
    ids = []
    for _ in range(n_steps):
        assert h.step(1) == backend.GLIMS_OK
        ids.append(h.snapshot_save())
    return h, ref, ids


@pytest.mark.parametrize("name", ["rect", "box"])
def test_snapshot_mode_matches_reference(backend, name):
    h, ref, ids = _coupled_run(backend, name)
    for sid in ids[-2:]:
        got = {kind: h.derive(kind, snapshot=sid) for kind in dc.KINDS}     # one elastic solve, from the derive's own guess
        c = h.snapshot_load(sid)
        u, st = h.snapshot_mechanics(sid)                                   # solved again, from the solve history
        assert st == backend.GLIMS_OK
        for kind in dc.KINDS:
            err = rel_l2(got[kind], ref.field(kind, c=c, u=u))
            print(name, sid, kind, "%.2e" % err)
            assert err <= 1e-8, (kind, err)
    # the handle's own state as it stands against the same arrays through the host
    assert h.solve_mechanics() == backend.GLIMS_OK
    c, u = h.get_state()
    for kind in dc.KINDS:
        assert np.array_equal(h.derive(kind), h.derive(kind, **_host_args(kind, c, u))), kind
    h.close()


# ---- 3. counters -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "box"])
def test_counters_of_the_stress_cache(backend, name):
    h, ref, ids = _coupled_run(backend, name, n_steps=2)
    d = ref.d
    ns = d * (d + 1) // 2
    i0 = h.derive_info()
    h.derive("pressure", snapshot=ids[-1])
    h.derive("van_mises_stress", snapshot=ids[-1])
    i1 = h.derive_info()
    delta = {k: i1[k] - i0[k] for k in i1}
    assert delta == {"cell_passes": 2, "mass_solves": ns + 1, "elastic_solves": 1, "cache_hits": 1}, delta
    h.derive("stress_tensor", snapshot=ids[-1])                             # a third kind of the same step: no solve at all
    i2 = h.derive_info()
    assert (i2["mass_solves"], i2["elastic_solves"], i2["cache_hits"]) == (i1["mass_solves"], i1["elastic_solves"], i1["cache_hits"] + 1)
    assert h.step(1) == backend.GLIMS_OK                                    # forgets whose displacement U holds
    h.derive("pressure", snapshot=ids[-1])
    h.derive("van_mises_stress", snapshot=ids[-1])
    i3 = h.derive_info()
    delta = {k: i3[k] - i2[k] for k in i3}
    assert delta == {"cell_passes": 2, "mass_solves": ns + 1, "elastic_solves": 1, "cache_hits": 1}, delta
    # glims_snapshot_mechanics sets the memory: the derive that follows does not solve again
    h.snapshot_mechanics(ids[0])
    h.derive("displacement_norm", snapshot=ids[0])
    assert h.derive_info()["elastic_solves"] == i3["elastic_solves"]
    h.close()


# ---- 4. bits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "box"])
def test_same_bits_on_every_call_and_in_the_steps_that_follow(backend, name):
    mesh, lab, ref, c, u = _problem(name)
    h = _handle(backend, mesh, lab)
    for kind in dc.KINDS:
        a = h.derive(kind, **_host_args(kind, c, u))
        b = h.derive(kind, **_host_args(kind, c, u))
        assert np.array_equal(a, b), kind
    h.close()
    runs = []
    for derive in (True, False):
        h, _, ids = _coupled_run(backend, name, n_steps=2)
        if derive:
            h.derive("van_mises_stress", snapshot=ids[-1])
            h.derive("log_growth")
            h.derive("growth_induced_jacobian", snapshot=ids[0])
        s0 = h.stats()
        assert h.step(2) == backend.GLIMS_OK
        s1 = h.stats()
        runs.append((h.get_state(want_u=False)[0],
                     {k: s1[k] - s0[k] for k in ("steps", "newton_its", "cg_its", "cheb_solves", "cheb_its")}))
        h.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1], runs


# ---- 5. sampling the device-resident result -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "box"])
def test_sampling_the_derived_field(backend, name):
    mesh, lab, ref, c, u = _problem(name)
    d = ref.d
    h = _handle(backend, mesh, lab)
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    size = np.array([11, 7, 5][:d])
    origin = lo - 0.113 * (hi - lo)                                          # a grid that sticks out of the mesh on every side
    spacing = 1.226 * (hi - lo) / (size - 1)
    sm = h.sampler_grid(origin, spacing, size)
    outside = sm.cells < 0
    assert outside.any() and (~outside).any()
    for kind in ("van_mises_stress", "pressure", "stress_tensor", "strain_tensor"):
        nodal = h.derive(kind, **_host_args(kind, c, u))
        img = sm.apply('derived', fill=-7.0)
        if nodal.ndim == 3:
            nodal = dc.sym_components(nodal)
            assert img.shape == (sm.n_points, d * (d + 1) // 2)
        else:
            assert img.shape == (sm.n_points,)
        assert np.array_equal(img, sm.apply(nodal, fill=-7.0)), kind
        assert np.all(img[outside] == -7.0)
    # fetch=False leaves the same result on the device
    assert h.derive("pressure", fetch=False, **_host_args("pressure", c, u)) is None
    nodal = h.derive("pressure", **_host_args("pressure", c, u))
    assert np.array_equal(sm.apply('derived'), sm.apply(nodal), equal_nan=True)
    h.close()


# ---- 7. misuse ---------------------------------------------------------------------------------------------------------------
def _refused(backend, call, needle):
    with pytest.raises(backend.BackendError) as ei:
        call()
    assert ei.value.code == backend.GLIMS_E_USAGE, ei.value
    assert needle in str(ei.value), (needle, str(ei.value))


def test_refusals(backend):
    mesh, lab, ref, c, u = _problem("rect")
    h = _handle(backend, mesh, lab)
    sm = h.sampler_points(mesh.points[:5] * 0.999 + 1e-4)
    _refused(backend, lambda: sm.apply('derived'), "nothing derived")
    _refused(backend, lambda: h.derive("log_growth"), "before glims_set_state")
    _refused(backend, lambda: h.derive(10, c=c, u=u), "unknown kind")
    _refused(backend, lambda: h.derive(-1, c=c, u=u), "unknown kind")
    _refused(backend, lambda: h.derive("pressure", snapshot=3), "unknown snapshot")
    _refused(backend, lambda: h.derive("pressure", c=c), "u_host")
    _refused(backend, lambda: h.derive("log_growth", u=u), "c_host")
    _refused(backend, lambda: h.derive("log_growth", c=c, rtol=0.0), "rtol")
    _refused(backend, lambda: h.derive("log_growth", c=c, rtol=-1e-3), "rtol")
    assert h.derive_info() == {"cell_passes": 0, "mass_solves": 0, "elastic_solves": 0, "cache_hits": 0}
    _refused(backend, lambda: sm.apply('derived'), "nothing derived")
    want = ref.field("log_growth", c=c)
    assert rel_l2(h.derive("log_growth", c=c), want) <= 1e-10              # ... and the handle works
    # another component count than the result's
    out = np.empty((sm.n_points, 3))
    st = h.lib.glims_sampler_apply(h._h, sm.id, backend.FIELD_DERIVED, -1, None, 3, 0.0,
                                   out.ctypes.data_as(C.POINTER(C.c_double)))
    assert st == backend.GLIMS_E_USAGE and b"component" in h.lib.glims_last_error(h._h)
    keep = sm.apply('derived')
    _refused(backend, lambda: h.derive("pressure", snapshot=0), "unknown snapshot")
    assert np.array_equal(sm.apply('derived'), keep)                        # a refused call leaves the earlier result
    # a partitioned handle
    halo = backend.HALO_FN(lambda *a: 0)
    red = backend.ALLREDUCE_FN(lambda *a: 0)
    h.set_transport(0, 2, halo, red)
    _refused(backend, lambda: h.derive("log_growth", c=c), "partitioned")
    h.set_transport(0, 1, halo, red)
    assert rel_l2(h.derive("log_growth", c=c), want) <= 1e-10
    h.close()
    # before glims_setup
    h = backend.Handle(mesh.points, mesh.cells, lab)
    _refused(backend, lambda: h.derive("log_growth", c=c), "before glims_setup")
    h.close()
    # a kind that needs u on a handle set up without mechanics
    h = _handle(backend, mesh, lab, mechanics=False)
    _refused(backend, lambda: h.derive("pressure", c=c, u=u), "needs the displacement")
    _refused(backend, lambda: h.derive("concentration_deformed_config", c=c, u=u), "needs the displacement")
    assert rel_l2(h.derive("log_growth", c=c), want) <= 1e-10
    h.close()


# ---- 6. public API -----------------------------------------------------------------------------------------------------------
class _Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def _sim(dim, on_device, iv=None, two_tissues=True, mechanics=True):
    """A coupled run; with two_tissues the tissues A / B of derive_common.two_labels differ in all five materials (the
    projected gamma_T c_h branch of the growth strain), else one tissue with the scalars of the known-answer tests."""
    from glimslib_amd.simulation import TumorGrowth
    mesh = (fenics.RectangleMesh((0, 0), (2, 1), 12, 9) if dim == 2 else fenics.BoxMesh((0, 0, 0), (2, 1, 1.5), 5, 4, 4))
    sim = TumorGrowth(mesh, **({} if mechanics else {'solver_options': {'mechanics': False}}))
    zero = fenics.Constant(np.zeros(dim))
    glob = dict(boundaries={'boundary_all': _Boundary()},
                dirichlet_bcs={'clamp': {'bc_value': zero, 'named_boundary': 'boundary_all', 'subspace_id': 0}})
    if two_tissues:
        glob.update(subdomains=dc.two_labels(mesh), domain_names={1: 'A', 2: 'B'})
        model = {k: {'A': dc.TABLES[t][1], 'B': dc.TABLES[t][2]} for k, t in
                 (('diffusion', 'D'), ('coupling', 'gamma'), ('proliferation', 'rho'), ('E', 'E'), ('poisson', 'nu'))}
    else:
        model = dict(diffusion=0.1, coupling=0.2, proliferation=0.1, E=0.003, poisson=0.4)
    sim.setup_global_parameters(**glob)
    if iv is None:
        iv = fenics.Expression('0.8*exp(-4*(pow(x[0]-0.9,2)+pow(x[1]-0.45,2)))', degree=1)
    sim.setup_model_parameters(iv_expression={0: zero, 1: iv}, sim_time=3, sim_time_step=1, **model)
    sim.run(save_method=None, plot=False, results_on_device=on_device)
    return sim


_GET = {"strain_tensor": "get_strain_tensor", "stress_tensor": "get_stress_tensor", "pressure": "get_pressure",
        "van_mises_stress": "get_van_mises_stress", "displacement_norm": "get_displacement_norm",
        "log_growth": "get_logistic_growth", "mech_expansion": "get_mech_expansion", "total_jacobian": "get_total_jacobian",
        "growth_induced_jacobian": "get_growth_induced_jacobian",
        "concentration_deformed_config": "get_concentration_deformed_configuration"}
_SAVED = ("concentration", "displacement", "pressure", "van_mises_stress", "total_jacobian", "growth_induced_jacobian",
          "concentration_deformed_config", "log_growth")


@pytest.mark.parametrize("dim", [2, 3])
def test_postprocess_takes_the_device_path(backend, dim, tmp_path):
    sim = _sim(dim, on_device=True)
    h = sim._backend
    ns = dim * (dim + 1) // 2
    steps = sim.results.get_recording_steps()
    pp = sim.init_postprocess(str(tmp_path / "dev"))
    assert pp.on_device(steps[-1])
    # save_all of one step: one elastic solve, the stress projected once
    i0, m0 = h.derive_info(), h.stats()['mech_solves']
    files = pp.save_all(selection=slice(-2, -1))
    i1, m1 = h.derive_info(), h.stats()['mech_solves']
    assert m1 - m0 == 1
    assert i1["cache_hits"] - i0["cache_hits"] == 1
    # stress; von Mises, total Jacobian, deformed c, growth: one each; growth-induced Jacobian: two (gamma_T c_h projected first)
    assert i1["mass_solves"] - i0["mass_solves"] == ns + 6
    twin = sim._make_postprocess(str(tmp_path / "np"), False)
    assert not twin.on_device(steps[-1])
    files_np = twin.save_all(selection=slice(-2, -1))
    assert h.derive_info() == i1                                # the numpy twin never derives on the device
    text, text_np = open(files[0]).read(), open(files_np[0]).read()
    for name in _SAVED:
        assert 'Name="%s"' % name in text and 'Name="%s"' % name in text_np, name
    assert text.count("<DataArray") == text_np.count("<DataArray")
    for step in steps[-2:]:
        before = h.derive_info()["cell_passes"]
        for kind, get in _GET.items():
            a, b = getattr(pp, get)(step).values(), getattr(twin, get)(step).values()
            assert a.shape == b.shape
            err = rel_l2(a, b)
            print(dim, step, kind, "%.2e" % err)
            assert err <= 1e-8, (kind, err)
        assert h.derive_info()["cell_passes"] > before
    assert np.allclose(pp.compute_force(steps[-1]), twin.compute_force(steps[-1]), rtol=0, atol=1e-8 * 0.003)
    # images of derived fields: derived and sampled on the device
    lo, hi = sim.mesh.points.min(axis=0), sim.mesh.points.max(axis=0)
    size = [9, 6, 5][:dim]
    grid = dict(origin=lo - 0.05 * (hi - lo), spacing=1.1 * (hi - lo) / (np.array(size) - 1), size=size)
    _, sampler = sim._grid_sampler(grid["origin"], grid["spacing"], grid["size"])
    img = sim.sample_image('pressure', steps[-1], **grid)
    want = sampler.apply(pp.get_pressure(steps[-1]).values())
    assert img.array.shape == tuple(reversed(size)) and np.isnan(img.array).any()
    assert np.array_equal(img.array.reshape(-1), want, equal_nan=True)
    img = sim.sample_image('stress_tensor', steps[-1], **grid)
    want = sampler.apply(dc.sym_components(pp.get_stress_tensor(steps[-1]).values()))
    assert img.array.shape == tuple(reversed(size)) + (ns,)
    assert np.array_equal(img.array.reshape(-1, ns), want, equal_nan=True)
    # the solver's displacement buffer belongs to a recorded step now: the next sync solves again
    assert sim.solver._mech_current is False
    sim.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_forced_device_path_on_host_resident_results(backend, dim, tmp_path):
    """device=True: host arrays go through GLIMS_DERIVE_HOST -- whatever the caller wrote into them included."""
    gamma, rho, E, nu, c0 = 0.2, 0.1, 0.003, 0.4, 0.35
    sim = _sim(dim, on_device=False, iv=fenics.Constant(0.3), two_tissues=False)
    pp = sim.init_postprocess(str(tmp_path), device=True)
    default = sim._make_postprocess(None, None)
    mesh = sim.mesh
    last = sim.results.get_recording_steps()[-1]
    assert pp.on_device(last) and not default.on_device(last)              # host-resident results stay with numpy by default
    A = 0.01 * (np.arange(dim * dim).reshape(dim, dim) + 1.0)
    A[0, 0] += 0.03
    field = sim.results.get_result(last).get_field()
    field.components[0] = mesh.points @ A.T
    field.components[1] = np.full(mesh.num_vertices(), c0)
    eps = 0.5 * (A + A.T)
    mu, lam = E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))
    sig = 2 * mu * eps + lam * np.trace(eps) * np.eye(dim)
    dev = sig - np.trace(sig) / 3.0 * np.eye(dim)
    jt = np.linalg.det(np.eye(dim) + A)
    answers = {"strain_tensor": eps, "stress_tensor": sig, "pressure": np.trace(sig) / 3.0,
               "van_mises_stress": np.sqrt(1.5 * (dev * dev).sum()), "log_growth": rho * c0 * (1 - c0),
               "mech_expansion": c0 * gamma * np.eye(dim), "total_jacobian": jt,
               "growth_induced_jacobian": (1 + gamma * c0) ** dim,
               "concentration_deformed_config": c0 * (1 + gamma * c0) ** dim / jt}
    before = sim._backend.derive_info()["cell_passes"]
    for kind, val in answers.items():
        got = getattr(pp, _GET[kind])().values()
        assert rel_l2(got, np.broadcast_to(val, got.shape)) <= 1e-10, kind
    assert sim._backend.derive_info()["cell_passes"] > before
    assert np.abs(np.asarray(pp.compute_force())).max() < 1e-10 * np.abs(sig).max()
    sim.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_run_without_mechanics_behaves_as_before(backend, dim, tmp_path):
    """solver_options={'mechanics': False}: the results hold u = 0 and the device has no displacement.  The fields that read u
    stay with numpy (zero stress, J = 1, c (1 + gamma c)^d), the others take the device path, and save_all writes its file --
    as a device=False twin does."""
    sim = _sim(dim, on_device=True, mechanics=False)
    h = sim._backend
    steps = sim.results.get_recording_steps()
    pp = sim.init_postprocess(str(tmp_path / "dev"))
    twin = sim._make_postprocess(str(tmp_path / "np"), False)
    assert pp.on_device(steps[-1]) and pp.on_device(steps[-1], "log_growth") and not pp.on_device(steps[-1], "pressure")
    i0 = h.derive_info()
    files, files_np = pp.save_all(selection=slice(-1, None)), twin.save_all(selection=slice(-1, None))
    i1 = h.derive_info()
    assert i1["elastic_solves"] == i0["elastic_solves"] and i1["cell_passes"] > i0["cell_passes"]
    text, text_np = open(files[0]).read(), open(files_np[0]).read()
    for name in _SAVED:
        assert 'Name="%s"' % name in text and 'Name="%s"' % name in text_np, name
    for kind, get in _GET.items():
        a, b = getattr(pp, get)(steps[-1]).values(), getattr(twin, get)(steps[-1]).values()
        assert a.shape == b.shape and rel_l2(a, b) <= 1e-8, kind
    assert np.abs(pp.get_stress_tensor(steps[-1]).values()).max() == 0.0
    assert np.abs(pp.get_total_jacobian(steps[-1]).values() - 1.0).max() < 1e-10
    assert np.abs(np.asarray(pp.compute_force(steps[-1]))).max() == 0.0
    lo, hi = sim.mesh.points.min(axis=0), sim.mesh.points.max(axis=0)
    size = [9, 6, 5][:dim]
    grid = dict(origin=lo + 0.01 * (hi - lo), spacing=0.98 * (hi - lo) / (np.array(size) - 1), size=size)
    assert np.nanmax(np.abs(sim.sample_image('pressure', steps[-1], **grid).array)) == 0.0      # numpy field, sampled
    assert np.nanmax(sim.sample_image('log_growth', steps[-1], **grid).array) > 0.0            # derived on the device
    sim.close()


def test_stress_cache_respects_the_tolerance(backend):
    """A stress projected loosely is not handed to a call that asks for a tighter solve; the other way round it is."""
    h, ref, ids = _coupled_run(backend, "box", n_steps=2)
    ns = 6
    h.derive("pressure", snapshot=ids[-1], rtol=1e-3)
    i0 = h.derive_info()
    tight = h.derive("van_mises_stress", snapshot=ids[-1], rtol=1e-12)
    i1 = h.derive_info()
    assert (i1["mass_solves"] - i0["mass_solves"], i1["cache_hits"] - i0["cache_hits"]) == (ns + 1, 0)
    h.derive("pressure", snapshot=ids[-1], rtol=1e-6)                      # the tight stress serves a looser call
    i2 = h.derive_info()
    assert (i2["mass_solves"] - i1["mass_solves"], i2["cache_hits"] - i1["cache_hits"]) == (0, 1)
    c = h.snapshot_load(ids[-1])
    u, _ = h.snapshot_mechanics(ids[-1])
    assert rel_l2(tight, ref.field("van_mises_stress", c=c, u=u)) <= 1e-8
    h.close()
