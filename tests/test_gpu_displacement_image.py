"""
Displacement-image misfit terms on the GPU (glims_adjoint_displacement_image_terms / _info; k_uimg_prepare, k_uimg_misfit,
k_uimg_misfit_dir and the device transposes): J, the gradient in D, rho, gamma, E, nu and c0 and the Hessian-vector products
against the numpy statement of tests/displacement_image_common.py (itself checked by central differences in
tests/test_displacement_image_cpu.py), the bitwise guarantees, the shared elastic solves, and the refusals.
"""
import ctypes as C

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as in test_gpu_adjoint_image.py)
import torch  # noqa: F401

import adjoint_deformed_common as adc
import displacement_image_common as dic
from adjoint_common import Problem
from adjoint_hessian_elastic_common import unit_directions
from test_gpu_adjoint import _handle, _record, _rel

pytestmark = pytest.mark.gpu

OUT = ("J", "D", "rho", "gamma", "c0", "E", "nu")
TOL = 1e-8       # tests/test_gpu_adjoint_image.py::_compare_gradient, :194-199; tests/test_gpu_adjoint_elastic.py:150-151
N = 4


def _problem(dim):
    return dic.clamped_problem(2, 9) if dim == 2 else dic.clamped_problem(3, 5)


def _attach(h, terms):
    """The library's sampler of every displacement image term: one per grid, one per point array."""
    made = {}
    for t in terms:
        if t["kind"] == dic.KIND and "sampler" not in t:
            key = id(t["x"]) if t["grid"] is None else tuple(np.ravel(np.concatenate([np.ravel(a) for a in t["grid"]])))
            if key not in made:
                made[key] = h.sampler_grid(*t["grid"]) if t["grid"] is not None else h.sampler_points(t["x"])
            t["sampler"] = made[key]
    return terms


def _gradient(h, terms, L):
    return dict(zip(OUT, h.adjoint_gradient(terms, L, elastic=True)))


def _same(a, b, keys):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)


@pytest.fixture(scope="module", params=[2, 3])
def case(request, backend):
    """One recorded run per dimension with the standard term list, the device's own trajectory and the numpy sweep on it
    (gradient and the products of the shared directions)."""
    dim = request.param
    prob = _problem(dim)
    terms = dic.standard_terms(prob, N, seed=dim)
    h = _handle(backend, prob)
    _attach(h, terms)
    traj = _record(h, N)
    rng = np.random.default_rng(13)
    L, n = prob.n_labels, len(prob.points)
    dirs = [dict(D=prob.D * rng.uniform(-1, 1, L), rho=prob.rho * rng.uniform(-1, 1, L), gamma=prob.gamma * rng.uniform(-1, 1, L),
                 c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)),
            dict(gamma=prob.gamma * rng.uniform(-1, 1, L)),
            dict(c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1), D=prob.D * rng.uniform(-1, 1, L))]
    full = [dict(dirs[0], E=prob.E * rng.uniform(-1, 1, L), nu=0.1 * rng.uniform(-1, 1, L)),
            dict(E=prob.E * rng.uniform(-1, 1, L)), dict(nu=0.1 * rng.uniform(-1, 1, L))]
    ref = dic.sweep(prob, dic.oracle_of(prob), traj, terms, dirs + full)
    yield dict(prob=prob, h=h, terms=terms, traj=traj, dirs=dirs, full=full, ref=ref, backend=backend)
    h.close()


# ---- 1. the gradient against numpy -----------------------------------------------------------------------------------------------
def test_gradient_and_J_match_the_numpy_statement(case):
    prob, h, terms = case["prob"], case["h"], case["terms"]
    s0 = h.adjoint_stats()["mech_solves"]
    g = _gradient(h, terms, prob.n_labels)
    J, ref, _ = case["ref"]
    ref = dict(ref, J=J)
    for key in OUT:
        print("%d-D %s: rel. difference to numpy %.3e" % (prob.dim, key, _rel(g[key], ref[key])))
    for key in OUT:
        assert _rel(g[key], ref[key]) <= TOL, (key, g[key], ref[key])
    assert J > 0 and all(np.all(g[key] != 0.0) for key in OUT[1:])
    for k, t in enumerate(dic.displacement_terms(terms)):
        ok, _ = dic.observed(t)
        assert h.displacement_image_term_info(k) == (t["sampler"].id, len(ok), int(ok.sum())), k
    # u_k and mu_k once at each of the three observed steps, whatever the number of terms there
    assert h.adjoint_stats()["mech_solves"] - s0 == 6


def test_displacement_image_terms_alone_give_gamma_E_and_nu(case):
    """No nodal displacement term: before this term existed, image data in the reference configuration gave exact zeros here."""
    prob, h = case["prob"], case["h"]
    only = dic.displacement_terms(case["terms"])
    g = _gradient(h, only, prob.n_labels)
    J, ref, _ = dic.sweep(prob, dic.oracle_of(prob), case["traj"], only)
    assert _rel(g["J"], J) <= TOL
    for key in ("gamma", "E", "nu"):
        assert np.all(g[key] != 0.0) and _rel(g[key], ref[key]) <= TOL, (key, g[key], ref[key])


# ---- 2. second order ---------------------------------------------------------------------------------------------------------------
def test_hessian_products_match_the_numpy_second_order_recursion(case):
    prob, h, terms, dirs, full = case["prob"], case["h"], case["terms"], case["dirs"], case["full"]
    J, g, hv = case["ref"]
    r = h.adjoint_hessian(terms, dirs)
    rf = h.adjoint_hessian_full(terms, full)
    g1 = _gradient(h, terms, prob.n_labels)
    for res, keys, hvs in ((r, ("D", "rho", "gamma", "c0"), hv[:len(dirs)]), (rf, ("D", "rho", "gamma", "c0", "E", "nu"), hv[len(dirs):])):
        assert res["J"] == g1["J"] and _same(res, g1, keys)       # J and the gradient are bitwise the gradient call's
        assert _rel(res["J"], J) <= TOL
        for key in keys:
            assert _rel(res[key], g[key]) <= TOL, (key, res[key], g[key])
        for p, want in enumerate(hvs):
            for key in keys:
                e = _rel(res["hv_" + key][p], want[key])
                print("%d-D column %d of %d, hv_%s: rel. difference to numpy %.3e" % (prob.dim, p, len(hvs), key, e))
                assert e <= TOL, (p, key, res["hv_" + key][p], want[key])
    # an n-direction call equals the one-direction calls bitwise
    for j in range(len(dirs)):
        r1 = h.adjoint_hessian(terms, [dirs[j]])
        for key in ("hv_D", "hv_rho", "hv_gamma", "hv_c0"):
            assert np.array_equal(r[key][j], r1[key][0]), (j, key)
    for j in range(len(full)):
        r1 = h.adjoint_hessian_full(terms, [full[j]])
        for key in ("hv_D", "hv_rho", "hv_gamma", "hv_c0", "hv_E", "hv_nu"):
            assert np.array_equal(rf[key][j], r1[key][0]), (j, key)


def test_control_space_hessian_is_symmetric(case):
    prob, h, terms = case["prob"], case["h"], case["terms"]
    dirs = unit_directions(prob)                       # (D, rho, gamma, E, nu) x labels
    cols = []
    for j in range(0, len(dirs), 8):
        r = h.adjoint_hessian_full(terms, dirs[j:j + 8])
        cols += [np.concatenate([r["hv_" + k][p] for k in dic.KEYS]) for p in range(len(dirs[j:j + 8]))]
    H = np.array(cols).T
    print("%d-D asymmetry %.3e of max |H| %.3e" % (prob.dim, np.abs(H - H.T).max(), np.abs(H).max()))
    assert H.shape == (5 * prob.n_labels,) * 2 and np.abs(H - H.T).max() <= TOL * np.abs(H).max(), H


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------
def test_bits(case):
    prob, h, terms = case["prob"], case["h"], case["terms"]
    L = prob.n_labels
    nodal = [t for t in terms if t["kind"] != dic.KIND]
    d = [case["full"][0]]
    hkeys = ("J",) + tuple("hv_" + k for k in ("D", "rho", "gamma", "c0", "E", "nu"))
    # the same call twice
    g1, g2 = _gradient(h, terms, L), _gradient(h, terms, L)
    assert _same(g1, g2, OUT)
    h1, h2 = h.adjoint_hessian_full(terms, d), h.adjoint_hessian_full(terms, d)
    assert _same(h1, h2, hkeys)
    # NaNs in an ignored component against zeros there
    t = dic.displacement_terms(terms)[2]
    ignored = t["cweight"] == 0.0
    assert ignored.any() and np.isnan(t["target"][:, ignored]).any()
    clean = dict(t, target=np.where(ignored[None], 0.0, t["target"]))
    ga, gb = _gradient(h, [t], L), _gradient(h, [clean], L)
    assert ga["J"] > 0 and _same(ga, gb, OUT)
    assert _same(h.adjoint_hessian_full([t], d), h.adjoint_hessian_full([clean], d), hkeys)
    # scale = 0: exactly zero derivatives
    zero = [dict(w, scale=0.0) for w in dic.displacement_terms(terms)]
    gz = _gradient(h, zero, L)
    assert gz["J"] > 0 and all(not np.any(gz[k]) for k in OUT[1:])
    hz = h.adjoint_hessian_full(zero, d)
    assert all(not np.any(hz[k]) for k in hkeys[1:])
    # a list without a displacement image term: the bits of before one was stored and cleared
    a = _handle(case["backend"], prob)
    a.adjoint_record(True)
    assert a.step(N) == 0
    g0, h0 = _gradient(a, nodal, L), a.adjoint_hessian_full(nodal, d)
    aa = a.adjoint_stats()
    own = [dict(w) for w in dic.displacement_terms(terms)]
    for w in own:
        del w["sampler"]
    a.set_displacement_image_terms(_attach(a, own))
    assert a.adjoint_stats() == aa                                 # the new entry points count nowhere
    gs = _gradient(a, nodal, L)                                    # (stored by the entry point itself: they stay)
    assert gs["J"] != g0["J"] and _rel(gs["J"], g1["J"]) <= 1e-9
    a.set_displacement_image_terms([])
    g3, h3 = _gradient(a, nodal, L), a.adjoint_hessian_full(nodal, d)
    assert _same(g0, g3, OUT) and _same(h0, h3, hkeys + ("D", "rho", "gamma", "c0", "E", "nu"))
    with pytest.raises(case["backend"].BackendError):
        a.displacement_image_term_info(0)
    a.close()


# ---- 4. shared solves ------------------------------------------------------------------------------------------------------------
def test_one_u_solve_and_one_mu_solve_per_step(backend):
    prob = _problem(2)
    terms = dic.standard_terms(prob, N, seed=5)
    warp = dic.displacement_terms(terms)[0]
    u_l2 = [t for t in terms if t["kind"] == "u_l2"][0]
    rng = np.random.default_rng(2)
    moving = adc.deformed_term(warp["x"], N, "img_l2", rng.uniform(0, 0.6, len(warp["x"])), None, weight=0.7,
                               grid=warp["grid"])
    assert warp["step"] == u_l2["step"] == moving["step"] == N
    h = _handle(backend, prob)
    _attach(h, [warp])
    _record(h, N)
    s0 = h.adjoint_stats()["mech_solves"]
    h.adjoint_gradient([u_l2, warp, moving], prob.n_labels, elastic=True)
    s1 = h.adjoint_stats()["mech_solves"]
    assert s1 - s0 == 2, (s0, s1)
    h.adjoint_gradient([warp], prob.n_labels)
    assert h.adjoint_stats()["mech_solves"] - s1 == 2
    h.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_misuse_gives_usage_status_not_a_fault(backend):
    prob = _problem(2)
    terms = _attach_free(dic.displacement_terms(dic.standard_terms(prob, N, seed=7)))
    h = _handle(backend, prob)
    _attach(h, terms)
    _record(h, N)
    h.set_displacement_image_terms(terms)
    J0 = h.adjoint_gradient([], 2)[0]
    good = terms[0]
    n = len(good["x"])
    info1 = h.displacement_image_term_info(1)

    def usage(fn, match):
        with pytest.raises(backend.BackendError) as e:
            fn()
        assert e.value.code == backend.GLIMS_E_USAGE, e.value
        assert match in str(e.value), e.value
        assert h.displacement_image_term_info(1) == info1 and h.adjoint_gradient([], 2)[0] == J0   # the old list is in place

    send = h.set_displacement_image_terms
    usage(lambda: send([dict(good, weight=np.nan)]), "weight")
    usage(lambda: send([good, dict(good, scale=np.inf)]), "scale")
    bad_q = np.ones(n)
    bad_q[5] = -1.0
    usage(lambda: send([dict(good, pweight=bad_q)]), "pweight[5]")
    bad_q[5] = np.nan
    usage(lambda: send([dict(good, pweight=bad_q)]), "pweight[5]")
    usage(lambda: send([dict(good, cweight=[1.0, -1.0])]), "cweight[1]")
    usage(lambda: send([dict(good, cweight=[np.inf, 1.0])]), "cweight[0]")
    usage(lambda: send([dict(good, cweight=[0.0, 0.0])]), "observes nothing")
    usage(lambda: send([dict(good, sampler=99)]), "sampler")
    arr = (backend.DisplacementImageMisfit * 1)()
    arr[0].step, arr[0].sampler, arr[0].weight, arr[0].scale = N, good["sampler"].id, 1.0, 1.0
    arr[0].cweight[0] = arr[0].cweight[1] = 1.0
    usage(lambda: h._check(h.lib.glims_adjoint_displacement_image_terms(h._h, 1, arr)), "null target")
    usage(lambda: h._check(h.lib.glims_adjoint_displacement_image_info(h._h, 9, (C.c_int64 * 3)())), "no stored term")
    # a deformed sampler
    u = np.zeros(prob.points.size)
    moved = h.sampler_grid(*good["grid"], deformed_by=u)
    usage(lambda: send([dict(good, sampler=moved)]), "deformed")
    # destroying a used sampler
    usage(lambda: h._check(h.lib.glims_sampler_destroy(h._h, good["sampler"].id)), "displacement image term")
    # a step beyond the recording is reported by the gradient and the Hessian call
    send([dict(good, step=N + 4)])
    for call in (lambda: h.adjoint_gradient([], 2), lambda: h.adjoint_hessian([], [dict(D=[1.0, 0.0])])):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == backend.GLIMS_E_USAGE and "observes step %d" % (N + 4) in str(e.value)
    send([])
    assert h.adjoint_gradient([], 2)[0] == 0.0
    h.close()
    # a handle set up without mechanics
    h = _handle(backend, prob, mechanics=False)
    sm = h.sampler_points(good["x"])
    with pytest.raises(backend.BackendError) as e:
        h.set_displacement_image_terms([dict(good, sampler=sm)])
    assert e.value.code == backend.GLIMS_E_USAGE and "with_mechanics" in str(e.value)
    h.set_displacement_image_terms([])
    h.close()


def _attach_free(terms):
    return [{k: v for k, v in t.items() if k != "sampler"} for t in terms]


def test_partitioned_handle_refuses_on_every_rank(backend):
    from glimslib_amd import _backend as B
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    prob = Problem(2, 12)
    world = 2

    def body(rank, tr):
        part = partition_mesh(prob.points, prob.cells, world, rank)
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt)
        h.setup(with_mechanics=False)
        h.set_state(prob.c0[part.global_ids])
        x = part.points[:part.n_own] * 0.999 + 0.0005
        sm = h.sampler_points(x)
        try:
            h.set_displacement_image_terms([dict(step=0, kind="img_u_l2", sampler=sm, target=np.zeros((len(x), 2)))])
            code, msg = 0, ""
        except B.BackendError as e:
            code, msg = e.code, str(e)
        h.set_displacement_image_terms([])         # clearing is fine there
        h.adjoint_record(True)
        assert h.step(2) == 0
        nodal = [dict(step=2, kind="c_l2", target=np.zeros(len(part.global_ids)))]
        h.adjoint_gradient(nodal)              # the handle still works (a collective call every rank makes)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return code, "partitioned" in msg

    assert run_threaded_ranks(world, body) == [(B.GLIMS_E_USAGE, True)] * world


# ---- 6. the public API ---------------------------------------------------------------------------------------------------------
def test_fit_of_coupling_and_D_through_the_public_api(tmp_path):
    """examples/adjoint_fit_displacement_image_2D.py at test size (displacement_image_common.FIT): the data are the T2-like
    threshold image and the displacement image (a disc around the seed masked out) of the last step of a truth run, on a grid
    that aligns with no mesh line.  The numpy / scipy twin of this fit (tests/test_displacement_image_cpu.py) recovers
    (coupling, D) to FIT["bar"] = 1e-12; the truth run and the fit solve to the tolerances of the sibling GPU tests.  Recorded
    on an MI355X: 11 iterations, 13 evaluations, relative errors (9.8e-15, 8.9e-14)."""
    import deformed_volume_common as dvc
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.optimization import ReducedFunctional, minimize
    from glimslib_amd.simulation import TumorGrowth
    from glimslib_amd.utils.data_io import Image
    F, V = dic.FIT, dvc.FIT
    tight = dict(newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12)

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    def make_sim(coupling, D, E=V["E"]):
        mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
        labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1),
                                fenics.FunctionSpace(mesh, "DG", 1))
        sim = TumorGrowth(mesh, solver_options=tight)
        sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                    boundaries={'boundary_all': Boundary()},
                                    dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                               'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                    von_neumann_bcs={})
        u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
        sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=coupling,
                                   proliferation=V["rho"], E=E, poisson=V["nu"], sim_time=F["steps"] * F["dt"],
                                   sim_time_step=F["dt"])
        return sim

    grid = dict(origin=F["origin"], spacing=F["spacing"], size=F["size"])
    truth = make_sim(*F["truth"])
    truth.run(save_method=None, plot=False, output_dir=str(tmp_path))
    last = max(truth.results.get_recording_steps())
    conc = truth.sample_image('concentration', last, **grid)
    warp = truth.sample_image('displacement', last, **grid)
    truth.close()
    assert warp.is_vector and warp.array.shape[-1] == 2 and 0.0 < np.isnan(warp.array[..., 0]).mean() < 0.5
    assert np.nanmax(np.abs(warp.array)) > 0.02, "no visible mass effect in the data"
    t2 = Image(0.5 * (np.tanh((conc.array - F["level"]) / F["smooth"]) + 1.0), conc.GetOrigin(), conc.GetSpacing())
    x = dic.sc.grid_points(F["origin"], F["spacing"], np.asarray(F["size"]))
    mask = dic.fit_mask(x).reshape(warp.array.shape[:-1])
    assert 0 < (mask == 0).sum() < mask.size / 4

    def terms(s, n_steps):
        return [s.image_term(n_steps, t2, kind='img_thresh', level=F["level"], smooth=F["smooth"]),
                s.displacement_image_term(n_steps, warp, weight=F["u_weight"], mask=mask)]

    sim = make_sim(*F["start"])
    rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=str(tmp_path)), names=("coupling", "diffusion"))
    res = minimize(rf, list(F["start"]), bounds=F["bounds"], options=dict(F["options"]), tol=F["tol"])
    t = np.array(F["truth"])
    err = np.abs(res.x - t) / t
    print("fit to a threshold and a displacement image: %d iterations, %d evaluations, (coupling, D) = (%.15g, %.15g), "
          "J %.3e, rel. error %s" % (res.nit, rf.evaluations, res.x[0], res.x[1], res.fun, err))
    assert sim.displacement_image_term(F["steps"], warp, weight=F["u_weight"], mask=mask) is terms(sim, F["steps"])[1]
    sid, n_pts, n_obs = sim._backend.displacement_image_term_info(0)
    assert n_pts == int(np.prod(F["size"])) and 0 < n_obs < n_pts - (mask == 0).sum() + 1
    H = rf.hessian_matrix(res.x)
    print("H at the optimum: %s, eigenvalues %s" % (H.tolist(), np.linalg.eigvalsh(0.5 * (H + H.T))))
    sim.close()
    # E is a control of the exact second order as well.  (TumorGrowth's controls are diffusion, proliferation and coupling --
    # ReducedFunctional refuses 'E' there, tests/test_adjoint_elastic_cpu.py:134 --, so the E control is TumorGrowthBrain's
    # 'E_WM', on the four-tissue disc of tests/test_gpu_adjoint_coverage.py, with landmark displacements as the data.)
    from glimslib_amd.simulation import TumorGrowthBrain
    from test_gpu_adjoint_coverage import _brain_sim
    brain, _ = _brain_sim(tmp_path, TumorGrowthBrain, 5)
    rng = np.random.default_rng(3)
    marks = rng.uniform(-4.5, 4.5, (40, 2))
    moved = 0.05 * rng.standard_normal((40, 2))
    rfe = ReducedFunctional(brain, 2, lambda s, k: [s.landmark_term(k, marks, moved, components=(1.0, 0.5))],
                            run_kwargs=dict(output_dir=str(tmp_path)), names=("E_WM", "coupling"), elastic_hessian=True)
    He = rfe.hessian_matrix(np.array([2e-3, 0.1]))
    assert brain._backend.displacement_image_term_info(0)[1:] == (40, 40)
    brain.close()
    assert abs(He[0, 1] - He[1, 0]) <= 1e-8 * np.abs(He).max() and He[0, 0] != 0.0 and He[0, 1] != 0.0, He
    assert He.shape == (2, 2) and np.all(np.isfinite(He))
    assert res.nit <= F["options"]["maxiter"]
    assert np.abs(H - H.T).max() <= 1e-8 * np.abs(H).max() and np.all(np.linalg.eigvalsh(0.5 * (H + H.T)) > 0), H
    assert np.all(err <= F["bar"]), (res.x, err)
