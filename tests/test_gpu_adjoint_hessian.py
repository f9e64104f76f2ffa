"""
Second-order discrete adjoint on the GPU (glims_adjoint_hessian): Hessian-vector products against the numpy tangent-linear +
second-order adjoint of tests/adjoint_hessian_common.py (Jacobi and stiff multigrid regimes), against central differences of
the GPU's own gradient on the brain-like mesh, bitwise column independence and neutrality, misuse statuses, and a (D, rho) fit
with trust-constr through the public API.
"""
import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as in test_gpu_adjoint_multirank.py: the threaded transport's
#  ctypes.CDLL("libamdhip64.so") must resolve to the runtime the library itself uses)
import torch  # noqa: F401

from adjoint_common import Problem
from adjoint_hessian_common import hessian

pytestmark = pytest.mark.gpu

_SKIP = {"ms_steps", "ms_spmv", "ms_mg_setup", "ms_mech", "ms_rd_mg_setup", "ms_spmv_steps", "ms_sweep_steps",
         "ms_update_steps", "ms_quad_steps", "ms_cheb_steps", "ms_exchange", "ms_exchange_exposed", "ms_mgfine_mech",
         "ms_spmvb_mech", "us_spmv_median", "us_sweep_median", "us_update_median", "us_quad_median", "us_cheb_median",
         "us_mgfine_median", "us_spmvb_median"}


def _handle(backend, prob, mechanics=True, **opts):
    h = backend.Handle(prob.points, prob.cells, prob.labels)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12, **opts)
    if prob.dir_c is not None:
        h.set_dirichlet_c(prob.dir_c[0], prob.dir_c[1])
    if mechanics:
        h.set_dirichlet_u(prob.dir_u[0], prob.dir_u[1])
    h.setup(with_mechanics=mechanics)
    h.set_state(prob.c0)
    return h


def _record(h, n_steps):
    h.adjoint_record(True)
    traj = [h.get_state(want_u=False)[0]]
    for _ in range(n_steps):
        assert h.step(1) == 0
        traj.append(h.get_state(want_u=False)[0])
    return traj


def _rel(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _directions(prob, seed, count=2):
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    out = []
    for k in range(count):
        d = dict(D=prob.D * rng.uniform(-1, 1, L), rho=prob.rho * rng.uniform(-1, 1, L),
                 gamma=prob.gamma * rng.uniform(-1, 1, L))
        if k % 2 == 0:
            d["c0"] = 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
        out.append(d)
    return out


def _compare_with_numpy(backend, prob, n_steps, terms, tol=1e-8, mechanics=True, **opts):
    h = _handle(backend, prob, mechanics=mechanics, **opts)
    traj = _record(h, n_steps)
    dirs = _directions(prob, 7)
    r = h.adjoint_hessian(terms, dirs, prob.n_labels)
    J, dD, drho, dgam, dc0, hv = hessian(prob, prob.oracle(), traj, terms, dirs)
    for a, b, what in ((r["J"], J, "J"), (r["D"], dD, "dD"), (r["rho"], drho, "drho"), (r["gamma"], dgam, "dgamma"),
                       (r["c0"], dc0, "dc0")):
        assert _rel(a, b) <= tol, (what, a, b)
    for p in range(len(dirs)):
        for key in ("D", "rho", "gamma", "c0"):
            assert _rel(r["hv_" + key][p], hv[p][key]) <= tol, (p, key, r["hv_" + key][p], hv[p][key])
    st = r["stats"]
    assert st["tlm_pcg_its"] > 0 and st["soa_pcg_its"] > 0
    return h, r


@pytest.mark.parametrize("dim", [2, 3])
def test_hessian_matches_numpy_second_order_adjoint(backend, dim):
    prob = Problem(2, 16) if dim == 2 else Problem(3, 6)
    terms = prob.terms(6, smooth=0.1)
    assert {t["kind"] for t in terms} == {"c_l2", "c_thresh", "u_l2"} and prob.dir_c is not None
    h, r = _compare_with_numpy(backend, prob, 6, terms)
    assert r["stats"]["mech_solves"] == 2 * 2   # du and dmu per direction at the one observed displacement step
    assert h.adjoint_stats()["gradients"] == 0   # a Hessian call is not counted as a gradient call
    h.close()


def test_stiff_regime_with_multigrid_preconditioner(backend):
    prob = Problem(3, 10, dt=1.0, D=(0.1, 0.2), rho=(0.05, 0.1), dirichlet_c=None)
    terms = prob.terms(4, with_u=False)
    h, _ = _compare_with_numpy(backend, prob, 4, terms, rd_precond=backend.RD_PRECOND_MULTIGRID)
    assert h.stats()["rd_precond_used"] == backend.RD_PRECOND_MULTIGRID
    h.close()


def test_columns_are_independent_and_first_order_outputs_bitwise(backend):
    prob = Problem(2, 16)
    terms = prob.terms(5)
    dirs = _directions(prob, 11, count=4)
    h = _handle(backend, prob)
    _record(h, 5)
    g = h.adjoint_gradient(terms, 2)
    r4 = h.adjoint_hessian(terms, dirs)
    assert r4["J"] == g[0] and all(np.array_equal(x, y) for x, y in zip((r4["D"], r4["rho"], r4["gamma"], r4["c0"]), g[1:]))
    for j, d in enumerate(dirs):
        r1 = h.adjoint_hessian(terms, [d])
        for key in ("hv_D", "hv_rho", "hv_gamma", "hv_c0"):
            assert np.array_equal(r4[key][j], r1[key][0]), (j, key)
    h.close()


def test_hessian_call_leaves_gradient_step_and_stats_bit_identical(backend):
    prob = Problem(2, 24)
    terms = prob.terms(6)
    a = _handle(backend, prob)
    b = _handle(backend, prob)
    a.adjoint_record(True)
    b.adjoint_record(True)
    assert a.step(6) == 0 and b.step(6) == 0
    sa = a.stats()
    a.adjoint_hessian(terms, _directions(prob, 3))
    assert {k: v for k, v in a.stats().items() if k not in _SKIP} == {k: v for k, v in sa.items() if k not in _SKIP}
    ga, gb = a.adjoint_gradient(terms, 2), b.adjoint_gradient(terms, 2)
    assert ga[0] == gb[0] and all(np.array_equal(x, y) for x, y in zip(ga[1:], gb[1:]))
    assert a.adjoint_stats() == {**b.adjoint_stats(), "ms_backward": a.adjoint_stats()["ms_backward"]}
    assert a.step(4) == 0 and b.step(4) == 0
    assert np.array_equal(a.get_state()[0], b.get_state()[0])
    assert {k: v for k, v in a.stats().items() if k not in _SKIP} == {k: v for k, v in b.stats().items() if k not in _SKIP}
    a.close()
    b.close()


def test_misuse_gives_usage_status(backend):
    prob = Problem(2, 8)
    terms = prob.terms(3, with_u=False)

    def usage(h, dirs, match):
        with pytest.raises(backend.BackendError) as e:
            h.adjoint_hessian(terms, dirs, 2)
        assert e.value.code == backend.GLIMS_E_USAGE
        assert match in str(e.value)

    h = _handle(backend, prob)
    usage(h, [dict(D=[1.0, 0.0])], "no valid trajectory")
    h.adjoint_record(True)
    assert h.step(3) == 0
    usage(h, [], "n_dir = 0")
    usage(h, [dict(D=[1.0, 0.0])] * 9, "n_dir = 9")
    h.adjoint_hessian(terms, [dict(D=[1.0, 0.0])], 2)   # a valid call
    h.close()


def test_partitioned_handle_refuses_on_every_rank(backend):
    from glimslib_amd import _backend as B
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    prob = Problem(2, 12)
    world = 2
    terms = prob.terms(2, with_u=False)

    def body(rank, tr):
        part = partition_mesh(prob.points, prob.cells, world, rank)
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt)
        h.setup(with_mechanics=False)
        h.set_state(prob.c0[part.global_ids])
        h.adjoint_record(True)
        assert h.step(2) == 0
        loc = [dict(t, target=np.asarray(t["target"])[part.global_ids]) for t in terms]
        try:
            h.adjoint_hessian(loc, [dict(D=[1.0, 0.0])])
            code = 0
        except B.BackendError as e:
            code = e.code
        h.adjoint_gradient(loc)   # the handle still works (a collective call every rank makes)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return code

    assert run_threaded_ranks(world, body) == [B.GLIMS_E_USAGE] * world


def test_brain_like_mesh_central_differences_and_symmetry(backend):
    from glimslib_amd import workloads
    w = workloads.config_brain_like(40000, isolate=True)
    t = {k: np.asarray(v, dtype=np.float64) for k, v in w.tables.items()}
    pts, cells, lab = w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32)
    L = len(t["D"])
    n_steps = 8
    wm, gm = [int(l) for l in np.nonzero(t["D"] != 0)[0][:2]]
    # the five TumorGrowthBrain controls as label directions: D_WM, D_GM, rho_WM, rho_GM, coupling (every tissue)
    unit = lambda l: np.eye(L)[l]
    five = [dict(D=unit(wm)), dict(D=unit(gm)), dict(rho=unit(wm)), dict(rho=unit(gm)), dict(gamma=np.ones(L))]

    def run(D, rho, gamma, fn):
        h = backend.Handle(pts, cells, lab)
        h.set_materials(D, rho, gamma, t["E"], t["nu"])
        h.set_options(dt=w.dt, newton_rtol=1e-13, newton_atol=1e-18)
        h.setup(with_mechanics=False)
        h.set_state(w.c0)
        h.adjoint_record(True)
        assert h.step(n_steps) == 0
        c = h.get_state(want_u=False)[0]
        if not hasattr(run, "targets"):
            h_ = lambda x, lv: 0.5 * (np.tanh((x - lv) / 0.1) + 1.0)
            run.targets = [h_(1.1 * c, 0.3), h_(0.9 * c, 0.7), 0.95 * c]
        terms = [dict(step=n_steps, kind="c_thresh", level=0.3, smooth=0.1, target=run.targets[0]),
                 dict(step=n_steps, kind="c_thresh", level=0.7, smooth=0.1, weight=0.5, target=run.targets[1]),
                 dict(step=n_steps, kind="c_l2", target=run.targets[2])]
        out = fn(h, terms)
        h.close()
        return out

    grad = lambda h, terms: np.concatenate(h.adjoint_gradient(terms, L, want_dc0=False)[1:3])
    D0, rho0, g0 = t["D"], t["rho"], t["gamma"]
    run(D0, rho0, g0, grad)   # fixes the targets
    r = run(D0, rho0, g0, lambda h, terms: h.adjoint_hessian(terms, five))
    flat = lambda d: np.concatenate([np.broadcast_to(d.get(k, np.zeros(L)), (L,)) for k in ("D", "rho", "gamma")])
    V = np.array([flat(d) for d in five])
    HV = np.array([np.concatenate([r["hv_D"][j], r["hv_rho"][j], r["hv_gamma"][j]]) for j in range(5)])
    H = V @ HV.T
    assert np.abs(H - H.T).max() <= 1e-8 * np.abs(H).max(), H
    # one direction against central differences of the GPU's own gradient
    rng = np.random.default_rng(4)
    pD, pr = D0 * rng.uniform(-1, 1, L), rho0 * rng.uniform(-1, 1, L)
    hv = run(D0, rho0, g0, lambda h, terms: h.adjoint_hessian(terms, [dict(D=pD, rho=pr)]))
    eps = 1e-4
    num = (run(D0 + eps * pD, rho0 + eps * pr, g0, grad) - run(D0 - eps * pD, rho0 - eps * pr, g0, grad)) / (2 * eps)
    ana = np.concatenate([hv["hv_D"][0], hv["hv_rho"][0]])
    assert _rel(ana, num) <= 1e-5, (ana, num)
    print("brain-like %d nodes: 5-direction Hessian %.1f ms (TLM %d, SOA %d PCG its)" %
          (len(pts), r["stats"]["ms"], r["stats"]["tlm_pcg_its"], r["stats"]["soa_pcg_its"]))


def test_fit_of_D_and_rho_with_trust_constr(tmp_path):
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.optimization import ReducedFunctional, minimize
    from glimslib_amd.simulation import TumorGrowth

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    def make_sim(D, rho):
        mesh = fenics.RectangleMesh(fenics.Point(-5, -5), fenics.Point(5, 5), 24, 24)
        labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1),
                                fenics.FunctionSpace(mesh, "DG", 1))
        sim = TumorGrowth(mesh)
        sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                    boundaries={'boundary_all': Boundary()},
                                    dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                               'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                    von_neumann_bcs={})
        u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
        sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                                   proliferation=rho, E=0.001, poisson=0.4, sim_time=10, sim_time_step=1)
        return sim

    truth = make_sim(0.1, 0.1)
    truth.run(save_method=None, plot=False, output_dir=str(tmp_path), record_adjoint=True)
    c_end = truth.solution.components[1].copy()
    truth.close()

    def terms(s, n_steps):
        return [dict(step=n_steps, kind="c_l2", weight=1.0, target=c_end),
                dict(step=n_steps, kind="c_thresh", level=0.4, smooth=0.1, weight=1.0,
                     target=0.5 * (np.tanh((c_end - 0.4) / 0.1) + 1.0))]

    sim = make_sim(0.05, 0.2)
    rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=str(tmp_path)))
    H = rf.hessian_matrix([0.05, 0.2])
    assert np.allclose(H, H.T, rtol=1e-8, atol=0) and rf.hessian_calls == 1
    assert np.allclose(rf.hessian([0.05, 0.2], [1.0, 0.0]), H[:, 0]) and rf.hessian_calls == 1   # cached with m
    res = minimize(rf, [0.05, 0.2], method="trust-constr", options={"maxiter": 60, "gtol": 1e-12, "xtol": 1e-14})
    assert abs(res.x[0] - 0.1) <= 1e-3 * 0.1 and abs(res.x[1] - 0.1) <= 1e-3 * 0.1, res
    n_tc, h_tc = rf.evaluations, rf.hessian_calls
    sim.close()
    sim = make_sim(0.05, 0.2)
    rf2 = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=str(tmp_path)))
    minimize(rf2, [0.05, 0.2], options={"maxiter": 30, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16)
    sim.close()
    print("(D, rho) fit: trust-constr %d evaluations + %d Hessian calls, L-BFGS-B %d evaluations" %
          (n_tc, h_tc, rf2.evaluations))


def test_tumor_growth_brain_hessian_through_reduced_functional(tmp_path):
    """The 5 x 5 TumorGrowthBrain Hessian (D_WM, D_GM, rho_WM, rho_GM, coupling; WM = 3 before GM = 2) through
    ReducedFunctional.hessian_matrix: symmetric, equal to the handle-level products of the same label directions, and its
    D_WM column equal to central differences of rf.derivative."""
    from glimslib_amd.simulation import TumorGrowthBrain
    from test_gpu_adjoint_coverage import _brain_sim
    sim, rf = _brain_sim(tmp_path, TumorGrowthBrain, 5)
    m0 = np.array([0.1, 0.02, 0.1, 0.05, 0.1])
    H = rf.hessian_matrix(m0)
    assert np.abs(H - H.T).max() <= 1e-8 * np.abs(H).max(), H
    h = sim._backend
    L = h.n_labels
    unit = lambda l: np.eye(L)[l]
    dirs = [dict(D=unit(3)), dict(D=unit(2)), dict(rho=unit(3)), dict(rho=unit(2)), dict(gamma=np.ones(L))]
    r = h.adjoint_hessian(rf.terms_builder(sim, rf._n_steps), dirs)
    Hh = np.array([[r["hv_D"][j][3], r["hv_D"][j][2], r["hv_rho"][j][3], r["hv_rho"][j][2], r["hv_gamma"][j].sum()]
                   for j in range(5)]).T
    assert np.allclose(H, Hh, rtol=1e-12, atol=0), (H, Hh)
    g, hv = sim.adjoint_hessian(rf.terms_builder(sim, rf._n_steps), [dict(D_WM=1.0), dict(coupling=1.0)])
    assert hv[0]["D_WM"] == r["hv_D"][0][3] and hv[1]["coupling"] == r["hv_gamma"][4].sum()
    with pytest.raises(ValueError, match="first order"):
        sim.adjoint_hessian([], [dict(E_WM=1.0)])
    eps = 1e-4 * m0[0]
    e = np.eye(5)[0] * eps
    num = (rf.derivative(m0 + e) - rf.derivative(m0 - e)) / (2 * eps)
    assert _rel(H[:, 0], num) <= 1e-5, (H[:, 0], num)
    sim.close()
