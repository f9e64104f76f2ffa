"""
dJ/dE and dJ/dnu per tissue label on the device (glims_adjoint_gradient_full): against the numpy
reference of adjoint_elastic_common, against central differences of the device's own J, the identities of the gradient, the
bits of the five older outputs, partitioned handles (process and threaded ranks) and the public API (TumorGrowthBrain keys and
an E_WM fit through ReducedFunctional(names=...)).
"""
import os
import pickle
import socket

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as test_gpu_adjoint_multirank.py explains: the threaded
#  transport's ctypes.CDLL("libamdhip64.so") must resolve to the runtime the library itself uses)
import torch  # noqa: F401

from adjoint_common import Problem, many_tissues, u_terms
from adjoint_elastic_common import elastic_adjoint, oracle_with

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _clamp_all_exterior(prob, u_clamp):
    """u clamped to a smooth non-zero field on every exterior node: every part of a partition owns constrained dofs."""
    from oracle.glims_oracle import boundary_facets
    x, d = prob.points, prob.dim
    xb = np.unique(boundary_facets(prob.cells)[0])
    dofs = (xb[:, None] * d + np.arange(d)[None]).ravel()
    lo, hi = x.min(axis=0), x.max(axis=0)
    s = (x[xb, 1:2] - lo[1]) / (hi[1] - lo[1])
    prob.dir_u = (dofs, (u_clamp * np.sin(3.0 * s + 1.0) * (1.0 + np.arange(d))[None]).ravel())
    return prob


def _rank(prob, world, rank, tr, n_steps, terms, opts=None, owner=None, dirichlet_at=None, calls=("full",)):
    """Records n_steps of prob on one rank (world = 1: the whole mesh) and calls the gradient once per entry of `calls`:
    'full' (elastic=True), 'old' (glims_adjoint_gradient).  Returns the results with the statistics after each call."""
    from glimslib_amd import _backend as B
    from glimslib_amd.partition import build_local_part, partition_mesh
    n, d = len(prob.points), prob.dim
    if world > 1:
        part = build_local_part(prob.points, prob.cells, owner, rank, world) if owner is not None else \
            partition_mesh(prob.points, prob.cells, world, rank)
        gid, n_own = part.global_ids, part.n_own
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(prob.points.min(axis=0), prob.points.max(axis=0))
    else:
        gid, n_own = np.arange(n), n
        h = B.Handle(prob.points, prob.cells, prob.labels)
    g2l = np.full(n, -1, dtype=np.int64)
    g2l[gid[:n_own]] = np.arange(n_own)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12, **(opts or {}))
    dir_nodes, dir_keep = np.zeros(0, dtype=np.int64), None
    if prob.dir_c is not None:
        loc = g2l[np.asarray(prob.dir_c[0])]
        dir_keep = loc >= 0
        dir_nodes = loc[dir_keep]
        h.set_dirichlet_c(dir_nodes, np.asarray(prob.dir_c[1], float)[dir_keep])
    dofs, vals = prob.dir_u
    loc = g2l[np.asarray(dofs) // d]
    keep = loc >= 0
    h.set_dirichlet_u(loc[keep] * d + (np.asarray(dofs) % d)[keep], np.asarray(vals, float)[keep])
    if prob.mech_load is not None:
        h.set_mech_load(np.asarray(prob.mech_load).reshape(n, d)[gid].reshape(-1))
    if prob.rd_load is not None:
        h.set_rd_load(np.asarray(prob.rd_load)[gid])
    h.setup(with_mechanics=True)
    h.set_state(prob.c0[gid])
    h.adjoint_record(True)
    for k in range(n_steps):
        if dirichlet_at is not None:
            h.set_dirichlet_c(dir_nodes, np.asarray(dirichlet_at(k), float)[dir_keep])
        assert h.step(1) == 0
    loc_terms = []
    for t in terms:
        t = dict(t)
        bs = d if t["kind"] == "u_l2" else 1
        t["target"] = np.asarray(t["target"], float).reshape(n, bs)[gid].reshape(-1)
        loc_terms.append(t)
    out = []
    for c in calls:
        g = h.adjoint_gradient(loc_terms, elastic=(c == "full"))
        r = dict(J=g[0], dD=g[1], drho=g[2], dgamma=g[3], dc0=g[4][:n_own], adj=h.adjoint_stats())
        if c == "full":
            r.update(dE=g[5], dnu=g[6])
        out.append(r)
    h.close()
    if tr is not None and getattr(tr, "failed", None) is not None:
        raise tr.failed
    return out[0] if len(out) == 1 else out


def _threads(prob, world, **kw):
    from glimslib_amd.parallel import run_threaded_ranks
    return run_threaded_ranks(world, lambda r, tr: _rank(prob, world, r, tr, **kw))


def _check_ranks(res, ref, tol):
    """The per-label arrays and J: bitwise the same on every rank, and within tol of the single rank."""
    for r in res[1:]:
        assert r["J"] == res[0]["J"]
        for k in ("dD", "drho", "dgamma", "dE", "dnu"):
            assert np.array_equal(r[k], res[0][k]), k
    for k in ("J", "dgamma", "dE", "dnu"):
        assert _rel(res[0][k], ref[k]) <= tol, (k, res[0][k], ref[k])


def _problem(dim, **kw):
    args = dict(n=10 if dim == 2 else 5, empty=(3,), zero_gamma=(1,), u_clamp=0.02, mech_load=0.5, seed=13 + dim)
    args.update(kw)
    return many_tissues(dim, 4, **args)


def _terms(prob, N, seed=4):
    rng = np.random.default_rng(seed)
    n = len(prob.points)
    return u_terms(prob, [1, N, N], seed=seed) + [dict(step=N, kind="c_l2", weight=1.0, target=rng.uniform(0, 0.4, n))]


# ---- 1. against the numpy reference ----------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("precond", ["MULTIGRID", "BLOCK_JACOBI"])
@pytest.mark.parametrize("dim", [2, 3])
def test_matches_numpy_reference(backend, dim, precond):
    prob = _problem(dim)
    N = 3
    terms = _terms(prob, N)
    g = _rank(prob, 1, 0, None, N, terms, opts=dict(mech_precond=getattr(backend, "PRECOND_" + precond)))
    o = oracle_with(prob)
    traj = [prob.c0.copy()]
    for _ in range(N):
        traj.append(o.rd_step(traj[-1], rtol=1e-14, atol=1e-16)[0])
    dE, dnu = elastic_adjoint(prob, o, traj, terms)
    assert _rel(g["dE"], dE) < 1e-8, (g["dE"], dE)
    assert _rel(g["dnu"], dnu) < 1e-8, (g["dnu"], dnu)
    assert g["dE"][3] == 0.0 and g["dnu"][3] == 0.0                     # empty label
    assert abs(g["dE"][1]) > 1e-3 * np.abs(g["dE"]).max()               # gamma = 0 label


# ---- 2. central differences of the device's own J on the brain-like mesh -------------------------------------------------
def _brain_like_problem(n_points=24000):
    from glimslib_amd import workloads
    w = workloads.config_brain_like(n_points, isolate=True)
    t = {k: np.asarray(v, dtype=np.float64) for k, v in w.tables.items()}
    prob = Problem.from_mesh(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32), t["D"], t["rho"],
                             t["gamma"], t["E"], t["nu"], np.asarray(w.c0, float), dt=w.dt)
    return _clamp_all_exterior(prob, 0.05)


def _brain_terms(prob, N, seed=3):
    """Displacement terms with target 0 (J of the size of its E-dependent part: central differences do not cancel)."""
    rng = np.random.default_rng(seed)
    n = len(prob.points)
    return [dict(step=N, kind="u_l2", weight=1.0, target=np.zeros(n * 3)),
            dict(step=1, kind="u_l2", weight=2.0, target=np.zeros(n * 3)),
            dict(step=N, kind="c_thresh", level=0.3, smooth=0.1, weight=1.0, target=rng.uniform(0, 1, n))]


@pytest.mark.timeout(900)
def test_central_differences_brain_like(backend):
    prob = _brain_like_problem()
    N = 2
    terms = _brain_terms(prob, N)
    g = _rank(prob, 1, 0, None, N, terms)
    present = np.unique(prob.labels)
    assert len(present) >= 2
    for key, grad in (("E", g["dE"]), ("nu", g["dnu"])):
        for t in present:
            base = getattr(prob, key).copy()
            hstep = 1e-4 * abs(base[t])
            J = []
            for s in (1.0, -1.0):
                tab = base.copy()
                tab[t] += s * hstep
                setattr(prob, key, tab)
                J.append(_rank(prob, 1, 0, None, N, terms)["J"])
            setattr(prob, key, base)
            fd = (J[0] - J[1]) / (2.0 * hstep)
            assert abs(grad[t] - fd) <= 1e-5 * abs(fd), (key, t, grad[t], fd)
    for t in range(prob.n_labels):
        if t not in present:
            assert g["dE"][t] == 0.0 and g["dnu"][t] == 0.0


# ---- 3. identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("dim", [2, 3])
def test_scale_invariance_without_load(backend, dim):
    prob = _problem(dim, mech_load=0.0)
    N = 2
    g = _rank(prob, 1, 0, None, N, _terms(prob, N))
    s = prob.E * g["dE"]
    assert np.abs(s).sum() > 0.0
    assert abs(s.sum()) <= 1e-9 * np.abs(s).sum(), s


@pytest.mark.timeout(600)
def test_concentration_terms_only_give_exact_zeros_and_the_same_solves(backend):
    prob = _problem(3)
    N = 3
    terms = [t for t in _terms(prob, N) if t["kind"] != "u_l2"]
    old, full = _rank(prob, 1, 0, None, N, terms, calls=("old", "full"))
    assert np.all(full["dE"] == 0.0) and np.all(full["dnu"] == 0.0)
    assert full["adj"]["mech_solves"] == old["adj"]["mech_solves"] == 0


# ---- 4. the older outputs keep their bits; the forward state is untouched --------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("dim", [2, 3])
def test_old_outputs_bitwise_and_reproducible(backend, dim):
    prob = _problem(dim)
    N = 3
    old, full, again = _rank(prob, 1, 0, None, N, _terms(prob, N), calls=("old", "full", "full"))
    for k in ("J", "dD", "drho", "dgamma", "dc0"):
        assert np.array_equal(old[k], full[k]), k
    for k in ("J", "dD", "drho", "dgamma", "dc0", "dE", "dnu"):
        assert np.array_equal(full[k], again[k]), k
    # no elastic solve is added: every call solves the same
    s = [old["adj"], full["adj"], again["adj"]]
    assert s[0]["mech_solves"] > 0
    assert s[1]["mech_solves"] - s[0]["mech_solves"] == s[0]["mech_solves"]
    assert s[1]["mech_its"] - s[0]["mech_its"] == s[0]["mech_its"]


@pytest.mark.timeout(600)
def test_forward_state_and_stats_untouched(backend):
    """Twin handles record the same run; one computes the full gradient twice, the other none: the next step, the state
    and glims_stats agree bit for bit."""
    from glimslib_amd import _backend as B
    prob = _problem(3)
    N = 3
    terms = _terms(prob, N)
    hs = []
    for _ in range(2):
        h = B.Handle(prob.points, prob.cells, prob.labels)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt)
        h.set_dirichlet_c(*prob.dir_c)
        h.set_dirichlet_u(*prob.dir_u)
        h.set_mech_load(prob.mech_load)
        h.setup(with_mechanics=True)
        h.set_state(prob.c0)
        h.adjoint_record(True)
        assert h.step(N) == 0
        assert h.solve_mechanics() == 0
        hs.append(h)
    a, b = hs
    a.adjoint_gradient(terms, elastic=True)
    a.adjoint_gradient(terms, elastic=True)
    for h in hs:
        assert h.step(1) == 0
        assert h.solve_mechanics() == 0
    ca, ua = a.get_state()
    cb, ub = b.get_state()
    assert np.array_equal(ca, cb) and np.array_equal(ua, ub)
    sa, sb = a.stats(), b.stats()
    for k in sa:
        if "ms" not in k and "time" not in k:
            assert sa[k] == sb[k], k
    for h in hs:
        h.close()


# ---- 5. partitioned handles ------------------------------------------------------------------------------------------------
def _proc_problem(dim):
    prob = _clamp_all_exterior(_problem(dim, n=16 if dim == 2 else 6, seed=50 + dim), 0.02)
    N = 3
    return prob, N, _terms(prob, N, seed=6)


def _proc_worker(rank, world, port, out_dir, dim):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["GLIMS_TRANSPORT"] = "gloo"
    os.environ["GLIMS_FORCE_DEVICE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from glimslib_amd.parallel import HostStagedTransport
        prob, N, terms = _proc_problem(dim)
        out = _rank(prob, world, rank, HostStagedTransport(dist), N, terms)
        with open(os.path.join(out_dir, "rank%d.pkl" % rank), "wb") as f:
            pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dim,world", [(2, 2), (3, 3)])
def test_process_ranks_match_single_rank(tmp_path, backend, dim, world):
    import torch.multiprocessing as mp
    mp.spawn(_proc_worker, args=(world, _free_port(), str(tmp_path), dim), nprocs=world, join=True)
    res = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), "rank%d.pkl" % r), "rb") as f:
            res.append(pickle.load(f))
    prob, N, terms = _proc_problem(dim)
    ref = _rank(prob, 1, 0, None, N, terms)
    _check_ranks(res, ref, 1e-9)
    assert all(r["adj"]["mech_solves"] == ref["adj"]["mech_solves"] for r in res)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [4, 8])
def test_brain_like_mesh_threaded_ranks(backend, world):
    prob = _brain_like_problem()
    N = 2
    terms = _brain_terms(prob, N)
    ref = _rank(prob, 1, 0, None, N, terms)
    res = _threads(prob, world, n_steps=N, terms=terms)
    _check_ranks(res, ref, 1e-9)


@pytest.mark.timeout(600)
def test_label_missing_on_ranks_and_moving_dirichlet_data(backend):
    """Label 2 only on cells of the last rank, label 3 empty; the concentration's Dirichlet values move every step and the
    displacement is clamped to non-zero values."""
    from glimslib_amd.partition import node_owners
    world = 3
    prob = _clamp_all_exterior(_problem(2, n=20, seed=61), 0.03)
    owner = node_owners(prob.points, world, prob.cells)
    oc = owner[prob.cells]
    last = (oc == world - 1).all(axis=1) & (prob.points[prob.cells].mean(axis=1)[:, 1] > 0.5)
    lab = prob.labels.copy()
    lab[lab == 2] = 0
    lab[last] = 2
    assert last.any() and not (lab == 3).any()
    prob.labels = lab
    N = 3
    terms = _terms(prob, N, seed=8)

    def vals(k):
        return np.full(len(prob.dir_c[0]), 0.05 + 0.02 * (k + 1))

    ref = _rank(prob, 1, 0, None, N, terms, dirichlet_at=vals)
    res = _threads(prob, world, n_steps=N, terms=terms, owner=owner, dirichlet_at=vals)
    _check_ranks(res, ref, 1e-9)
    assert res[0]["dE"][3] == 0.0 and res[0]["dnu"][3] == 0.0
    assert abs(res[0]["dE"][2]) > 1e-3 * np.abs(res[0]["dE"]).max()


# ---- 6. public API -----------------------------------------------------------------------------------------------------------
def _brain_sim(E_WM):
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.simulation import TumorGrowthBrain

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    mesh = fenics.BoxMesh(fenics.Point(0, 0, 0), fenics.Point(20, 18, 16), 10, 9, 8)
    mid = mesh.cell_midpoints()
    r = np.linalg.norm((mid - np.array([10, 9, 8])) / np.array([10, 9, 8]), axis=1)
    lab = np.where(r < 0.25, 4, np.where(r < 0.6, 3, np.where(r < 0.85, 2, 1)))
    sim = TumorGrowthBrain(mesh)
    sim.setup_global_parameters(subdomains=lab, domain_names={1: 'CSF', 3: 'WM', 2: 'GM', 4: 'Ventricles'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped_0': {'bc_value': fenics.Constant((0.0, 0.0, 0.0)),
                                                             'named_boundary': 'boundary_all', 'subspace_id': 0}})
    iv = fenics.Expression('exp(-a*pow(x[0]-x0, 2) - a*pow(x[1]-y0, 2) - a*pow(x[2]-z0,2))', degree=1, a=0.05,
                           x0=12, y0=9, z0=8)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0., 0., 0.)), 1: iv}, sim_time=4, sim_time_step=1,
                               E_GM=1.0, E_WM=E_WM, E_CSF=0.5, E_VENT=0.5, nu_GM=0.45, nu_WM=0.4, nu_CSF=0.45,
                               nu_VENT=0.3, D_GM=0.01, D_WM=0.05, rho_GM=0.05, rho_WM=0.05, coupling=0.1)
    return sim


@pytest.mark.timeout(900)
def test_public_api_keys_and_E_WM_fit(backend, tmp_path):
    from glimslib_amd.optimization import ReducedFunctional, minimize
    out = str(tmp_path)
    run = dict(keep_nth=10 ** 9, save_method=None, clear_all=False, plot=False, output_dir=out)
    # a displacement target from the forward run at E_WM = 1.5
    sim = _brain_sim(1.5)
    sim.run(record_adjoint=True, **run)
    n_steps = int(sim._backend.stats()["steps"])
    assert sim._backend.solve_mechanics() == 0
    target = sim._backend.get_state()[1].copy()
    n = sim.mesh.num_vertices()
    rng = np.random.default_rng(2)
    extra = [dict(step=n_steps, kind="c_thresh", level=0.3, smooth=0.1, target=rng.uniform(0, 1, n))]
    g = sim.adjoint_gradient(extra + [dict(step=n_steps, kind="u_l2", weight=1.0, target=0.5 * target)])
    raw = sim._adjoint_raw(extra + [dict(step=n_steps, kind="u_l2", weight=1.0, target=0.5 * target)], elastic=True)
    names = ("E_GM", "E_WM", "E_CSF", "E_VENT", "nu_GM", "nu_WM", "nu_CSF", "nu_VENT")
    for k in names:
        assert k in g and np.isfinite(g[k]), k
    assert "E_outside" not in g and "nu_outside" not in g
    wm, gm = sim._tissue_id('WM'), sim._tissue_id('GM')
    assert g["E_WM"] == raw[5][wm] and g["nu_GM"] == raw[6][gm] and g["E_WM"] != 0.0
    # the older keys keep their bits
    J, dD, drho, dgamma, dc0 = sim._adjoint_raw(extra + [dict(step=n_steps, kind="u_l2", weight=1.0, target=0.5 * target)])
    assert g["J"] == J and g["D_WM"] == dD[wm] and g["coupling"] == float(np.sum(dgamma)) and np.array_equal(g["c0"], dc0)
    gc = sim.adjoint_gradient(extra)
    assert all(gc[k] == 0.0 for k in names)
    sim.close()

    def terms(s, k):
        return [dict(step=k, kind="u_l2", weight=1.0, target=target)]

    sim = _brain_sim(1.0)
    rf = ReducedFunctional(sim, 1, terms, run_kwargs=dict(output_dir=out), names=("E_WM",))
    res = minimize(rf, [1.0], bounds=(0.5, 3.0), tol=1e-15, options={"maxiter": 40, "gtol": 1e-14})
    sim.close()
    assert abs(res.x[0] - 1.5) <= 1e-4 * 1.5, (res.x, rf.history[-3:])
