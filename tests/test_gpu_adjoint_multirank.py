"""
Discrete adjoint on partitioned handles: J and dJ/d(D, rho, gamma, c0) of a run partitioned over ranks
against the single-rank gradient of the same problem (itself checked against the numpy adjoint and finite differences in
tests/test_gpu_adjoint*.py).  Process ranks share one GPU through the gloo-staged transport (GLIMS_TRANSPORT=gloo semantics,
parallel.HostStagedTransport); 4 and 8 ranks run as threads of one process (parallel.ThreadedTransport).  J and the per-label
arrays must be bitwise the same on every rank: L-BFGS-B runs SPMD on them.
"""
import os
import pickle
import socket
import time

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as in test_gpu_multirank.py: torch ships its own HIP runtime,
#  and the threaded transport's ctypes.CDLL("libamdhip64.so") must resolve to the runtime the library itself uses)
import torch  # noqa: F401

from adjoint_common import Problem, many_tissues, u_terms

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


# ---- one rank of a partitioned (or, world = 1, single-rank) run with the adjoint ------------------------------------------
def _rank(prob, world, rank, tr, n_steps, terms, mech=True, opts=None, dirichlet_at=None, owner=None, neutral=False,
          grad=True):
    """Records n_steps, returns the gradient (dc0 as the owned values with their global ids), the statistics and, with
    `neutral`, the state after one more step (grad=False: no gradient call at all).  dirichlet_at(k): new Dirichlet values
    of prob.dir_c before step k (all ranks call set_dirichlet_c, with n = 0 where they own no constrained node).
    owner: node -> rank map (default: RCB parts)."""
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
    dir_nodes = np.zeros(0, dtype=np.int64)
    if prob.dir_c is not None:
        loc = g2l[np.asarray(prob.dir_c[0])]
        keep = loc >= 0
        dir_nodes, dir_keep = loc[keep], keep
        h.set_dirichlet_c(dir_nodes, np.asarray(prob.dir_c[1], float)[keep])
    if mech:
        dofs, vals = prob.dir_u
        node, comp = np.asarray(dofs) // d, np.asarray(dofs) % d
        loc = g2l[node]
        keep = loc >= 0
        h.set_dirichlet_u(loc[keep] * d + comp[keep], np.asarray(vals, float)[keep])
        if prob.mech_load is not None:
            h.set_mech_load(np.asarray(prob.mech_load).reshape(n, d)[gid].reshape(-1))
    if prob.rd_load is not None:
        h.set_rd_load(np.asarray(prob.rd_load)[gid])
    h.setup(with_mechanics=mech)
    h.set_state(prob.c0[gid])
    h.adjoint_record(True)
    t0 = time.perf_counter()
    for k in range(n_steps):
        if dirichlet_at is not None:
            h.set_dirichlet_c(dir_nodes, np.asarray(dirichlet_at(k), float)[dir_keep])
        assert h.step(1) == 0
    t_fwd = time.perf_counter() - t0
    loc_terms = []
    for t in terms:
        t = dict(t)
        bs = d if t["kind"] == "u_l2" else 1
        t["target"] = np.asarray(t["target"], float).reshape(n, bs)[gid].reshape(-1)
        loc_terms.append(t)
    t0 = time.perf_counter()
    J, dD, drho, dgam, dc0 = h.adjoint_gradient(loc_terms) if grad else (0.0, None, None, None, np.zeros(n_own))
    t_bwd = time.perf_counter() - t0
    out = dict(J=J, dD=dD, drho=drho, dgamma=dgam, gid=gid[:n_own], dc0=dc0[:n_own], adj=h.adjoint_stats(),
               n_dir=len(dir_nodes), t_fwd=t_fwd, t_bwd=t_bwd, peers=0 if world == 1 else len(part.peer_rank))
    if neutral:
        assert h.step(1) == 0
        out["c_next"] = h.get_state(want_u=False)[0][:n_own]
    h.close()
    if tr is not None and getattr(tr, "failed", None) is not None:
        raise tr.failed
    return out


def _clamp_all_exterior(prob, u_clamp):
    """u clamped on the whole boundary of the unit square / cube (a smooth non-zero field): every part of the partition owns
    constrained displacement dofs, as in test_gpu_multirank.py -- the partitioned elasticity set-up exchanges the constrained-dof
    mask on the ranks that have one."""
    x, d = prob.points, prob.dim
    xb = np.nonzero(((x <= 1e-12) | (x >= 1.0 - 1e-12)).any(axis=1))[0]
    dofs = (xb[:, None] * d + np.arange(d)[None]).ravel()
    vals = u_clamp * (np.sin(3.0 * x[xb, 1:2] + 1.0) * (1.0 + np.arange(d))[None]).ravel()
    prob.dir_u = (dofs, vals)
    return prob


def _gather(res, n):
    dc0 = np.full(n, np.nan)
    for r in res:
        dc0[r["gid"]] = r["dc0"]
    assert not np.isnan(dc0).any()
    return dc0


def _threads(prob, world, **kw):
    from glimslib_amd.parallel import run_threaded_ranks
    return run_threaded_ranks(world, lambda r, tr: _rank(prob, world, r, tr, **kw))


def _check(res, ref, n, tol):
    """Every rank: the same bits of J and the per-label arrays; they and the gathered dc0 agree with the single rank."""
    for r in res[1:]:
        assert r["J"] == res[0]["J"]
        for k in ("dD", "drho", "dgamma"):
            assert np.array_equal(r[k], res[0][k]), k
    for k in ("J", "dD", "drho", "dgamma"):
        assert _rel(res[0][k], ref[k]) <= tol, (k, res[0][k], ref[k])
    assert _rel(_gather(res, n), ref["dc0"]) <= tol


# ---- 1. process ranks (gloo-staged transport) ------------------------------------------------------------------------------
def _spec_problem(dim):
    prob = Problem(2, 20) if dim == 2 else Problem(3, 7)
    N = 5
    rng = np.random.default_rng(7)
    n = len(prob.points)
    terms = [dict(step=N, kind="c_thresh", level=0.25, smooth=0.1, weight=1.0, target=rng.uniform(0, 1, n)),
             dict(step=N, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5, target=rng.uniform(0, 1, n)),
             dict(step=2, kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, n)),
             dict(step=0, kind="c_l2", weight=0.7, target=rng.uniform(0, 0.5, n)),
             dict(step=4, kind="c_thresh", level=0.4, smooth=0.2, weight=1.5, target=rng.uniform(0, 1, n))]
    return prob, N, terms


def _proc_worker(rank, world, port, out_dir, dim):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["GLIMS_TRANSPORT"] = "gloo"
    os.environ["GLIMS_FORCE_DEVICE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from glimslib_amd.parallel import HostStagedTransport
        prob, N, terms = _spec_problem(dim)
        out = _rank(prob, world, rank, HostStagedTransport(dist), N, terms, mech=False)
        with open(os.path.join(out_dir, "rank%d.pkl" % rank), "wb") as f:
            pickle.dump(out, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dim,world", [(2, 2), (3, 2), (2, 3), (3, 3)])
def test_process_ranks_match_single_rank(tmp_path, backend, dim, world):
    import torch.multiprocessing as mp
    mp.spawn(_proc_worker, args=(world, _free_port(), str(tmp_path), dim), nprocs=world, join=True)
    res = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), "rank%d.pkl" % r), "rb") as f:
            res.append(pickle.load(f))
    prob, N, terms = _spec_problem(dim)
    ref = _rank(prob, 1, 0, None, N, terms, mech=False)
    _check(res, ref, len(prob.points), 1e-10)
    assert all(r["adj"]["backward_steps"] == N and r["adj"]["recorded_states"] == N + 1 for r in res)
    assert min(r["peers"] for r in res) >= 1


# ---- 2. 4 and 8 ranks as threads on the brain-like mesh --------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [2, 4, 8])
def test_brain_like_mesh_threaded_ranks(backend, world):
    """Also reports the backward / forward wall-time ratio of the partitioned run (threads of one process share the GPU)."""
    from glimslib_amd import workloads
    w = workloads.config_brain_like(24000, isolate=True)
    t = {k: np.asarray(v, dtype=np.float64) for k, v in w.tables.items()}
    pts, cells = w.mesh.points, w.mesh.cells
    prob = Problem.from_mesh(pts, cells, np.asarray(w.cell_label, dtype=np.int32), t["D"], t["rho"], t["gamma"], t["E"],
                             t["nu"], np.asarray(w.c0, float), dt=w.dt)
    N = 6
    rng = np.random.default_rng(11)
    n = len(pts)
    terms = [dict(step=N, kind="c_thresh", level=0.3, smooth=0.1, weight=1.0, target=rng.uniform(0, 1, n)),
             dict(step=3, kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, n))]
    ref = _rank(prob, 1, 0, None, N, terms, mech=False, )
    res = _threads(prob, world, n_steps=N, terms=terms, mech=False, )
    _check(res, ref, n, 1e-9)
    fwd, bwd = max(r["t_fwd"] for r in res), max(r["t_bwd"] for r in res)
    print("brain-like %d nodes, %d threaded ranks: forward %.1f ms/step, backward %.1f ms/step, ratio %.2f "
          "(single rank: %.2f); adjoint PCG its %s vs %d" %
          (n, world, 1e3 * fwd / N, 1e3 * bwd / N, bwd / fwd, ref["t_bwd"] / ref["t_fwd"],
           [r["adj"]["pcg_its"] for r in res], ref["adj"]["pcg_its"]))


# ---- 3. a label band along a partition cut, a label absent from some ranks, an empty label ---------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("dim,world", [(2, 3), (3, 2)])
def test_cut_band_and_labels_missing_on_ranks(backend, dim, world):
    """Label 1: exactly the cells that straddle a partition cut (each exists on two or more ranks: a double-counted or a
    dropped one shows at full size).  Label 2: cells whose vertices all belong to the last rank (no cell of it on rank 0).
    Label 3: no cells at all -- its entries must be exactly 0."""
    from glimslib_amd.partition import node_owners
    prob = many_tissues(dim, 4, n=24 if dim == 2 else 8, empty=(3,), seed=40 + dim)
    owner = node_owners(prob.points, world, prob.cells)
    oc = owner[prob.cells]
    cut = (oc != oc[:, :1]).any(axis=1)
    last = (oc == world - 1).all(axis=1) & (prob.points[prob.cells].mean(axis=1)[:, 1] > 0.5)
    lab = np.zeros(len(prob.cells), dtype=np.int32)
    lab[last] = 2
    lab[cut] = 1
    assert cut.any() and last.any()
    prob.labels = lab
    N = 4
    terms = prob.terms(N, with_u=False)
    ref = _rank(prob, 1, 0, None, N, terms, mech=False)
    res = _threads(prob, world, n_steps=N, terms=terms, mech=False, owner=owner)
    _check(res, ref, len(prob.points), 1e-10)
    for k in ("dD", "drho", "dgamma"):
        assert res[0][k][3] == 0.0
    assert abs(res[0]["dD"][1]) > 1e-3 * np.abs(res[0]["dD"]).max()   # the cut band carries a real sensitivity


# ---- 4. displacement terms under partitioned multigrid / block-Jacobi mechanics -------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("precond", ["MULTIGRID", "BLOCK_JACOBI"])
@pytest.mark.parametrize("dim,world", [(2, 3), (3, 2)])
def test_displacement_terms_partitioned_mechanics(backend, dim, world, precond):
    prob = _clamp_all_exterior(many_tissues(dim, 3, n=16 if dim == 2 else 6, mech_load=1.0, seed=20 + dim), 0.02)
    N = 4
    terms = u_terms(prob, [0, 2, N, N], seed=21) + [dict(step=N, kind="c_l2", weight=1.0,
                                                         target=np.full(len(prob.points), 0.2))]
    opts = dict(mech_precond=getattr(backend, "PRECOND_" + precond))
    ref = _rank(prob, 1, 0, None, N, terms, opts=opts)
    res = _threads(prob, world, n_steps=N, terms=terms, opts=opts)
    _check(res, ref, len(prob.points), 1e-9)
    assert np.abs(ref["dgamma"]).max() > 0.0
    assert all(r["adj"]["mech_solves"] == ref["adj"]["mech_solves"] == 6 for r in res)


# ---- 5. time-dependent Dirichlet data, a rank that owns no constrained node ------------------------------------------------
@pytest.mark.timeout(600)
def test_moving_dirichlet_with_a_rank_without_constrained_nodes(backend):
    prob = Problem(2, 24, dirichlet_c=0.05)
    prob.rd_load = None
    N = 5
    terms = prob.terms(N, with_u=False)

    def vals(k):
        return np.full(len(prob.dir_c[0]), 0.05 + 0.02 * (k + 1))

    ref = _rank(prob, 1, 0, None, N, terms, mech=False, dirichlet_at=vals)
    res = _threads(prob, 3, n_steps=N, terms=terms, mech=False, dirichlet_at=vals)
    assert min(r["n_dir"] for r in res) == 0 and max(r["n_dir"] for r in res) > 0
    _check(res, ref, len(prob.points), 1e-10)


# ---- 6. neutrality --------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_partitioned_gradient_leaves_the_forward_run_bit_identical(backend):
    from glimslib_amd.parallel import run_threaded_ranks
    prob = _clamp_all_exterior(many_tissues(2, 3, n=20, mech_load=0.5, seed=30), 0.01)
    N = 4
    terms = prob.terms(N)

    def body(rank, tr):
        a = _rank(prob, 3, rank, tr, N, terms, neutral=True)
        b = _rank(prob, 3, rank, tr, N, terms, neutral=True, grad=False)   # twin: records, never computes a gradient
        return a, b

    for a, b in run_threaded_ranks(3, body):
        assert a["adj"]["pcg_its"] > 0 and b["adj"]["gradients"] == 0
        assert np.array_equal(a["c_next"], b["c_next"])


# ---- 7. misuse: every rank returns the same status -------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_misuse_returns_the_same_status_on_every_rank(backend):
    from glimslib_amd import _backend as B
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    prob = Problem(2, 16)
    world = 3
    terms = prob.terms(3, with_u=False)

    def body(rank, tr):
        part = partition_mesh(prob.points, prob.cells, world, rank)
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt)
        h.setup(with_mechanics=False)
        h.set_state(prob.c0[part.global_ids])
        loc = [dict(t, target=np.asarray(t["target"])[part.global_ids]) for t in terms]
        got = []

        def call(t):
            try:
                h.adjoint_gradient(t)
                got.append(0)
            except B.BackendError as e:
                got.append(e.code)

        call(loc)                                                  # nothing recorded
        h.adjoint_record(True)
        assert h.step(3) == 0
        call([dict(loc[0], step=7)])                               # beyond the recording, on every rank
        call([dict(loc[0], step=7 if rank == 1 else 3)])           # ... on rank 1 only: the others must not wait for it
        call(loc)                                                  # valid
        h.set_options(newton_maxit=0)
        st = h.step(1)                                             # a step that gives up (a solver status on every rank)
        call(loc)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return st, got

    res = run_threaded_ranks(world, body)
    U = B.GLIMS_E_USAGE
    for st, got in res:
        assert st != 0
        assert got == [U, U, U, 0, U], got


# ---- 8. public API: TumorGrowthBrain under torch.distributed, and an SPMD fit ----------------------------------------------
def _brain_sim():
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
                           x0=14, y0=9, z0=8)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0., 0., 0.)), 1: iv}, sim_time=4, sim_time_step=1,
                               E_GM=3000E-6, E_WM=3000E-6, E_CSF=1000E-6, E_VENT=1000E-6, nu_GM=0.45, nu_WM=0.45,
                               nu_CSF=0.45, nu_VENT=0.3, D_GM=0.01, D_WM=0.05, rho_GM=0.05, rho_WM=0.05, coupling=0.1)
    return sim


def _brain_terms(sim, n_steps):
    n = sim.mesh.num_vertices()
    rng = np.random.default_rng(5)
    return [dict(step=n_steps, kind="c_thresh", level=0.3, smooth=0.1, target=rng.uniform(0, 1, n)),
            dict(step=max(1, n_steps // 2), kind="c_l2", weight=2.0, target=rng.uniform(0, 0.3, n)),
            dict(step=n_steps, kind="u_l2", weight=50.0, target=0.01 * rng.standard_normal(n * 3))]


def _brain_api(out_dir, tag):
    from glimslib_amd.optimization import ReducedFunctional, minimize
    sim = _brain_sim()
    sim.run(keep_nth=10 ** 9, save_method=None, clear_all=False, plot=False, output_dir=out_dir, record_adjoint=True)
    n_steps = int(sim._backend.stats()["steps"])
    g = sim.adjoint_gradient(_brain_terms(sim, n_steps))
    rf = ReducedFunctional(sim, 3, _brain_terms, run_kwargs=dict(output_dir=out_dir))
    res = minimize(rf, [0.04, 0.06, 0.08], options={"maxiter": 3})
    out = dict(grad=g, hist=[(m, J, gn) for m, J, gn in rf.history], x=res.x)
    with open(os.path.join(out_dir, "%s.pkl" % tag), "wb") as f:
        pickle.dump(out, f)
    sim.close()
    return out


def _api_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["GLIMS_TRANSPORT"] = "gloo"
    os.environ["GLIMS_FORCE_DEVICE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _brain_api(out_dir, "api_rank%d" % rank)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_public_api_two_process_ranks_gradient_and_fit(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_api_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    z = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), "api_rank%d.pkl" % r), "rb") as f:
            z.append(pickle.load(f))
    ref = _brain_api(str(tmp_path), "single")
    keys = ("J", "D_WM", "D_GM", "rho_WM", "rho_GM", "coupling")
    for k in keys:
        assert z[0]["grad"][k] == z[1]["grad"][k], k
        assert _rel(z[0]["grad"][k], ref["grad"][k]) <= 1e-9, (k, z[0]["grad"][k], ref["grad"][k])
    assert np.array_equal(z[0]["grad"]["c0"], z[1]["grad"]["c0"])
    assert _rel(z[0]["grad"]["c0"], ref["grad"]["c0"]) <= 1e-9
    # the SPMD fit: the same iterates on both ranks, bit for bit, and those of the single-process fit to 1e-6
    assert len(z[0]["hist"]) == len(z[1]["hist"]) == len(ref["hist"]) and len(ref["hist"]) >= 2
    for (m0, J0, g0), (m1, J1, g1), (mr, Jr, gr) in zip(z[0]["hist"], z[1]["hist"], ref["hist"]):
        assert np.array_equal(m0, m1) and J0 == J1 and g0 == g1
        assert _rel(m0, mr) <= 1e-6 and _rel(J0, Jr) <= 1e-6
    assert np.array_equal(z[0]["x"], z[1]["x"]) and _rel(z[0]["x"], ref["x"]) <= 1e-6
