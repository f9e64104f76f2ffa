"""
Hessian-vector products on partitioned handles (glims_adjoint_hessian_spmd; DESIGN.md section 13, "Second order", "Partitioned
handles"): the collective call on threaded ranks (parallel.run_threaded_ranks: one process, one GPU) against the numpy
second-order adjoint of tests/adjoint_hessian_common.py on the gathered GPU trajectory (1e-8, the single-GPU bar) and against
the single-rank glims_adjoint_hessian; the same bits on every rank and on every call, J and the gradient of
glims_adjoint_gradient, column independence, cut cells and labels missing on a rank, displacement and image terms, the stiff
multigrid regime, neutrality, misuse statuses on every rank, and the public API on two process ranks.

Partitioned against single rank: both lie within 1e-8 of numpy, so within 2e-8 of each other; the largest distance measured on
the cases of this file is in DESIGN.md section 13, TOL_SINGLE is ten times that.
"""
import os
import pickle

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship: the threaded transport's ctypes.CDLL("libamdhip64.so") must
#  resolve to the runtime the library itself uses)
import torch  # noqa: F401

import adjoint_image_common as aic
from adjoint_common import Problem, many_tissues, u_terms
from adjoint_hessian_common import hessian
from test_gpu_adjoint import _SKIP
from test_gpu_adjoint_multirank import _clamp_all_exterior, _free_port, _rel

pytestmark = pytest.mark.gpu

TOL_NUMPY = 1e-8
TOL_SINGLE = 1.7e-13
HV = ("hv_D", "hv_rho", "hv_gamma")
_DIST = []   # (case, largest distance to the single rank) of every test that measures one (also printed)


def _open(prob, world, rank, tr, mech=False, opts=None, owner=None):
    """(handle, part, global ids of the local nodes, n_own) after setup and set_state; world = 1: the single-rank handle."""
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
        part, gid, n_own = None, np.arange(n), n
        h = B.Handle(prob.points, prob.cells, prob.labels)
    g2l = np.full(n, -1, dtype=np.int64)
    g2l[gid[:n_own]] = np.arange(n_own)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12, **(opts or {}))
    if prob.dir_c is not None:
        loc = g2l[np.asarray(prob.dir_c[0])]
        h.set_dirichlet_c(loc[loc >= 0], np.asarray(prob.dir_c[1], float)[loc >= 0])
    if mech:
        dofs, vals = prob.dir_u
        loc = g2l[np.asarray(dofs) // d]
        keep = loc >= 0
        h.set_dirichlet_u(loc[keep] * d + (np.asarray(dofs) % d)[keep], np.asarray(vals, float)[keep])
        if prob.mech_load is not None:
            h.set_mech_load(np.asarray(prob.mech_load).reshape(n, d)[gid].reshape(-1))
    if prob.rd_load is not None:
        h.set_rd_load(np.asarray(prob.rd_load)[gid])
    h.setup(with_mechanics=mech)
    h.set_state(prob.c0[gid])
    return h, part, gid, n_own


def _close(h, tr):
    h.close()
    if tr is not None and getattr(tr, "failed", None) is not None:
        raise tr.failed


def _threads(world, fn):
    from glimslib_amd.parallel import run_threaded_ranks
    return run_threaded_ranks(world, fn)


def _localise(prob, terms, dirs, gid, sampler=None):
    d = prob.dim
    lt = []
    for t in terms:
        if t["kind"] in aic.IMAGE_KINDS:
            lt.append(dict(t, sampler=sampler))
        else:
            bs = d if t["kind"] == "u_l2" else 1
            lt.append(dict(t, target=np.asarray(t["target"], float).reshape(len(prob.points), bs)[gid].reshape(-1)))
    ld = [dict(dd, c0=np.asarray(dd["c0"])[gid]) if dd.get("c0") is not None else dict(dd) for dd in dirs]
    return lt, ld


def _cut(r, n_own):
    """A Hessian result with its node vectors cut to the owned entries (the ghost entries of hv_c0 must be 0)."""
    assert not np.any(r["hv_c0"][:, n_own:])
    return dict(r, c0=r["c0"][:n_own], hv_c0=r["hv_c0"][:, :n_own])


def _hess_rank(prob, world, rank, tr, n_steps, terms, dirs, calls, mech=False, opts=None, owner=None, points=None):
    """Records n_steps (the owned c_n kept), calls the gradient and then adjoint_hessian(dirs[s]) for every index set s in
    `calls` (world = 1: glims_adjoint_hessian itself)."""
    h, part, gid, n_own = _open(prob, world, rank, tr, mech=mech, opts=opts, owner=owner)
    h.adjoint_record(True)
    traj = [h.get_state(want_u=False)[0][:n_own]]
    for _ in range(n_steps):
        assert h.step(1) == 0
        traj.append(h.get_state(want_u=False)[0][:n_own])
    sampler = None
    if points is not None:
        sampler = h.sampler_points(points)
        if world > 1:
            sampler.resolve(part.cell_ids)
    lt, ld = _localise(prob, terms, dirs, gid, sampler)
    g = h.adjoint_gradient(lt)
    out = dict(gid=gid[:n_own], traj=traj, grad=(g[0], g[1], g[2], g[3], g[4][:n_own]), stats=h.stats(),
               res=[_cut(h.adjoint_hessian(lt, [ld[j] for j in s], collective=world > 1), n_own) for s in calls])
    _close(h, tr)
    return out


def _gather(res, n, pick):
    out = np.full(n, np.nan)
    for r in res:
        out[r["gid"]] = pick(r)
    assert not np.isnan(out).any()
    return out


def _same_bits(a, b, node=True):
    assert a["J"] == b["J"]
    for k in ("D", "rho", "gamma") + HV + (("c0", "hv_c0") if node else ()):
        assert np.array_equal(a[k], b[k]), k


def _check_ranks(res, calls):
    """Every rank: the same bits of J and every per-label output; J and the gradient are adjoint_gradient's."""
    for r in res:
        for i in range(len(calls)):
            _same_bits(r["res"][i], res[0]["res"][i], node=False)
            x, g = r["res"][i], r["grad"]
            assert x["J"] == g[0] and all(np.array_equal(p, q) for p, q in zip((x["D"], x["rho"], x["gamma"], x["c0"]), g[1:]))
        assert len({(x["stats"]["tlm_pcg_its"], x["stats"]["soa_pcg_its"]) for x in (q["res"][0] for q in res)}) == 1


def _dist(a, b):
    return _rel(a, b) if np.any(b) else float(np.abs(np.asarray(a)).max())


def _check_numpy(prob, res, terms, dirs, call, tol=TOL_NUMPY):
    """Call `call` (over all of dirs) against the numpy second-order adjoint on the gathered GPU trajectory."""
    n = len(prob.points)
    traj = [_gather(res, n, lambda r, k=k: r["traj"][k]) for k in range(len(res[0]["traj"]))]
    J, dD, drho, dgam, dc0, hv = hessian(prob, prob.oracle(), traj, terms, dirs)
    x = res[0]["res"][call]
    for a, b, what in ((x["J"], J, "J"), (x["D"], dD, "D"), (x["rho"], drho, "rho"), (x["gamma"], dgam, "gamma"),
                       (_gather(res, n, lambda r: r["res"][call]["c0"]), dc0, "c0")):
        assert _dist(a, b) <= tol, (what, a, b)
    for p in range(len(dirs)):
        for key in ("D", "rho", "gamma"):
            assert _dist(x["hv_" + key][p], hv[p][key]) <= tol, (p, key, x["hv_" + key][p], hv[p][key])
        assert _dist(_gather(res, n, lambda r: r["res"][call]["hv_c0"][p]), hv[p]["c0"]) <= tol, (p, "c0")


def _check_single(case, prob, res, ref, call, ref_call=None, tol=TOL_SINGLE):
    n = len(prob.points)
    x, y = res[0]["res"][call], ref["res"][call if ref_call is None else ref_call]
    worst = 0.0
    for k in ("J", "D", "rho", "gamma") + HV:
        worst = max(worst, _dist(x[k], y[k]))
    worst = max(worst, _dist(_gather(res, n, lambda r: r["res"][call]["c0"]), y["c0"]))
    for p in range(len(y["hv_c0"])):
        worst = max(worst, _dist(_gather(res, n, lambda r: r["res"][call]["hv_c0"][p]), y["hv_c0"][p]))
    _DIST.append((case, worst))
    print("%s: largest rel. distance of the partitioned call to the single rank %.3e" % (case, worst))
    assert worst <= tol, (case, worst)


def _directions(prob, seed, count, gamma=False):
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    out = []
    for k in range(count):
        d = dict(D=prob.D * rng.uniform(-1, 1, L), rho=prob.rho * rng.uniform(-1, 1, L))
        if gamma:
            d["gamma"] = prob.gamma * rng.uniform(-1, 1, L)
        if k % 2 == 0:
            d["c0"] = 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
        out.append(d)
    return out


# ---- 1. lattices: P = 1, 3 and 8, column independence, the same bits on every call -------------------------------------------
_CALLS8 = [tuple(range(8)), (0,), (0, 1, 2), (7,), tuple(range(8))]
_REF = {}


def _lattice(dim):
    prob, N = (Problem(2, 12), 3) if dim == 2 else (Problem(3, 7), 3)
    terms = prob.terms(N, with_u=False)
    assert {t["kind"] for t in terms} == {"c_l2", "c_thresh"}
    return prob, N, terms, _directions(prob, 7, 8)


@pytest.mark.parametrize("dim,world", [(2, 2), (2, 3), (3, 2)])
def test_lattice_matches_numpy_and_single_rank(backend, dim, world):
    prob, N, terms, dirs = _lattice(dim)
    if dim not in _REF:
        _REF[dim] = _hess_rank(prob, 1, 0, None, N, terms, dirs, _CALLS8[:1])
    res = _threads(world, lambda r, tr: _hess_rank(prob, world, r, tr, N, terms, dirs, _CALLS8))
    _check_ranks(res, _CALLS8)
    _check_numpy(prob, res, terms, dirs, 0)
    _check_single("lattice %d-D, %d ranks" % (dim, world), prob, res, _REF[dim], 0)
    for r in res:
        p8, p1, p3, p7, again = r["res"]
        _same_bits(p8, again)                                   # a second call: the same bits
        for key in HV + ("hv_c0",):
            assert np.array_equal(p8[key][0], p1[key][0]), key  # column j of P = 8: the bits of a one-direction call
            assert np.array_equal(p8[key][7], p7[key][0]), key
            assert np.array_equal(p8[key][:3], p3[key]), key
        assert p8["stats"]["tlm_pcg_its"] > 0 and p8["stats"]["soa_pcg_its"] > 0


# ---- 2. cut cells and labels ---------------------------------------------------------------------------------------------------
def test_stripes_cut_cells_of_many_labels_and_a_label_missing_on_a_rank(backend):
    """Stripes of y alternate between the two ranks: three cuts, each through cells of several labels; label 8 (the second
    k_hsens label chunk) only on cells whose vertices all belong to rank 0."""
    world, N = 2, 3
    prob = many_tissues(2, 9, n=12, seed=5)
    owner = (np.floor(prob.points[:, 1] * 4 - 1e-9).astype(np.int64).clip(0, 3) % 2).astype(np.int32)
    oc = owner[prob.cells]
    lab = prob.labels.copy()
    lab[(lab == 8) & (oc != 0).any(axis=1)] = 0
    prob.labels = lab
    cut = (oc != oc[:, :1]).any(axis=1)
    assert (lab == 8).any() and len(np.unique(lab[cut])) >= 2 and len(np.unique(lab)) == 9
    terms = prob.terms(N, with_u=False)
    dirs = _directions(prob, 9, 3)
    calls = [(0, 1, 2)]
    ref = _hess_rank(prob, 1, 0, None, N, terms, dirs, calls)
    res = _threads(world, lambda r, tr: _hess_rank(prob, world, r, tr, N, terms, dirs, calls, owner=owner))
    _check_ranks(res, calls)
    _check_numpy(prob, res, terms, dirs, 0)
    _check_single("stripes, 9 labels", prob, res, ref, 0)
    assert np.abs(res[0]["res"][0]["hv_D"][:, 8]).max() > 0.0


# ---- 3. displacement terms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["MULTIGRID", "BLOCK_JACOBI"])
def test_displacement_terms_with_a_gamma_direction(backend, precond):
    world, N = 2, 3
    prob = _clamp_all_exterior(many_tissues(2, 3, n=16, mech_load=1.0, seed=22), 0.02)
    terms = u_terms(prob, [1, N], seed=21) + [dict(step=N, kind="c_l2", weight=1.0, target=np.full(len(prob.points), 0.2))]
    dirs = _directions(prob, 13, 2, gamma=True)
    opts = dict(mech_precond=getattr(backend, "PRECOND_" + precond))
    calls = [(0, 1)]
    res = _threads(world, lambda r, tr: _hess_rank(prob, world, r, tr, N, terms, dirs, calls, mech=True, opts=opts))
    _check_ranks(res, calls)
    _check_numpy(prob, res, terms, dirs, 0)
    x = res[0]["res"][0]
    assert np.abs(x["hv_gamma"]).min() > 0.0 and x["stats"]["mech_solves"] == 2 * 2 * 2   # du, dmu per direction and step


# ---- 4. the stiff regime: column by column through the V-cycle PCG ----------------------------------------------------------------
def test_stiff_regime_with_rd_multigrid_and_dirichlet_c(backend):
    """Dirichlet c on the whole boundary of the cube: every rank owns constrained nodes (the partitioned multigrid set-up
    exchanges the constrained-node mask on the ranks that have one, as test_gpu_adjoint_multirank.py notes for u)."""
    world, N = 2, 3
    prob = Problem(3, 10, dt=1.0, D=(0.1, 0.2), rho=(0.05, 0.1))
    xb = np.nonzero(((prob.points <= 1e-12) | (prob.points >= 1.0 - 1e-12)).any(axis=1))[0]
    prob.dir_c = (xb, np.full(len(xb), 0.05))
    terms = prob.terms(N, with_u=False)
    dirs = _directions(prob, 17, 2)
    opts = dict(rd_precond=backend.RD_PRECOND_MULTIGRID)
    calls = [(0, 1)]
    res = _threads(world, lambda r, tr: _hess_rank(prob, world, r, tr, N, terms, dirs, calls, opts=opts))
    assert all(r["stats"]["rd_precond_used"] == backend.RD_PRECOND_MULTIGRID for r in res)
    _check_ranks(res, calls)
    _check_numpy(prob, res, terms, dirs, 0)


# ---- 5. image terms ------------------------------------------------------------------------------------------------------------
def test_image_term_on_a_resolved_point_sampler(backend):
    world, N = 2, 3
    prob = Problem(2, 12)
    rng = np.random.default_rng(3)
    x = rng.uniform(0.02, 0.98, (150, 2))
    terms = [dict(step=N, kind="img_thresh", level=0.3, smooth=0.1, weight=1.0, target=rng.uniform(0, 1, len(x))),
             dict(step=2, kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, len(prob.points)))]
    dirs = _directions(prob, 19, 2)
    calls = [(0, 1)]
    ref = _hess_rank(prob, 1, 0, None, N, terms, dirs, calls, points=x)
    res = _threads(world, lambda r, tr: _hess_rank(prob, world, r, tr, N, terms, dirs, calls, points=x))
    _check_ranks(res, calls)
    _check_single("image term, 2 ranks", prob, res, ref, 0)


# ---- 6. brain-like mesh --------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_brain_like_mesh_four_ranks(backend):
    from glimslib_amd import workloads
    w = workloads.config_brain_like(24000, isolate=True)
    t = {k: np.asarray(v, dtype=np.float64) for k, v in w.tables.items()}
    prob = Problem.from_mesh(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32), t["D"], t["rho"],
                             t["gamma"], t["E"], t["nu"], np.asarray(w.c0, float), dt=w.dt)
    n, world, N = len(prob.points), 4, 3
    assert n == 26588
    rng = np.random.default_rng(11)
    terms = [dict(step=N, kind="c_thresh", level=0.3, smooth=0.1, weight=1.0, target=rng.uniform(0, 1, n)),
             dict(step=2, kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, n))]
    dirs = _directions(prob, 23, 2)
    calls = [(0, 1)]
    ref = _hess_rank(prob, 1, 0, None, N, terms, dirs, calls)
    res = _threads(world, lambda r, tr: _hess_rank(prob, world, r, tr, N, terms, dirs, calls))
    _check_ranks(res, calls)
    _check_single("brain-like, 4 ranks", prob, res, ref, 0)


# ---- 7. neutrality -------------------------------------------------------------------------------------------------------------
def test_collective_call_leaves_the_run_bit_identical(backend):
    world, N = 2, 3
    prob = _clamp_all_exterior(many_tissues(2, 3, n=12, mech_load=0.5, seed=30), 0.01)
    terms = prob.terms(N)
    dirs = _directions(prob, 29, 2, gamma=True)

    def nostat(st):
        return {k: v for k, v in st.items() if k not in _SKIP}

    def body(rank, tr, call):
        h, part, gid, n_own = _open(prob, world, rank, tr, mech=True)
        h.adjoint_record(True)
        assert h.step(N) == 0
        lt, ld = _localise(prob, terms, dirs, gid)
        if call:
            st, ad = nostat(h.stats()), h.adjoint_stats()
            h.adjoint_hessian(lt, ld, collective=True)
            assert nostat(h.stats()) == st and h.adjoint_stats() == ad
        g = h.adjoint_gradient(lt)
        assert h.step(2) == 0
        out = dict(g=(g[0], g[1], g[2], g[3], g[4][:n_own]), c=h.get_state(want_u=False)[0][:n_own], st=nostat(h.stats()),
                   ad={k: v for k, v in h.adjoint_stats().items() if k != "ms_backward"})
        _close(h, tr)
        return out

    a = _threads(world, lambda r, tr: body(r, tr, True))
    b = _threads(world, lambda r, tr: body(r, tr, False))
    for x, y in zip(a, b):
        assert x["g"][0] == y["g"][0] and all(np.array_equal(p, q) for p, q in zip(x["g"][1:], y["g"][1:]))
        assert np.array_equal(x["c"], y["c"]) and x["st"] == y["st"] and x["ad"] == y["ad"]


# ---- 8. misuse: the same status on every rank ------------------------------------------------------------------------------------
def test_misuse_is_refused_on_every_rank_and_the_handle_goes_on(backend):
    from glimslib_amd import _backend as B
    world, N = 2, 2
    prob = Problem(2, 12)
    terms = prob.terms(N, with_u=False)
    dirs = _directions(prob, 31, 9)

    def body(rank, tr):
        h, part, gid, n_own = _open(prob, world, rank, tr)
        h.adjoint_record(True)
        assert h.step(N) == 0
        lt, ld = _localise(prob, terms, dirs, gid)
        got = []

        def status(t, d, word):
            try:
                h.adjoint_hessian(t, d, collective=True)
                got.append(0)
            except B.BackendError as e:
                assert word is None or word in str(e) or "refused on rank" in str(e), str(e)
                got.append(e.code)
            assert h.adjoint_gradient(lt)[0] > 0               # the handle still computes a gradient (collective)

        status(lt, ld[:2] if rank == 0 else ld[:3], "n_dir")                            # the ranks disagree on n_dir
        status(lt, [ld[0]] if rank == 0 else [dict(D=ld[0]["D"], rho=ld[0]["rho"])], "NULL")   # ... on dir_c0 being NULL
        status([dict(lt[0], step=N + 5 if rank == 1 else N)], ld[:1], "observes step")  # beyond the trajectory on rank 1
        status(lt, ld, "n_dir = 9")
        status(lt, ld[:2], None)                                                         # valid
        _close(h, tr)
        return got

    U = B.GLIMS_E_USAGE
    for got in _threads(world, body):
        assert got == [U, U, U, U, 0], got


# ---- 9. public API: two process ranks (gloo-staged transport) --------------------------------------------------------------------
def _api(out_dir, tag):
    from glimslib_amd.simulation import TumorGrowthBrain
    from test_gpu_adjoint_coverage import _brain_sim
    sim, rf = _brain_sim(out_dir, TumorGrowthBrain, 5)
    H = rf.hessian_matrix(np.array([0.1, 0.02, 0.1, 0.05, 0.1]))
    sim.close()
    with open(os.path.join(out_dir, "%s.pkl" % tag), "wb") as f:
        pickle.dump(H, f)
    return H


def _api_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["GLIMS_TRANSPORT"] = "gloo"
    os.environ["GLIMS_FORCE_DEVICE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _api(out_dir, "hess_rank%d" % rank)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_public_api_two_process_ranks_hessian_matrix(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_api_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    z = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), "hess_rank%d.pkl" % r), "rb") as f:
            z.append(pickle.load(f))
    ref = _api(str(tmp_path), "single")
    assert np.array_equal(z[0], z[1])
    e = _rel(z[0], ref)
    print("hessian_matrix on 2 process ranks: %.3e from the single process" % e)
    assert e <= TOL_SINGLE
    assert np.abs(z[0] - z[0].T).max() <= 1e-8 * np.abs(z[0]).max()
