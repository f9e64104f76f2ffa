"""
Image-space misfit terms and the sampler transpose on partitioned handles (glims_sampler_resolve / glims_sampler_get_counted;
k_resolve_keys, k_resolve_pick, the counted sums of k_img_misfit; DESIGN.md sections 13 and 14): the resolved sampler against
the single-rank sampler, P^T by owned rows, J and the gradient against the single-rank handle, chunks across the cut, ranks
that keep nothing, neutrality, misuse statuses on every rank, and the public API under torch.distributed.

Threaded ranks (parallel.run_threaded_ranks: one process, one GPU) unless a test names process ranks.  The tolerance against
the single-rank handle is the one of tests/test_gpu_adjoint_multirank.py on the same meshes: 1e-9 relative.
"""
import os
import pickle

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship: the threaded transport's ctypes.CDLL("libamdhip64.so") must
#  resolve to the runtime the library itself uses)
import torch  # noqa: F401

import adjoint_image_common as aic
import sampler_common as sc
import sampler_partition_common as spc
from adjoint_common import Problem
from test_gpu_adjoint import _SKIP
from test_gpu_adjoint_multirank import _brain_sim, _free_port, _rel

pytestmark = pytest.mark.gpu

TOL = 1e-9


# ---- one rank ---------------------------------------------------------------------------------------------------------------
def _open(prob, world, rank, tr, setup=True):
    """(handle, part, global ids of the local nodes, n_own); world = 1: the single-rank handle."""
    from glimslib_amd import _backend as B
    from glimslib_amd.partition import partition_mesh
    n = len(prob.points)
    if world > 1:
        part = partition_mesh(prob.points, prob.cells, world, rank)
        gid, n_own = part.global_ids, part.n_own
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(prob.points.min(axis=0), prob.points.max(axis=0))
    else:
        part, gid, n_own = None, np.arange(n), n
        h = B.Handle(prob.points, prob.cells, prob.labels)
    if setup:
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16)
        if prob.dir_c is not None:
            g2l = np.full(n, -1, dtype=np.int64)
            g2l[gid[:n_own]] = np.arange(n_own)
            loc = g2l[np.asarray(prob.dir_c[0])]
            h.set_dirichlet_c(loc[loc >= 0], np.asarray(prob.dir_c[1], float)[loc >= 0])
        h.setup(with_mechanics=False)
        h.set_state(prob.c0[gid])
    return h, part, gid, n_own


def _close(h, tr):
    h.close()
    if tr is not None and getattr(tr, "failed", None) is not None:
        raise tr.failed


def _threads(world, fn):
    from glimslib_amd.parallel import run_threaded_ranks
    return run_threaded_ranks(world, fn)


def _local_terms(terms, gid, sg, sp):
    """The term list of one rank: image terms with the rank's samplers (target / pweight in point order, as they are), nodal
    targets localised."""
    out = []
    for t in terms:
        if t["kind"] in aic.IMAGE_KINDS:
            out.append(dict(t, sampler=sg if t["where"] == "grid" else sp))
        else:
            out.append(dict(t, target=np.asarray(t["target"], float)[gid]))
    return out


def _grad_rank(prob, world, rank, tr, n_steps, terms, grid, xp, calls=2):
    """Records n_steps and calls the gradient `calls` times.  Returns what the checks below compare."""
    h, part, gid, n_own = _open(prob, world, rank, tr)
    h.adjoint_record(True)
    if n_steps:
        assert h.step(n_steps) == 0
    sg = h.sampler_grid(*grid) if grid is not None else None
    sp = h.sampler_points(xp) if xp is not None else None
    for s in (sg, sp):
        if s is not None and world > 1:
            s.resolve(part.cell_ids)
    loc = _local_terms(terms, gid, sg, sp)
    res = [h.adjoint_gradient(loc) for _ in range(calls)]
    n_img = sum(t["kind"] in aic.IMAGE_KINDS for t in terms)
    out = dict(J=res[0][0], dD=res[0][1], drho=res[0][2], dgamma=res[0][3], gid=gid[:n_own], dc0=res[0][4][:n_own],
               again=[(r[0], r[1], r[2], r[3], r[4][:n_own]) for r in res[1:]],
               n_obs=[h.image_term_info(k)[2] for k in range(n_img)],
               n_kept=[s.n_found for s in (sg, sp) if s is not None])
    _close(h, tr)
    return out


def _gather(res, n, key="dc0"):
    out = np.full(n, np.nan)
    for r in res:
        out[r["gid"]] = r[key]
    assert not np.isnan(out).any()
    return out


def _check_gradient(res, ref, n):
    """Every rank: the same bits of J and the per-label arrays, and of a second call; they, the gathered dc0 and the observed
    counts summed over the ranks agree with the single rank."""
    for r in res:
        assert r["J"] == res[0]["J"]
        for k in ("dD", "drho", "dgamma"):
            assert np.array_equal(r[k], res[0][k]), k
        for J, dD, drho, dgamma, dc0 in r["again"]:
            assert J == r["J"] and np.array_equal(dD, r["dD"]) and np.array_equal(drho, r["drho"])
            assert np.array_equal(dgamma, r["dgamma"]) and np.array_equal(dc0, r["dc0"])
    for k in ("J", "dD", "drho", "dgamma"):
        e = _rel(res[0][k], ref[k]) if np.any(ref[k]) else float(np.abs(res[0][k]).max())
        print("%s: rel. difference to the single rank %.3e" % (k, e))
        assert e <= TOL, (k, res[0][k], ref[k])
    e = _rel(_gather(res, n), ref["dc0"])
    print("dc0: rel. difference to the single rank %.3e" % e)
    assert e <= TOL
    assert [sum(r["n_obs"][k] for r in res) for k in range(len(ref["n_obs"]))] == ref["n_obs"]


_REF = {}


def _reference(key, prob, n_steps, terms, grid, xp):
    """The single-rank result of a case, computed once and shared by its worlds."""
    if key not in _REF:
        _REF[key] = _grad_rank(prob, 1, 0, None, n_steps, terms, grid, xp, calls=1)
        assert _REF[key]["J"] > 0
    return _REF[key]


# ---- 1. the resolved sampler and P^T ---------------------------------------------------------------------------------------
def _sampler_rank(prob, world, rank, tr, sets, comps):
    h, part, gid, n_own = _open(prob, world, rank, tr)
    f = np.random.default_rng(21).standard_normal(len(prob.points))
    out = []
    for kind, arg in sets:
        s = h.sampler_grid(*arg) if kind == "grid" else h.sampler_points(arg)
        o = dict(n=s.n_points)
        if world > 1:
            lc = s.cells
            o["cells_before"] = np.where(lc >= 0, part.cell_ids[np.maximum(lc, 0)], -1).astype(np.int64)
            o["apply_before"] = s.apply(f[gid])
            s.resolve(part.cell_ids)
            s.resolve(part.cell_ids)                  # twice: a no-op
        lc = s.cells
        o["cells"] = lc.astype(np.int64) if world == 1 else \
            np.where(lc >= 0, part.cell_ids[np.maximum(lc, 0)], -1).astype(np.int64)
        o["weights"], o["counted"], o["n_found"] = s.weights, s.counted, s.n_found
        o["apply"] = s.apply(f[gid])
        o["apply_t"] = {}
        for k in comps:
            r = np.random.default_rng(100 + k).standard_normal((s.n_points, k))
            g = s.apply_t(r if k > 1 else r[:, 0])
            assert np.array_equal(g, s.apply_t(r if k > 1 else r[:, 0]))        # the same bits on every call
            g = g.reshape(len(gid), k)
            assert not np.any(g[n_own:])                                         # ghost rows are exactly 0
            o["apply_t"][k] = g[:n_own]
        out.append(o)
    res = dict(sets=out, gid=gid[:n_own])
    _close(h, tr)
    return res


@pytest.mark.parametrize("dim,n,world", [(2, 12, 2), (2, 12, 3), (3, 6, 2), (3, 6, 4)])
def test_resolved_sampler_and_transpose_match_the_single_rank(backend, dim, n, world):
    prob = Problem(dim, n)
    size = (15, 14) if dim == 2 else (9, 8, 7)
    sets = [("points", prob.points.copy()), ("grid", sc.overhanging_grid(prob.points, size) + (size,)),
            ("points", np.zeros((0, dim)))]
    comps = (1, 3, 8)
    key = ("sampler", dim, n)
    if key not in _REF:
        _REF[key] = _sampler_rank(prob, 1, 0, None, sets, comps)
    ref = _REF[key]
    res = _threads(world, lambda r, tr: _sampler_rank(prob, world, r, tr, sets, comps))
    nn = len(prob.points)
    for i, one in enumerate(ref["sets"]):
        per = [r["sets"][i] for r in res]
        found = one["cells"] >= 0
        if one["n"] == 0:
            assert all(p["n_found"] == 0 and p["counted"].size == 0 for p in per)
            assert all(not np.any(p["apply_t"][k]) for p in per for k in comps)
            continue
        assert found.any() and (i != 1 or (~found).any())
        # counted: every found point on exactly one rank
        assert np.array_equal(sum(p["counted"].astype(np.int64) for p in per), found.astype(np.int64))
        assert np.array_equal(one["counted"], found)                             # single rank: 1 where found
        kept_any = np.zeros(one["n"], dtype=bool)
        for p in per:
            kept = p["cells"] >= 0
            assert np.array_equal(p["cells"][kept], one["cells"][kept])          # the kept winner is the global winner
            assert p["n_found"] == int(kept.sum()) and (p["counted"] <= kept).all()
            assert not np.any(p["weights"][~kept])
            assert (kept <= (p["cells_before"] >= 0)).all()
            kept_any |= kept
        assert np.array_equal(kept_any, found)
        if i == 0:   # vertices: ties on the cut, the resolve dropped local winners
            assert any(((p["cells_before"] >= 0) & (p["cells"] < 0)).any() for p in per)
        # P f merged by the rule of DistributedSampler: the bits of before the resolve
        big = np.iinfo(np.int64).max
        allg = np.stack([np.where(p["cells_before"] >= 0, p["cells_before"], big) for p in per])
        supplier = (allg == allg.min(axis=0)[None]).argmax(axis=0)
        before = np.where(found, np.stack([p["apply_before"] for p in per])[supplier, np.arange(one["n"])], np.nan)
        after = np.full(one["n"], np.nan)
        for p in per:
            after[p["counted"]] = p["apply"][p["counted"]]
        assert np.array_equal(before, after, equal_nan=True)
        assert all(np.array_equal(np.flatnonzero(p["counted"]), np.flatnonzero(found & (supplier == r)))
                   for r, p in enumerate(per))
        for k in comps:
            g = np.full((nn, k), np.nan)
            for r, p in zip(res, per):
                g[r["gid"]] = p["apply_t"][k]
            e = np.abs(g - one["apply_t"][k]).max() / np.abs(one["apply_t"][k]).max()
            print("set %d, %d components: P^T r by owned rows, %.3e from the single rank" % (i, k, e))
            assert e <= 1e-12


# ---- 2. chunks across the cut ----------------------------------------------------------------------------------------------
def test_chunks_of_a_cut_cell_on_both_ranks(backend):
    """3 x 3 cells under the 97 x 61 grid of test_gpu_adjoint_image.py's chunk test: a cell on the cut holds several 256-point
    chunks, on both ranks."""
    prob, world, N = Problem(2, 3), 2, 3
    terms, grid, xp = aic.standard_terms(prob, N, seed=3, grid_size=[97, 61], n_pts=77)
    x = sc.grid_points(*grid)
    parts, loc = spc.locate_on_parts(prob.points, prob.cells, world, x)
    _, keep, _ = spc.resolve(parts, loc)
    both = keep[0] & keep[1]
    cut_cells = np.bincount(np.asarray(parts[0].cell_ids)[loc[0][0][both]], minlength=len(prob.cells))
    assert cut_cells.max() > 256                                # more than one chunk of one cell, kept by both ranks
    ref = _reference("chunks", prob, N, terms, grid, xp)
    res = _threads(world, lambda r, tr: _grad_rank(prob, world, r, tr, N, terms, grid, xp))
    assert [r["n_kept"][0] for r in res] == [int(k.sum()) for k in keep]
    _check_gradient(res, ref, len(prob.points))


# ---- 3. a rank that keeps nothing --------------------------------------------------------------------------------------------
def test_rank_without_a_kept_point_makes_every_collective(backend):
    prob, world, N = Problem(2, 12), 3, 3
    lo, hi = prob.points.min(axis=0), prob.points.max(axis=0)
    size = np.array([11, 9])
    spacing = 0.2 * (hi - lo) / (size - 1)
    grid = (lo + 0.013 * (hi - lo), spacing, size)             # one corner of the domain
    x = sc.grid_points(*grid)
    rng = np.random.default_rng(8)
    terms = [dict(aic.image_term(prob, x, N, "img_thresh", rng.uniform(0, 1, len(x)), level=0.3, smooth=0.1), where="grid")]
    parts, loc = spc.locate_on_parts(prob.points, prob.cells, world, x)
    _, keep, counted = spc.resolve(parts, loc)
    assert min(int(k.sum()) for k in keep) == 0 and counted.sum() == len(x)
    ref = _reference("corner", prob, N, terms, grid, None)
    res = _threads(world, lambda r, tr: _grad_rank(prob, world, r, tr, N, terms, grid, None))
    assert [r["n_kept"][0] for r in res] == [int(k.sum()) for k in keep]
    assert [r["n_obs"][0] for r in res] == [int(c.sum()) for c in counted]
    _check_gradient(res, ref, len(prob.points))


# ---- 4. gradients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n,world", [(2, 12, 2), (2, 12, 3), (3, 6, 2), (3, 6, 4)])
def test_gradient_and_J_match_the_single_rank_handle(backend, dim, n, world):
    """adjoint_image_common.standard_terms: img_thresh (grid; 10 % NaN targets, a pweight with zeros) + img_l2 (point set) + a
    nodal c_thresh on the last step, an image term midway and one at step 0 (dc0)."""
    prob, N = Problem(dim, n), 4
    terms, grid, xp = aic.standard_terms(prob, N)
    assert [t["kind"] for t in terms] == ["img_thresh", "img_l2", "c_thresh", "img_l2", "img_thresh"]
    assert [t["step"] for t in terms] == [N, N, N, N // 2, 0]
    assert 0.05 < np.isnan(terms[0]["target"]).mean() < 0.2 and (terms[0]["pweight"] == 0).any()
    ref = _reference(("grad", dim, n), prob, N, terms, grid, xp)
    assert ref["n_obs"] == [int(aic.observed(t)[0].sum()) for t in terms if t["kind"] in aic.IMAGE_KINDS]
    res = _threads(world, lambda r, tr: _grad_rank(prob, world, r, tr, N, terms, grid, xp))
    _check_gradient(res, ref, len(prob.points))


def test_gradient_with_vertex_aligned_points(backend):
    """The points are the mesh's own vertices: every point is a tie of the cells around it, on the cut of cells of several
    ranks -- a point counted twice or not at all shows in J at full size."""
    prob, world, N = Problem(2, 12), 3, 3
    x = prob.points.copy()
    rng = np.random.default_rng(12)
    terms = [dict(aic.image_term(prob, x, N, "img_l2", rng.uniform(0, 0.6, len(x)), weight=2.0), where="points")]
    ref = _reference("vertices", prob, N, terms, None, x)
    res = _threads(world, lambda r, tr: _grad_rank(prob, world, r, tr, N, terms, None, x))
    assert sum(r["n_kept"][0] for r in res) > len(x)            # points kept by several ranks
    _check_gradient(res, ref, len(prob.points))


# ---- 5. brain-like mesh ----------------------------------------------------------------------------------------------------
def _brain_case():
    if "brain" not in _REF:
        from glimslib_amd import workloads
        w = workloads.config_brain_like(24000, isolate=True)
        t = {k: np.asarray(v, dtype=np.float64) for k, v in w.tables.items()}
        prob = Problem.from_mesh(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32), t["D"], t["rho"],
                                 t["gamma"], t["E"], t["nu"], np.asarray(w.c0, float), dt=w.dt)
        N = 6
        size = np.array([32, 32, 32])
        grid = sc.overhanging_grid(prob.points, size) + (size,)
        # (the device's own sampler, not numpy's locate: 32 k points in 140 k cells)
        h, _, _, _ = _open(prob, 1, 0, None, setup=False)
        inside = h.sampler_grid(*grid).cells >= 0
        h.close()
        assert 0.05 < (~inside).mean() < 0.8
        terms = [dict(step=N, kind="img_thresh", level=0.3, smooth=0.1, weight=1.0, where="grid", pweight=None,
                      target=np.random.default_rng(11).uniform(0, 1, int(size.prod())))]
        _REF["brain"] = (prob, N, terms, grid)
    return _REF["brain"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [4, 8])
def test_brain_like_mesh_threaded_ranks(backend, world):
    prob, N, terms, grid = _brain_case()
    assert len(prob.points) == 26588
    ref = _reference("brain-ref", prob, N, terms, grid, None)
    res = _threads(world, lambda r, tr: _grad_rank(prob, world, r, tr, N, terms, grid, None, calls=1))
    _check_gradient(res, ref, len(prob.points))


# ---- 6. neutrality ---------------------------------------------------------------------------------------------------------
def test_resolve_and_image_terms_leave_the_rest_bit_identical(backend):
    prob, world, N = Problem(2, 12), 2, 3
    terms, grid, xp = aic.standard_terms(prob, N, seed=2)
    nodal = [t for t in terms if t["kind"] not in aic.IMAGE_KINDS]

    def nostat(st):
        return {k: v for k, v in st.items() if k not in _SKIP}

    def body(rank, tr, with_images):
        h, part, gid, n_own = _open(prob, world, rank, tr)
        h.adjoint_record(True)
        assert h.step(N) == 0
        loc_nodal = _local_terms(nodal, gid, None, None)
        if with_images:
            st0 = nostat(h.stats())
            sg, sp = h.sampler_grid(*grid), h.sampler_points(xp)
            sg.resolve(part.cell_ids)
            sp.resolve(part.cell_ids)
            loc = _local_terms(terms, gid, sg, sp)
            h.set_image_terms([t for t in loc if t["kind"] in aic.IMAGE_KINDS])
            assert h.image_term_info(0)[0] == sg.id
            assert nostat(h.stats()) == st0                     # glims_stats: untouched by resolve and by storing the terms
            h.adjoint_gradient(loc)
            # (a gradient call of a partitioned handle moves the communication counters, with or without image terms)
            comm = ("halo_exchanges", "halo_bytes", "halo_exchanges_timed", "allreduces")
            assert {k: v for k, v in nostat(h.stats()).items() if k not in comm} == \
                {k: v for k, v in st0.items() if k not in comm}
            h.set_image_terms([])
        g = h.adjoint_gradient(loc_nodal)
        assert h.step(2) == 0
        out = dict(g=(g[0], g[1], g[2], g[3], g[4][:n_own]), c=h.get_state(want_u=False)[0][:n_own])
        _close(h, tr)
        return out

    a = _threads(world, lambda r, tr: body(r, tr, True))
    b = _threads(world, lambda r, tr: body(r, tr, False))
    for x, y in zip(a, b):
        assert x["g"][0] == y["g"][0] and all(np.array_equal(p, q) for p, q in zip(x["g"][1:], y["g"][1:]))
        assert np.array_equal(x["c"], y["c"])


# ---- 7. misuse: the same status on every rank --------------------------------------------------------------------------------
def test_misuse_is_refused_on_every_rank_and_the_handle_goes_on(backend):
    from glimslib_amd import _backend as B
    prob, world, N = Problem(2, 12), 2, 2
    x = prob.points[::3] * 0.98 + 0.01
    nodal = [dict(step=N, kind="c_l2", target=np.linspace(0, 1, len(prob.points)))]

    def body(rank, tr):
        h, part, gid, n_own = _open(prob, world, rank, tr)
        h.adjoint_record(True)
        assert h.step(N) == 0
        loc_nodal = _local_terms(nodal, gid, None, None)
        got = []

        def status(fn, word=None):
            try:
                fn()
                got.append(0)
            except B.BackendError as e:
                assert word is None or word in str(e), str(e)
                got.append(e.code)
            # the handle still computes a nodal gradient (a collective call every rank makes) and steps
            assert h.adjoint_gradient(loc_nodal)[0] > 0

        s = h.sampler_points(x)
        bad = np.array(part.cell_ids, dtype=np.int64)
        if rank == 1:
            bad[[3, 4]] = bad[[4, 3]]                           # not increasing, on rank 1 only
        status(lambda: s.resolve(bad))
        other = h.sampler_points(x if rank == 0 else x[:-1])    # the ranks disagree on n_points
        status(lambda: other.resolve(part.cell_ids), "n_points")
        term = dict(step=N, kind="img_l2", sampler=s, target=np.zeros(s.n_points))
        status(lambda: h.set_image_terms([term]), "partitioned")         # unresolved: as before this sampler could resolve
        status(lambda: s.apply_t(np.zeros(s.n_points)), "partitioned")
        assert np.array_equal(s.counted, s.cells >= 0)          # the refused calls left the sampler as it was
        status(lambda: s.resolve(part.cell_ids))                # valid
        status(lambda: h.set_image_terms([term]))               # valid
        status(lambda: s.resolve(part.cell_ids), "stored image term")
        status(lambda: h.adjoint_hessian([], [dict(D=[1.0, 0.0])]), "partitioned")
        J = h.adjoint_gradient(loc_nodal)[0]                    # (with the stored term)
        h.set_image_terms([])
        assert h.step(1) == 0
        _close(h, tr)
        return got, J

    res = _threads(world, body)
    U = B.GLIMS_E_USAGE
    for got, J in res:
        assert got == [U, U, U, U, 0, 0, U, U], got
        assert J == res[0][1]


def test_resolve_on_a_single_rank_handle_changes_nothing(backend):
    prob = Problem(2, 12)
    h, _, _, _ = _open(prob, 1, 0, None)
    x = np.concatenate([prob.points, sc.grid_points(*sc.overhanging_grid(prob.points, (15, 14)), (15, 14))])
    s = h.sampler_points(x)
    f = np.random.default_rng(1).standard_normal(len(prob.points))
    r = np.random.default_rng(2).standard_normal((len(x), 3))
    before = (s.cells, s.weights, s.apply(f), s.apply_t(r), s.n_found, s.counted)
    s.resolve(np.arange(len(prob.cells)))
    s.resolve(np.arange(len(prob.cells))[::-1])                 # (not even read: the sampler is global already)
    after = (s.cells, s.weights, s.apply(f), s.apply_t(r), s.n_found, s.counted)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    assert np.array_equal(s.counted, s.cells >= 0)
    h.close()


# ---- 8. public API, 2 process ranks (gloo-staged transport) ------------------------------------------------------------------
def _fit_sim(D, rho):
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.simulation import TumorGrowth
    F = aic.FIT

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
    labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1), fenics.FunctionSpace(mesh, "DG", 1))
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                               proliferation=rho, E=0.001, poisson=0.4, sim_time=F["steps"] * F["dt"],
                               sim_time_step=F["dt"])
    return sim


def _image_api(out_dir, tag):
    from glimslib_amd.optimization import ReducedFunctional, minimize
    from glimslib_amd.utils.data_io import Image
    # sim.image_term + sim.adjoint_gradient on a TumorGrowthBrain run
    sim = _brain_sim()
    sim.run(keep_nth=10 ** 9, save_method=None, clear_all=False, plot=False, output_dir=out_dir, record_adjoint=True)
    n_steps = int(sim._backend.stats()["steps"])
    origin, spacing, size = (-0.7, -0.6, -0.5), (1.13, 1.07, 1.21), (19, 18, 14)
    rng = np.random.default_rng(6)
    arr = rng.uniform(0, 1, size[::-1])
    arr[rng.random(arr.shape) < 0.1] = np.nan
    im = Image(arr, origin, spacing)
    terms = [sim.image_term(n_steps, im, kind='img_thresh', level=0.3, smooth=0.1),
             sim.image_term(max(1, n_steps // 2), im, kind='img_l2', weight=0.5),
             dict(step=n_steps, kind="c_l2", weight=2.0, target=rng.uniform(0, 0.3, sim.mesh.num_vertices()))]
    g = sim.adjoint_gradient(terms)
    info = sim._backend.image_term_info(0)
    sim.close()
    # the (D, rho) fit to two threshold images of test_gpu_adjoint_image.py
    F = aic.FIT
    truth = _fit_sim(*F["truth"])
    truth.run(save_method=None, plot=False, output_dir=out_dir)
    c_img = truth.sample_image('concentration', max(truth.results.get_recording_steps()), origin=F["origin"],
                               spacing=F["spacing"], size=F["size"])
    truth.close()
    th = lambda x, lv: 0.5 * (np.tanh((x - lv) / F["smooth"]) + 1.0)
    images = [Image(th(c_img.array, lv), F["origin"], F["spacing"]) for lv in F["levels"]]
    fit = _fit_sim(*F["start"])
    rf = ReducedFunctional(fit, 2, lambda s, n: [s.image_term(n, i, kind='img_thresh', level=lv, smooth=F["smooth"])
                                                 for i, lv in zip(images, F["levels"])],
                           run_kwargs=dict(output_dir=out_dir))
    res = minimize(rf, list(F["start"]), bounds=F["bounds"], options=dict(F["options"]), tol=F["tol"])
    out = dict(grad=g, n_obs=info[2], x=res.x, nit=res.nit, n_obs_fit=fit._backend.image_term_info(1)[2])
    fit.close()
    with open(os.path.join(out_dir, "%s.pkl" % tag), "wb") as f:
        pickle.dump(out, f)
    return out


def _api_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["GLIMS_TRANSPORT"] = "gloo"
    os.environ["GLIMS_FORCE_DEVICE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _image_api(out_dir, "img_rank%d" % rank)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_public_api_two_process_ranks_image_gradient_and_fit(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_api_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    z = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), "img_rank%d.pkl" % r), "rb") as f:
            z.append(pickle.load(f))
    ref = _image_api(str(tmp_path), "single")
    for k in ("J", "D_WM", "D_GM", "rho_WM", "rho_GM", "coupling"):
        assert z[0]["grad"][k] == z[1]["grad"][k], k
        assert _rel(z[0]["grad"][k], ref["grad"][k]) <= TOL, (k, z[0]["grad"][k], ref["grad"][k])
    assert np.array_equal(z[0]["grad"]["c0"], z[1]["grad"]["c0"])
    assert _rel(z[0]["grad"]["c0"], ref["grad"]["c0"]) <= TOL
    assert z[0]["n_obs"] == z[1]["n_obs"] == ref["n_obs"] > 0 and z[0]["n_obs_fit"] == z[1]["n_obs_fit"] == ref["n_obs_fit"]
    print("fit: %s after %d iterations on 2 ranks, %s after %d on one" % (z[0]["x"], z[0]["nit"], ref["x"], ref["nit"]))
    assert np.array_equal(z[0]["x"], z[1]["x"])
    assert _rel(z[0]["x"], ref["x"]) <= 1e-6
