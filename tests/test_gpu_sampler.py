"""Samplers on the device (glims_sampler_*) against the numpy statement of their contract in
tests/sampler_common.py: location and P on unstructured 2-D / 3-D meshes (grid and point set, device and host symbolic phase),
exact ties on power-of-two lattices, independence of the internal renumbering, the device fields, P^T (reference, adjointness,
bitwise repeatability, skewed lists), neutrality towards the solver and the adjoint, a 200 k-node mesh under a 128^3 grid,
misuse, partitioned handles and the public API.

Tolerances: weights 1e-10 absolute, values 1e-10 relative to max|f| (both sides solve the same d x d system in fp64, error
~ kappa 2^-52 <= 3e-13 for the kappa <= 1.3e3 of these meshes; two decades for contraction and summation order).  Every test
that compares cell indices first asserts, on the reference alone, that no decision of its points sits within EPS / 2 of the
acceptance threshold (sampler_common.assert_decisive).

Wall time on an MI355X box: 30 s for the file, 16 s of it the 200 k-node case (mesh generation and the numpy reference)."""
import os
import pickle
import socket
import time

import numpy as np
import pytest

import torch  # noqa: F401

import sampler_common as sc
from adjoint_common import Problem, renumber
from glimslib_amd import workloads
from glimslib_amd.mesh import BoxMesh, RectangleMesh

pytestmark = pytest.mark.gpu

_SKIP = {"ms_steps", "ms_spmv", "ms_mg_setup", "ms_mech", "ms_rd_mg_setup", "ms_spmv_steps", "ms_sweep_steps",
         "ms_update_steps", "ms_quad_steps", "ms_cheb_steps", "ms_exchange", "ms_exchange_exposed", "ms_mgfine_mech",
         "ms_spmvb_mech", "us_spmv_median", "us_sweep_median", "us_update_median", "us_quad_median", "us_cheb_median",
         "us_mgfine_median", "us_spmvb_median"}

_BL = {}


def _brain_like(n):
    if n not in _BL:
        wl = workloads.config_brain_like(n, mechanics=True)
        sc.assert_mesh_ok(wl.mesh.points, wl.mesh.cells)
        _BL[n] = wl
    return _BL[n]


def _bare(backend, pts, cells):
    return backend.Handle(pts, cells, np.zeros(len(cells), dtype=np.int32))


def _affine(x, k=3, seed=0):
    rng = np.random.default_rng(seed)
    return x @ rng.standard_normal((x.shape[1], k)) + rng.standard_normal(k)


def _check_against_reference(s, pts, cells, x, ref=None):
    """cells, n_found, weights, a random scalar field, a 3-component field, an affine field, both fills."""
    cell, w, margin, _ = ref if ref is not None else sc.locate(pts, cells, x)
    sc.assert_decisive(margin)
    found = cell >= 0
    assert s.n_points == len(x)
    got = s.cells
    assert np.array_equal(got, cell), "%d cells differ" % (got != cell).sum()
    assert s.n_found == found.sum()
    gw = s.weights
    print("weights: max |dw| = %.3e" % np.abs(gw - w).max())
    assert np.abs(gw - w).max() <= 1e-10
    assert (gw[~found] == 0).all()
    rng = np.random.default_rng(11)
    for f in (rng.standard_normal(len(pts)), rng.standard_normal((len(pts), 3))):
        a, b = s.apply(f), sc.apply(cells, cell, w, f)
        assert a.shape == b.shape
        err = np.abs(a[found] - b[found]).max() / np.abs(f).max()
        print("values (%s): %.3e" % (f.shape, err))
        assert err <= 1e-10
        assert np.isnan(a[~found]).all() and not np.isnan(a[found]).any()
        a = s.apply(f, fill=-3.5)
        assert (a[~found] == -3.5).all() and np.array_equal(a[found], s.apply(f)[found])
    aff = s.apply(_affine(pts))
    want = _affine(x)
    err = np.abs(aff[found] - want[found]).max() / np.abs(want).max()
    print("affine: %.3e" % err)
    assert err <= 1e-12
    return cell, w


# ---- 3. location and P -----------------------------------------------------------------------------------------------------
def test_location_and_values_2d_delaunay(backend):
    pts, cells = sc.jittered_delaunay_2d(24, 12)
    sc.assert_mesh_ok(pts, cells)
    size = (37, 29)
    origin, spacing = sc.overhanging_grid(pts, size)
    x = sc.grid_points(origin, spacing, size)
    ref = sc.locate(pts, cells, x)
    h = _bare(backend, pts, cells)
    _check_against_reference(h.sampler_grid(origin, spacing, size), pts, cells, x, ref)
    _check_against_reference(h.sampler_points(x), pts, cells, x, ref)
    h.close()


def _brain_case(backend):
    wl = _brain_like(5000)
    pts, cells = wl.mesh.points, wl.mesh.cells
    size = (23, 19, 17)
    origin, spacing = sc.overhanging_grid(pts, size)
    x = sc.grid_points(origin, spacing, size)
    ref = sc.locate(pts, cells, x)
    assert (ref[0] < 0).sum() > 100 and (ref[0] >= 0).sum() > 1000
    h = _bare(backend, pts, cells)
    _check_against_reference(h.sampler_grid(origin, spacing, size), pts, cells, x, ref)
    _check_against_reference(h.sampler_points(x), pts, cells, x, ref)
    # a point set in no particular order, with points far away and a lone point
    perm = np.random.default_rng(2).permutation(len(x))
    xs = np.concatenate([x[perm], [[1e6, 0.0, 0.0]]])
    cs = h.sampler_points(xs).cells
    assert np.array_equal(cs[:-1], ref[0][perm]) and cs[-1] == -1
    one = h.sampler_points(x[ref[0] >= 0][:1])
    assert one.n_found == 1 and one.cells[0] == ref[0][ref[0] >= 0][0]
    h.close()


def test_location_and_values_3d_brain_like(backend):
    _brain_case(backend)


def test_location_and_values_3d_host_symbolic_phase(backend):
    old = os.environ.get("GLIMS_HOST_SYMBOLIC")
    os.environ["GLIMS_HOST_SYMBOLIC"] = "1"        # cell_new2old is empty there: identity
    try:
        _brain_case(backend)
    finally:
        if old is None:
            os.environ.pop("GLIMS_HOST_SYMBOLIC", None)
        else:
            os.environ["GLIMS_HOST_SYMBOLIC"] = old


# ---- 4. ties, exactly ------------------------------------------------------------------------------------------------------
def _lattices():
    return ((BoxMesh((0., 0., 0.), (2., 1., 1.), 8, 2, 4), (0, 0, 0), (2, 1, 1), (8, 2, 4), 24),
            (RectangleMesh((-1., -1.), (1., 1.), 8, 4), (-1, -1), (1, 1), (8, 4), 6))


def _check_ties(s, pts, cells, x, cell, w, f):
    assert s.n_found == len(x)
    assert np.array_equal(s.cells, cell)
    assert np.array_equal(s.weights, w)                     # lambda in {0, 1/2, 1}: no rounding on either side
    out = s.apply(f)
    at_node = (w == 1.0).any(axis=1)
    nodes = cells[cell]
    assert np.array_equal(out[at_node], f[nodes[at_node][w[at_node] == 1.0]])
    mid = ~at_node
    ends = nodes[mid][w[mid] == 0.5].reshape(-1, 2)
    assert np.array_equal(out[mid], 0.5 * f[ends[:, 0]] + 0.5 * f[ends[:, 1]])


def test_ties_on_power_of_two_lattices_are_exact(backend):
    for mesh, lo, hi, n, most in _lattices():
        pts, cells = mesh.points, mesh.cells
        origin, spacing, size = sc.half_spacing_grid(lo, hi, n)
        x = sc.grid_points(origin, spacing, size)
        cell, w, margin, n_acc = sc.locate(pts, cells, x)
        assert margin.min() == sc.EPS and n_acc.max() == most and (cell >= 0).all()
        assert np.isin(w, (0.0, 0.5, 1.0)).all()
        f = np.random.default_rng(4).standard_normal(len(pts))
        h = _bare(backend, pts, cells)
        _check_ties(h.sampler_grid(origin, spacing, size), pts, cells, x, cell, w, f)
        _check_ties(h.sampler_points(x), pts, cells, x, cell, w, f)
        # the nodes themselves as a point set: the nodal values come back bitwise
        sn = h.sampler_points(pts)
        assert sn.n_found == len(pts) and np.array_equal(sn.apply(f), f)
        h.close()


# ---- 5. numbering ----------------------------------------------------------------------------------------------------------
def _shuffled(pts, cells, seed):
    p2, c2, perm = renumber(pts, cells, seed)              # new node i = old perm[i]
    cp = np.random.default_rng(seed + 100).permutation(len(cells))
    return p2, np.ascontiguousarray(c2[cp]), perm, cp      # new cell j = old cp[j]


def test_winner_follows_the_callers_numbering(backend):
    wl = _brain_like(5000)
    pts, cells = wl.mesh.points, wl.mesh.cells
    size = (23, 19, 17)
    origin, spacing = sc.overhanging_grid(pts, size)
    x = sc.grid_points(origin, spacing, size)
    sc.assert_decisive(sc.locate(pts, cells, x)[2])
    f = np.random.default_rng(8).standard_normal((len(pts), 2))
    res = []
    for seed in (1, 2):
        p2, c2, perm, cp = _shuffled(pts, cells, seed)
        h = _bare(backend, p2, c2)
        s = h.sampler_grid(origin, spacing, size)
        c = s.cells
        res.append((np.where(c >= 0, cp[np.maximum(c, 0)], -1), s.apply(f[perm])))
        h.close()
    assert np.array_equal(res[0][0], res[1][0])            # the same geometric cell under both numberings
    found = res[0][0] >= 0
    assert np.abs(res[0][1][found] - res[1][1][found]).max() <= 1e-12 * np.abs(f).max()
    # where several cells accept, the winner is the smallest index in the numbering the caller gave
    for mesh, lo, hi, n, most in _lattices():
        origin, spacing, size = sc.half_spacing_grid(lo, hi, n)
        x = sc.grid_points(origin, spacing, size)
        winners = []
        for seed in (3, 4):
            p2, c2, perm, cp = _shuffled(mesh.points, mesh.cells, seed)
            cell, w, margin, _ = sc.locate(p2, c2, x)
            assert margin.min() == sc.EPS
            h = _bare(backend, p2, c2)
            s = h.sampler_grid(origin, spacing, size)
            assert np.array_equal(s.cells, cell) and np.array_equal(s.weights, w)
            winners.append(cp[cell])
            h.close()
        assert not np.array_equal(winners[0], winners[1])  # ... which is a different geometric cell at some ties


# ---- 6. fields -------------------------------------------------------------------------------------------------------------
def _coupled(backend, wl, steps=3, **opts):
    pts, cells = wl.mesh.points, wl.mesh.cells
    h = backend.Handle(pts, cells, wl.cell_label)
    t = wl.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    h.set_options(dt=1.0, **opts)
    dn = np.asarray(wl.dirichlet_nodes)
    dofs = (dn[:, None] * 3 + np.arange(3)).ravel()
    h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
    h.setup(True)
    h.set_state(_c0(pts))
    if steps:
        assert h.step(steps) == 0
        assert h.solve_mechanics() == 0
    return h


# both sides of the partitioned comparison solve to well below its 1e-10: what is left is the samplers' difference
_TIGHT = dict(newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12)


def _c0(pts):
    return 0.8 * np.exp(-0.5 * ((pts - np.array([118.0, -109.0, 72.0])) ** 2).sum(axis=1) / 20.0 ** 2)


def test_device_fields_are_sampled_without_a_host_round_trip(backend):
    wl = _brain_like(5000)
    h = _coupled(backend, wl)
    size = (23, 19, 17)
    origin, spacing = sc.overhanging_grid(wl.mesh.points, size)
    s = h.sampler_grid(origin, spacing, size)
    c, u = h.get_state()
    sid = h.snapshot_save()
    assert h.step(1) == 0                                   # the snapshot is no longer the current state
    a, b = s.apply('c', snapshot=sid), s.apply(h.snapshot_load(sid))
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, s.apply(c), equal_nan=True)
    assert np.nanmax(np.abs(a)) > 1e-3
    assert h.solve_mechanics() == 0
    c1, u1 = h.get_state()
    assert not np.array_equal(c1, c)
    assert np.array_equal(s.apply('c'), s.apply(c1), equal_nan=True)
    au = s.apply('u')
    assert au.shape == (s.n_points, 3) and np.array_equal(au, s.apply(u1.reshape(-1, 3)), equal_nan=True)
    assert np.nanmax(np.abs(au)) > 0
    h.close()


# ---- 7. the transpose ------------------------------------------------------------------------------------------------------
def _check_transpose(backend, pts, cells, make, x, ncomps=(1, 3, 8)):
    cell, w, margin, _ = sc.locate(pts, cells, x)
    sc.assert_decisive(margin)
    rng = np.random.default_rng(21)
    out = {}
    for round_ in range(2):                                 # two fresh handles
        h = _bare(backend, pts, cells)
        s = make(h)
        assert np.array_equal(s.cells, cell)
        for k in ncomps:
            r = np.random.default_rng(30 + k).standard_normal((len(x), k))
            r[cell < 0] = np.nan if k == 1 else 1e300         # values at outside points are not read into any sum
            g = s.apply_t(r if k > 1 else r[:, 0])
            g2 = s.apply_t(r if k > 1 else r[:, 0])
            assert np.array_equal(g, g2)                    # two calls
            if round_:
                assert np.array_equal(g, out[k])            # two handles
            out[k] = g
            rr = np.where((cell >= 0)[:, None], r, 0.0)
            ref = sc.apply_t(cells, cell, w, rr, len(pts)).reshape(g.shape)
            scale = max(np.abs(ref).max(), 1e-300)
            print("P^T ncomp %d: %.3e" % (k, np.abs(g - ref).max() / scale))
            assert np.abs(g - ref).max() <= 1e-10 * scale
            f = rng.standard_normal((len(pts), k))
            lhs = (np.where((cell >= 0)[:, None], s.apply(f, fill=0.0).reshape(len(x), k), 0.0) * rr).sum()
            rhs = (f * g.reshape(len(pts), k)).sum()
            assert abs(lhs - rhs) <= 1e-12 * np.abs(s.apply(f, fill=0.0).reshape(len(x), k) * rr).sum()
        h.close()


def test_transpose_on_the_brain_like_mesh(backend):
    wl = _brain_like(5000)
    pts, cells = wl.mesh.points, wl.mesh.cells
    size = (23, 19, 17)
    origin, spacing = sc.overhanging_grid(pts, size)
    x = sc.grid_points(origin, spacing, size)
    _check_transpose(backend, pts, cells, lambda h: h.sampler_grid(origin, spacing, size), x)
    _check_transpose(backend, pts, cells, lambda h: h.sampler_points(x), x, ncomps=(1,))


def test_transpose_with_thousands_of_points_per_cell(backend):
    mesh = BoxMesh((0., 0., 0.), (1., 1., 1.), 4, 4, 4)
    size = (64, 64, 64)
    origin, spacing = sc.overhanging_grid(mesh.points, size, overhang=0.02)
    x = sc.grid_points(origin, spacing, size)
    _check_transpose(backend, mesh.points, mesh.cells, lambda h: h.sampler_grid(origin, spacing, size), x, ncomps=(1, 3))
    _check_transpose(backend, mesh.points, mesh.cells, lambda h: h.sampler_points(x), x, ncomps=(1,))


def test_transpose_with_almost_every_list_empty(backend):
    wl = _brain_like(40000)
    pts, cells = wl.mesh.points, wl.mesh.cells
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    x = lo + (hi - lo) * np.array([[0.31, 0.42, 0.53], [0.11, 0.77, 0.29], [0.5, 0.5, 0.5], [0.93, 0.08, 0.61],
                                   [1.5, 0.5, 0.5]])
    _check_transpose(backend, pts, cells, lambda h: h.sampler_points(x), x)


# ---- 8. neutrality ---------------------------------------------------------------------------------------------------------
def test_samplers_leave_the_solver_and_the_adjoint_alone(backend):
    wl = _brain_like(5000)
    pts = wl.mesh.points
    size = (23, 19, 17)
    origin, spacing = sc.overhanging_grid(pts, size)
    a, b = _coupled(backend, wl, steps=0), _coupled(backend, wl, steps=0)
    assert a.step(2) == 0 and b.step(2) == 0
    s = a.sampler_grid(origin, spacing, size)
    s.apply('c')
    s.apply(np.ones((len(pts), 3)))
    s.apply_t(np.ones(s.n_points))
    p = a.sampler_points(pts[:100])
    p.apply('c')
    s.close()
    assert a.step(2) == 0 and b.step(2) == 0
    assert a.solve_mechanics() == 0 and b.solve_mechanics() == 0
    p.apply('u')
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    sa, sb = a.stats(), b.stats()
    assert {k: v for k, v in sa.items() if k not in _SKIP} == {k: v for k, v in sb.items() if k not in _SKIP}
    a.close()
    b.close()
    # the cell -> vertex map is shared with the adjoint: a gradient taken after a sampler was created has the bits of one
    # taken before any
    prob = Problem(3, 6)
    grads = []
    for with_sampler in (False, True):
        h = backend.Handle(prob.points, prob.cells, prob.labels)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt)
        h.set_dirichlet_c(prob.dir_c[0], prob.dir_c[1])
        h.set_dirichlet_u(prob.dir_u[0], prob.dir_u[1])
        h.setup(True)
        h.set_state(prob.c0)
        if with_sampler:
            assert h.sampler_points(prob.points).n_found == len(prob.points)
        h.adjoint_record(True)
        assert h.step(3) == 0
        grads.append(h.adjoint_gradient(prob.terms(3)))
        h.close()
    for x, y in zip(grads[0], grads[1]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- 9. size ---------------------------------------------------------------------------------------------------------------
def test_200k_node_mesh_under_a_128_cubed_grid(backend):
    t0 = time.perf_counter()
    wl = _brain_like(200000)
    pts, cells = wl.mesh.points, wl.mesh.cells
    size = (128, 128, 128)
    origin, spacing = sc.overhanging_grid(pts, size)
    t1 = time.perf_counter()
    h = _bare(backend, pts, cells)
    t2 = time.perf_counter()
    s = h.sampler_grid(origin, spacing, size)
    t3 = time.perf_counter()
    aff = s.apply(_affine(pts))
    t4 = time.perf_counter()
    print("mesh %.1f s, handle %.1f s, sampler of %d points in %d cells %.3f s (%d found), apply of 3 components %.3f s"
          % (t1 - t0, t2 - t1, s.n_points, len(cells), t3 - t2, s.n_found, t4 - t3))
    x = sc.grid_points(origin, spacing, size)
    cells_dev = s.cells
    found = cells_dev >= 0
    want = _affine(x)
    assert found.sum() > 1000000
    assert np.abs(aff[found] - want[found]).max() <= 1e-12 * np.abs(want).max()
    assert np.isnan(aff[~found]).all()
    draw = np.random.default_rng(17).choice(len(x), 2000, replace=False)
    cell, w, margin, _ = sc.locate(pts, cells, x[draw])
    sc.assert_decisive(margin)
    assert np.array_equal(cells_dev[draw], cell)            # one by one
    f = np.random.default_rng(18).standard_normal(len(pts))
    got, ref = s.apply(f)[draw], sc.apply(cells, cell, w, f)
    ok = cell >= 0
    assert np.abs(got[ok] - ref[ok]).max() <= 1e-10 * np.abs(f).max() and np.isnan(got[~ok]).all()
    h.close()


# ---- 10. misuse ------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_with_a_reason(backend):
    import ctypes as C
    mesh = BoxMesh((0., 0., 0.), (1., 1., 1.), 4, 4, 4)        # power-of-two spacing: the last line below is exact
    h = _bare(backend, mesh.points, mesh.cells)
    s = h.sampler_points(mesh.points)
    f = np.zeros(len(mesh.points))

    def refused(fn, *needles):
        with pytest.raises(backend.BackendError) as ei:
            fn()
        assert ei.value.code == backend.GLIMS_E_USAGE
        for n in needles:
            assert n in str(ei.value), str(ei.value)

    refused(lambda: s.apply(np.zeros((len(f), 9))), "ncomp", "outside 1 .. 8")
    refused(lambda: s.apply_t(np.zeros((s.n_points, 9))), "ncomp")
    refused(lambda: s.apply('u'), "GLIMS_FIELD_U", "with_mechanics")
    refused(lambda: s.apply('c', snapshot=5), "unknown snapshot")
    refused(lambda: s.apply('c'), "glims_set_state")
    refused(lambda: h.sampler_grid((0, 0, 0), (0.1, 0.1, 0.1), (4, 0, 4)), "size", "not positive")
    refused(lambda: h.sampler_grid((0, 0, 0), (0.1, -0.1, 0.1), (4, 4, 4)), "spacing", "not positive")
    sid = C.c_int64(-1)
    st = h.lib.glims_sampler_create_points(h._h, 0, None, 1, C.byref(sid))
    assert st == backend.GLIMS_E_USAGE and b"flags" in h.lib.glims_last_error(h._h)
    st = h.lib.glims_sampler_info(h._h, 77, None, None)
    assert st == backend.GLIMS_E_USAGE and b"unknown sampler id" in h.lib.glims_last_error(h._h)
    s.close()
    st = h.lib.glims_sampler_destroy(h._h, 0)
    assert st == backend.GLIMS_E_USAGE and b"unknown sampler id" in h.lib.glims_last_error(h._h)
    # no points at all is valid, and the handle works afterwards
    e = h.sampler_points(np.zeros((0, 3)))
    assert e.n_points == 0 and e.n_found == 0 and e.apply(f).shape == (0,) and len(e.cells) == 0
    assert np.array_equal(e.apply_t(np.zeros(0)), np.zeros(len(f)))
    s2 = h.sampler_points(mesh.points)
    assert s2.n_found == len(f) and np.array_equal(s2.apply(np.arange(len(f), dtype=float)), np.arange(len(f)))
    h.close()


# ---- 11. partitioned handles -----------------------------------------------------------------------------------------------
def _part_handle(backend, pts, cells, labels, world, rank, tr):
    from glimslib_amd.partition import partition_mesh
    part = partition_mesh(pts, cells, world, rank)
    h = backend.Handle(part.points, part.cells, labels[part.cell_ids], n_own=part.n_own, device=0)
    h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
    h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
    h.set_mg_frame(pts.min(axis=0), pts.max(axis=0))
    return h, part


def _merge(res):
    """The rule of DistributedSampler: smallest global cell id, value from the smallest rank that holds it.  Also returns
    the largest difference between two ranks that hold the winner."""
    big = np.iinfo(np.int64).max
    allg = np.stack([np.where(r["cells"] >= 0, r["cells"], big) for r in res])
    win = allg.min(axis=0)
    cells = np.where(win < big, win, -1)
    out, spread = {}, {}
    for k in res[0]["values"]:
        vals = np.stack([r["values"][k] for r in res])
        holds = (allg == win[None]) & (win < big)[None]
        first = holds.argmax(axis=0)
        out[k] = np.take_along_axis(vals, first.reshape((1, -1) + (1,) * (vals.ndim - 2)), axis=0)[0]
        hv = np.where(holds.reshape(holds.shape + (1,) * (vals.ndim - 2)), vals, np.nan)
        multi = holds.sum(axis=0) > 1
        spread[k] = float(np.nanmax(np.nanmax(hv[:, multi], axis=0) - np.nanmin(hv[:, multi], axis=0))) if multi.any() else 0.0
    return cells, out, spread


def _ranks_sample_coupled(backend, wl, world, origin, spacing, size, steps):
    from glimslib_amd.parallel import run_threaded_ranks
    pts, cells = wl.mesh.points, wl.mesh.cells
    t = wl.tables

    def body(rank, tr):
        h, part = _part_handle(backend, pts, cells, wl.cell_label, world, rank, tr)
        g2l = np.full(len(pts), -1, dtype=np.int64)
        g2l[part.global_ids[:part.n_own]] = np.arange(part.n_own)
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        h.set_options(dt=1.0, **_TIGHT)
        loc = g2l[np.asarray(wl.dirichlet_nodes)]
        loc = loc[loc >= 0]
        dofs = (loc[:, None] * 3 + np.arange(3)).ravel()
        h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
        h.setup(True)
        h.set_state(_c0(pts)[part.global_ids])
        assert h.step(steps) == 0
        assert h.solve_mechanics() == 0
        s = h.sampler_grid(origin, spacing, size)
        lc = s.cells
        out = dict(cells=np.where(lc >= 0, part.cell_ids[np.maximum(lc, 0)], -1).astype(np.int64),
                   values=dict(c=s.apply('c'), u=s.apply('u')))
        with pytest.raises(backend.BackendError) as ei:
            s.apply_t(np.zeros(s.n_points))
        assert ei.value.code == backend.GLIMS_E_USAGE and "partitioned" in str(ei.value)
        h.close()
        if getattr(tr, "failed", None) is not None:
            raise tr.failed
        return out

    return run_threaded_ranks(world, body)


def test_partitioned_samplers_merge_to_the_single_rank_sampler(backend):
    wl = _brain_like(5000)
    pts, cells = wl.mesh.points, wl.mesh.cells
    size = (23, 19, 17)
    origin, spacing = sc.overhanging_grid(pts, size)
    x = sc.grid_points(origin, spacing, size)
    sc.assert_decisive(sc.locate(pts, cells, x)[2])
    steps = 3
    h = _coupled(backend, wl, steps=steps, **_TIGHT)
    s = h.sampler_grid(origin, spacing, size)
    one = dict(cells=s.cells.astype(np.int64), c=s.apply('c'), u=s.apply('u'))
    h.close()
    found = one["cells"] >= 0
    for world in (2, 4):
        cells_m, vals, spread = _merge(_ranks_sample_coupled(backend, wl, world, origin, spacing, size, steps))
        assert np.array_equal(cells_m, one["cells"])         # found and not found alike
        for k in ("c", "u"):
            scale = np.abs(one[k][found]).max()
            err = np.abs(vals[k][found] - one[k][found]).max() / scale
            print("world %d, %s: %.3e from the single rank, %.3e between ranks that hold the winner" % (world, k, err, spread[k] / scale))
            assert err <= 1e-10
            assert spread[k] <= 1e-12 * scale
            assert np.isnan(vals[k][~found]).all()


def test_partitioned_ties_on_the_cut(backend):
    from glimslib_amd.parallel import run_threaded_ranks
    mesh, lo, hi, n, most = _lattices()[0]
    pts, cells = mesh.points, mesh.cells
    origin, spacing, size = sc.half_spacing_grid(lo, hi, n)
    x = sc.grid_points(origin, spacing, size)
    cell, w, margin, _ = sc.locate(pts, cells, x)
    f = np.random.default_rng(4).standard_normal(len(pts))
    ref = sc.apply(cells, cell, w, f)

    def body(rank, tr):
        h, part = _part_handle(backend, pts, cells, np.zeros(len(cells), dtype=np.int32), 2, rank, tr)
        s = h.sampler_grid(origin, spacing, size)
        lc = s.cells
        out = dict(cells=np.where(lc >= 0, part.cell_ids[np.maximum(lc, 0)], -1).astype(np.int64),
                   values=dict(f=s.apply(f[part.global_ids])))
        h.close()
        return out

    res = run_threaded_ranks(2, body)
    assert all((r["cells"] >= 0).any() and (r["cells"] < 0).any() for r in res)      # each rank holds a part only
    cells_m, vals, spread = _merge(res)
    assert np.array_equal(cells_m, cell)
    assert np.array_equal(vals["f"], ref) and spread["f"] == 0.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _image_sim():
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.simulation import TumorGrowth

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    mesh = fenics.BoxMesh(fenics.Point(0, 0, 0), fenics.Point(20, 18, 16), 10, 9, 8)
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped_0': {'bc_value': fenics.Constant((0.0, 0.0, 0.0)),
                                                             'named_boundary': 'boundary_all', 'subspace_id': 0}})
    iv = fenics.Expression('exp(-a*pow(x[0]-x0, 2) - a*pow(x[1]-y0, 2) - a*pow(x[2]-z0,2))', degree=1, a=0.05,
                           x0=12, y0=9, z0=8)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0., 0., 0.)), 1: iv}, diffusion=0.05, coupling=0.1,
                               proliferation=0.05, E=3000e-6, poisson=0.45, sim_time=3, sim_time_step=1)
    return sim


_IMG_GRID = dict(origin=(-1.3, -0.7, 0.4), spacing=(0.9, 1.1, 0.8), size=(26, 18, 20))


def _image_api(out_dir, tag, **run_kw):
    sim = _image_sim()
    sim.run(save_method=None, clear_all=False, plot=False, output_dir=out_dir, **run_kw)
    step = max(sim.results.get_recording_steps())
    out = dict(c=sim.sample_image('concentration', step, **_IMG_GRID), u=sim.sample_image('displacement', step, **_IMG_GRID),
               step=step, c_nodal=np.asarray(sim.results.get_solution_function(subspace_id=1, recording_step=step).values()),
               u_nodal=np.asarray(sim.results.get_solution_function(subspace_id=0, recording_step=step).values()),
               points=sim.mesh.points, cells=sim.mesh.cells)
    with open(os.path.join(out_dir, "%s.pkl" % tag), "wb") as f:
        pickle.dump({k: (v.array if hasattr(v, "array") else v) for k, v in out.items()}, f)
    sim.close()
    return out


def _image_worker(rank, world, port, out_dir):
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
def test_public_api_two_process_ranks_sample_image(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_image_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    z = []
    for r in range(world):
        with open(os.path.join(str(tmp_path), "img_rank%d.pkl" % r), "rb") as f:
            z.append(pickle.load(f))
    ref = _image_api(str(tmp_path), "single")
    for k in ("c", "u"):
        assert np.array_equal(z[0][k], z[1][k], equal_nan=True)          # bitwise the same on both ranks
        a, b = z[0][k], ref[k].array
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(b).any() and not np.isnan(b).all()
        ok = ~np.isnan(b)
        assert np.abs(a[ok] - b[ok]).max() <= 1e-10 * np.abs(b[ok]).max()


# ---- 12. public API --------------------------------------------------------------------------------------------------------
def test_interpolate_non_matching_and_images_of_functions(backend, tmp_path):
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.mesh import Mesh
    from glimslib_amd.utils import data_io
    cp, cc = sc.jittered_delaunay_2d(12, 6, seed=1)
    fp, fc = sc.jittered_delaunay_2d(31, 17, seed=2)
    sc.assert_mesh_ok(cp, cc)
    coarse, fine = Mesh(cp, cc), Mesh(fp, fc)
    vals = np.random.default_rng(9).standard_normal((len(cp), 2))
    src = fenics.Function(coarse, {None: vals})
    cell, w, margin, _ = sc.locate(cp, cc, fp)
    sc.assert_decisive(margin)
    ref = sc.apply(cc, cell, w, vals)
    got = data_io.interpolate_non_matching(src, fine)
    assert got.mesh is fine
    g = got.values()
    assert np.array_equal(np.isnan(g), np.isnan(ref))        # exactly the reference's outside set
    ok = cell >= 0
    assert np.abs(g[ok] - ref[ok]).max() <= 1e-10 * np.abs(vals).max()
    arr = data_io.interpolate_non_matching(src, fp, fill=0.0)
    assert np.array_equal(arr[ok], g[ok]) and (arr[~ok] == 0.0).all()
    # an image of a function of a structured mesh: the device path against the host path of the same call
    mesh = fenics.RectangleMesh(fenics.Point(0, 0), fenics.Point(2, 1), 8, 5)
    fn = fenics.Function(mesh, {None: np.random.default_rng(10).standard_normal(mesh.num_vertices())})
    host = data_io.create_image_from_fenics_function(fn, size_new=(21, 11))
    dev = data_io.create_image_from_fenics_function(fn, size_new=(21, 11), device=0)
    assert dev.array.shape == host.array.shape == (11, 21)
    assert np.abs(dev.array - host.array).max() <= 1e-12 * np.abs(fn.values()).max()
    assert np.allclose(dev.spacing, host.spacing, rtol=1e-14) and np.allclose(dev.origin, host.origin)
    own = data_io.create_image_from_fenics_function(fn, device=0)
    assert np.abs(own.array - data_io.create_image_from_fenics_function(fn).array).max() <= 1e-12 * np.abs(fn.values()).max()
    img = data_io.sample_function_on_grid(fn, (-0.25, -0.25), (0.125, 0.125), (21, 13))
    assert np.isnan(img.array[0]).all() and np.isnan(img.array[:, 0]).all() and not np.isnan(img.array[2:11, 2:19]).any()


def test_sample_image_of_device_resident_results(tmp_path):
    from glimslib_amd.utils import data_io
    out = _image_api(str(tmp_path), "device", results_on_device=True)
    from glimslib_amd.simulation.simulation_tumor_growth import DeviceSnapshotFunction  # noqa: F401
    x = sc.grid_points(_IMG_GRID["origin"], _IMG_GRID["spacing"], _IMG_GRID["size"])
    cell, w, margin, _ = sc.locate(out["points"], out["cells"], x)
    shape = tuple(reversed(_IMG_GRID["size"]))
    for k, nodal in (("c", out["c_nodal"]), ("u", out["u_nodal"])):
        img = out[k]
        ref = sc.apply(out["cells"], cell, w, nodal).reshape(shape + nodal.shape[1:])
        assert img.array.shape == ref.shape and img.is_vector == (k == "u")
        assert np.array_equal(np.isnan(img.array), np.isnan(ref)) and np.isnan(ref).any()
        ok = ~np.isnan(ref)
        assert np.abs(img.array[ok] - ref[ok]).max() <= 1e-10 * np.abs(nodal).max()
        assert np.abs(nodal).max() > 0
        path = os.path.join(str(tmp_path), "%s.mha" % k)
        img.write(path)
        back = data_io.Image.read(path)
        assert np.array_equal(back.array, img.array, equal_nan=True)
        assert back.origin == img.origin and back.spacing == img.spacing and back.is_vector == img.is_vector
