"""Deformed-configuration samplers and image warping on the device (glims_sampler_create_*_deformed, glims_sampler_warp,
GLIMS_FIELD_XYZ) against the numpy statement of their contract in tests/deformed_common.py.

Tolerances are those of tests/test_gpu_sampler.py: cells equal, weights 1e-10 absolute, values 1e-10 relative to max|f|,
affine fields 1e-12 (both sides solve the same d x d fp64 system on the same displaced coordinates -- X + scale * u is formed
with two roundings on both sides --, error ~ kappa 2^-52 for the kappa <= 5.1e3 of these meshes).  Every comparison of cell
indices first asserts, on the reference alone, that no decision sits within EPS / 2 of the acceptance threshold
(sampler_common.assert_decisive); every comparison of warped values first asserts that no inside / outside or voxel decision
sits within 1e-9 of a voxel of flipping (deformed_common.assert_resample_decisive)."""
import ctypes as C
import os

import numpy as np
import pytest

import torch  # noqa: F401

import deformed_common as dfc
import derive_common as dc
import sampler_common as sc
from glimslib_amd import fenics_local as fenics
from glimslib_amd import workloads
from glimslib_amd.mesh import RectangleMesh

pytestmark = pytest.mark.gpu

_CASES = {}


def _bare(backend, pts, cells):
    return backend.Handle(pts, cells, np.zeros(len(cells), dtype=np.int32))


def _case(name):
    """(points, cells, u, origin, spacing, size, x): built once per session, never modified.  The grid overhangs the DEFORMED
    mesh (scale 1)."""
    if name not in _CASES:
        if name in ("delaunay", "fold"):
            pts, cells = sc.jittered_delaunay_2d(24, 12)
            amp, size = (0.08, (37, 29)) if name == "delaunay" else (0.6, (37, 29))
        else:
            wl = workloads.config_brain_like(5000, mechanics=True)
            pts, cells = wl.mesh.points, wl.mesh.cells
            amp, size = 0.05, (23, 19, 17)
        sc.assert_mesh_ok(pts, cells)
        u = dfc.smooth_displacement(pts, amp)
        origin, spacing = sc.overhanging_grid(dfc.deformed_points(pts, u), size)
        _CASES[name] = (pts, cells, u, origin, spacing, size, sc.grid_points(origin, spacing, size))
    return _CASES[name]


_REFS = {}


def _ref(name, scale):
    """(cell, w, margin, n_accept) of the case's grid points in the mesh displaced by scale u."""
    if (name, scale) not in _REFS:
        pts, cells, u, _, _, _, x = _case(name)
        yd = dfc.deformed_points(pts, u, scale)
        if scale != 0.0:
            k = sc.kappa(yd, cells)
            assert np.isfinite(k).all() and k.max() < sc.KAPPA_MAX, "deformed cells up to kappa = %.3g" % k.max()
        _REFS[(name, scale)] = sc.locate(yd, cells, x)
    return _REFS[(name, scale)]


def _affine(x, k=3, seed=0):
    rng = np.random.default_rng(seed)
    return x @ rng.standard_normal((x.shape[1], k)) + rng.standard_normal(k)


def _check(s, pts, cells, u, scale, x, ref):
    """cells, n_found, weights, a random scalar and a 3-component field, the back map, the deformation info, P^T."""
    cell, w, margin, _ = ref
    sc.assert_decisive(margin)
    found = cell >= 0
    assert s.deformed and s.n_points == len(x)
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
    # the back map: P applied to the reference coordinates; P applied to the displaced coordinates gives the points back
    X = s.back_map()
    Xr = dfc.back_map(pts, cells, cell, w)
    err = np.abs(X[found] - Xr[found]).max() / np.abs(pts).max()
    print("back map: %.3e" % err)
    assert err <= 1e-10 and np.isnan(X[~found]).all()
    assert np.array_equal(X, s.apply('x'), equal_nan=True)
    assert (s.back_map(fill=-2.0)[~found] == -2.0).all()
    xs = s.apply(dfc.deformed_points(pts, u, scale))
    assert np.abs(xs[found] - x[found]).max() <= 1e-12 * max(1.0, np.abs(x).max())     # an affine field of the displaced mesh
    # det(E_deformed) / det(E_reference)
    r = dfc.cell_ratios(pts, cells, u, scale)
    assert s.n_inverted == dfc.n_inverted(r)
    print("min ratio: %.6e (numpy %.6e)" % (s.min_jacobian, r.min()))
    assert abs(s.min_jacobian - r.min()) <= 1e-12 * abs(r.min())
    # P^T
    rr = rng.standard_normal((len(x), 2))
    g, gr = s.apply_t(rr), sc.apply_t(cells, cell, w, rr, len(pts))
    err = np.abs(g - gr).max() / np.abs(gr).max()
    print("transpose: %.3e" % err)
    assert err <= 1e-10
    assert np.array_equal(g, s.apply_t(rr))


# ---- 1. / 2. location, P, P^T, back map ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["delaunay", "brain"])
def test_host_source_grid_and_points(backend, name):
    pts, cells, u, origin, spacing, size, x = _case(name)
    h = _bare(backend, pts, cells)
    ref = _ref(name, 1.0)
    # the displacement matters: most voxels land in another cell than on the undeformed mesh
    ref0 = _ref(name, 0.0)
    moved = (ref[0] != ref0[0]).sum()
    print("%d of %d voxels land in another cell" % (moved, len(x)))
    assert moved > len(x) // 4
    assert dfc.n_inverted(dfc.cell_ratios(pts, cells, u)) == 0
    sg = h.sampler_grid(origin, spacing, size, deformed_by=u)
    assert h.last_sampler_status == backend.GLIMS_OK and sg.n_inverted == 0
    _check(sg, pts, cells, u, 1.0, x, ref)
    _check(h.sampler_points(x, deformed_by=u), pts, cells, u, 1.0, x, ref)
    if name == "delaunay":
        refm = _ref(name, -1.0)
        _check(h.sampler_grid(origin, spacing, size, deformed_by=u, scale=-1.0), pts, cells, u, -1.0, x, refm)
        _check(h.sampler_points(x, deformed_by=u, scale=-1.0), pts, cells, u, -1.0, x, refm)
    # scale = 0: bit for bit the undeformed sampler
    for make in (lambda **kw: h.sampler_grid(origin, spacing, size, **kw), lambda **kw: h.sampler_points(x, **kw)):
        s0, sd = make(), make(deformed_by=u, scale=0.0)
        assert not s0.deformed and s0.n_inverted == 0 and s0.min_jacobian == 1.0
        assert sd.deformed and sd.n_inverted == 0 and sd.min_jacobian == 1.0
        assert np.array_equal(s0.cells, sd.cells) and np.array_equal(s0.weights, sd.weights) and s0.n_found == sd.n_found
        # GLIMS_FIELD_XYZ on an undeformed sampler: the points themselves
        f = s0.cells >= 0
        assert np.abs(s0.apply('x')[f] - x[f]).max() <= 1e-12 * max(1.0, np.abs(x).max())
    h.close()


# ---- 3. the fold ----------------------------------------------------------------------------------------------------------------
def test_folded_mesh_smallest_cell_index_wins(backend):
    pts, cells, u, origin, spacing, size, x = _case("fold")
    cell, w, margin, n_acc = _ref("fold", 1.0)
    sc.assert_decisive(margin)
    r = dfc.cell_ratios(pts, cells, u)
    n_inv = dfc.n_inverted(r)
    multi = n_acc > 1
    print("%d inverted cells, %d voxels accepted by more than one cell" % (n_inv, multi.sum()))
    assert n_inv > 0 and multi.sum() >= 10
    h = _bare(backend, pts, cells)
    for s in (h.sampler_grid(origin, spacing, size, deformed_by=u), h.sampler_points(x, deformed_by=u)):
        assert s.n_inverted == n_inv
        assert s.min_jacobian < 0 and abs(s.min_jacobian - r.min()) <= 1e-10 * abs(r.min())
        got = s.cells
        assert np.array_equal(got, cell), "%d cells differ" % (got != cell).sum()
        assert np.array_equal(got[multi], cell[multi])
        assert np.abs(s.weights - w).max() <= 1e-10
    h.close()


# ---- 4. the big-cell queue ------------------------------------------------------------------------------------------------------
def test_big_cell_queue_affine_back_map(backend):
    mesh = RectangleMesh((0., 0.), (1., 1.), 4, 4)
    pts, cells = mesh.points, mesh.cells
    A = np.array([[0.20, -0.10], [0.05, 0.15]])
    b = np.array([0.07, -0.04])
    u = pts @ A.T + b
    F = np.eye(2) + A
    yd = dfc.deformed_points(pts, u)
    size = (97, 97)
    origin, spacing = sc.overhanging_grid(yd, size)
    x = sc.grid_points(origin, spacing, size)
    # every cell's bounding box holds more candidates than the per-thread path takes (256)
    ext = (yd[cells].max(axis=1) - yd[cells].min(axis=1)) / spacing
    assert (np.floor(ext).prod(axis=1) > 256).all()
    cell, w, margin, _ = sc.locate(yd, cells, x)
    sc.assert_decisive(margin)
    found = cell >= 0
    assert found.sum() > 4000 and (~found).sum() > 500
    Xp = np.linalg.solve(F, (x - b).T).T
    h = _bare(backend, pts, cells)
    for s in (h.sampler_grid(origin, spacing, size, deformed_by=u), h.sampler_points(x, deformed_by=u)):
        assert np.array_equal(s.cells, cell)
        X = s.back_map()
        err = np.abs(X[found] - Xp[found]).max()
        print("analytic back map: %.3e" % err)
        assert err <= 1e-12 and np.isnan(X[~found]).all()
        assert abs(s.min_jacobian - np.linalg.det(F)) <= 1e-12 and s.n_inverted == 0
    h.close()


# ---- 5. device sources ----------------------------------------------------------------------------------------------------------
_BOX = {}


def _box():
    if not _BOX:
        mesh = fenics.BoxMesh((0, 0, 0), (2, 1, 1.5), 6, 6, 6)
        _BOX["mesh"], _BOX["lab"] = mesh, dc.two_labels(mesh)
    return _BOX["mesh"], _BOX["lab"]


def _coupled(backend, n_steps=3):
    mesh, lab = _box()
    t = dict(dc.TABLES)
    t["gamma"] = np.asarray(t["gamma"], dtype=np.float64) * 2.0          # a displacement of a few per cent of the box
    h = backend.Handle(mesh.points, mesh.cells, lab)
    h.set_materials(*[t[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=1.0, mech_rtol=1e-12)
    f = mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    bn = bn[mesh.points[bn, 0] == 0.0]                                   # clamped on one face: the rest of the box moves
    dofs = (bn[:, None] * 3 + np.arange(3)).ravel()
    h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
    h.setup(True)
    X = mesh.points
    ctr = X.min(axis=0) + 0.45 * (X.max(axis=0) - X.min(axis=0))
    h.set_state(0.8 * np.exp(-4.0 * ((X - ctr) ** 2).sum(axis=1)))
    ids = []
    for _ in range(n_steps):
        assert h.step(1) == backend.GLIMS_OK
        ids.append(h.snapshot_save())
    return h, ids


def _box_grid(pts, u):
    size = (13, 9, 11)
    origin, spacing = sc.overhanging_grid(dfc.deformed_points(pts, u), size)
    return origin, spacing, size


def _same(a, b, tol=0.0):
    assert np.array_equal(a.cells, b.cells) and a.n_found == b.n_found
    d = np.abs(a.weights - b.weights).max()
    assert d <= tol, d
    return d


def test_device_sources_share_the_displacement(backend):
    h, ids = _coupled(backend)
    pts, cells = _box()[0].points, _box()[0].cells
    sid = ids[1]
    # the snapshot source solves the displacement itself ...
    n0 = h.derive_info()["elastic_solves"]
    m0 = h.stats()["mech_solves"]
    probe = h.sampler_points(pts[:1], deformed_by=sid)
    assert h.last_sampler_status == backend.GLIMS_OK and probe.deformed
    assert h.derive_info()["elastic_solves"] == n0 + 1 and h.stats()["mech_solves"] == m0 + 1
    u_own = h.get_state()[1].reshape(-1, 3)                               # U as the sampler left it
    assert np.abs(u_own).max() > 0.005
    origin, spacing, size = _box_grid(pts, u_own)
    x = sc.grid_points(origin, spacing, size)
    s_snap = h.sampler_grid(origin, spacing, size, deformed_by=sid)       # ... once: U belongs to the snapshot now
    assert h.stats()["mech_solves"] == m0 + 1
    ref = sc.locate(dfc.deformed_points(pts, u_own), cells, x)
    sc.assert_decisive(ref[2])
    assert np.array_equal(s_snap.cells, ref[0]) and np.abs(s_snap.weights - ref[1]).max() <= 1e-10
    assert (ref[0] >= 0).sum() > 300 and (ref[0] < 0).sum() > 100
    _same(s_snap, h.sampler_grid(origin, spacing, size, deformed_by=u_own))
    # ... and a derive of the same snapshot finds it in place
    h.derive("displacement_norm", snapshot=sid)
    assert h.derive_info()["elastic_solves"] == n0 + 1 and h.stats()["mech_solves"] == m0 + 1
    # the other way round: derive first, then the sampler
    h.derive("total_jacobian", snapshot=ids[2])
    n1, m1 = h.derive_info()["elastic_solves"], h.stats()["mech_solves"]
    assert (n1, m1) == (n0 + 2, m0 + 2)
    s2 = h.sampler_grid(origin, spacing, size, deformed_by=ids[2])
    assert (h.derive_info()["elastic_solves"], h.stats()["mech_solves"]) == (n1, m1)
    assert not np.array_equal(s2.weights, s_snap.weights)
    # snapshot_mechanics' u through the host: the same sampler (an independent solve of the same system, both to 1e-12)
    u_sm, st = h.snapshot_mechanics(sid)
    assert st == backend.GLIMS_OK
    s_host = h.sampler_grid(origin, spacing, size, deformed_by=u_sm.reshape(-1, 3))
    print("snapshot source vs HOST(snapshot_mechanics): max |dw| = %.3e" % _same(s_snap, s_host, 1e-10))
    # CURRENT after snapshot_mechanics: U as it stands, bit for bit the HOST source of the same array
    m2 = h.stats()["mech_solves"]
    s_cur = h.sampler_grid(origin, spacing, size, deformed_by='current')
    assert h.stats()["mech_solves"] == m2
    _same(s_cur, s_host)
    # (the point-set creator reads its coordinates from memory, the grid creator forms them in registers: the project's
    # tolerance for weights, as between any grid and its point set in tests/test_gpu_sampler.py)
    _same(s_cur, h.sampler_points(x, deformed_by='current'), 1e-10)
    # frozen: further steps, solves and snapshot_clear do not move it
    c0, w0 = s_cur.cells.copy(), s_cur.weights.copy()
    f = np.random.default_rng(5).standard_normal(len(pts))
    a0 = s_cur.apply(f)
    assert h.step(2) == backend.GLIMS_OK
    assert h.solve_mechanics() == backend.GLIMS_OK
    h.snapshot_clear()
    assert np.array_equal(s_cur.cells, c0) and np.array_equal(s_cur.weights, w0)
    assert np.array_equal(s_cur.apply(f), a0, equal_nan=True)
    h.close()


def test_the_steps_that_follow_keep_their_bits(backend):
    runs = []
    pts = _box()[0].points
    for call in (True, False):
        h, ids = _coupled(backend, n_steps=2)
        if call:
            u = dfc.smooth_displacement(pts, 0.05)
            origin, spacing, size = _box_grid(pts, u)
            s = h.sampler_grid(origin, spacing, size, deformed_by=ids[0])
            h.sampler_points(pts[:50] + 0.01, deformed_by='current')
            h.sampler_grid(origin, spacing, size, deformed_by=u, scale=0.5)
            s.warp(np.random.default_rng(1).standard_normal((4, 5, 6)), origin, np.asarray(spacing) * 2.0)
            s.back_map()
        s0 = h.stats()
        assert h.step(2) == backend.GLIMS_OK
        s1 = h.stats()
        runs.append((h.get_state(want_u=False)[0],
                     {k: s1[k] - s0[k] for k in ("steps", "newton_its", "cg_its", "cheb_solves", "cheb_its")}))
        h.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1], runs


# ---- 6. warp --------------------------------------------------------------------------------------------------------------------
def _source_image(pts, size, k, seed):
    """A source grid that differs from the target grid and covers only a part of the mesh."""
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    o = lo + 0.13 * (hi - lo)
    sp = 0.61 * (hi - lo) / (np.array(size) - 1)
    rng = np.random.default_rng(seed)
    shape = tuple(reversed(size)) + ((k,) if k > 1 else ())
    return rng.standard_normal(shape), o, sp


@pytest.mark.parametrize("name", ["delaunay", "brain"])
def test_warp_against_resample(backend, name):
    pts, cells, u, origin, spacing, size, x = _case(name)
    d = pts.shape[1]
    cell, w, margin, _ = _ref(name, 1.0)
    sc.assert_decisive(margin)
    found = cell >= 0
    X = dfc.back_map(pts, cells, cell, w)
    h = _bare(backend, pts, cells)
    s = h.sampler_grid(origin, spacing, size, deformed_by=u)
    assert np.array_equal(s.cells, cell)
    src_size = (11, 8) if d == 2 else (7, 6, 5)
    for k in (1, 3):
        img, o, sp = _source_image(pts, src_size, k, seed=20 + k)
        for order, oname in ((1, 'linear'), (0, 'nearest')):
            want, rm = dfc.resample(img, o, sp, X, order, fill=-9.0)
            dfc.assert_resample_decisive(rm)
            got = s.warp(img, o, sp, order=oname, fill=-9.0)
            assert got.shape == want.shape
            filled = (want == -9.0).reshape(len(x), -1).all(axis=1)
            # `fill` appears outside the mesh AND inside the mesh but outside the source
            assert (~found).sum() > 10 and (found & filled).sum() > 10 and (~filled).sum() > 50
            assert np.array_equal((got == -9.0).reshape(len(x), -1).all(axis=1), filled)
            if order == 0:
                assert np.array_equal(got, want)
            else:
                err = np.abs(got - want).max() / np.abs(img).max()
                print(name, k, "linear: %.3e" % err)
                assert err <= 1e-10
            assert np.array_equal(got, s.warp(img, o, sp, order=oname, fill=-9.0))       # the same bits on every call
            gn = s.warp(img, o, sp, order=oname)                                           # default fill: NaN
            assert np.array_equal(np.isnan(gn).reshape(len(x), -1).all(axis=1), filled)
    # an affine image is reproduced
    g = sc.grid_points(o, sp, src_size)
    aff = _affine(g, k=2, seed=4).reshape(tuple(reversed(src_size)) + (2,))
    want, rm = dfc.resample(aff, o, sp, X, 1)
    ins = ~np.isnan(want).any(axis=1)
    got = s.warp(aff, o, sp)
    err = np.abs(got[ins] - _affine(X[ins], k=2, seed=4)).max() / np.abs(aff).max()
    print(name, "affine image: %.3e" % err)
    assert err <= 1e-12 and np.array_equal(np.isnan(got), np.isnan(want))
    # one NaN voxel propagates exactly where the reference says
    img, o, sp = _source_image(pts, src_size, 1, seed=31)
    img[tuple(n // 2 for n in img.shape)] = np.nan
    for order, oname in ((1, 'linear'), (0, 'nearest')):
        want, rm = dfc.resample(img, o, sp, X, order, fill=-9.0)
        got = s.warp(img, o, sp, order=oname, fill=-9.0)
        assert np.isnan(want).sum() > 0 and np.array_equal(np.isnan(got), np.isnan(want))
    # the point-set sampler of the same points warps the same image, and an undeformed sampler resamples at the points themselves
    img, o, sp = _source_image(pts, src_size, 3, seed=23)
    gp, gg = h.sampler_points(x, deformed_by=u).warp(img, o, sp), s.warp(img, o, sp)
    assert np.array_equal(np.isnan(gp), np.isnan(gg))
    assert np.abs(gp - gg)[~np.isnan(gg)].max() <= 1e-10 * np.abs(img).max()
    s0 = h.sampler_grid(origin, spacing, size)
    c0, w0, m0, _ = _ref(name, 0.0)
    sc.assert_decisive(m0)
    want, rm = dfc.resample(img, o, sp, dfc.back_map(pts, cells, c0, w0), 1)
    dfc.assert_resample_decisive(rm)
    got = s0.warp(img, o, sp)
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok) and np.abs(got[ok] - want[ok]).max() <= 1e-10 * np.abs(img).max()
    h.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_by_code_and_reason(backend):
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    mesh, lab = _box()
    pts, cells = mesh.points, mesh.cells
    n = len(pts)
    u = dfc.smooth_displacement(pts, 0.03)
    grid = ((0., 0., 0.), (0.25, 0.25, 0.25), (5, 4, 4))

    def refused(fn, *needles):
        with pytest.raises(backend.BackendError) as ei:
            fn()
        assert ei.value.code == backend.GLIMS_E_USAGE, ei.value
        for nd in needles:
            assert nd in str(ei.value), str(ei.value)

    # a handle set up without mechanics: host sources work, device sources do not
    h = backend.Handle(pts, cells, lab)
    h.set_materials(*[dc.TABLES[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=1.0)
    h.setup(False)
    refused(lambda: h.sampler_grid(*grid, deformed_by='current'), "with_mechanics")
    h.set_state(np.full(n, 0.1))
    sid = h.snapshot_save()
    refused(lambda: h.sampler_grid(*grid, deformed_by=sid), "with_mechanics")
    refused(lambda: h.sampler_points(pts, deformed_by='current'), "with_mechanics")
    n_before = len(h.sampler_grid(*grid, deformed_by=u).cells)
    assert n_before == 80
    h.close()

    h, ids = _coupled(backend, n_steps=1)
    refused(lambda: h.sampler_grid(*grid, deformed_by=77), "unknown snapshot")
    refused(lambda: h.sampler_points(pts, deformed_by=77), "unknown snapshot")
    refused(lambda: h.sampler_grid(*grid, deformed_by=u, scale=np.nan), "scale")
    refused(lambda: h.sampler_points(pts, deformed_by=u, scale=np.inf), "scale")
    refused(lambda: h.sampler_grid((0, 0, 0), (0.1, 0.1, 0.1), (4, 0, 4), deformed_by=u), "size", "not positive")
    refused(lambda: h.sampler_grid((0, 0, 0), (0.1, -0.1, 0.1), (4, 4, 4), deformed_by=u), "spacing", "not positive")
    m0 = h.stats()["mech_solves"]
    refused(lambda: h.sampler_grid((0, 0, 0), (0.1, 0.1, 0.1), (4, 0, 4), deformed_by=ids[0]), "size")     # before any solve
    assert h.stats()["mech_solves"] == m0
    sidc = C.c_int64(-1)
    o, sp, sz = (np.array(v, dtype=t) for v, t in zip(grid, (np.float64, np.float64, np.int64)))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    uf = np.ascontiguousarray(u.reshape(-1))
    err = lambda: h.lib.glims_last_error(h._h)
    st = h.lib.glims_sampler_create_grid_deformed(h._h, o.ctypes.data_as(dp), sp.ctypes.data_as(dp), sz.ctypes.data_as(ip),
                                                  backend.DERIVE_HOST, None, 1.0, 0, C.byref(sidc))
    assert st == backend.GLIMS_E_USAGE and b"u_host" in err()
    st = h.lib.glims_sampler_create_points_deformed(h._h, n, pts.ctypes.data_as(dp), backend.DERIVE_HOST, None, 1.0, 0,
                                                    C.byref(sidc))
    assert st == backend.GLIMS_E_USAGE and b"u_host" in err()
    st = h.lib.glims_sampler_create_grid_deformed(h._h, o.ctypes.data_as(dp), sp.ctypes.data_as(dp), sz.ctypes.data_as(ip),
                                                  backend.DERIVE_HOST, uf.ctypes.data_as(dp), 1.0, 1, C.byref(sidc))
    assert st == backend.GLIMS_E_USAGE and b"flags" in err()
    st = h.lib.glims_sampler_create_points_deformed(h._h, n, pts.ctypes.data_as(dp), backend.DERIVE_HOST, uf.ctypes.data_as(dp),
                                                    1.0, 2, C.byref(sidc))
    assert st == backend.GLIMS_E_USAGE and b"flags" in err()
    st = h.lib.glims_sampler_create_points_deformed(h._h, -1, pts.ctypes.data_as(dp), backend.DERIVE_HOST, uf.ctypes.data_as(dp),
                                                    1.0, 0, C.byref(sidc))
    assert st == backend.GLIMS_E_USAGE and sidc.value == -1
    st = h.lib.glims_sampler_deformation_info(h._h, 55, None, None)
    assert st == backend.GLIMS_E_USAGE and b"unknown sampler id" in err()
    # warp
    s = h.sampler_grid(*grid, deformed_by=u)
    img = np.zeros((3, 3, 3))
    out = np.zeros((s.n_points, 9))
    a3 = lambda v, t: np.array(v, dtype=t)

    def warp(image=img, size=(3, 3, 3), spacing=(1., 1., 1.), ncomp=1, order=1):
        szz, spp, og = a3(size, np.int64), a3(spacing, np.float64), a3((0, 0, 0), np.float64)
        return h.lib.glims_sampler_warp(h._h, s.id, None if image is None else image.ctypes.data_as(dp), og.ctypes.data_as(dp),
                                        spp.ctypes.data_as(dp), szz.ctypes.data_as(ip), ncomp, order, 0.0,
                                        out.ctypes.data_as(dp))

    assert warp() == backend.GLIMS_OK
    for kw, needle in ((dict(order=2), b"order"), (dict(order=-1), b"order"), (dict(ncomp=0), b"ncomp"),
                       (dict(ncomp=9), b"ncomp"), (dict(image=None), b"null image"), (dict(size=(3, 0, 3)), b"size"),
                       (dict(size=(3, 3, -1)), b"size"), (dict(spacing=(1., 0., 1.)), b"spacing"),
                       (dict(spacing=(1., 1., np.nan)), b"spacing")):
        assert warp(**kw) == backend.GLIMS_E_USAGE and needle in err(), kw
    st = h.lib.glims_sampler_apply(h._h, s.id, backend.FIELD_XYZ, -1, None, 1, 0.0, out.ctypes.data_as(dp))
    assert st == backend.GLIMS_E_USAGE and b"GLIMS_FIELD_XYZ" in err() and b"dim components" in err()
    # image terms refuse a deformed sampler, accept the undeformed one of the same grid
    tgt = np.zeros(s.n_points)
    refused(lambda: h.set_image_terms([dict(step=1, kind='img_l2', sampler=s, target=tgt)]), "deformed", "location")
    s_und = h.sampler_grid(*grid)
    h.set_image_terms([dict(step=1, kind='img_l2', sampler=s_und, target=tgt)])
    assert h.image_term_info(0)[:2] == (s_und.id, s_und.n_points)
    h.set_image_terms([])
    # the handle still works afterwards
    s3 = h.sampler_grid(*grid, deformed_by=ids[0])
    assert s3.deformed and s3.n_found > 0 and h.step(1) == backend.GLIMS_OK
    h.close()

    # CURRENT before glims_set_state
    h = backend.Handle(pts, cells, lab)
    h.set_materials(*[dc.TABLES[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=1.0)
    h.setup(True)
    refused(lambda: h.sampler_grid(*grid, deformed_by='current'), "glims_set_state")
    h.close()

    # a partitioned handle
    def body(rank, tr):
        part = partition_mesh(pts, cells, 2, rank)
        hp = backend.Handle(part.points, part.cells, lab[part.cell_ids], n_own=part.n_own, device=0)
        hp.set_transport(rank, 2, tr.halo_cb, tr.allreduce_cb)
        hp.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        msgs = []
        for fn in (lambda: hp.sampler_grid(*grid, deformed_by=u[part.global_ids]),
                   lambda: hp.sampler_points(pts, deformed_by=u[part.global_ids]),
                   lambda: hp.sampler_grid(*grid).warp(img, (0, 0, 0), (1, 1, 1))):
            try:
                fn()
                msgs.append((0, "accepted"))
            except backend.BackendError as e:
                msgs.append((e.code, str(e)))
        hp.close()
        return msgs

    for msgs in run_threaded_ranks(2, body):
        for code, text in msgs:
            assert code == backend.GLIMS_E_USAGE and "partitioned" in text, (code, text)


# ---- 8. public API --------------------------------------------------------------------------------------------------------------
class _Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def _sim(on_device):
    from glimslib_amd.simulation import TumorGrowth
    mesh = fenics.RectangleMesh((0, 0), (2, 2), 20, 20)
    sim = TumorGrowth(mesh, solver_options={'mech_rtol': 1e-12})
    zero = fenics.Constant(np.zeros(2))
    lab = np.where(mesh.cell_midpoints()[:, 0] < 1.0, 1, 2).astype(np.int32)
    sim.setup_global_parameters(boundaries={'boundary_all': _Boundary()},
                                dirichlet_bcs={'clamp': {'bc_value': zero, 'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                subdomains=lab, domain_names={1: 'A', 2: 'B'})
    iv = fenics.Expression('0.9*exp(-6*(pow(x[0]-0.9,2)+pow(x[1]-1.1,2)))', degree=1)
    sim.setup_model_parameters(iv_expression={0: zero, 1: iv}, sim_time=3, sim_time_step=1,
                               diffusion={'A': 0.02, 'B': 0.04}, coupling={'A': 0.5, 'B': 0.4},
                               proliferation={'A': 0.3, 'B': 0.2}, E={'A': 1.0, 'B': 2.0}, poisson={'A': 0.3, 'B': 0.4})
    sim.run(save_method=None, plot=False, results_on_device=on_device)
    return sim, lab


def _like(sim):
    from glimslib_amd.utils.data_io import Image
    pts = sim.mesh.points
    size = (31, 27)
    origin, spacing = sc.overhanging_grid(pts, size, overhang=0.04)
    return Image(np.zeros(tuple(reversed(size))), origin, spacing)


def test_public_api_deformed_images(backend, tmp_path):
    from glimslib_amd.utils.data_io import Image
    sim, lab = _sim(True)
    pts, cells = sim.mesh.points, sim.mesh.cells
    like = _like(sim)
    size = like.GetSize()
    shape = tuple(reversed(size))
    x = sc.grid_points(like.GetOrigin(), like.GetSpacing(), size)
    steps = sim.results.get_recording_steps()
    a, b = steps[-1], steps[-2]
    images = {}
    old = None
    for step in (b, a):                                                  # (a last: its sampler stays cached for what follows)
        field = sim.results.get_result(step).get_field()
        u = np.asarray(field.components[0]).copy()                       # the step's host displacement (solved here)
        c = np.asarray(field.components[1])
        assert np.abs(u).max() > 0.005
        cell, w, margin, _ = sc.locate(dfc.deformed_points(pts, u), cells, x)
        sc.assert_decisive(margin)
        found = cell >= 0
        img = sim.sample_image('concentration', step, like, deformed=True)
        ref = sc.apply(cells, cell, w, c).reshape(shape)
        assert img.array.shape == shape and np.array_equal(np.isnan(img.array), np.isnan(ref)) and np.isnan(ref).any()
        err = np.abs(img.array - ref)[~np.isnan(ref)].max() / np.abs(c).max()
        print(step, "concentration: %.3e" % err)
        assert err <= 1e-10
        und = sim.sample_image('concentration', step, like)
        both = ~np.isnan(und.array) & ~np.isnan(img.array)
        assert np.abs(und.array - img.array)[both].max() > 1e-3 * np.abs(c).max()
        # one deformed sampler per grid: the step asked for last; the one before it is closed
        ent = [v for k, v in sim._deformed_samplers[2].items() if k[2] == tuple(size)]
        assert len(ent) == 1 and ent[0][0] == step and ent[0][1].deformed
        assert old is None or (old.id is None and old is not ent[0][1])
        old = ent[0][1]
        pp = sim.init_postprocess(str(tmp_path / "pp"))
        nodal = pp.get_concentration_deformed_configuration(step).values()
        img2 = sim.sample_image('concentration_deformed_config', step, like, deformed=True)
        ref2 = sc.apply(cells, cell, w, nodal).reshape(shape)
        assert np.array_equal(np.isnan(img2.array), np.isnan(ref2))
        err = np.abs(img2.array - ref2)[~np.isnan(ref2)].max() / np.abs(nodal).max()
        print(step, "concentration_deformed_config: %.3e" % err)
        assert err <= 1e-10
        und2 = sim.sample_image('concentration_deformed_config', step, like)
        both = ~np.isnan(und2.array) & ~np.isnan(img2.array)
        assert np.abs(und2.array - img2.array)[both].max() > 1e-3 * np.abs(nodal).max()
        dimg = sim.sample_image('displacement', step, like, deformed=True)
        refu = sc.apply(cells, cell, w, u).reshape(shape + (2,))
        assert dimg.is_vector and np.abs(dimg.array - refu)[~np.isnan(refu)].max() <= 1e-10 * np.abs(u).max()
        # labels
        lim = sim.label_image(step, like=like, deformed=True)
        assert lim.array.dtype == np.int32
        assert np.array_equal(lim.array.reshape(-1), np.where(found, lab[np.maximum(cell, 0)], 0))
        c0, w0, m0, _ = sc.locate(pts, cells, x)
        sc.assert_decisive(m0)
        l0 = sim.label_image(like=like, fill=-1)
        assert np.array_equal(l0.array.reshape(-1), np.where(c0 >= 0, lab[np.maximum(c0, 0)], -1))
        assert np.array_equal(sim.label_image(step, like=like).array, sim.label_image(like=like).array)
        # warp: the reference image through the back map
        src = Image(np.random.default_rng(int(step)).standard_normal((14, 17)), (0.3, 0.2), (0.09, 0.11))
        X = dfc.back_map(pts, cells, cell, w)
        for order, oi in (('linear', 1), ('nearest', 0)):
            want, rm = dfc.resample(src.array, src.origin, src.spacing, X, oi)
            dfc.assert_resample_decisive(rm)
            got = sim.warp_image(src, step, like=like, order=order)
            assert got.array.shape == shape and got.origin == like.origin and got.spacing == like.spacing
            ok = ~np.isnan(want)
            assert ok.sum() > 50 and np.array_equal(np.isnan(got.array.reshape(-1)), ~ok)
            assert np.abs(got.array.reshape(-1)[ok] - want[ok]).max() <= 1e-10 * np.abs(src.array).max()
        own = sim.warp_image(src, step)                                   # default grid: the image's own
        assert own.array.shape == src.array.shape and own.origin == src.origin
        images[step] = (img.array, img2.array)
    assert not np.array_equal(images[a][0], images[b][0], equal_nan=True)         # each step its own image
    # create_deformed_images, with files
    step = a
    field = sim.results.get_result(step).get_field()
    u = np.asarray(field.components[0])
    cell, w, margin, _ = sc.locate(dfc.deformed_points(pts, u), cells, x)
    found = cell >= 0
    ref_img = Image(np.random.default_rng(77).standard_normal(shape), like.origin, like.spacing)
    out = sim.create_deformed_images(step, ref_img, output_dir=str(tmp_path / "deformed"))
    assert sorted(out) == ['displacement_img', 'displacement_img_inv', 'image_warped', 'label_img_orig', 'labels_warped']
    assert np.array_equal(out['labels_warped'].array.reshape(-1), np.where(found, lab[np.maximum(cell, 0)], 0))
    assert np.array_equal(out['label_img_orig'].array, sim.label_image(like=like).array)
    assert np.array_equal(out['displacement_img'].array, sim.sample_image('displacement', step, like).array, equal_nan=True)
    X = dfc.back_map(pts, cells, cell, w)
    inv = out['displacement_img_inv']
    assert inv.is_vector and inv.array.shape == shape + (2,)
    assert np.abs(inv.array.reshape(-1, 2)[found] - (X - x)[found]).max() <= 1e-10 * np.abs(pts).max()
    assert np.isnan(inv.array.reshape(-1, 2)[~found]).all()
    # X(x) + u_h(X(x)) = x: the inverse of the P1 map, not its first-order approximation -u
    ux = sc.apply(cells, cell, w, u)
    assert np.abs(inv.array.reshape(-1, 2)[found] + ux[found]).max() <= 1e-10
    want, rm = dfc.resample(ref_img.array, ref_img.origin, ref_img.spacing, X, 1)
    dfc.assert_resample_decisive(rm)
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(out['image_warped'].array.reshape(-1)), ~ok)
    assert np.abs(out['image_warped'].array.reshape(-1)[ok] - want[ok]).max() <= 1e-10 * np.abs(ref_img.array).max()
    for name, im in out.items():
        back = Image.read(os.path.join(str(tmp_path / "deformed"), name + ".mha"))
        assert np.array_equal(back.array, im.array, equal_nan=True) and back.array.dtype == im.array.dtype
        assert back.origin == im.origin and back.spacing == im.spacing and back.is_vector == im.is_vector
    dev = {k: v.array for k, v in out.items()}
    dev_c = sim.sample_image('concentration', step, like, deformed=True).array
    dev_d = sim.sample_image('concentration_deformed_config', step, like, deformed=True).array
    sim.close()

    # host-resident results give the same images
    sim, _ = _sim(False)
    out = sim.create_deformed_images(step, ref_img)
    for k in ('displacement_img', 'displacement_img_inv', 'image_warped'):
        p, q = out[k].array, dev[k]
        assert np.array_equal(np.isnan(p), np.isnan(q)), k
        assert np.abs(p - q)[~np.isnan(q)].max() <= 1e-8 * max(1.0, np.abs(q[~np.isnan(q)]).max()), k
    assert np.array_equal(out['labels_warped'].array, dev['labels_warped'])
    for kind, q in (('concentration', dev_c), ('concentration_deformed_config', dev_d)):
        p = sim.sample_image(kind, step, like, deformed=True).array
        assert np.array_equal(np.isnan(p), np.isnan(q)), kind
        assert np.abs(p - q)[~np.isnan(q)].max() <= 1e-8 * np.abs(q[~np.isnan(q)]).max(), kind
    sim.close()
