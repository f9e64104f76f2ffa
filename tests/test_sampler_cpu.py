"""Samplers without a GPU: the C-ABI surface is there, and the numpy reference of the sampler tests (tests/sampler_common.py)
checks itself -- partition of unity, affine fields, adjointness of its P and P^T, agreement with the host evaluation
fenics_local.Function.__call__, and the decision margins / condition numbers the GPU tests rely on."""
import os
import re

import numpy as np

import sampler_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLER_SYMBOLS = ("glims_sampler_create_points", "glims_sampler_create_grid", "glims_sampler_info", "glims_sampler_get",
                   "glims_sampler_apply", "glims_sampler_apply_t", "glims_sampler_destroy")


def test_header_library_and_binding_carry_the_sampler_entry_points():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(glims_[a-z_0-9]+)\s*\(", code))
    lib = _backend.load_library()
    for name in SAMPLER_SYMBOLS:
        assert name in declared, "%s is not declared in glims_hip.h" % name
        assert hasattr(lib, name), "libglimship.so does not export %s" % name
        assert name in _backend.SIGNATURES
    assert re.search(r"#define\s+GLIMS_SAMPLE_EPS\s+1e-10\b", code)
    assert _backend.SAMPLE_EPS == sc.EPS == 1e-10
    assert lib.glims_abi_version() == 6
    for k, name in enumerate(("GLIMS_FIELD_C", "GLIMS_FIELD_U", "GLIMS_FIELD_SNAPSHOT_C", "GLIMS_FIELD_HOST")):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, k), code)
    assert (_backend.FIELD_C, _backend.FIELD_U, _backend.FIELD_SNAPSHOT_C, _backend.FIELD_HOST) == (0, 1, 2, 3)


def _affine(x, dyadic=False, seed=0):
    """An affine 3-component field; dyadic: small integer coefficients, so that its values at dyadic points and the
    interpolation sums with weights 0, 1/2, 1 carry no rounding at all."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-4, 5, (x.shape[1], 3)).astype(np.float64) if dyadic else rng.standard_normal((x.shape[1], 3))
    b = rng.integers(-4, 5, 3).astype(np.float64) if dyadic else rng.standard_normal(3)
    return sum(x[:, a:a + 1] * A[a][None, :] for a in range(x.shape[1])) + b


def _self_check(points, cells, x, exact):
    cell, w, margin, n_acc = sc.locate(points, cells, x)
    found = cell >= 0
    assert found.any()
    assert (w[~found] == 0).all()
    # partition of unity, and weights no further below zero than the acceptance rule lets them
    assert np.abs(w[found].sum(axis=1) - 1.0).max() <= 1e-13
    assert w[found].min() >= -sc.EPS
    f = _affine(points, exact)
    got = sc.apply(cells, cell, w, f)
    want = _affine(x, exact)
    err = np.abs(got[found] - want[found]).max() / np.abs(want).max()
    assert err <= (0.0 if exact else 1e-13), err
    assert np.isnan(got[~found]).all()
    assert (sc.apply(cells, cell, w, f[:, 0], fill=-7.0)[~found] == -7.0).all()
    # <P f, r> = <f, P^T r>
    rng = np.random.default_rng(1)
    fr = rng.standard_normal((len(points), 2))
    r = rng.standard_normal((len(x), 2))
    lhs = (sc.apply(cells, cell, w, fr, fill=0.0) * r).sum()
    rhs = (fr * sc.apply_t(cells, cell, w, r, len(points))).sum()
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), np.abs(fr).max() * np.abs(r).sum())
    return cell, w, margin, n_acc


def test_reference_on_the_jittered_delaunay_rectangle():
    pts, cells = sc.jittered_delaunay_2d(24, 12)
    k = sc.assert_mesh_ok(pts, cells)
    origin, spacing = sc.overhanging_grid(pts, (37, 29))
    x = sc.grid_points(origin, spacing, (37, 29))
    cell, w, margin, n_acc = _self_check(pts, cells, x, exact=False)
    m = sc.assert_decisive(margin)
    print("2-D Delaunay: %d cells, kappa <= %.3g, %d inside, %d outside, smallest margin %.3g, most accepting cells %d"
          % (len(cells), k.max(), (cell >= 0).sum(), (cell < 0).sum(), m, n_acc.max()))
    assert (cell < 0).any()


def test_reference_on_the_small_brain_like_mesh():
    from glimslib_amd import workloads
    wl = workloads.config_brain_like(5000, workers=1)
    pts, cells = wl.mesh.points, wl.mesh.cells
    k = sc.assert_mesh_ok(pts, cells)
    size = (23, 19, 17)
    origin, spacing = sc.overhanging_grid(pts, size)
    x = sc.grid_points(origin, spacing, size)
    cell, w, margin, n_acc = _self_check(pts, cells, x, exact=False)
    m = sc.assert_decisive(margin)
    print("brain-like 5000: %d nodes, %d cells, kappa <= %.3g (median %.3g), %d inside, %d outside, smallest margin %.3g, "
          "most accepting cells %d" % (len(pts), len(cells), k.max(), np.median(k), (cell >= 0).sum(), (cell < 0).sum(), m,
                                       n_acc.max()))
    assert (cell < 0).sum() > 100 and (cell >= 0).sum() > 1000
    assert n_acc.max() == 1                                  # no point has two accepting cells


def test_reference_is_exact_on_power_of_two_lattices():
    from glimslib_amd.mesh import BoxMesh, RectangleMesh
    for mesh, lo, hi, n, most in ((BoxMesh((0., 0., 0.), (2., 1., 1.), 8, 2, 4), (0, 0, 0), (2, 1, 1), (8, 2, 4), 24),
                                  (RectangleMesh((-1., -1.), (1., 1.), 8, 4), (-1, -1), (1, 1), (8, 4), 6)):
        pts, cells = mesh.points, mesh.cells
        sc.assert_mesh_ok(pts, cells)
        origin, spacing, size = sc.half_spacing_grid(lo, hi, n)
        x = sc.grid_points(origin, spacing, size)
        cell, w, margin, n_acc = _self_check(pts, cells, x, exact=True)
        assert (cell >= 0).all()
        assert np.isin(w, (0.0, 0.5, 1.0)).all()             # every lambda of a winner exactly 0, 1/2 or 1
        assert margin.min() == sc.EPS                        # ties: lambda = 0 exactly, no rounding involved
        assert n_acc.max() == most, n_acc.max()
        # the nodes as query points: the nodal values come back bitwise
        cn, wn, _, _ = sc.locate(pts, cells, pts)
        f = np.random.default_rng(3).standard_normal(len(pts))
        assert (sc.apply(cells, cn, wn, f) == f).all()


def test_reference_agrees_with_the_host_evaluation_of_functions():
    from glimslib_amd import fenics_local as fenics
    mesh = fenics.RectangleMesh(fenics.Point(0, 0), fenics.Point(2, 1), 7, 5)
    vals = np.random.default_rng(5).standard_normal(mesh.num_vertices())
    fn = fenics.Function(mesh, {None: vals})
    x = np.random.default_rng(6).random((200, 2)) * np.array([2.0, 1.0])
    cell, w, margin, _ = sc.locate(mesh.points, mesh.cells, x)
    assert (cell >= 0).all()
    got = sc.apply(mesh.cells, cell, w, vals)
    assert np.abs(got - np.asarray(fn(x))).max() <= 1e-13 * np.abs(vals).max()


def test_grid_points_are_x_fastest():
    x = sc.grid_points((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), (3, 2, 2))
    assert x.shape == (12, 3)
    assert (x[1] == (1.5, 2.0, 3.0)).all() and (x[3] == (1.0, 2.25, 3.0)).all() and (x[6] == (1.0, 2.0, 5.0)).all()
