"""The numpy statement of the deformed-sampler contract (tests/deformed_common.py) checked against closed forms, and the parts of
the feature that need no GPU: the header's constant, the ctypes table, the refusals of the Python layer."""
import os
import re

import numpy as np
import pytest

import deformed_common as dfc
import sampler_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("glims_sampler_create_grid_deformed", "glims_sampler_create_points_deformed",
                "glims_sampler_deformation_info", "glims_sampler_warp")


def test_affine_displacement_locates_like_the_pulled_back_points():
    """u = A X + b: x lies in the deformed cell T iff F^-1 (x - b) lies in the reference cell T (F = I + A), with the same
    barycentric coordinates; the back map is F^-1 (x - b)."""
    pts, cells = sc.jittered_delaunay_2d(10, 6)
    A = np.array([[0.10, -0.07], [0.04, 0.15]])
    b = np.array([0.03, -0.02])
    u = pts @ A.T + b
    F = np.eye(2) + A
    size = (19, 13)
    origin, spacing = sc.overhanging_grid(dfc.deformed_points(pts, u), size)
    x = sc.grid_points(origin, spacing, size)
    Xp = np.linalg.solve(F, (x - b).T).T
    cell, w, margin, _ = dfc.locate(pts, cells, u, 1.0, x)
    cell0, w0, margin0, _ = sc.locate(pts, cells, Xp)
    sc.assert_decisive(margin)
    sc.assert_decisive(margin0)
    assert (cell >= 0).sum() > 100 and (cell < 0).sum() > 10
    assert np.array_equal(cell, cell0)
    assert np.abs(w - w0).max() <= 1e-12
    found = cell >= 0
    X = dfc.back_map(pts, cells, cell, w)
    assert np.abs(X[found] - Xp[found]).max() <= 1e-12
    assert np.isnan(X[~found]).all()
    r = dfc.cell_ratios(pts, cells, u)
    assert np.abs(r - np.linalg.det(F)).max() <= 1e-12
    # scale: -1 inverts the sign of u, 0 is the reference mesh itself
    assert np.array_equal(dfc.deformed_points(pts, u, 0.0), pts)
    assert np.array_equal(dfc.deformed_points(pts, u, -1.0), pts - u)


def test_smooth_displacement_is_the_formula():
    pts = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 1.0], [0.0, 1.0], [1.0, 0.5]])
    u = dfc.smooth_displacement(pts, 0.08)
    # node 4: t = (0.5, 0.5): u_x = 0.08 * 2 * sin(pi/2) cos(pi/4) + 0.06, u_y = 0.08 * 1 * sin(pi/2) cos(pi/4) + 0.03
    assert np.allclose(u[4], [0.16 * np.sqrt(0.5) + 0.06, 0.08 * np.sqrt(0.5) + 0.03], rtol=0, atol=1e-15)
    assert np.allclose(u[0], [0.06, 0.03], rtol=0, atol=1e-15)


def test_resample_linear_reproduces_an_affine_image():
    rng = np.random.default_rng(3)
    for d, size in ((2, (7, 5)), (3, (6, 4, 5))):
        origin, spacing = rng.standard_normal(d), 0.2 + rng.random(d)
        g = sc.grid_points(origin, spacing, size)
        coef, c0 = rng.standard_normal((d, 2)), rng.standard_normal(2)
        img = (g @ coef + c0).reshape(tuple(reversed(size)) + (2,))
        lo, hi = origin, origin + spacing * (np.array(size) - 1)
        X = lo + (hi - lo) * (0.001 + 0.998 * rng.random((200, d)))
        v, margin = dfc.resample(img, origin, spacing, X, 1)
        dfc.assert_resample_decisive(margin)
        assert np.abs(v - (X @ coef + c0)).max() <= 1e-12
        s, _ = dfc.resample(img[..., 0], origin, spacing, X, 1)
        assert s.shape == (200,) and np.array_equal(s, v[:, 0])


def test_resample_nearest_picks_the_voxel_named_by_hand():
    img = np.arange(12, dtype=np.float64).reshape(3, 4)           # [y, x]: 4 voxels along x, 3 along y
    origin, spacing = (10.0, -1.0), (2.0, 0.5)
    X = np.array([[10.0, -1.0],        # voxel (0, 0)
                  [12.9, -0.3],        # t = (1.45, 1.4) -> (1, 1): 1 * 4 + 1
                  [13.1, 0.2],         # t = (1.55, 2.4) -> (2, 2): 2 * 4 + 2
                  [16.9, 0.24],        # t = (3.45, 2.48) -> (3, 2): 11, the last voxel
                  [17.1, 0.0],         # t_x = 3.55 >= n - 0.5: outside
                  [9.1, 0.0],          # t_x = -0.45: inside, voxel 0 along x; t_y = 2 -> 8
                  [8.9, 0.0],          # t_x = -0.55: outside
                  [np.nan, 0.0]])      # not found
    v, margin = dfc.resample(img, origin, spacing, X, 0, fill=-7.0)
    dfc.assert_resample_decisive(margin)
    assert v.tolist() == [0.0, 5.0, 10.0, 11.0, -7.0, 8.0, -7.0, -7.0]
    assert margin[-1] == np.inf


def test_resample_inside_rule_on_both_edges():
    img = np.arange(6, dtype=np.float64).reshape(2, 3)
    origin, spacing = (0.0, 0.0), (1.0, 1.0)
    eps = 1e-6
    X = np.array([[0.0 + eps, 0.5], [2.0 - eps, 0.5], [0.0 - eps, 0.5], [2.0 + eps, 0.5], [1.0, 1.0 + eps], [1.0, 0.0 - eps],
                  [0.0, 0.0], [2.0, 1.0]])
    v, margin = dfc.resample(img, origin, spacing, X, 1)
    assert np.isfinite(v[:2]).all() and np.isnan(v[2:6]).all()
    assert abs(margin[:6].max() - eps) <= 1e-12 and (margin[6:] == 0).all()
    assert v[6] == 0.0 and v[7] == 5.0                            # exactly on the first and the last voxel centre: inside
    assert abs(v[0] - (0.5 * (0 + 3) + eps)) <= 1e-12
    # order 0: [-0.5, n - 0.5)
    X = np.array([[-0.5 + eps, 0.0], [2.5 - eps, 0.0], [-0.5 - eps, 0.0], [2.5 + eps, 0.0]])
    v, margin = dfc.resample(img, origin, spacing, X, 0)
    assert v[:2].tolist() == [0.0, 2.0] and np.isnan(v[2:]).all()
    assert abs(margin.max() - eps) <= 1e-9
    # a source of one voxel along an axis: order 1 is inside only on that voxel's centre, f = 0
    one = np.array([[1.0, 2.0, 4.0]])                             # [y = 1, x = 3]
    v, _ = dfc.resample(one, origin, spacing, np.array([[0.5, 0.0], [0.5, 0.1]]), 1)
    assert v[0] == 1.5 and np.isnan(v[1])
    # a NaN voxel propagates through every stencil that holds it, and only those
    img = np.arange(12, dtype=np.float64).reshape(3, 4)
    img[1, 1] = np.nan
    X = np.array([[0.5, 0.5], [1.5, 1.5], [2.5, 0.5], [2.5, 1.5], [0.25, 1.75]])
    v, _ = dfc.resample(img, origin, spacing, X, 1)
    assert np.isnan(v).tolist() == [True, True, False, False, True]


def test_cell_ratios_on_a_two_triangle_fold():
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    cells = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    u = np.zeros((4, 2))
    u[3] = [-1.5, -1.5]                                            # node 3 pulled through the diagonal: the second cell folds
    r = dfc.cell_ratios(pts, cells, u)
    # cell 1 (area 1/2, edges (0, 1), (-1, 1)) -> vertices (1, 0), (-0.5, -0.5), (0, 1): edges (-1.5, -0.5), (-1, 1): det -2
    assert np.allclose(r, [1.0, -2.0], rtol=0, atol=1e-15)
    assert dfc.n_inverted(r) == 1
    assert np.allclose(dfc.cell_ratios(pts, cells, u, 0.5), [1.0, -0.5], rtol=0, atol=1e-15)
    u[3] = [-0.5, -0.5]                                            # onto the diagonal: flat
    r = dfc.cell_ratios(pts, cells, u)
    assert r[1] == 0.0 and dfc.n_inverted(r) == 1
    assert dfc.n_inverted(np.array([1.0, np.nan, np.inf, 0.5])) == 2
    # in the overlap of the fold the smallest cell index wins
    u[3] = [-1.5, -1.5]
    x = np.array([[0.2, 0.2]])
    cell, w, margin, n_acc = dfc.locate(pts, cells, u, 1.0, x)
    sc.assert_decisive(margin)
    assert n_acc[0] == 2 and cell[0] == 0


def test_header_and_ctypes_table_carry_the_new_surface():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    assert re.search(r"^#define GLIMS_FIELD_XYZ 5\b", src, re.M)
    assert _backend.FIELD_XYZ == 5
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _backend.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _backend.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.glims_abi_version() == _backend.ABI_VERSION


def _tiny_sim():
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.simulation import TumorGrowth
    mesh = fenics.RectangleMesh(fenics.Point(0, 0), fenics.Point(1, 1), 4, 4)
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters()
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: fenics.Constant(0.1)}, diffusion=0.1,
                               coupling=0.1, proliferation=0.1, E=1.0, poisson=0.3, sim_time=1, sim_time_step=1)
    return sim


GRID = dict(origin=(0.0, 0.0), spacing=(0.25, 0.25), size=(5, 5))


def test_deformed_images_need_a_run_first():
    from glimslib_amd.utils.data_io import Image
    sim = _tiny_sim()
    with pytest.raises(RuntimeError, match="run"):
        sim.sample_image('concentration', 1, deformed=True, **GRID)
    with pytest.raises(RuntimeError, match="run"):
        sim.label_image(1, deformed=True, **GRID)
    with pytest.raises(RuntimeError, match="run"):
        sim.warp_image(Image(np.zeros((5, 5)), GRID['origin'], GRID['spacing']), 1)


def test_partitioned_runs_refuse_deformed_images():
    from glimslib_amd.parallel import DistributedHandle
    from glimslib_amd.utils.data_io import Image
    dh = object.__new__(DistributedHandle)                         # (no process group here: the refusal comes first)
    with pytest.raises(NotImplementedError, match="partitioned"):
        dh.sampler_grid(GRID['origin'], GRID['spacing'], GRID['size'], deformed_by='current')
    with pytest.raises(NotImplementedError, match="partitioned"):
        dh.sampler_points(np.zeros((1, 2)), deformed_by=0)
    sim = _tiny_sim()
    sim._backend = dh
    img = Image(np.zeros((5, 5)), GRID['origin'], GRID['spacing'])
    try:
        with pytest.raises(NotImplementedError, match="partitioned"):
            sim.sample_image('concentration', 1, deformed=True, **GRID)
        with pytest.raises(NotImplementedError, match="partitioned"):
            sim.warp_image(img, 1)
        with pytest.raises(NotImplementedError, match="partitioned"):
            sim.create_deformed_images(1, img)
    finally:
        sim._backend = None
