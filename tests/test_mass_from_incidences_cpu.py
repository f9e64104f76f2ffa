"""
The identity behind the mass product that the assembly sweep forms from its incidence loop (kernels.hip, rd_assemble_s_slice
with MB = 1), stated in numpy against the oracle's consistent mass matrix.

The sweep holds, for every (row i, cell T) incidence, the reaction weight w_T = rho_T |T| d!/(d+3)!, the cell's sum
s_T = sum_{k in T} c_k and the row's own value c_i.  The consistent P1 mass row is (M c)_i = sum_{T ni i} m_T (s_T + c_i) with
m_T = |T| d!/(d+2)! = w_T (d+3) / rho_T, so for a row whose cells all carry one rho > 0:  (M c)_i = q_i sum_T w_T (s_T + c_i),
q_i = (d+3) / rho.  Rows with cells of different rho, or touching a tissue with rho = 0, are fallback rows (q_i = 0: they keep
the mass SpMV); the classification compares rho VALUES, so an interface between two labels of equal rho is no fallback.

Reference counterpart: 'u_previous1 * v1 * dx' (simulation_tumor_growth.py:117), the mass term of the time-discrete form.
"""
import math

import numpy as np
import pytest

from oracle.glims_oracle import assemble_mass, box_mesh, p1_geometry, rectangle_mesh

RHO = np.array([0.05, 0.05, 0.0])      # labels 0 and 1 share rho; label 2 is inert (CSF-like)


def _meshes():
    p2, c2 = rectangle_mesh((0.0, 0.0), (5.0, 4.0), 5, 5)
    p3, c3 = box_mesh((0.0, 0.0, 0.0), (4.0, 3.0, 2.0), 4, 4, 4)
    return {"2-D 5x5": (p2, c2), "3-D 4x4x4": (p3, c3)}


def _labels(points, cells):
    """Three labels in slabs along x: 0 | 1 | 2 (an equal-rho interface and an interface with rho = 0)."""
    mid = points[cells].mean(axis=1)[:, 0]
    lo, hi = points[:, 0].min(), points[:, 0].max()
    t = (mid - lo) / (hi - lo)
    return np.where(t < 0.35, 0, np.where(t < 0.7, 1, 2))


def _mass_from_incidences(points, cells, rho_cell, c):
    """(q, macc): per row the factor (d+3)/rho or 0 (fallback), and sum_T w_T (s_T + c_i) in cell order -- as the device does."""
    d = points.shape[1]
    vol, _ = p1_geometry(points, cells)
    w = rho_cell * vol * (math.factorial(d) / math.factorial(d + 3))
    n = len(points)
    macc = np.zeros(n)
    first = np.full(n, np.nan)
    uniform = np.ones(n, dtype=bool)
    for e, cell in enumerate(cells):
        st = c[cell].sum()
        for i in cell:
            macc[i] += w[e] * (st + c[i])
            if np.isnan(first[i]):
                first[i] = rho_cell[e]
            elif first[i].tobytes() != np.float64(rho_cell[e]).tobytes():      # bitwise, as k_corner_weights compares
                uniform[i] = False
    ok = uniform & np.isfinite(first) & (first > 0.0)
    q = np.where(ok, (d + 3) / np.where(ok, first, 1.0), 0.0)
    return q, macc


@pytest.mark.parametrize("name", list(_meshes()))
def test_rows_of_uniform_positive_rho_equal_the_mass_row(name):
    """q sum_T w_T (s_T + c_i) = (M c)_i to 128 eps (|M| |c|)_i: both sides are sums of a few dozen terms (up to 24 cells x 4 vertices)
    with a handful of roundings each."""
    points, cells = _meshes()[name]
    rho_cell = RHO[_labels(points, cells)]
    M = assemble_mass(points, cells)
    rng = np.random.default_rng(7)
    c = rng.standard_normal(len(points))
    assert (c < 0).any() and (c > 0).any()
    q, macc = _mass_from_incidences(points, cells, rho_cell, c)
    rows = q != 0.0
    assert rows.any()
    ref = M @ c
    bound = 128.0 * np.finfo(float).eps * (abs(M) @ np.abs(c))
    err = np.abs(q * macc - ref)
    print("%s: %d of %d rows, largest error / bound %.3f" % (name, rows.sum(), len(points), (err[rows] / bound[rows]).max()))
    assert np.all(err[rows] <= bound[rows])


@pytest.mark.parametrize("name", list(_meshes()))
def test_fallback_rows_are_exactly_those_touching_the_inert_label(name):
    points, cells = _meshes()[name]
    lab = _labels(points, cells)
    assert set(lab) == {0, 1, 2}
    q, _ = _mass_from_incidences(points, cells, RHO[lab], np.ones(len(points)))
    touches_inert = np.zeros(len(points), dtype=bool)
    touches_inert[np.unique(cells[lab == 2])] = True
    in0, in1 = np.zeros(len(points), dtype=bool), np.zeros(len(points), dtype=bool)
    in0[np.unique(cells[lab == 0])] = True
    in1[np.unique(cells[lab == 1])] = True
    at_equal_rho_interface = in0 & in1 & ~touches_inert
    assert at_equal_rho_interface.any() and touches_inert.any() and not touches_inert.all()
    assert np.array_equal(q == 0.0, touches_inert)
    assert np.all(q[at_equal_rho_interface] == (points.shape[1] + 3) / 0.05)
