"""
The reference, the error bound and the meshes of tests/test_gpu_quad_pass.py, checked without a GPU (tests/quad_pass_common.py):
the float64 reference is the formula the kernel claims to compute, a float32 emulation of the kernel lies inside the bound on
every mesh, and three defects the pass could have -- a record dropped, a wrong diagonal factor, a wrong slot -- lie outside it.
The last point is what shows that the bound bites: the GPU test would see each of them.

Reference counterpart: the logistic term 'rho * sol1 * (1 - sol1) * v1 * dx' (simulation_tumor_growth.py:118), whose second
derivative is the bilinear form N.
"""
import numpy as np
import pytest

from quad_pass_common import (CASES, FAN_K, U32, case, fan_mesh, inputs, pair_of, quad_abs, quad_bound, quad_direct,
                              quad_emulate, quad_ref, rho_of, row_lengths)

# unroll bound of the straight-line instance a row length reaches (longer rows: the looped kernels)
FAN_INSTANCE = {15: 16, 19: 20, 23: 24, 31: 32, 40: None}


@pytest.mark.parametrize("k", FAN_K)
def test_fan_mesh_row_lengths(k):
    mesh = fan_mesh(k)
    assert len(mesh.points) == 2 * k + 1 and len(mesh.cells) == 3 * k
    assert np.all(mesh.cell_volumes() > 0.0)
    rl = row_lengths(mesh.cells, len(mesh.points))
    assert rl[0] == k + 1 and rl[1:].max() == 6 and rl[1:].min() == 5
    inst = next((c for c in (16, 20, 24, 32) if rl.max() <= c), None)
    assert inst == FAN_INSTANCE[k]
    if inst is not None and inst > 16:
        assert rl.max() == inst           # the last unrolled slot of the instance is in use
    assert (2 * k + 1 > 64) == (k == 40)  # two slices only for the looped case


@pytest.mark.parametrize("cid", sorted(CASES))
def test_reference_is_the_kernels_formula_and_symmetric(cid):
    w = case(cid)
    p, c, rho = w.mesh.points, w.mesh.cells, rho_of(w)
    assert set(np.unique(w.cell_label)) == {1, 2, 3} and (rho == 0.0).any() and (rho > 0.0).any()
    for which, what, x in inputs(w):
        a, d = pair_of(which, x, w.c0)
        ref = quad_ref(p, c, rho, a, d)
        scale = np.abs(ref).max()
        assert scale > 0.0
        assert np.abs(quad_direct(p, c, rho, a, d) - ref).max() <= 1e-13 * scale, what
        # the trilinear form is symmetric in its arguments: N(a) delta = N(delta) a
        assert np.abs(quad_ref(p, c, rho, d, a) - ref).max() <= 1e-13 * scale, what


def test_row_counts_reach_the_second_record_round_trip():
    """Rows of more than 32 (row, cell) records: the straight-line pass fetches them in a second round trip."""
    w = case('random_3000')
    Q, R = quad_abs(w.mesh.points, w.mesh.cells, rho_of(w), w.c0, w.c0)
    assert R.max() > 32 and row_lengths(w.mesh.cells, len(w.mesh.points)).max() > 32
    assert R.sum() == w.mesh.cells.size


@pytest.mark.parametrize("cid", sorted(CASES))
def test_emulation_inside_the_bound_and_mutations_outside(cid):
    w = case(cid)
    p, c, rho = w.mesh.points, w.mesh.cells, rho_of(w)
    dim, dt = p.shape[1], w.dt
    worst = 0.0
    for which, what, x in inputs(w):
        a, d = pair_of(which, x, w.c0)
        ref = -dt * quad_ref(p, c, rho, a, d)
        Q, R = quad_abs(p, c, rho, a, d)
        y = -dt * quad_emulate(p, c, rho, a, d)
        bound = quad_bound(dim, 1, dt, Q, R, y)
        err = np.abs(y - ref)
        worst = max(worst, (err[Q > 0] / (U32 * dt * Q[Q > 0])).max())
        assert np.all(err <= bound), (what, int(np.argmax(err - bound)))
        assert np.all(y[Q == 0] == 0.0)
        for mutation in ('drop_last', 'diag3', 'slot_shift'):
            ym = -dt * quad_emulate(p, c, rho, a, d, mutation)
            out = np.abs(ym - ref) > quad_bound(dim, 1, dt, Q, R, ym)
            assert out.any(), (what, mutation)
    print("%s: float32 emulation, largest err / (2^-24 Q_i) = %.3f" % (w.name, worst))
