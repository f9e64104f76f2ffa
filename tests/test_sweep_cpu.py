"""
The reference, the bounds and the emulation of tests/test_gpu_sweep_operator.py, checked without a GPU (tests/sweep_common.py).
For every mesh of quad_pass_common.CASES and three iterates (the case's bump, a random field in [0.02, 1], the ball field of the
exactly-linear slices):

  * the float64 emulation of the sweep lies inside every bound on every row: stored entries (fp64 and fp32), products with the
    probe vectors, the residual with and without a load, dinv, the slice sum;
  * the oracle's own rd_jacobian and rd_residual lie inside the reference-rounding term alone, which pins the new reference to
    the one the rest of the suite uses;
  * each defect of sweep_common.MUTATIONS leaves the bound of every output it corrupts by at least a factor 10 on at least one
    row, and stays inside the bounds of the outputs it does not touch (sweep_common.CORRUPTS) -- so the GPU test would see
    each of them, and would name the output:

                             A (products)   R           dinv
      drop_last              outside        outside     outside
      diag3                  outside        outside     outside
      slot_shift             outside        outside     outside
      stored_dt              outside        inside      inside
      dinv_from_S            inside         inside      outside
      residual_from_rounded  inside (fp32)  outside     inside       (fp32 storage; R against the fp64 bound)

Reference counterpart: the Jacobian and residual of 'F == 0' (simulation_tumor_growth.py:115-120).
"""
import numpy as np
import pytest

from oracle.glims_oracle import OracleTumorGrowth
from sweep_common import (CASES, CORRUPTS, LD, MUTATIONS, REF_EVALS, SweepRef, ball_field, case, f64, fields, inside,
                          lin_reference, sums_bound, sweep_emulate, worst)

_BASE = {}


def _base(cid):
    if cid not in _BASE:
        _BASE[cid] = SweepRef(case(cid))
    return _BASE[cid]


def _inputs(w):
    n = len(w.mesh.points)
    rng = np.random.default_rng(23)
    c_prev = rng.random(n)
    load = 0.05 * np.cos(3.0 * w.mesh.points[:, 0]) * (1.0 + w.mesh.points[:, 1] ** 2)
    probes = {'normal': rng.standard_normal(n), 'ones': np.ones(n), 'x': np.asarray(w.mesh.points[:, 0], dtype=np.float64)}
    return c_prev, load, probes


def _errors(at, em, c_prev, load, probes, fp32):
    """{output: (err, bound)} of an emulation against the reference; 'A' = the three products stacked."""
    pat = at.base.pat
    e_a = np.concatenate([np.abs(pat.matvec(em['A'], z) - at.product(z)) for z in probes.values()])
    b_a = np.concatenate([at.product_bound(z, fp32) for z in probes.values()])
    return {'A': (e_a, b_a),
            'R': (np.abs(em['R'].astype(LD) - at.residual(c_prev, load)), at.residual_bound(c_prev, load)),
            'dinv': (np.abs(em['dinv'].astype(LD) * at.diag() - 1.0), at.dinv_bound())}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_emulation_inside_the_bounds_and_mutations_outside(cid):
    w = case(cid)
    base = _base(cid)
    pat = base.pat
    c_prev, load, probes = _inputs(w)
    assert base.kappa.min() >= 1.0 and np.all(f64(base.Sabs) >= np.abs(f64(base.S)))
    for name, c in fields(w).items():
        at = base.at(c)
        for fp32 in (False, True):
            for ld in (None, load):
                em = sweep_emulate(w, pat, c, c_prev, ld, fp32=fp32)
                assert inside(np.abs(em['A'].astype(LD) - at.A), at.entry_bound(fp32)), (name, fp32)
                for what, (err, bound) in _errors(at, em, c_prev, ld, probes, fp32).items():
                    assert inside(err, bound), (name, fp32, what, int(np.argmax(err - bound)))
                    print("%s, %s, %s%s: %s largest err / bound = %.3f" % (w.name, name, "fp32" if fp32 else "fp64",
                                                                           "" if ld is None else ", load", what, worst(err, bound)))
                s = float(np.sum(em['R'] * em['R']))
                assert abs(em['sumsq'] - s) <= sums_bound(pat.n, s)
        for mutation in MUTATIONS:
            fp32 = mutation == 'residual_from_rounded'
            em = sweep_emulate(w, pat, c, c_prev, load, fp32=fp32, mutation=mutation)
            for what, (err, bound) in _errors(at, em, c_prev, load, probes, fp32).items():
                if what in CORRUPTS[mutation]:
                    assert np.any(err > 10.0 * bound), (name, mutation, what, worst(err, bound))
                else:
                    assert inside(err, bound), (name, mutation, what, worst(err, bound))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_oracle_inside_the_reference_rounding_term(cid):
    w = case(cid)
    base = _base(cid)
    pat = base.pat
    c_prev, load, _ = _inputs(w)
    o = OracleTumorGrowth(w.mesh.points, w.mesh.cells, w.per_cell('D'), w.per_cell('rho'), w.per_cell('gamma'),
                          w.per_cell('E'), w.per_cell('nu'), w.dt, rd_load=load)
    for name, c in fields(w).items():
        at = base.at(c)
        J = o.rd_jacobian(c).tocsr()
        J.sort_indices()
        assert np.array_equal(J.indptr, pat.ptr) and np.array_equal(J.indices, pat.cols)
        err, bound = np.abs(J.data.astype(LD) - at.A), at.entry_bound(evals=REF_EVALS)
        assert inside(err, bound), (name, int(np.argmax(err - bound)))
        err_r = np.abs(o.rd_residual(c, c_prev).astype(LD) - at.residual(c_prev, load))
        bound_r = at.residual_bound(c_prev, load, evals=REF_EVALS)
        assert inside(err_r, bound_r), (name, int(np.argmax(err_r - bound_r)))
        print("%s, %s: oracle Jacobian err / term = %.3f, residual %.3f" % (w.name, name, worst(err, bound), worst(err_r, bound_r)))


@pytest.mark.parametrize("cid", sorted(CASES))
def test_lin_reference_on_the_ball_fields(cid):
    """No entry of a ball field is too close to call, N vanishes on some entries and not on others, and the flags follow the
    numbering they are given."""
    w = case(cid)
    base = _base(cid)
    n = base.n
    for k in range(3):
        c = ball_field(w, k)
        assert (c == 0.0).any() and (c >= 0.02).any() and np.all((c == 0.0) | (c >= 0.02))
        flags, ambiguous = lin_reference(w, c, np.arange(n), base)
        assert ambiguous == 0 and len(flags) == (n + 63) // 64
        at = base.at(c)
        changed = f64(at.N) != 0.0
        assert changed.any() and not changed.all()
        rev, _ = lin_reference(w, c, np.arange(n)[::-1].copy(), base)
        expect = np.ones(len(flags), dtype=bool)
        expect[(n - 1 - base.pat.rows[changed]) // 64] = False
        assert np.array_equal(rev, expect)
    # a field that is positive everywhere leaves no slice linear unless every cell at its rows has rho = 0
    flags, _ = lin_reference(w, fields(w)['random'], np.arange(n), base)
    rows_rho0 = np.ones(n, dtype=bool)
    rows_rho0[np.unique(np.asarray(w.mesh.cells)[w.per_cell('rho') != 0.0])] = False
    for s in np.flatnonzero(flags):
        assert rows_rho0[64 * s:64 * s + 64].all()


def test_ball_fields_leave_linear_rows_on_the_larger_meshes():
    """Rows whose entries all keep the bits of S exist next to rows that do not, for every centre: the GPU test's equality
    of slice counts is not 0 == 0 by construction of the field (which slices they fill is the device numbering's to say)."""
    for cid in ('c3_n8', 'random_1000', 'jittered_seed0', 'jittered_seed1', 'random_3000'):
        w, base = case(cid), _base(cid)
        for k in range(3):
            row_changed = np.zeros(base.n, dtype=bool)
            row_changed[base.pat.rows[f64(base.at(ball_field(w, k)).N) != 0.0]] = True
            assert 64 <= row_changed.sum() <= base.n - 64
