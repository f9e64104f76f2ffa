"""
dJ/dE and dJ/dnu of the discrete adjoint on the CPU: the numpy reference of adjoint_elastic_common
against central differences of the oracle's J, the per-label-sum formula the device pass uses against the reference, the
identities the gradient obeys, and the C-ABI surface that carries it (glims_adjoint_gradient_full).  No GPU.
"""
import os
import re

import numpy as np
import pytest

from adjoint_common import many_tissues, u_terms
from adjoint_elastic_common import central_differences, elastic_adjoint, formula_gradient, oracle_with

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def _problem(dim, **kw):
    """Four tissues: label 3 empty, label 1 with gamma = 0; clamp values and a mechanical load unless overridden."""
    args = dict(n=6 if dim == 2 else 3, empty=(3,), zero_gamma=(1,), u_clamp=0.02, mech_load=0.5, seed=3 + dim)
    args.update(kw)
    return many_tissues(dim, 4, **args)


def _terms(prob, N):
    n = len(prob.points)
    rng = np.random.default_rng(9)
    return u_terms(prob, [1, N, N], seed=8) + [dict(step=N, kind="c_l2", weight=1.0, target=rng.uniform(0, 0.4, n))]


def _run(prob, N):
    o = oracle_with(prob)
    c = [prob.c0.copy()]
    for _ in range(N):
        c.append(o.rd_step(c[-1], rtol=1e-14, atol=1e-16)[0])
    return o, c


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_matches_central_differences(dim):
    prob = _problem(dim)
    assert prob.gamma[1] == 0.0 and not (prob.labels == 3).any()
    N = 3
    o, traj = _run(prob, N)
    terms = _terms(prob, N)
    dE, dnu = elastic_adjoint(prob, o, traj, terms)
    fE, fnu = central_differences(prob, traj, terms)
    assert _rel(dE, fE) < 1e-6, (dE, fE)
    assert _rel(dnu, fnu) < 1e-6, (dnu, fnu)
    assert dE[3] == 0.0 and dnu[3] == 0.0                      # the empty label
    assert abs(dE[1]) > 1e-3 * np.abs(dE).max()                # gamma = 0: dK/dE still acts on u


@pytest.mark.parametrize("dim", [2, 3])
def test_per_label_sum_formula_matches_reference(dim):
    """A_t, B_t, C_t as the device pass forms them give the assembled derivatives (also with u_D != 0 and a load)."""
    prob = _problem(dim)
    N = 3
    o, traj = _run(prob, N)
    terms = _terms(prob, N)
    dE, dnu = elastic_adjoint(prob, o, traj, terms)
    gE, gnu = formula_gradient(prob, o, traj, terms)
    assert _rel(gE, dE) < 1e-12 and _rel(gnu, dnu) < 1e-12


def test_only_concentration_terms_give_exact_zeros():
    prob = _problem(2)
    N = 2
    o, traj = _run(prob, N)
    terms = [t for t in _terms(prob, N) if t["kind"] != "u_l2"]
    for g in elastic_adjoint(prob, o, traj, terms) + formula_gradient(prob, o, traj, terms):
        assert np.all(g == 0.0)


@pytest.mark.parametrize("dim", [2, 3])
def test_scale_invariance_without_load(dim):
    """f = 0: scaling every E scales K and G alike, u does not move, so sum_t E_t dJ/dE_t = 0."""
    prob = _problem(dim, mech_load=0.0)
    assert prob.mech_load is None
    N = 2
    o, traj = _run(prob, N)
    dE, _ = elastic_adjoint(prob, o, traj, _terms(prob, N))
    s = prob.E * dE
    assert abs(s.sum()) <= 1e-9 * np.abs(s).sum()
    assert np.abs(s).sum() > 0.0


def test_load_breaks_scale_invariance():
    """The identity needs f = 0: with a load the weighted sum is far from 0 (the test above is not vacuous)."""
    prob = _problem(2, mech_load=2.0)
    N = 2
    o, traj = _run(prob, N)
    dE, _ = elastic_adjoint(prob, o, traj, _terms(prob, N))
    s = prob.E * dE
    assert abs(s.sum()) > 1e-3 * np.abs(s).sum()


def test_header_and_ctypes_table_carry_the_full_gradient():
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+glims_adjoint_gradient_full\s*\(([^)]*)\)", code)
    assert m, "glims_adjoint_gradient_full is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[-2:] == ["double* dJ_dE", "double* dJ_dnu"], args
    assert re.search(r"#define\s+GLIMS_ABI_VERSION\s+6\b", code)
    from glimslib_amd import _backend
    restype, argtypes = _backend.SIGNATURES["glims_adjoint_gradient_full"]
    assert len(argtypes) == 10
    assert argtypes[:8] == _backend.SIGNATURES["glims_adjoint_gradient"][1]


def test_reduced_functional_names_select_brain_controls():
    """names= picks TumorGrowthBrain parameters with P = identity; the n-parameter maps are unchanged."""
    from types import SimpleNamespace
    from glimslib_amd.optimization import ReducedFunctional, parameter_map
    brain = SimpleNamespace(params=SimpleNamespace(D_WM=0.1))
    rf = ReducedFunctional(brain, 2, None, names=("E_WM", "coupling"))
    assert rf.names == ("E_WM", "coupling") and np.array_equal(rf.P, np.eye(2))
    rf._set_params(np.array([2.5, 0.3]))
    assert brain.params.E_WM == 2.5 and brain.params.coupling == 0.3
    assert rf._model_gradient({"E_WM": 4.0, "coupling": -1.0}).tolist() == [4.0, -1.0]
    for n in (2, 3, 4, 5):
        names, P = parameter_map(n)
        rf = ReducedFunctional(brain, n, None)
        assert rf.names == names and np.array_equal(rf.P, P)
    for bad in (("E_WM",), ("E_XX", "coupling"), ("E_WM", "E_WM")):
        with pytest.raises(ValueError):
            ReducedFunctional(brain, 2, None, names=bad)
    with pytest.raises(ValueError):
        ReducedFunctional(SimpleNamespace(params=SimpleNamespace()), 1, None, names=("E",))
