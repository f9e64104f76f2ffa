"""
The numpy second-order elastic adjoint (tests/adjoint_hessian_elastic_common.py) -- the reference of
glims_adjoint_hessian_full -- against central differences of the numpy full gradient (adjoint_hessian_common.gradient_at +
adjoint_elastic_common.elastic_adjoint), by symmetry of the per-label matrix over (D, rho, gamma, E, nu), and by the scale
identity differentiated once; the opt-in of ReducedFunctional and the new entry point.  No GPU.
"""
import numpy as np
import pytest

from adjoint_common import make_problem, many_tissues, u_terms
from adjoint_hessian_elastic_common import KEYS, flat_full, full_gradient_at, hessian_full, unit_directions

N_STEPS = 4


def _direction(prob, seed):
    """Every block at once, on every label (absolute sizes in D, rho, gamma: a passive tissue's entries are not 0)."""
    rng = np.random.default_rng(seed)
    L, n = prob.n_labels, len(prob.points)
    return dict(D=0.03 * rng.uniform(-1, 1, L), rho=0.4 * rng.uniform(-1, 1, L), gamma=0.15 * rng.uniform(-1, 1, L),
                E=prob.E * rng.uniform(-1, 1, L), nu=0.1 * rng.uniform(-1, 1, L), c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1))


def _base(prob):
    return dict(D=prob.D, rho=prob.rho, gamma=prob.gamma, E=prob.E, nu=prob.nu, c0=prob.c0)


def _shift(m, d, eps):
    return {k: m[k] + eps * d[k] for k in m}


def _case(case):
    """(problem, N, terms)"""
    if case in ("2d", "3d"):
        prob = make_problem(2 if case == "2d" else 3)
        return prob, N_STEPS, prob.terms(N_STEPS)
    if case == "clamp_values_and_load":
        prob = many_tissues(2, 4, n=6, empty=(3,), zero_gamma=(1,), u_clamp=0.02, mech_load=0.5, seed=5)
        assert np.any(prob.dir_u[1] != 0.0) and prob.mech_load is not None
        return prob, N_STEPS, prob.terms(N_STEPS)
    prob = many_tissues(3, 3, n=3, u_clamp=0.02, mech_load=1.0, seed=2)   # u terms at steps 0, 1, N, N
    n = len(prob.points)
    return prob, N_STEPS, u_terms(prob, [0, 1, N_STEPS, N_STEPS], seed=3) + [
        dict(step=N_STEPS, kind="c_l2", weight=1.0, target=np.full(n, 0.2))]


@pytest.mark.parametrize("case", ["2d", "3d", "clamp_values_and_load", "u_terms_at_0_1_N_N"])
def test_products_match_central_differences_of_the_full_gradient(case):
    prob, N, terms = _case(case)
    d = _direction(prob, 1)
    o = prob.oracle()
    hv = hessian_full(prob, o, prob.trajectory(o, N), terms, [d])[2][0]
    ana = flat_full(prob, hv)
    eps = 1e-4
    m = _base(prob)
    num = (full_gradient_at(prob, _shift(m, d, eps), N, terms)[1] -
           full_gradient_at(prob, _shift(m, d, -eps), N, terms)[1]) / (2 * eps)
    L = prob.n_labels
    for i, what in enumerate(KEYS + ("c0",)):
        sl = slice(i * L, (i + 1) * L) if what != "c0" else slice(5 * L, None)
        err = np.linalg.norm(ana[sl] - num[sl]) / np.linalg.norm(num[sl])
        assert err <= 1e-6, (what, err, ana[sl][:4], num[sl][:4])


@pytest.mark.parametrize("key", ["E", "nu"])
def test_pure_elastic_directions_match_central_differences(key):
    """dE alone and dnu alone (the tangent-linear concentration is 0: only the elastic part of the sweep acts)."""
    prob, N, terms = _case("clamp_values_and_load")
    L = prob.n_labels
    d = {key: _direction(prob, 2)[key]}
    o = prob.oracle()
    hv = hessian_full(prob, o, prob.trajectory(o, N), terms, [d])[2][0]
    ana = flat_full(prob, hv)
    full = dict(_base(prob))
    dd = {k: (np.asarray(d[k]) if k in d else np.zeros_like(full[k])) for k in full}
    eps = 1e-4
    num = (full_gradient_at(prob, _shift(full, dd, eps), N, terms)[1] -
           full_gradient_at(prob, _shift(full, dd, -eps), N, terms)[1]) / (2 * eps)
    for i, what in enumerate(KEYS + ("c0",)):
        sl = slice(i * L, (i + 1) * L) if what != "c0" else slice(5 * L, None)
        err = np.linalg.norm(ana[sl] - num[sl]) / np.linalg.norm(num[sl])
        assert err <= 1e-6, (what, err, ana[sl][:4], num[sl][:4])


@pytest.mark.parametrize("dim", [2, 3])
def test_full_per_label_matrix_is_symmetric(dim):
    prob = make_problem(dim)
    terms = prob.terms(N_STEPS)
    dirs = unit_directions(prob)
    o = prob.oracle()
    hv = hessian_full(prob, o, prob.trajectory(o, N_STEPS), terms, dirs)[2]
    H = np.array([np.concatenate([h[k] for k in KEYS]) for h in hv]).T    # column j = H e_j
    assert H.shape == (5 * prob.n_labels,) * 2
    assert np.abs(H - H.T).max() <= 1e-9 * np.abs(H).max(), H
    L = prob.n_labels
    assert np.abs(H[3 * L:, :3 * L]).max() > 1e-6 * np.abs(H).max()      # the mixed blocks are not empty


@pytest.mark.parametrize("dim", [2, 3])
def test_scale_identity_differentiated_once(dim):
    """No load, zero clamp values: scaling every E scales K and G alike and u does not move, so sum_s E_s dJ/dE_s = 0 for
    every value of the other parameters.  Differentiated once: sum_s E_s H[q, E_s] = 0 for q in D, rho, gamma, nu and
    sum_s E_s H[E_t, E_s] = -dJ/dE_t."""
    prob = make_problem(dim)
    assert prob.mech_load is None and not np.any(prob.dir_u[1])
    terms = prob.terms(N_STEPS)
    L = prob.n_labels
    o = prob.oracle()
    _, g, hv = hessian_full(prob, o, prob.trajectory(o, N_STEPS), terms, unit_directions(prob, keys=("E",)))
    for q in ("D", "rho", "gamma", "nu"):
        for t in range(L):
            s = np.array([prob.E[j] * hv[j][q][t] for j in range(L)])
            assert abs(s.sum()) <= 1e-9 * np.abs(s).sum(), (q, t, s)
    seen = 0.0
    for t in range(L):
        s = np.array([prob.E[j] * hv[j]["E"][t] for j in range(L)] + [g["E"][t]])
        assert abs(s.sum()) <= 1e-9 * np.abs(s).sum(), (t, s)
        seen += np.abs(s).sum()
    assert seen > 0.0


def test_without_a_displacement_term_the_elastic_rows_are_exactly_zero():
    prob = make_problem(2)
    terms = [t for t in prob.terms(N_STEPS) if t["kind"] != "u_l2"]
    o = prob.oracle()
    _, g, hv = hessian_full(prob, o, prob.trajectory(o, N_STEPS), terms, [_direction(prob, 3), dict(E=prob.E), dict(nu=0.1)])
    assert not g["E"].any() and not g["nu"].any()
    for h in hv:
        assert np.all(h["E"] == 0.0) and np.all(h["nu"] == 0.0)
    assert hv[0]["D"].any() and not hv[1]["D"].any() and not hv[2]["c0"].any()


def test_reduced_functional_takes_e_and_nu_for_the_hessian_when_asked():
    from glimslib_amd.optimization import ReducedFunctional

    class Params:
        D_WM = D_GM = rho_WM = rho_GM = coupling = E_WM = 0.1

    class Sim:
        params = Params()

        def run(self, **kw):
            raise AssertionError("no forward run before the names are checked")

    rf = ReducedFunctional(Sim(), 2, lambda s, n: [], names=("D_WM", "E_WM"), elastic_hessian=True)
    assert rf._model_directions() == [{"D_WM": 1.0}, {"E_WM": 1.0}]
    with pytest.raises(AssertionError, match="no forward run"):     # past the names check: the forward run is next
        rf.hessian_matrix([0.1, 0.1])
    with pytest.raises(ValueError, match="E / nu"):                 # the default refuses as before
        ReducedFunctional(Sim(), 2, lambda s, n: [], names=("D_WM", "E_WM")).hessian_matrix([0.1, 0.1])


def test_full_hessian_entry_point_is_exported():
    from glimslib_amd import _backend
    lib = _backend.load_library()
    assert hasattr(lib, "glims_adjoint_hessian_full")
    assert len(_backend.SIGNATURES["glims_adjoint_hessian_full"][1]) == 24
    assert lib.glims_abi_version() == 6
