"""
The numpy second-order adjoint (tests/adjoint_hessian_common.py) -- the reference of glims_adjoint_hessian -- against central
differences of the numpy adjoint gradient, by symmetry and by a Taylor test of J; and the new entry point is exported.
"""
import numpy as np
import pytest

from adjoint_common import make_problem, many_tissues, misfit, u_terms
from adjoint_hessian_common import flat, gradient_at, hessian

N_STEPS = 4


def _direction(prob, seed):
    rng = np.random.default_rng(seed)
    n = len(prob.points)
    return dict(D=prob.D * rng.uniform(-1, 1, prob.n_labels), rho=prob.rho * rng.uniform(-1, 1, prob.n_labels),
                gamma=prob.gamma * rng.uniform(-1, 1, prob.n_labels), c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1))


def _base(prob):
    return dict(D=prob.D, rho=prob.rho, gamma=prob.gamma, c0=prob.c0)


def _shift(m, d, eps):
    return {k: m[k] + eps * d[k] for k in m}


@pytest.mark.parametrize("dim", [2, 3])
def test_hessian_matches_central_differences_of_the_gradient(dim):
    prob = make_problem(dim)
    terms = prob.terms(N_STEPS)
    kinds = {t["kind"] for t in terms}
    assert kinds == {"c_l2", "c_thresh", "u_l2"} and prob.dir_c is not None
    d = _direction(prob, 1)
    o = prob.oracle()
    traj = prob.trajectory(o, N_STEPS)
    hv = hessian(prob, o, traj, terms, [d])[5][0]
    ana = flat(prob, hv)
    eps = 1e-4
    m = _base(prob)
    num = (gradient_at(prob, _shift(m, d, eps), N_STEPS, terms)[1] -
           gradient_at(prob, _shift(m, d, -eps), N_STEPS, terms)[1]) / (2 * eps)
    L = prob.n_labels
    for what, sl in (("D", slice(0, L)), ("rho", slice(L, 2 * L)), ("gamma", slice(2 * L, 3 * L)),
                     ("c0", slice(3 * L, None))):
        err = np.linalg.norm(ana[sl] - num[sl]) / np.linalg.norm(num[sl])
        assert err <= 1e-6, (what, err, ana[sl][:4], num[sl][:4])


# ---- the regimes of tests/test_gpu_adjoint_hessian_coverage.py ------------------------------------------------------------
def _everywhere(prob, seed):
    """dD, drho, dgamma on every label (absolute sizes, so a passive tissue's entries are not 0) and a dc0."""
    rng = np.random.default_rng(seed)
    L, n = prob.n_labels, len(prob.points)
    return dict(D=0.03 * rng.uniform(-1, 1, L), rho=0.4 * rng.uniform(-1, 1, L), gamma=0.15 * rng.uniform(-1, 1, L),
                c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1))


def _regime(case):
    """(problem, N, terms)"""
    if case == "tissues_clamp_and_loads":
        prob = many_tissues(2, 9, n=8, empty=(3,), zero=(5,), zero_gamma=(5,), u_clamp=0.02, mech_load=1.0, rd_load=0.3)
        return prob, N_STEPS, prob.terms(N_STEPS)
    prob = many_tissues(2, 3, n=8, u_clamp=0.02, mech_load=1.0, seed=2)
    n = len(prob.points)
    if case == "u_terms_at_0_1_N_N":
        return prob, N_STEPS, u_terms(prob, [0, 1, N_STEPS, N_STEPS], seed=3) + [
            dict(step=N_STEPS, kind="c_l2", weight=1.0, target=np.full(n, 0.2))]
    rng = np.random.default_rng(4)   # no steps: every term observes c_0
    return prob, 0, [dict(step=0, kind="c_thresh", level=0.3, smooth=0.1, weight=1.5, target=rng.uniform(0, 1, n)),
                     dict(step=0, kind="c_l2", weight=0.5, target=rng.uniform(0, 0.5, n))] + u_terms(prob, [0], seed=5)


@pytest.mark.parametrize("case", ["tissues_clamp_and_loads", "u_terms_at_0_1_N_N", "no_steps"])
def test_hessian_matches_central_differences_in_the_device_test_regimes(case):
    """9 tissues (id 3 carried by no cell, id 5 with D = rho = gamma = 0) with clamp values, a mechanical and an RD load;
    displacement terms at steps 0, 1, N, N; a recording of no steps, where the D and rho rows are exactly 0."""
    prob, N, terms = _regime(case)
    d = _everywhere(prob, 1)
    o = prob.oracle()
    hv = hessian(prob, o, prob.trajectory(o, N), terms, [d])[5][0]
    ana = flat(prob, hv)
    eps = 1e-4
    m = _base(prob)
    num = (gradient_at(prob, _shift(m, d, eps), N, terms)[1] - gradient_at(prob, _shift(m, d, -eps), N, terms)[1]) / (2 * eps)
    L = prob.n_labels
    for what, sl in (("D", slice(0, L)), ("rho", slice(L, 2 * L)), ("gamma", slice(2 * L, 3 * L)),
                     ("c0", slice(3 * L, None))):
        if N == 0 and what in ("D", "rho"):
            assert not ana[sl].any() and not num[sl].any(), (what, ana[sl], num[sl])
            continue
        err = np.linalg.norm(ana[sl] - num[sl]) / np.linalg.norm(num[sl])
        assert err <= 1e-6, (what, err, ana[sl][:4], num[sl][:4])
    if case == "tissues_clamp_and_loads":
        assert hv["D"][3] == 0 and hv["rho"][3] == 0 and hv["gamma"][3] == 0
        assert hv["D"][5] != 0 and hv["rho"][5] != 0 and hv["gamma"][5] != 0


@pytest.mark.parametrize("dim", [2, 3])
def test_full_hessian_matrix_is_symmetric(dim):
    prob = make_problem(dim)
    terms = prob.terms(N_STEPS)
    L, n = prob.n_labels, len(prob.points)
    rng = np.random.default_rng(5)
    dirs = []
    for key in ("D", "rho", "gamma"):
        for l in range(L):
            e = np.zeros(L)
            e[l] = 1.0
            dirs.append({key: e})
    dirs += [dict(c0=rng.uniform(-1, 1, n)) for _ in range(2)]
    o = prob.oracle()
    hv = hessian(prob, o, prob.trajectory(o, N_STEPS), terms, dirs)[5]
    V = np.array([flat(prob, d) for d in dirs])       # directions as rows
    H = np.array([[flat(prob, hv[j]) @ V[i] for j in range(len(dirs))] for i in range(len(dirs))])
    assert np.abs(H - H.T).max() <= 1e-9 * np.abs(H).max(), H


def test_taylor_remainder_is_third_order():
    prob = make_problem(2)
    terms = prob.terms(N_STEPS)
    d = _direction(prob, 2)
    o = prob.oracle()
    J, dD, drho, dgam, dc0, hv = hessian(prob, o, prob.trajectory(o, N_STEPS), terms, [d])
    g = np.concatenate([dD, drho, dgam, dc0])
    dm = flat(prob, d)
    dHd = flat(prob, hv[0]) @ dm
    m = _base(prob)
    rem = []
    epss = [0.2, 0.1, 0.05, 0.025]
    for eps in epss:
        me = _shift(m, d, eps)
        oe = prob.oracle(D=me["D"], rho=me["rho"], gamma=me["gamma"])
        Je = misfit(prob, oe, prob.trajectory(oe, N_STEPS, c0=me["c0"]), terms)
        rem.append(abs(Je - J - eps * (g @ dm) - 0.5 * eps ** 2 * dHd))
    rates = [np.log2(rem[i] / rem[i + 1]) for i in range(len(rem) - 1)]
    assert min(rates[-2:]) >= 2.8, (rem, rates)


def test_reduced_functional_refuses_e_and_nu_for_the_hessian_only():
    from glimslib_amd.optimization import ReducedFunctional

    class Params:
        D_WM = D_GM = rho_WM = rho_GM = coupling = E_WM = 0.1

    class Sim:
        params = Params()

        def run(self, **kw):
            raise AssertionError("no forward run before the names are checked")

    rf = ReducedFunctional(Sim(), 2, lambda s, n: [], names=("D_WM", "E_WM"))
    with pytest.raises(ValueError, match="E / nu"):
        rf.hessian([0.1, 0.1], [1.0, 0.0])
    with pytest.raises(ValueError, match="E / nu"):
        rf.hessian_matrix([0.1, 0.1])


def test_hessian_entry_point_is_exported():
    from glimslib_amd import _backend
    lib = _backend.load_library()
    assert hasattr(lib, "glims_adjoint_hessian")
    assert "glims_adjoint_hessian" in _backend.SIGNATURES
    assert lib.glims_abi_version() == 6
