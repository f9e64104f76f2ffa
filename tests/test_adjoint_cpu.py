"""Discrete adjoint, CPU side: the ABI surface, the numpy reference adjoint against finite differences of the oracle, and the
chain rule of glimslib_amd.optimization's parameter maps (no GPU)."""
import os
import re

import numpy as np
import pytest

from adjoint_common import Problem, adjoint, dthresh, many_tissues, misfit, thresh, u_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_adjoint_entry_points():
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    src_nc = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("glims_adjoint_record", "glims_adjoint_gradient", "glims_adjoint_stats"):
        assert re.search(r"\b%s\s*\(" % name, src_nc), name
    assert "typedef struct glims_misfit" in src
    from glimslib_amd import _backend
    for name in ("glims_adjoint_record", "glims_adjoint_gradient", "glims_adjoint_stats"):
        assert name in _backend.SIGNATURES
    body = re.search(r"typedef struct glims_misfit \{(.*?)\} glims_misfit;", src, re.S).group(1)
    fields = re.findall(r"\*?([a-z_]+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _backend.Misfit._fields_]


@pytest.fixture(scope="module")
def prob():
    return Problem(2, 6)


def _J(prob, N, terms, D=None, rho=None, gamma=None, c0=None):
    o = prob.oracle(D, rho, gamma)
    return misfit(prob, o, prob.trajectory(o, N, c0), terms)


def test_numpy_adjoint_matches_central_differences(prob):
    N = 8
    terms = prob.terms(N)
    o = prob.oracle()
    J, dD, drho, dgam, dc0 = adjoint(prob, o, prob.trajectory(o, N), terms)
    assert J > 0 and np.all(np.isfinite(dc0))

    def fd(fun, x0, h):
        g = np.zeros_like(x0)
        for i in range(len(x0)):
            e = np.zeros_like(x0)
            e[i] = h * abs(x0[i])
            g[i] = (fun(x0 + e) - fun(x0 - e)) / (2 * e[i])
        return g

    checks = [(dD, fd(lambda p: _J(prob, N, terms, D=p), prob.D, 1e-5)),
              (drho, fd(lambda p: _J(prob, N, terms, rho=p), prob.rho, 1e-5)),
              (dgam, fd(lambda p: _J(prob, N, terms, gamma=p), prob.gamma, 1e-5))]
    for ad, num in checks:
        assert np.linalg.norm(ad - num) <= 1e-6 * np.linalg.norm(num), (ad, num)
    # dJ/dc0 along a random direction
    p = np.random.default_rng(1).standard_normal(len(prob.points))
    h = 1e-4
    num = (_J(prob, N, terms, c0=prob.c0 + h * p) - _J(prob, N, terms, c0=prob.c0 - h * p)) / (2 * h)
    assert abs(dc0 @ p - num) <= 1e-6 * abs(num)


# ---- the reference's generalised problems: many tissues, clamps, loads, displacement terms, degenerate term sets ------------
def _fd(fun, x0, h):
    """Central differences, step h |x_i| (h times the mean |x| for a zero entry)."""
    g = np.zeros_like(x0)
    ref = np.mean(np.abs(x0[x0 != 0]))
    for i in range(len(x0)):
        e = np.zeros_like(x0)
        e[i] = h * (abs(x0[i]) if x0[i] != 0 else ref)
        g[i] = (fun(x0 + e) - fun(x0 - e)) / (2 * e[i])
    return g


def _check_fd(prob, N, terms, params=("D", "rho", "gamma"), dc0_dir_seed=1):
    o = prob.oracle()
    J, dD, drho, dgam, dc0 = adjoint(prob, o, prob.trajectory(o, N), terms)
    assert J == pytest.approx(_J(prob, N, terms), rel=1e-14)
    ad = dict(D=dD, rho=drho, gamma=dgam)
    for name in params:
        num = _fd(lambda q: _J(prob, N, terms, **{name: q}), getattr(prob, name), 1e-5)
        scale = np.linalg.norm(num)
        assert scale > 0, name
        assert np.linalg.norm(ad[name] - num) <= 1e-6 * scale, (name, ad[name], num)
        assert np.all(np.abs(ad[name] - num) <= 1e-6 * scale), (name, ad[name], num)   # label by label
    p = np.random.default_rng(dc0_dir_seed).standard_normal(len(prob.points))
    h = 1e-5   # (the central-difference error, O(h^2), is 1e-6 relative at h = 1e-4 on these problems)
    num = (_J(prob, N, terms, c0=prob.c0 + h * p) - _J(prob, N, terms, c0=prob.c0 - h * p)) / (2 * h)
    assert abs(dc0 @ p - num) <= 1e-6 * abs(num), (dc0 @ p, num)
    return J, dD, drho, dgam, dc0


def test_many_tissues_with_an_empty_and_a_passive_label_match_central_differences():
    """11 labels (more than one sensitivity chunk of the device pass), id 4 carried by no cell, id 7 with D = rho = 0."""
    prob = many_tissues(2, 11, n=6, empty=(4,), zero=(7,), u_clamp=0.01, mech_load=0.5, rd_load=0.3)
    assert np.bincount(prob.labels, minlength=11)[4] == 0 and np.all(np.bincount(prob.labels, minlength=11)[[0, 7, 10]] > 0)
    N = 4
    terms = prob.terms(N) + u_terms(prob, [2])
    J, dD, drho, dgam, _ = _check_fd(prob, N, terms)
    assert dD[4] == 0.0 and drho[4] == 0.0 and dgam[4] == 0.0
    assert dD[7] != 0.0 and drho[7] != 0.0   # a passive tissue still has a sensitivity


@pytest.mark.parametrize("dim", [2, 3])
def test_displacement_terms_at_several_steps_with_clamps_and_load_match_central_differences(dim):
    """u_l2 at step 0, midway and twice at the last step, non-zero Dirichlet displacement, a mechanical load, an RD source."""
    prob = many_tissues(dim, 3, n=6 if dim == 2 else 3, u_clamp=0.02, mech_load=1.0, rd_load=0.2, seed=2)
    N = 4
    terms = u_terms(prob, [0, 2, N, N], seed=3) + [dict(step=N, kind="c_l2", weight=1.0,
                                                        target=np.full(len(prob.points), 0.2))]
    o = prob.oracle()
    u = o.mech_solve(prob.c0)
    assert np.allclose(u[prob.dir_u[0]], prob.dir_u[1]) and np.abs(prob.dir_u[1]).max() > 0   # the clamp values reach u
    _check_fd(prob, N, terms)


def _g0(prob, o, terms):
    """dJ/dc_0 (explicit) of concentration terms observing step 0."""
    c, M = prob.c0, o.M
    g = np.zeros(len(c))
    for t in terms:
        if t["kind"] == "c_thresh":
            g += t["weight"] * dthresh(c, t["level"], t["smooth"]) * (M @ (thresh(c, t["level"], t["smooth"]) - t["target"]))
        else:
            g += t["weight"] * (M @ (c - t["target"]))
    return g


@pytest.mark.parametrize("case", ["no_steps", "no_terms", "step0_only"])
def test_degenerate_term_sets_have_closed_form_gradients(case):
    prob = many_tissues(2, 3, n=6, seed=4)
    o = prob.oracle()
    rng = np.random.default_rng(5)
    n = len(prob.points)
    terms = [dict(step=0, kind="c_thresh", level=0.3, smooth=0.1, weight=1.5, target=rng.uniform(0, 1, n)),
             dict(step=0, kind="c_l2", weight=0.5, target=rng.uniform(0, 0.5, n))]
    N = {"no_steps": 0, "no_terms": 3, "step0_only": 3}[case]
    if case == "no_terms":
        terms = []
    J, dD, drho, dgam, dc0 = adjoint(prob, o, prob.trajectory(o, N), terms)
    assert np.all(dD == 0) and np.all(drho == 0) and np.all(dgam == 0)
    assert np.array_equal(dc0, _g0(prob, o, terms))
    if case == "no_terms":
        assert J == 0.0 and np.all(dc0 == 0)
    else:
        assert J > 0
        p = rng.standard_normal(n)
        h = 1e-4
        num = (_J(prob, N, terms, c0=prob.c0 + h * p) - _J(prob, N, terms, c0=prob.c0 - h * p)) / (2 * h)
        assert abs(dc0 @ p - num) <= 1e-6 * abs(num)


def test_renumbered_mesh_gives_the_renumbered_gradient():
    """The reference does not depend on the node numbering: a randomly renumbered lattice gives the permuted dc0 and the same
    per-label sums."""
    from adjoint_common import renumber
    a = many_tissues(2, 4, n=8, u_clamp=0.01, seed=6)
    pts, cells, perm = renumber(a.points, a.cells, 7)
    b = Problem.from_mesh(pts, cells, a.labels, a.D, a.rho, a.gamma, a.E, a.nu, a.c0[perm], dt=a.dt,
                          dir_c=(np.argsort(perm)[a.dir_c[0]], a.dir_c[1]),
                          dir_u=(np.argsort(perm)[a.dir_u[0] // 2] * 2 + a.dir_u[0] % 2, a.dir_u[1]))
    N = 3
    ta = a.terms(N) + u_terms(a, [N])
    tb = [dict(t, target=np.asarray(t["target"]).reshape(len(perm), -1)[perm].ravel()) for t in ta]
    ra = adjoint(a, a.oracle(), a.trajectory(a.oracle(), N), ta)
    rb = adjoint(b, b.oracle(), b.trajectory(b.oracle(), N), tb)
    assert ra[0] == pytest.approx(rb[0], rel=1e-12)
    for x, y in zip(ra[1:4], rb[1:4]):
        assert np.allclose(x, y, rtol=1e-10, atol=1e-14 * np.abs(x).max())
    assert np.allclose(ra[4][perm], rb[4], rtol=1e-10, atol=1e-14 * np.abs(ra[4]).max())


# ---- parameter maps of glimslib_amd.optimization -------------------------------------------------------------------------
class _Params:
    pass


class _StubSim:
    """J(q) = sum_i a_i q_i^2 over the model parameters; adjoint_gradient returns dJ/dq_i = 2 a_i q_i per label
    (split over two labels, so the per-label sum of the map is exercised too)."""

    def __init__(self, names):
        self.params = _Params()
        self.names = names
        for k in names:
            setattr(self.params, k, 0.1)
        self.a = {k: 1.0 + i for i, k in enumerate(names)}
        self.runs = 0

        class _B:
            def stats(self_inner):
                return {"steps": 3}
        self._backend = _B()

    def run(self, **kw):
        assert kw.get("record_adjoint") is True
        self.runs += 1

    def J(self):
        return sum(self.a[k] * getattr(self.params, k) ** 2 for k in self.names)

    def adjoint_gradient(self, terms):
        g = {"J": self.J()}
        for k in self.names:
            v = 2 * self.a[k] * getattr(self.params, k)
            g[k] = np.array([0.25 * v, 0.75 * v])
        return g


@pytest.mark.parametrize("brain,n", [(True, 2), (True, 3), (True, 4), (True, 5), (False, 2), (False, 3)])
def test_reduced_functional_chain_rule(brain, n):
    from glimslib_amd.optimization import BRAIN_NAMES, TUMOR_NAMES, ReducedFunctional
    sim = _StubSim(BRAIN_NAMES if brain else TUMOR_NAMES)
    rf = ReducedFunctional(sim, n, lambda s, k: [])
    m = np.linspace(0.05, 0.3, n)
    J = rf(m)
    g = rf.derivative(m)
    assert sim.runs == 1   # fun + jac at one m: one forward (and one backward) run
    h = 1e-6
    num = np.array([(rf(m + h * e) - rf(m - h * e)) / (2 * h) for e in np.eye(n)])
    assert np.allclose(g, num, rtol=1e-7, atol=1e-10), (g, num)
    assert J == pytest.approx(rf(m))
    if brain and n in (2, 3):   # D_GM = 0.2 D_WM, rho_GM = rho_WM
        assert sim.params.D_GM == pytest.approx(0.2 * sim.params.D_WM)
        assert sim.params.rho_GM == pytest.approx(sim.params.rho_WM)
