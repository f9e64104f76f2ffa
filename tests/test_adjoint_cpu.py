"""Discrete adjoint, CPU side: the ABI surface, the numpy reference adjoint against finite differences of the oracle, and the
chain rule of glimslib_amd.optimization's parameter maps (no GPU)."""
import os
import re

import numpy as np
import pytest

from adjoint_common import Problem, adjoint, misfit

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
