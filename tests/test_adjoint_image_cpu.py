"""
Image-space misfit terms, CPU side: the numpy statement of tests/adjoint_image_common.py -- the reference of
glims_adjoint_image_terms -- against central differences of its own J (the step sizes and bars of tests/test_adjoint_cpu.py and
tests/test_adjoint_hessian_cpu.py for the nodal kinds), and the ABI surface of the two new entry points (no GPU).
"""
import os
import re

import numpy as np
import pytest

from adjoint_common import Problem
from adjoint_image_common import (IMAGE_KINDS, adjoint, flat, gradient_at, hessian, misfit, observed, standard_terms)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 4


@pytest.fixture(scope="module")
def setting():
    prob = Problem(2, 8)          # 81 nodes, two tissues, Dirichlet c on x = 1
    assert len(prob.points) <= 100
    terms, _, _ = standard_terms(prob, N_STEPS)
    return prob, terms


def _J(prob, terms, D=None, rho=None, c0=None):
    o = prob.oracle(D, rho)
    return misfit(prob, o, prob.trajectory(o, N_STEPS, c0), terms)


def test_the_term_list_exercises_what_it_claims(setting):
    prob, terms = setting
    img = [t for t in terms if t["kind"] in IMAGE_KINDS]
    assert {t["kind"] for t in img} == set(IMAGE_KINDS) and {t["step"] for t in img} == {0, N_STEPS // 2, N_STEPS}
    for t in img:
        ok, q = observed(t)
        assert 2 * ok.sum() >= len(ok), "fewer than half of the points observed"
    g = img[0]
    ok, q = observed(g)
    assert (g["loc"][0] < 0).any() and np.isnan(g["target"]).any() and (q == 0).any() and (q[ok] != 1.0).any()


def test_numpy_image_adjoint_matches_central_differences(setting):
    prob, terms = setting
    o = prob.oracle()
    J, dD, drho, dc0 = adjoint(prob, o, prob.trajectory(o, N_STEPS), terms)
    assert J > 0 and J == pytest.approx(_J(prob, terms), rel=1e-14)

    def fd(fun, x0, h):
        g = np.zeros_like(x0)
        for i in range(len(x0)):
            e = np.zeros_like(x0)
            e[i] = h * abs(x0[i])
            g[i] = (fun(x0 + e) - fun(x0 - e)) / (2 * e[i])
        return g

    for name, ad in (("D", dD), ("rho", drho)):
        num = fd(lambda p: _J(prob, terms, **{name: p}), getattr(prob, name), 1e-5)
        assert np.linalg.norm(ad - num) <= 1e-6 * np.linalg.norm(num), (name, ad, num)
    p = np.random.default_rng(1).standard_normal(len(prob.points))
    h = 1e-5
    num = (_J(prob, terms, c0=prob.c0 + h * p) - _J(prob, terms, c0=prob.c0 - h * p)) / (2 * h)
    assert abs(dc0 @ p - num) <= 1e-6 * abs(num), (dc0 @ p, num)


def test_image_terms_alone_match_central_differences(setting):
    """No nodal term in the list: the image kinds carry the whole gradient."""
    prob, terms = setting
    img = [t for t in terms if t["kind"] in IMAGE_KINDS]
    o = prob.oracle()
    J, dD, drho, dc0 = adjoint(prob, o, prob.trajectory(o, N_STEPS), img)
    for name, ad in (("D", dD), ("rho", drho)):
        x0 = getattr(prob, name)
        num = np.zeros_like(x0)
        for i in range(len(x0)):
            e = np.zeros_like(x0)
            e[i] = 1e-5 * abs(x0[i])
            num[i] = (_J(prob, img, **{name: x0 + e}) - _J(prob, img, **{name: x0 - e})) / (2 * e[i])
        assert np.linalg.norm(ad - num) <= 1e-6 * np.linalg.norm(num), (name, ad, num)


def _direction(prob, seed):
    rng = np.random.default_rng(seed)
    return dict(D=prob.D * rng.uniform(-1, 1, prob.n_labels), rho=prob.rho * rng.uniform(-1, 1, prob.n_labels),
                c0=0.2 * rng.uniform(-1, 1, len(prob.points)) * (prob.c0 + 0.1))


def test_numpy_image_hessian_matches_central_differences_of_the_gradient(setting):
    prob, terms = setting
    d = _direction(prob, 1)
    o = prob.oracle()
    hv = hessian(prob, o, prob.trajectory(o, N_STEPS), terms, [d])[4][0]
    ana = flat(prob, hv)
    eps = 1e-4
    m = dict(D=prob.D, rho=prob.rho, c0=prob.c0)
    shift = lambda s: {k: m[k] + s * d[k] for k in m}
    num = (gradient_at(prob, shift(eps), N_STEPS, terms)[1] - gradient_at(prob, shift(-eps), N_STEPS, terms)[1]) / (2 * eps)
    L = prob.n_labels
    for what, sl in (("D", slice(0, L)), ("rho", slice(L, 2 * L)), ("c0", slice(2 * L, None))):
        err = np.linalg.norm(ana[sl] - num[sl]) / np.linalg.norm(num[sl])
        assert err <= 1e-6, (what, err, ana[sl][:4], num[sl][:4])


def test_numpy_image_hessian_is_symmetric(setting):
    prob, terms = setting
    L, n = prob.n_labels, len(prob.points)
    rng = np.random.default_rng(5)
    dirs = [{key: np.eye(L)[l]} for key in ("D", "rho") for l in range(L)] + [dict(c0=rng.uniform(-1, 1, n)) for _ in range(2)]
    o = prob.oracle()
    hv = hessian(prob, o, prob.trajectory(o, N_STEPS), terms, dirs)[4]
    V = np.array([flat(prob, d) for d in dirs])
    H = np.array([[flat(prob, hv[j]) @ V[i] for j in range(len(dirs))] for i in range(len(dirs))])
    assert np.abs(H - H.T).max() <= 1e-9 * np.abs(H).max(), H


def test_library_exports_the_image_entry_points_and_the_binding_mirrors_the_struct():
    import ctypes as C
    from glimslib_amd import _backend
    lib = _backend.load_library()
    assert lib.glims_abi_version() == 6
    for name in ("glims_adjoint_image_terms", "glims_adjoint_image_info"):
        assert hasattr(lib, name) and name in _backend.SIGNATURES, name
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    body = re.search(r"typedef struct glims_image_misfit \{(.*?)\} glims_image_misfit;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*?\s*([a-z_]+)\s*[;,]", body)
    assert fields == [f for f, _ in _backend.ImageMisfit._fields_], fields
    assert fields == ["step", "sampler", "kind", "level", "smooth", "weight", "target", "pweight"]

    class Mirror(C.Structure):   # the C layout, spelt out: int64, int64, int (+ padding), 3 doubles, 2 pointers
        _fields_ = [("step", C.c_int64), ("sampler", C.c_int64), ("kind", C.c_int), ("level", C.c_double),
                    ("smooth", C.c_double), ("weight", C.c_double), ("target", C.c_void_p), ("pweight", C.c_void_p)]

    assert C.sizeof(_backend.ImageMisfit) == C.sizeof(Mirror) == 64
    for f, _ in Mirror._fields_:
        assert getattr(_backend.ImageMisfit, f).offset == getattr(Mirror, f).offset, f
    assert (_backend.MISFIT_IMG_L2, _backend.MISFIT_IMG_THRESH) == (0, 1)


def test_numpy_fit_to_two_threshold_images_converges_within_the_iteration_cap():
    """The setting of the public-API fit of tests/test_gpu_adjoint_image.py (adjoint_image_common.FIT), run with the numpy
    statement and scipy's L-BFGS-B under the same options: it recovers (D, rho) to 1e-3 within the cap of 30 iterations."""
    from scipy.optimize import minimize
    from glimslib_amd import fenics_local as fenics
    import adjoint_image_common as aic
    F = aic.FIT
    mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
    pts, cells = np.asarray(mesh.points), np.asarray(mesh.cells)
    truth = aic.fit_problem(pts, cells, *F["truth"])
    terms = aic.fit_image_terms(truth, truth.trajectory(truth.oracle(), F["steps"])[-1])
    ok, _ = observed(terms[0])
    assert 2 * ok.sum() >= len(ok) and not ok.all()          # the grid overhangs the mesh

    def fun(m):
        p = aic.fit_problem(pts, cells, m[0], m[1])
        o = p.oracle()
        J, dD, drho, _ = adjoint(p, o, p.trajectory(o, F["steps"]), terms)
        return J, np.array([dD.sum(), drho.sum()])

    res = minimize(fun, np.array(F["start"]), jac=True, bounds=[F["bounds"]] * 2, method="L-BFGS-B", tol=F["tol"],
                   options=dict(F["options"], disp=False))
    assert res.nit <= F["options"]["maxiter"]
    assert np.all(np.abs(res.x - np.array(F["truth"])) <= 1e-3 * np.array(F["truth"])), res
