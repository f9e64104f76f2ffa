"""
Image terms in the deformed configuration, CPU side: the identity behind the location's load, the numpy statement of
tests/adjoint_deformed_common.py -- the reference of glims_adjoint_deformed_image_terms -- against central differences of its
own J (the step and the bar of tests/test_adjoint_image_cpu.py for the same construction: relative step 1e-5, agreement 1e-6),
and the ABI surface of the two new entry points (no GPU).
"""
import os
import re

import numpy as np
import pytest

import adjoint_deformed_common as adc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 6
REL_STEP, BAR = 1e-5, 1e-6          # tests/test_adjoint_image_cpu.py


@pytest.mark.parametrize("dim", [2, 3])
def test_location_identity_on_one_simplex(dim):
    """dv/dy_b = -w_b grad_y c for v = sum_a w_a(y) c_a with sum_a w_a y_a = x fixed: central differences in every vertex
    coordinate of one triangle / tetrahedron."""
    rng = np.random.default_rng(3 + dim)
    y = np.vstack([np.zeros(dim), np.eye(dim)]) + 0.2 * rng.uniform(-1, 1, (dim + 1, dim))
    c = rng.uniform(0, 1, dim + 1)
    w0 = rng.dirichlet(np.ones(dim + 1))
    x = w0 @ y

    def weights(yy):
        lam = np.linalg.solve((yy[1:] - yy[0]).T, x - yy[0])
        return np.concatenate([[1.0 - lam.sum()], lam])

    assert np.allclose(weights(y), w0, atol=1e-14)
    G = np.linalg.inv((y[1:] - y[0]).T)                    # rows: grad lambda_1..d
    grads = np.vstack([-G.sum(axis=0), G])
    gc = c @ grads
    ana = -w0[:, None] * gc[None, :]
    num = np.zeros_like(ana)
    h = 1e-6
    for b in range(dim + 1):
        for a in range(dim):
            e = np.zeros_like(y)
            e[b, a] = h
            num[b, a] = (weights(y + e) @ c - weights(y - e) @ c) / (2 * h)
    err = np.abs(ana - num).max() / np.abs(num).max()
    print("dim %d: identity against central differences: %.2e" % (dim, err))
    assert err <= 1e-8


@pytest.fixture(scope="module", params=[2, 3])
def setting(request):
    dim = request.param
    prob = adc.clamped_problem(dim, 16 if dim == 2 else 6)
    terms = adc.standard_terms(prob, N_STEPS, masked=True)
    o = adc.oracle_of(prob)
    traj = prob.trajectory(o, N_STEPS)
    res = adc.evaluate(prob, o, traj, terms)
    return prob, terms, o, traj, res


def test_the_problem_displaces_the_mesh_enough_to_matter(setting):
    prob, terms, o, traj, res = setting
    for t, info in zip([t for t in terms if adc.is_deformed(t)], res["info"]):
        moved, ratio = adc.displacement_matters(prob, t, o.mech_solve(traj[t["step"]]))
        print("dim %d, scale %.1f: %.0f %% of the found points change their cell, smallest ratio %.3f, %d of %d observed"
              % (prob.dim, t["scale"], 100 * moved, ratio, info["observed"], info["n_points"]))
        assert 2 * info["observed"] >= info["found"] > 0 and info["folded"] == 0
    g = [t for t in terms if adc.is_deformed(t)][0]
    assert res["info"][0]["found"] < res["info"][0]["n_points"], "the grid does not overhang the mesh"
    assert np.isnan(g["target"]).any() and (g["pweight"] == 0).any() and (g["pweight"] > 1.0).any()


def test_numpy_deformed_adjoint_matches_central_differences(setting):
    prob, terms, o, traj, res = setting
    J0, cells0 = adc.J_at(prob, terms, N_STEPS)
    assert res["J"] > 0 and res["J"] == pytest.approx(J0, rel=1e-13)
    worst = {}
    for name in ("D", "rho", "gamma", "E", "nu"):
        base = getattr(prob, name)
        for label in (0,) if name != "gamma" else (0, 1):
            e = np.zeros_like(base)
            e[label] = REL_STEP * abs(base[label])
            Jp, cp = adc.J_at(prob, terms, N_STEPS, **{name: base + e})
            Jm, cm = adc.J_at(prob, terms, N_STEPS, **{name: base - e})
            for a, b, c in zip(cells0, cp, cm):
                assert np.array_equal(a, b) and np.array_equal(a, c), "a point changed its cell at m +- eps (%s)" % name
            num = (Jp - Jm) / (2 * e[label])
            err = abs(res[name][label] - num) / abs(num)
            worst[name] = max(worst.get(name, 0.0), err)
            assert abs(num) > 0 and err <= BAR, (name, label, res[name][label], num, err)
    p = np.random.default_rng(1).standard_normal(len(prob.points))
    if prob.dir_c is not None:
        p[prob.dir_c[0]] = 0.0
    h = 1e-5
    Jp, cp = adc.J_at(prob, terms, N_STEPS, c0=prob.c0 + h * p)
    Jm, cm = adc.J_at(prob, terms, N_STEPS, c0=prob.c0 - h * p)
    for a, b, c in zip(cells0, cp, cm):
        assert np.array_equal(a, b) and np.array_equal(a, c), "a point changed its cell at c0 +- eps"
    num = (Jp - Jm) / (2 * h)
    worst["c0"] = abs(res["c0"] @ p - num) / abs(num)
    print("dim %d: numpy gradient against central differences: %s" % (prob.dim, {k: "%.1e" % v for k, v in worst.items()}))
    assert worst["c0"] <= BAR, (res["c0"] @ p, num)


def test_deformed_terms_alone_carry_gamma_E_and_nu(setting):
    """No u_l2 term in the list: the location's load is the only source of dJ/dgamma, dJ/dE and dJ/dnu."""
    prob, terms, o, traj, _ = setting
    only = [t for t in terms if adc.is_deformed(t)]
    res = adc.evaluate(prob, o, traj, only)
    for name in ("gamma", "E", "nu"):
        base = getattr(prob, name)
        e = np.zeros_like(base)
        e[0] = REL_STEP * abs(base[0])
        num = (adc.J_at(prob, only, N_STEPS, **{name: base + e})[0] - adc.J_at(prob, only, N_STEPS, **{name: base - e})[0]) \
            / (2 * e[0])
        assert res[name][0] != 0.0 and abs(res[name][0] - num) <= BAR * abs(num), (name, res[name][0], num)


def test_library_exports_the_deformed_entry_points_and_the_binding_mirrors_the_struct():
    import ctypes as C
    from glimslib_amd import _backend
    lib = _backend.load_library()
    assert lib.glims_abi_version() == 6 == _backend.ABI_VERSION
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    assert re.search(r"#define\s+GLIMS_ABI_VERSION\s+6\b", src)
    for name in ("glims_adjoint_deformed_image_terms", "glims_adjoint_deformed_image_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _backend.SIGNATURES, name
    body = re.search(r"typedef struct glims_deformed_image_misfit \{(.*?)\} glims_deformed_image_misfit;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*?\s*([a-z_]+)\s*(?:\[3\])?\s*[;,]", body)
    assert fields == [f for f, _ in _backend.DeformedImageMisfit._fields_], fields

    class Mirror(C.Structure):   # the C layout, spelt out
        _fields_ = [("step", C.c_int64), ("kind", C.c_int), ("level", C.c_double), ("smooth", C.c_double),
                    ("weight", C.c_double), ("scale", C.c_double), ("n_points", C.c_int64), ("xyz", C.c_void_p),
                    ("origin", C.c_double * 3), ("spacing", C.c_double * 3), ("size", C.c_int64 * 3),
                    ("target", C.c_void_p), ("pweight", C.c_void_p)]

    assert C.sizeof(_backend.DeformedImageMisfit) == C.sizeof(Mirror) == 152
    for f, _ in Mirror._fields_:
        assert getattr(_backend.DeformedImageMisfit, f).offset == getattr(Mirror, f).offset, f
