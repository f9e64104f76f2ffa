"""
Displacement-image misfit terms, CPU side: the numpy statement of tests/displacement_image_common.py -- the reference of
glims_adjoint_displacement_image_terms -- against central differences of its own J (step and bar of
tests/test_observable_terms_cpu.py: relative step 1e-5, agreement 1e-6) and of its own gradient (eps = 1e-4, relative 1e-6:
tests/test_adjoint_hessian_elastic_cpu.py:54-62, the step and bar of the u_l2 products), the conditions the GPU tests rely on,
the invariants of the term, and the surface of the new entry points (no GPU).
"""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import displacement_image_common as dic
from test_observable_terms_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 3
REL_STEP, BAR = 1e-5, 1e-6          # tests/test_observable_terms_cpu.py:79-85
HESS_EPS, HESS_BAR = 1e-4, 1e-6     # tests/test_adjoint_hessian_elastic_cpu.py:54, :62
GPU_STEPS = 4                       # tests/test_gpu_displacement_image.py


def _problem(dim):
    return dic.clamped_problem(2, 9) if dim == 2 else dic.clamped_problem(3, 5)


@pytest.fixture(scope="module", params=[2, 3])
def setting(request):
    prob = _problem(request.param)
    return prob, dic.standard_terms(prob, N_STEPS, seed=request.param)


# ---- 1. the gradient against central differences of J ---------------------------------------------------------------------------
def test_numpy_gradient_matches_central_differences(setting):
    prob, terms = setting
    m = dic.base(prob)
    J, g = dic.gradient_at(prob, m, N_STEPS, terms)
    assert J > 0 and J == pytest.approx(dic.J_at(prob, m, N_STEPS, terms), rel=1e-13)
    L = prob.n_labels
    for i, key in enumerate(dic.KEYS):
        for l in range(L):
            e = np.zeros(L)
            e[l] = REL_STEP * abs(m[key][l])
            num = (dic.J_at(prob, dict(m, **{key: m[key] + e}), N_STEPS, terms) -
                   dic.J_at(prob, dict(m, **{key: m[key] - e}), N_STEPS, terms)) / (2 * e[l])
            ad = g[i * L + l]
            print("%d-D dJ/d%s[%d]: adjoint %.12e central differences %.12e" % (prob.dim, key, l, ad, num))
            assert ad != 0.0 and num != 0.0
            assert abs(ad - num) <= BAR * abs(num), (key, l, ad, num)
    p = np.random.default_rng(1).standard_normal(len(prob.points))
    h = REL_STEP
    num = (dic.J_at(prob, dict(m, c0=prob.c0 + h * p), N_STEPS, terms) -
           dic.J_at(prob, dict(m, c0=prob.c0 - h * p), N_STEPS, terms)) / (2 * h)
    ad = g[5 * L:] @ p
    assert ad != 0.0 and abs(ad - num) <= BAR * abs(num), (ad, num)


def test_displacement_image_terms_alone_carry_every_parameter(setting):
    """Without the nodal terms of the list: gamma, E and nu get their gradient from the displacement images alone."""
    prob, terms = setting
    only = dic.displacement_terms(terms)
    g = dic.gradient_at(prob, dic.base(prob), N_STEPS, only)[1]
    assert np.all(g[:5 * prob.n_labels] != 0.0)


# ---- 2. the products against central differences of the gradient -----------------------------------------------------------------
@pytest.mark.parametrize("keys", [None, ("E",), ("nu",)])
def test_numpy_products_match_central_differences_of_the_gradient(setting, keys):
    prob, terms = setting
    m = dic.base(prob)
    d = dic.random_direction(prob, 1)
    if keys is not None:
        d = {k: d[k] for k in keys}
    full = {k: (np.asarray(d[k]) if k in d else np.zeros_like(m[k])) for k in m}
    o = dic.oracle_of(prob)
    hv = dic.sweep(prob, o, prob.trajectory(o, N_STEPS), terms, [d])[2][0]
    ana = dic.flat(prob, hv)
    shift = lambda s: {k: m[k] + s * HESS_EPS * full[k] for k in m}
    num = (dic.gradient_at(prob, shift(1.0), N_STEPS, terms)[1] -
           dic.gradient_at(prob, shift(-1.0), N_STEPS, terms)[1]) / (2 * HESS_EPS)
    L = prob.n_labels
    for i, what in enumerate(dic.KEYS + ("c0",)):
        sl = slice(i * L, (i + 1) * L) if what != "c0" else slice(5 * L, None)
        err = np.linalg.norm(ana[sl] - num[sl]) / np.linalg.norm(num[sl])
        print("%d-D %s rows of H d (%s): relative error %.3e" % (prob.dim, what, keys, err))
        assert err <= HESS_BAR, (what, err, ana[sl][:4], num[sl][:4])


def test_numpy_per_label_matrix_is_symmetric(setting):
    from adjoint_hessian_elastic_common import unit_directions
    prob, terms = setting
    o = dic.oracle_of(prob)
    hv = dic.sweep(prob, o, prob.trajectory(o, N_STEPS), terms, unit_directions(prob))[2]
    H = np.array([np.concatenate([h[k] for k in dic.KEYS]) for h in hv]).T
    assert np.abs(H - H.T).max() <= 1e-9 * np.abs(H).max(), H


# ---- 3. what the GPU tests rely on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_conditions_of_the_gpu_tests(dim):
    prob = _problem(dim)
    terms = dic.standard_terms(prob, GPU_STEPS, seed=dim)        # the problems and seeds of tests/test_gpu_displacement_image.py
    warp = dic.displacement_terms(terms)
    assert len(warp) == 4 and any(t["scale"] != 1.0 for t in warp) and len({t["step"] for t in warp}) == 3
    assert any(t["pweight"] is not None and np.any(np.asarray(t["pweight"]) == 0.0) for t in warp)
    assert any(np.any(t["cweight"] == 0.0) and np.isnan(t["target"][:, t["cweight"] == 0.0]).any() and
               not np.isnan(t["target"][:, t["cweight"] != 0.0]).any() for t in warp)
    assert any(np.isnan(t["target"]).any() and np.all(t["cweight"] != 0.0) and (t["loc"][0] < 0).any() for t in warp)
    for t in warp:
        ok, _ = dic.observed(t)
        print("%d-D term at step %d: %d of %d points observed" % (dim, t["step"], ok.sum(), len(ok)))
        assert len(ok) / 2 <= ok.sum() < len(ok)
    o = dic.oracle_of(prob)
    assert dic.misfit(prob, o, prob.trajectory(o, GPU_STEPS), warp) > 0
    assert {t["kind"] for t in terms if t["step"] == GPU_STEPS} >= {"c_thresh", "u_l2", dic.KIND}


# ---- 4. invariants ----------------------------------------------------------------------------------------------------------------
def test_scale_zero_leaves_the_data_norm_and_no_gradient(setting):
    prob, terms = setting
    only = [dict(t, scale=0.0) for t in dic.displacement_terms(terms)]
    J, g = dic.gradient_at(prob, dic.base(prob), N_STEPS, only)
    want = 0.0
    for t in only:
        ok, q = dic.observed(t)
        d2 = np.where(t["cweight"][None] != 0.0, t["target"], 0.0) ** 2
        want += 0.5 * t["weight"] * np.sum(q[ok, None] * t["cweight"][None] * d2[ok])
    assert want > 0 and J == pytest.approx(want, rel=1e-14)
    assert not np.any(g)


def test_the_term_is_exactly_quadratic_in_u(setting):
    """J along a line u0 + s v has a zero third difference: |D3| <= 1e-12 of the sum of the |J| sampled (rounding alone)."""
    prob, terms = setting
    rng = np.random.default_rng(4)
    nd = prob.points.size
    u0, v = 0.05 * rng.standard_normal(nd), 0.05 * rng.standard_normal(nd)
    for t in dic.displacement_terms(terms):
        Js = np.array([dic.term_J(prob, t, u0 + s * v) for s in (0.0, 1.0, 2.0, 3.0)])
        d3 = Js[3] - 3 * Js[2] + 3 * Js[1] - Js[0]
        assert abs(d3) <= 1e-12 * np.abs(Js).sum(), (d3, Js)
        # and the load is the derivative of J, the second-order load that of the load
        h = 1e-6
        num = (dic.term_J(prob, t, u0 + h * v) - dic.term_J(prob, t, u0 - h * v)) / (2 * h)
        assert dic.term_load(prob, t, u0) @ v == pytest.approx(num, rel=1e-8)
        assert np.allclose(dic.term_second(prob, t, v), dic.term_load(prob, t, u0 + v) - dic.term_load(prob, t, u0),
                           rtol=0, atol=1e-13 * np.abs(dic.term_load(prob, t, u0)).max())


# ---- 5. surface ---------------------------------------------------------------------------------------------------------------------
FIELDS = ["step", "sampler", "weight", "scale", "cweight", "target", "pweight"]
NAMES = ("glims_adjoint_displacement_image_terms", "glims_adjoint_displacement_image_info")


def test_header_and_ctypes_carry_the_entry_points(tmp_path):
    from glimslib_amd import _backend
    lib = _backend.load_library()
    assert lib.glims_abi_version() == 6 == _backend.ABI_VERSION
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    assert re.search(r"#define\s+GLIMS_ABI_VERSION\s+6\b", src)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _backend.SIGNATURES, name
    body = re.search(r"typedef struct glims_displacement_image_misfit \{(.*?)\} glims_displacement_image_misfit;", src,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b([a-z_]+)\s*(?:\[\d+\])?\s*[,;]", body)
    assert fields == FIELDS == [f for f, _ in _backend.DisplacementImageMisfit._fields_], fields
    assert _backend.SIGNATURES[NAMES[0]][1][-1] == C.POINTER(_backend.DisplacementImageMisfit)
    # sizeof and offsetof as the C compiler lays the header's struct out
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glims_hip.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(glims_displacement_image_misfit));\n' +
                    "".join('  printf(" %%zu", offsetof(glims_displacement_image_misfit, %s));\n' % f for f in fields) +
                    '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([_compiler(), "-x", "c", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe],
                   check=True, timeout=180)
    nums = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert nums[0] == C.sizeof(_backend.DisplacementImageMisfit) == 72
    assert nums[1:] == [getattr(_backend.DisplacementImageMisfit, f).offset for f in fields]


def test_distributed_handle_refuses_displacement_image_terms():
    from glimslib_amd.parallel import DistributedHandle
    dh = DistributedHandle.__new__(DistributedHandle)         # (no ranks needed: the refusal comes before any collective)
    t = dict(step=0, kind="img_u_l2", sampler=None, target=np.zeros((1, 2)))
    with pytest.raises(NotImplementedError):
        dh.set_displacement_image_terms([t])
    with pytest.raises(NotImplementedError):
        dh.displacement_image_term_info(0)
    with pytest.raises(NotImplementedError):
        dh._local_terms([t])


def test_simulation_refusals_on_a_stub():
    from glimslib_amd import _backend
    from glimslib_amd.simulation.simulation_tumor_growth import TumorGrowth
    from glimslib_amd.utils.data_io import Image

    def stub(mechanics, handle=True):
        h = _backend.Handle.__new__(_backend.Handle) if handle else types.SimpleNamespace()
        h.dim = 2
        ns = types.SimpleNamespace(_backend=h, solver=types.SimpleNamespace(mechanics=mechanics),
                                   _component_weights=TumorGrowth._component_weights)
        ns._displacement_term_checks = lambda who: TumorGrowth._displacement_term_checks(ns, who)
        return ns

    scalar = Image(np.zeros((4, 5)), [0.0, 0.0], [1.0, 1.0])
    three = Image(np.zeros((4, 5, 3)), [0.0, 0.0], [1.0, 1.0], is_vector=True)
    good = Image(np.zeros((4, 5, 2)), [0.0, 0.0], [1.0, 1.0], is_vector=True)
    s = stub(True)
    with pytest.raises(ValueError, match="vector image"):
        TumorGrowth.displacement_image_term(s, 1, scalar)
    with pytest.raises(ValueError, match="channels"):
        TumorGrowth.displacement_image_term(s, 1, three)
    with pytest.raises(ValueError, match="components"):
        TumorGrowth.displacement_image_term(s, 1, good, components=(1.0, 0.0, 0.0))
    s = stub(False)
    with pytest.raises(ValueError, match="mechanics"):
        TumorGrowth.displacement_image_term(s, 1, good)
    with pytest.raises(ValueError, match="mechanics"):
        TumorGrowth.landmark_term(s, 1, np.zeros((3, 2)), np.zeros((3, 2)))
    s = stub(True, handle=False)
    with pytest.raises(NotImplementedError):
        TumorGrowth.displacement_image_term(s, 1, good)
    # image_term keeps refusing a vector image
    with pytest.raises(ValueError, match="scalar image"):
        TumorGrowth.image_term(stub(True), 1, good)


# ---- 6. the numpy twin of the public-API fit --------------------------------------------------------------------------------------
def test_numpy_fit_of_coupling_and_D():
    """The setting of the public-API fit of tests/test_gpu_displacement_image.py (displacement_image_common.FIT: the T2-like
    threshold image and the masked displacement image of the last step of a truth run), run with the numpy statement and
    scipy's L-BFGS-B from the displaced first guess.  Recorded recovery: 11 iterations, J 1.053e+01 -> 9.3e-26, relative errors of
    (coupling, D) (1.1e-14, 1.4e-13).  The bar B is the worst of them rounded up to the next power of ten: B = 1e-12
    (displacement_image_common.FIT["bar"]) -- the GPU fit uses the same B."""
    from scipy.optimize import minimize
    import deformed_volume_common as dvc
    from glimslib_amd import fenics_local as fenics
    F = dic.FIT
    mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
    pts, cells = np.asarray(mesh.points), np.asarray(mesh.cells)
    lab = dvc.fit_labels(mesh)
    truth = dvc.fit_problem(pts, cells, lab, *F["truth"])
    o = truth.oracle()
    c_true = truth.trajectory(o, F["steps"])[-1]
    terms = dic.fit_terms(truth, c_true, o.mech_solve(c_true))
    ok, q = dic.observed(terms[1])
    assert 0 < (q == 0).sum() and len(ok) / 2 <= ok.sum() < len(ok)

    def fun(m):
        p = dvc.fit_problem(pts, cells, lab, *m)
        oo = p.oracle()
        J, g, _ = dic.sweep(p, oo, p.trajectory(oo, F["steps"]), terms)
        return J, np.array([g["gamma"].sum(), g["D"].sum()])

    J0, g0 = fun(np.array(F["start"]))
    res = minimize(fun, np.array(F["start"]), jac=True, bounds=[F["bounds"]] * 2, method="L-BFGS-B", tol=F["tol"],
                   options=dict(F["options"], disp=False))
    t = np.array(F["truth"])
    err = np.abs(res.x - t) / t
    print("numpy fit to a threshold and a displacement image: %d iterations, J %.3e -> %.3e, (coupling, D) = %s, rel. error %s"
          % (res.nit, J0, res.fun, res.x, err))
    assert res.nit <= F["options"]["maxiter"]
    assert np.all(err <= F["bar"]), (res.x, err)
