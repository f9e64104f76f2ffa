"""
Anisotropic diffusion, the parts that need no GPU ("Anisotropic diffusion"):
  1. the numpy statement of tests/anisotropic_common.py: the identity field is the oracle's K, the stretch identity
     (TT = diag(a^2, 1) on the mesh = the isotropic problem on the mesh with x / a), its adjoint against central differences
     of its J, its second-order adjoint against central differences of its gradient;
  2. csrc/diffusion_tensor.h on the host through tests/diffusion_tensor_check.cpp (the host compiler alone, -Wall -Werror,
     plain and with -fsanitize=address,undefined);
  3. the two new symbols in include/glims_hip.h and in _backend.SIGNATURES, and the Python-side refusals;
  4. the scipy twin of examples/anisotropic_growth_2D.py's fit on the numpy statement -- its recovery error sets the bar of the
     device fit in tests/test_gpu_anisotropic.py.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import anisotropic_common as ac
from adjoint_common import Problem, misfit
from adjoint_hessian_common import flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the numpy statement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_identity_field_is_the_oracles_stiffness(dim):
    prob = Problem(2, 9) if dim == 2 else Problem(3, 5)
    o = prob.oracle()
    K = ac.stiffness(o.points, o.cells, o.D, ac.identity_field(len(prob.cells), dim))
    assert abs(K - o.K).max() == 0.0
    a = ac.aniso_oracle(prob, ac.identity_field(len(prob.cells), dim))
    assert abs(a.S - o.S).max() == 0.0


def test_stretch_identity():
    """TT = diag(a^2, 1): with x = a x', grad = (1/a d/dx', d/dy), so grad phi_i^T TT grad phi_j on the mesh equals
    grad' phi_i . grad' phi_j on the squeezed mesh, and every cell volume is a times the squeezed one: M, Mrho, K, N(c) and
    with them the residual differ by the common factor a, the Newton iterates are the same.  Bar 1e-12 (the measured distance
    after 4 steps is 1.3e-16)."""
    a = 2.0
    prob = Problem(2, 17)
    T = ac.uniform_stretch(len(prob.cells), 2, a)
    oa = ac.aniso_oracle(prob, T)
    sq = Problem(2, 17)
    sq.points = prob.points / np.array([a, 1.0])
    oi = sq.oracle()
    assert abs(oa.S - a * oi.S).max() <= 1e-14 * abs(oa.S).max()
    ta, ti = prob.trajectory(oa, 4), sq.trajectory(oi, 4)
    e = max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(ta[1:], ti[1:]))
    print("stretch identity, numpy against numpy: %.2e" % e)
    assert e <= 1e-12


def _problem(dim):
    return Problem(2, 9) if dim == 2 else Problem(3, 5)


@pytest.mark.parametrize("dim", [2, 3])
def test_adjoint_matches_central_differences(dim):
    """dJ/dD of the numpy adjoint against (J(D + h e_t) - J(D - h e_t)) / 2h with h = 1e-5 D_t, random field of ratio <= 10.
    Bar 1e-8 (measured 2.5e-10 in 2-D, 2.6e-10 in 3-D)."""
    prob, N = _problem(dim), 4
    T = ac.random_spd(len(prob.cells), dim, seed=11)
    terms = prob.terms(N, with_u=False)
    o = ac.aniso_oracle(prob, T)
    dD = ac.adjoint(prob, o, prob.trajectory(o, N), terms, T)[1]
    fd = np.zeros(prob.n_labels)
    for t in range(prob.n_labels):
        h = 1e-5 * prob.D[t]
        e = np.zeros(prob.n_labels)
        e[t] = h
        fd[t] = (ac.J_at(prob, prob.D + e, N, terms, T) - ac.J_at(prob, prob.D - e, N, terms, T)) / (2 * h)
    err = np.linalg.norm(dD - fd) / np.linalg.norm(fd)
    print("numpy adjoint dJ/dD against central differences, %d-D: %.2e" % (dim, err))
    assert err <= 1e-8


# measured: the relative distance of H d to the central difference of the numpy gradient (printed by the test); the bar is
# 10 x that, and at most 1e-5
_HESS_MEASURED = {2: 4.4e-10, 3: 3.2e-11}


@pytest.mark.parametrize("dim", [2, 3])
def test_hessian_matches_central_differences_of_the_gradient(dim):
    prob, N = _problem(dim), 3
    T = ac.random_spd(len(prob.cells), dim, seed=12)
    terms = prob.terms(N, with_u=False)
    rng = np.random.default_rng(5)
    n, L = len(prob.points), prob.n_labels
    d = dict(D=prob.D * rng.uniform(-1, 1, L), rho=prob.rho * rng.uniform(-1, 1, L), gamma=np.zeros(L),
             c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1))
    o = ac.aniso_oracle(prob, T)
    hv = ac.hessian(prob, o, prob.trajectory(o, N), terms, [d], T)[5][0]
    Hd = np.concatenate([hv["D"], hv["rho"], hv["gamma"], hv["c0"]])
    m0 = dict(D=prob.D, rho=prob.rho, gamma=prob.gamma, c0=prob.c0)
    eps = 1e-5
    gp = ac.gradient_at(prob, {k: m0[k] + eps * d[k] for k in m0}, N, terms, T)[1]
    gm = ac.gradient_at(prob, {k: m0[k] - eps * d[k] for k in m0}, N, terms, T)[1]
    fd = (gp - gm) / (2 * eps)
    assert len(fd) == len(flat(prob, d))
    err = np.linalg.norm(Hd - fd) / np.linalg.norm(fd)
    print("numpy Hessian-vector product against central differences of the gradient, %d-D: %.2e" % (dim, err))
    assert err <= min(10 * _HESS_MEASURED[dim], 1e-5)


# ---- 2. the header on the host -------------------------------------------------------------------------------------------------
def _compiler():
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    return cxx


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run([_compiler(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I",
                    os.path.join(ROOT, "glimslib_amd", "csrc"), os.path.join(ROOT, "tests", "diffusion_tensor_check.cpp"), "-o", exe],
                   check=True, timeout=180)
    return exe


def test_header_on_the_host_plain_and_under_the_sanitizers(tmp_path):
    outs = []
    for name, extra in (("diffusion_tensor_check", ()),
                        ("diffusion_tensor_check_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        r = subprocess.run([_build(tmp_path, name, extra)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout, r.stderr)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        assert "diffusion_tensor_check: ok" in r.stdout
        outs.append(r.stdout)
    assert outs[0] == outs[1]


# ---- 3. ABI table and Python-side refusals ---------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_and_bound():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+glims_set_diffusion_tensor\s*\(\s*glims_ctx\s*\*\s*h\s*,\s*const\s+double\s*\*\s*T\s*\)\s*;", src)
    assert re.search(r"int\s+glims_diffusion_tensor_info\s*\(\s*const\s+glims_ctx\s*\*\s*h\s*,\s*int64_t\s+out\[2\]\s*,"
                     r"\s*double\s*\*\s*max_ratio\s*\)\s*;", src)
    assert len(_backend.SIGNATURES["glims_set_diffusion_tensor"][1]) == 2
    assert len(_backend.SIGNATURES["glims_diffusion_tensor_info"][1]) == 3
    assert _backend.ABI_VERSION == 6


def test_python_side_refusals_and_accepted_shapes():
    from glimslib_amd._backend import pack_diffusion_tensor
    from glimslib_amd.utils.data_io import tensor_from_fibres
    T = ac.random_spd(7, 3, seed=1)
    P = pack_diffusion_tensor(T, 7, 3)
    assert P.shape == (7, 6) and np.array_equal(P, ac.pack(T))
    assert np.array_equal(P[:, [0, 3, 5]], T[:, [0, 1, 2], [0, 1, 2]]) and np.array_equal(P[:, 4], T[:, 1, 2])
    assert np.array_equal(pack_diffusion_tensor(P, 7, 3), P)
    one = pack_diffusion_tensor(np.diag([4.0, 1.0]), 5, 2)
    assert one.shape == (5, 3) and np.array_equal(one, np.tile([4.0, 0.0, 1.0], (5, 1)))
    for bad in (np.zeros((7, 5)), np.zeros((6, 3, 3)), np.zeros((7, 2, 2)), np.zeros(6), np.zeros((3, 2))):
        with pytest.raises(ValueError, match="shape"):
            pack_diffusion_tensor(bad, 7, 3)
    with pytest.raises(ValueError, match="not symmetric"):
        pack_diffusion_tensor(np.array([[1.0, 0.5], [0.0, 1.0]]), 5, 2)
    skew = T.copy()
    skew[4, 0, 1] += 1e-3
    with pytest.raises(ValueError, match="cell 4 is not symmetric"):
        pack_diffusion_tensor(skew, 7, 3)
    # fibre tensors: ratio along / across, trace d
    e = np.array([[1.0, 1.0], [0.0, 2.0], [0.0, 0.0]])
    F = tensor_from_fibres(e, 5.0)
    w = np.linalg.eigvalsh(F)
    assert np.allclose(w[:2, 1] / w[:2, 0], 5.0) and np.allclose(np.trace(F, axis1=1, axis2=2), 2.0)
    assert np.allclose(F[2], np.eye(2))                     # no direction: the identity
    assert np.allclose(F[1] @ [0.0, 1.0], np.array([0.0, 1.0]) * w[1, 1])
    G = tensor_from_fibres(e[:2], 5.0, normalise=False)
    assert np.allclose(np.linalg.eigvalsh(G), [[1.0, 5.0], [1.0, 5.0]])


def test_tensor_image_sampling_replaces_outside_and_nan_voxels_by_the_identity():
    from glimslib_amd.utils.data_io import Image, tensor_image_at_points
    arr = np.zeros((3, 4, 3))                               # [y, x, component], spacing 1, origin (0, 0)
    arr[...] = [2.0, 0.5, 1.0]
    arr[1, 2] = [3.0, 0.0, 4.0]
    arr[2, 3, 1] = np.nan
    img = Image(arr, origin=(0.0, 0.0), spacing=(1.0, 1.0), is_vector=True)
    pts = np.array([[0.2, 0.1], [2.1, 0.9], [3.0, 2.0], [7.0, 1.0], [-0.6, 0.0]])
    T, n_out = tensor_image_at_points(img, pts)
    assert n_out == 3
    assert np.array_equal(T, [[2.0, 0.5, 1.0], [3.0, 0.0, 4.0], [1.0, 0.0, 1.0], [1.0, 0.0, 1.0], [1.0, 0.0, 1.0]])
    with pytest.raises(ValueError):
        tensor_image_at_points(Image(arr[..., :2], is_vector=True), pts)


# ---- 4. the scipy twin of the example's fit ------------------------------------------------------------------------------------
def fit_twin(gradient_error=0.0):
    """scipy's L-BFGS-B on the numpy statement, as glimslib_amd.optimization.minimize runs it on the device: (D, rho), one
    value each for both tissues, from the threshold images of the true run's final state, the tensor field given, started
    from FIT['start'].  gradient_error: a constant error of that size relative to |dJ/dm| at the start, added to every
    gradient.  Returns (largest relative recovery error, scipy's result)."""
    from scipy.optimize import minimize
    prob, T = ac.fit_problem()
    N = ac.FIT["steps"]
    o = ac.aniso_oracle(prob, T)
    terms = ac.fit_terms(prob.trajectory(o, N)[-1], N)
    tissue = np.array([0.0, 1.0, 1.0])
    g0 = []

    def fun(m):
        J, g = ac.gradient_at(prob, dict(D=m[0] * tissue, rho=m[1] * tissue, gamma=prob.gamma, c0=prob.c0), N, terms, T)
        g = np.array([g[:3].sum(), g[3:6].sum()])
        g0.append(np.linalg.norm(g))
        return J, g + gradient_error * g0[0] * np.array([1.0, -1.0]) / np.sqrt(2.0)

    r = minimize(fun, np.array(ac.FIT["start"]), jac=True, method="L-BFGS-B", bounds=[(0.005, 0.5)] * 2, tol=1e-16,
                 options=dict(maxiter=60, ftol=1e-16, gtol=1e-12))
    true = np.array([ac.FIT["D"], ac.FIT["rho"]])
    return float(np.abs(r.x / true - 1.0).max()), r


# The bar of the device fit in tests/test_gpu_anisotropic.py.  The data are noise free and made by the model itself, so J = 0 at
# the true parameters and the twin's own recovery error is the optimiser's (measured: 2.0e-11).  The device's gradient is
# held to 1e-8 of this statement's, relative to the gradient's size; an error of that size -- taken relative to the gradient at
# the START of the fit, its largest value, and constant over the iterations, its worst case -- moves the point where L-BFGS-B
# stops by the amount the second run below measures (FIT_SHIFT_MEASURED).  FIT_BAR is that shift, rounded up to the next
# power of ten.
FIT_TWIN_MEASURED = 2.0e-11
FIT_SHIFT_MEASURED = 3.4e-8
FIT_BAR = 1e-7


def test_scipy_twin_of_the_examples_fit_recovers_the_parameters():
    err, r = fit_twin()
    print("scipy twin of the fit: recovery error %.2e, J = %.2e, %d iterations" % (err, r.fun, r.nit))
    assert err <= 10 * FIT_TWIN_MEASURED
    shift, r = fit_twin(gradient_error=1e-8)
    print("scipy twin of the fit, gradient off by 1e-8 of its initial size: recovery error %.2e" % shift)
    assert err < shift <= FIT_BAR
