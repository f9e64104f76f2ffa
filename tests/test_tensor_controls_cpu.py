"""
Tensor-field controls, the parts that need no GPU ("Anisotropic diffusion", section "Tangent fields"):
  1. the numpy statement tests/tensor_controls_common.tangent_gradient against central differences of the misfit in the ratio
     of a random-fibre family, the identity (tangent = TT gives D_t dJ/dD_t) and linearity in the tangent;
  2. data_io.tensor_from_fibres(derivative=True);
  3. the two new symbols in include/glims_hip.h and in _backend.SIGNATURES, the Python-side packing of tangent fields, and
     ReducedFunctional(tensor_controls=...) on a stub simulation;
  4. the scipy twin of examples/adjoint_fit_anisotropy_2D.py's fit -- its recovery error sets FIT_RATIO_BAR, the bar of the
     device fit in tests/test_gpu_tensor_controls.py;
  5. csrc/diffusion_tensor.h as the tangents use it, on the host through tests/diffusion_tangent_check.cpp (the host compiler
     alone, -Wall -Werror, plain and with -fsanitize=address,undefined).
"""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import anisotropic_common as ac
import tensor_controls_common as tc
from adjoint_common import Problem, many_tissues
from test_anisotropic_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The bar of the central-difference check: 10 x the worst distance measured (1.3e-8, in 3-D).  That distance is the
# difference's own rounding floor -- eps J / h with h = 1e-4 against a derivative of 1e-5 .. 1e-4 --, not the adjoint's error.
FD_BAR = 1e-7
# tangent = TT against D_t dJ/dD_t, and linearity: both are identities of the same sums (measured 2.4e-16 and 1.2e-15)
IDENTITY_BAR = 1e-13


def _cases():
    return (("2d", Problem(2, 17), 4), ("3d", Problem(3, 6), 4), ("tissues", many_tissues(2, 9, n=12, seed=5), 3))


# ---- 1. the numpy statement ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    """name -> (prob, N, terms, family, ratio, T, dT, oracle, trajectory): computed once, read by the tests below."""
    out = {}
    for name, prob, N in _cases():
        fam = tc.fibre_family(tc.random_directions(len(prob.cells), prob.dim, 21))
        ratio = 4.0
        T, dT = fam(ratio)
        o = ac.aniso_oracle(prob, T)
        out[name] = (prob, N, prob.terms(N, with_u=False), fam, ratio, T, dT, o, prob.trajectory(o, N))
    return out


@pytest.mark.parametrize("name", ["2d", "3d", "tissues"])
def test_tangent_gradient_matches_central_differences_in_the_ratio(solved, name):
    prob, N, terms, fam, ratio, T, dT, o, traj = solved[name]
    g = tc.tangent_gradient(prob, o, traj, terms, T, [dT])
    assert g.shape == (1, prob.n_labels)
    h = 1e-4
    fd = (ac.J_at(prob, prob.D, N, terms, fam(ratio + h)[0]) - ac.J_at(prob, prob.D, N, terms, fam(ratio - h)[0])) / (2 * h)
    err = abs(g.sum() - fd) / abs(fd)
    print("numpy dJ/dratio against central differences, %s: %.6e against %.6e, relative distance %.2e (bar %.0e)"
          % (name, g.sum(), fd, err, FD_BAR))
    assert err <= FD_BAR


@pytest.mark.parametrize("name", ["2d", "3d", "tissues"])
def test_tangent_equal_to_the_tensor_gives_D_times_dJ_dD(solved, name):
    prob, N, terms, fam, ratio, T, dT, o, traj = solved[name]
    dD = ac.adjoint(prob, o, traj, terms, T)[1]
    g = tc.tangent_gradient(prob, o, traj, terms, T, [T])[0]
    err = tc.rel(g, prob.D * dD)
    print("tangent = TT against D dJ/dD, %s: %.2e (bar %.0e)" % (name, err, IDENTITY_BAR))
    assert np.abs(dD).max() > 0 and err <= IDENTITY_BAR


@pytest.mark.parametrize("name", ["2d", "3d", "tissues"])
def test_tangent_gradient_is_linear_in_the_tangent(solved, name):
    prob, N, terms, fam, ratio, T, dT, o, traj = solved[name]
    X = tc.random_tangents(len(prob.cells), prob.dim, 2, seed=4)        # indefinite fields
    g = tc.tangent_gradient(prob, o, traj, terms, T, [X[0], X[1], X[0] + X[1], np.zeros_like(X[0])])
    err = tc.rel(g[2], g[0] + g[1])
    print("linearity in the tangent, %s: %.2e (bar %.0e)" % (name, err, IDENTITY_BAR))
    assert np.abs(g[0]).max() > 0 and err <= IDENTITY_BAR
    assert not np.any(g[3])


# ---- 2. tensor_from_fibres(derivative=True) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_fibre_tangent_is_the_derivative_of_the_fibre_tensor(dim):
    from glimslib_amd.utils.data_io import tensor_from_fibres
    e = np.random.default_rng(dim).standard_normal((40, dim))
    e[7] = 0.0                                                   # no direction: (I, 0)
    for normalise in (True, False):
        for r in (1.0, 2.5, 6.0, np.linspace(1.5, 9.0, 40)):
            T, dT = tensor_from_fibres(e, r, normalise=normalise, derivative=True)
            assert np.array_equal(T, tensor_from_fibres(e, r, normalise=normalise))       # the default call, bit for bit
            h = 1e-5
            fd = (tensor_from_fibres(e, r + h, normalise=normalise) - tensor_from_fibres(e, r - h, normalise=normalise)) / (2 * h)
            err = np.abs(dT - fd).max()
            assert err <= 1e-9, (normalise, r, err)
            assert np.abs(dT - np.swapaxes(dT, 1, 2)).max() <= 1e-15   # (as T itself: ((r - 1) e_a) e_b rounds once more)
            assert np.array_equal(T[7], np.eye(dim)) and not np.any(dT[7])
            if normalise:
                assert np.abs(np.trace(dT, axis1=1, axis2=2)).max() <= 1e-14
                # the closed form: s = d / (d + r - 1), dT = s' (I + (r - 1) e e^T) + s e e^T
                u = e[0] / np.linalg.norm(e[0])
                r0 = np.broadcast_to(r, (40,))[0]
                q = dim + r0 - 1.0
                want = -dim / q ** 2 * (np.eye(dim) + (r0 - 1.0) * np.outer(u, u)) + dim / q * np.outer(u, u)
                assert np.abs(dT[0] - want).max() <= 1e-14


def test_default_call_of_tensor_from_fibres_returns_an_array_with_todays_bits():
    """The statement of the function as it was before the `derivative` argument, written out."""
    from glimslib_amd.utils.data_io import tensor_from_fibres
    e = np.random.default_rng(9).standard_normal((25, 3))
    e[3] = 0.0
    for r in (6.0, np.linspace(0.5, 8.0, 25)):
        rr = np.broadcast_to(np.asarray(r, dtype=np.float64), (25,))
        norm = np.linalg.norm(e, axis=1)
        u = np.where(norm[:, None] > 0.0, e / np.where(norm > 0.0, norm, 1.0)[:, None], 0.0)
        U = np.eye(3)[None] + (rr - 1.0)[:, None, None] * u[:, :, None] * u[:, None, :]
        N = U * (3 / np.trace(U, axis1=1, axis2=2))[:, None, None]
        got = tensor_from_fibres(e, r)
        assert isinstance(got, np.ndarray) and np.array_equal(got, N)
        assert np.array_equal(tensor_from_fibres(e, r, normalise=False), U)


# ---- 3. the surface -----------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_and_bound():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+glims_set_diffusion_tensor_tangents\s*\(\s*glims_ctx\s*\*\s*h\s*,\s*int\s+K\s*,\s*const\s+double\s*\*"
                     r"\s*dT\s*\)\s*;", src)
    assert re.search(r"int\s+glims_adjoint_tensor_gradient\s*\(\s*glims_ctx\s*\*\s*h\s*,\s*int\s+K\s*,\s*int\s+n_labels\s*,"
                     r"\s*double\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"#define\s+GLIMS_DT_MAX_TANGENTS\s+4\b", src) and _backend.DT_MAX_TANGENTS == 4
    assert len(_backend.SIGNATURES["glims_set_diffusion_tensor_tangents"][1]) == 3
    assert len(_backend.SIGNATURES["glims_adjoint_tensor_gradient"][1]) == 4
    assert re.search(r"#define\s+GLIMS_ABI_VERSION\s+6\b", src) and _backend.ABI_VERSION == 6
    # appended: both come after every symbol the header had
    assert src.index("glims_set_diffusion_tensor_tangents") > src.index("glims_diffusion_tensor_info")


def test_tangent_fields_are_packed_like_the_tensor():
    from glimslib_amd._backend import pack_diffusion_tensor, pack_diffusion_tensor_tangents
    X = tc.random_tangents(7, 3, 3, seed=1)
    P = pack_diffusion_tensor_tangents(X, 7, 3)
    assert P.shape == (3, 7, 6) and P.flags.c_contiguous
    assert all(np.array_equal(P[k], pack_diffusion_tensor(X[k], 7, 3)) for k in range(3))
    assert np.array_equal(pack_diffusion_tensor_tangents(P, 7, 3), P)
    mixed = pack_diffusion_tensor_tangents([X[0], P[1], np.diag([1.0, -2.0, 0.0])], 7, 3)   # a list, any form per field
    assert np.array_equal(mixed[:2], P[:2]) and np.array_equal(mixed[2], np.tile([1.0, 0, 0, -2.0, 0, 0.0], (7, 1)))
    skew = X.copy()
    skew[1, 4, 0, 2] += 1e-3
    with pytest.raises(ValueError, match="cell 4 is not symmetric"):
        pack_diffusion_tensor_tangents(skew, 7, 3)
    for bad in (np.zeros((2, 6, 3, 3)), np.zeros((2, 7, 5)), np.zeros((7, 6)), [np.zeros((7, 2, 2))]):
        with pytest.raises(ValueError, match="shape"):
            pack_diffusion_tensor_tangents(bad, 7, 3)


class _StubSim:
    """What ReducedFunctional touches of a simulation: params, tensor_params, run, adjoint_gradient, _backend.stats."""

    def __init__(self, tensor_names=("ratio", "tilt")):
        self.params = types.SimpleNamespace(diffusion=0.1, proliferation=0.1, coupling=0.1)
        self.tensor_params = {n: 1.0 for n in tensor_names}
        self._backend = types.SimpleNamespace(stats=lambda: dict(steps=3))
        self.runs = 0

    def run(self, **kw):
        self.runs += 1

    def adjoint_gradient(self, terms):
        p, t = self.params, self.tensor_params
        return dict(J=1.0, diffusion=np.array([0.0, 1.0, 2.0]) * p.diffusion, proliferation=np.array([0.0, 10.0, 20.0]),
                    coupling=np.zeros(3), c0=np.zeros(4),
                    tensor={"ratio": np.array([0.0, 100.0, 200.0]) * t["ratio"], "tilt": np.array([0.0, -1.0, -2.0])})


def test_reduced_functional_orders_the_tensor_controls_last():
    from glimslib_amd.optimization import ReducedFunctional, minimize
    sim = _StubSim()
    rf = ReducedFunctional(sim, 2, lambda s, n: [], tensor_controls=("tilt", "ratio"))
    dJ = rf.derivative([0.5, 0.2, 7.0, 3.0])
    assert sim.params.diffusion == 0.5 and sim.params.proliferation == 0.2
    assert sim.tensor_params == dict(tilt=7.0, ratio=3.0)
    assert np.array_equal(dJ, [1.5, 30.0, -3.0, 900.0])          # model parameters, then the tensor controls in their order
    # a vector without tensor controls is a prefix
    plain = ReducedFunctional(_StubSim(), 2, lambda s, n: [])
    assert np.array_equal(plain.derivative([0.5, 0.2]), dJ[:2])
    with pytest.raises(ValueError, match="expected 4 controls"):
        rf.derivative([0.5, 0.2, 7.0])
    for bad in (("aspect",), ("ratio", "ratio")):
        with pytest.raises(ValueError, match="tensor_controls"):
            ReducedFunctional(_StubSim(), 2, lambda s, n: [], tensor_controls=bad)
    with pytest.raises(ValueError, match="tensor_controls"):      # no family: no names
        ReducedFunctional(_StubSim(tensor_names=()), 2, lambda s, n: [], tensor_controls=("ratio",))
    # first order only, refused before any run
    sim2 = _StubSim()
    rf2 = ReducedFunctional(sim2, 2, lambda s, n: [], tensor_controls=("ratio",))
    with pytest.raises(NotImplementedError, match="first order only"):
        rf2.hessian_matrix([0.5, 0.2, 3.0])
    with pytest.raises(NotImplementedError, match="first order only"):
        rf2.hessian([0.5, 0.2, 3.0], [1.0, 0.0, 0.0])
    assert sim2.runs == 0
    with pytest.raises(ValueError, match="bounds"):               # a ratio is not a rate
        minimize(rf2, [0.5, 0.2, 3.0])


def test_set_diffusion_tensor_family_builds_the_field_and_its_tangents():
    sim = ac.make_fit_sim(0.1, 0.1)
    labels = sim._labels()
    assert getattr(sim, "_tensor_family", None) is None and not sim.tensor_params
    sim.set_diffusion_tensor_family(tc.fit_family(labels), dict(ratio=6.0), ("ratio",))
    assert sim.tensor_params == dict(ratio=6.0)
    xm = sim.mesh.cell_midpoints()
    assert np.array_equal(sim._diffusion_tensor, ac.pack(ac.fit_tensor(xm, labels)))
    assert sim._diffusion_tangents.shape == (1, len(labels), 3)
    assert not np.any(sim._diffusion_tangents[0, labels != 1]) and np.all(sim._diffusion_tangents[0, labels == 1, 0] > 0)
    sim.tensor_params["ratio"] = 2.0                               # the next run builds from the present values
    sim._build_tensor_family()
    assert np.array_equal(sim._diffusion_tensor, ac.pack(tc.fit_family(labels)(dict(ratio=2.0), xm)[0]))
    for bad in (dict(theta=[1.0, 2.0], names=("ratio",)), dict(theta=dict(r=1.0), names=("ratio",)),
                dict(theta=[1.0] * 5, names=tuple("abcde")), dict(theta=[1.0, 1.0], names=("a", "a"))):
        with pytest.raises(ValueError):
            sim.set_diffusion_tensor_family(tc.fit_family(labels), **bad)
    with pytest.raises(ValueError, match="tangent fields"):        # one tangent per name
        sim.set_diffusion_tensor_family(lambda th, x: (np.eye(2), []), [1.0], ("ratio",))
    sim.set_diffusion_tensor(np.eye(2))                            # a plain field clears the family
    assert sim._tensor_family is None and sim._diffusion_tangents is None and not sim.tensor_params


# ---- 4. the scipy twin of the example's fit ------------------------------------------------------------------------------------
# The bar of the device fit in tests/test_gpu_tensor_controls.py, derived as FIT_BAR of tests/test_anisotropic_cpu.py.  The data
# are noise free and made by the model itself, so J = 0 at (D, rho, ratio) = (0.1, 0.1, 6) and the twin's own recovery error is
# the optimiser's (measured: 1.4e-10 after 33 evaluations).  The device's gradient is held to 1e-8 of this statement's; an error
# of that size -- relative to the gradient at the START of the fit, its largest value, and constant over the iterations, its
# worst case -- moves the point where L-BFGS-B stops by the amount the second run measures (FIT_RATIO_SHIFT_MEASURED; larger
# than FIT_BAR's 3.4e-8 because J is flat in the ratio: d^2 J / d ratio^2 is about 1e-4 of d^2 J / dD^2).  FIT_RATIO_BAR is
# that shift, rounded up to the next power of ten.
FIT_RATIO_TWIN_MEASURED = 1.4e-10
FIT_RATIO_SHIFT_MEASURED = 8.1e-6
FIT_RATIO_BAR = 1e-5


def test_scipy_twin_of_the_anisotropy_fit_recovers_the_three_parameters():
    err, r, n = tc.fit_twin()
    print("scipy twin of the anisotropy fit: (D, rho, ratio) = (%.10f, %.10f, %.8f), recovery error %.2e, J = %.2e, "
          "%d evaluations" % (r.x[0], r.x[1], r.x[2], err, r.fun, n))
    assert err <= 10 * FIT_RATIO_TWIN_MEASURED
    shift, r, n = tc.fit_twin(gradient_error=1e-8)
    print("scipy twin of the anisotropy fit, gradient off by 1e-8 of its initial size: recovery error %.2e" % shift)
    assert err < shift <= FIT_RATIO_BAR


# ---- 5. the header on the host -------------------------------------------------------------------------------------------------
def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run([_compiler(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I",
                    os.path.join(ROOT, "glimslib_amd", "csrc"), os.path.join(ROOT, "tests", "diffusion_tangent_check.cpp"), "-o", exe],
                   check=True, timeout=180)
    return exe


def test_tangent_helpers_on_the_host_plain_and_under_the_sanitizers(tmp_path):
    outs = []
    for name, extra in (("diffusion_tangent_check", ()),
                        ("diffusion_tangent_check_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))):
        r = subprocess.run([_build(tmp_path, name, extra)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout, r.stderr)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        assert "diffusion_tangent_check: ok" in r.stdout
        outs.append(r.stdout)
    assert outs[0] == outs[1]
