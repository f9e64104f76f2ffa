"""
Centre-of-mass misfit terms (glims_adjoint_observable_terms3) and seed controls, the parts that need no GPU:
  1. the numpy statement of tests/com_terms_common.py -- the reference of the device path -- against central differences of its
     own J in D, rho (reference configuration) and gamma, E, nu (deformed) per label and a c0 direction, with the step and the
     bar of tests/test_observable_terms_cpu.py and tests/test_deformed_volume_cpu.py (h = 1e-5 relative, agreement 1e-6), the
     terms together and each centre-of-mass term alone, in 2-D and 3-D; the conditions the GPU tests rely on; invariants;
  2. the first-moment templates of csrc/observe_grad.h, run on the host through tests/observe_moment_grad_check.cpp (the host
     compiler alone, -Wall -Werror, and once more with the address and undefined-behaviour sanitizers), against the numpy
     statement and central differences of glims_oc_*;
  3. the surface: header, ctypes table, exported symbols, the struct's size and offsets on both sides, the refusing
     DistributedHandle, ReducedFunctional(iv_controls=...) on a stub simulation;
  4. the numpy twin of the public-API fit of tests/test_gpu_com_terms.py.
"""
import ctypes as C
import itertools
import os
import re
import subprocess
import types

import numpy as np
import pytest

import com_terms_common as cc
import deformed_volume_common as dvc
import observable_terms_common as otc
import observe_common as oc
from test_observable_terms_cpu import _compiler
from test_observe_cpu import LEVELS, SIMPLEX, VALUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 3
REL_STEP, BAR = 1e-5, 1e-6          # tests/test_observable_terms_cpu.py, tests/test_deformed_volume_cpu.py


# ---- 1. the numpy statement ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(2, False), (2, True), (3, False), (3, True)], ids=["2d", "2d-deformed", "3d", "3d-deformed"])
def setting(request):
    dim, deformed = request.param
    prob = dvc.clamped_problem(dim, 9 if dim == 2 else 5)
    o = dvc.oracle_of(prob)
    traj = prob.trajectory(o, N_STEPS)
    terms = cc.standard_terms(prob, traj, o.mech_solve, seed=dim, deformed=deformed)
    lists = [terms] + [[t] for t in terms if t["kind"] == cc.KIND]
    return prob, o, traj, lists, deformed


def _conditions(prob, o, traj, terms):
    """What the bars rely on: the gap rule for SHARP, |r| >= 1e-2 diameter, V > 0"""
    diam = cc.diameter(prob)
    for t in [t for t in terms if t["kind"] == cc.KIND]:
        c = traj[t["step"]]
        u = o.mech_solve(c) if t.get("deformed") else None
        _, X, V, _, empty = cc.com_of(prob, t, c, u)
        assert V > 0 and not empty
        assert np.linalg.norm(X - t["target"]) >= 1e-2 * diam, (X, t["target"])
        if t["observable"] == "sharp":
            assert np.abs(c - t["level"]).min() >= 1e-2
            assert otc.cut_cells(prob, t, c) >= 1


def test_the_term_list_exercises_what_it_claims(setting):
    prob, o, traj, lists, deformed = setting
    terms = lists[0]
    assert [(t["kind"], t.get("observable"), bool(t.get("deformed"))) for t in terms] == \
        [(cc.KIND, "smooth", deformed), (cc.KIND, "sharp", deformed), (cc.KIND, "mass", deformed), (cc.VOLUME, "smooth", deformed),
         (cc.KIND, "mass", deformed), ("c_thresh", None, False)]
    assert terms[2]["labels"] is not None and terms[0]["labels"] is None and terms[1]["step"] != terms[0]["step"]
    _conditions(prob, o, traj, terms)
    res = cc.evaluate(prob, o, traj, terms)
    assert res["mech_steps"] == (2 if deformed else 0)


def test_conditions_hold_on_the_problems_of_the_gpu_tests():
    """tests/test_gpu_com_terms.py runs clamped_problem(2, 9) and (3, 5) for N = 4 steps with the seeds below."""
    for dim in (2, 3):
        prob = dvc.clamped_problem(dim, 9 if dim == 2 else 5)
        o = dvc.oracle_of(prob)
        traj = prob.trajectory(o, 4)
        for seed, deformed in ((dim, False), (dim, True), (dim + 10, False), (5, False), (9, True), (7, True)):
            _conditions(prob, o, traj, cc.standard_terms(prob, traj, o.mech_solve, seed=seed, deformed=deformed))


def test_numpy_adjoint_matches_central_differences(setting):
    prob, o, traj, lists, deformed = setting
    res = [cc.evaluate(prob, o, traj, terms) for terms in lists]
    J0 = cc.J_of_lists(prob, lists, N_STEPS)
    for r, j in zip(res, J0):
        assert r["J"] > 0 and r["J"] == pytest.approx(j, rel=1e-13)
    worst = {}
    for name in ("D", "rho") + (("gamma", "E", "nu") if deformed else ()):
        base = getattr(prob, name)
        for label in range(prob.n_labels):
            e = np.zeros_like(base)
            e[label] = REL_STEP * abs(base[label])
            num = (cc.J_of_lists(prob, lists, N_STEPS, **{name: base + e}) -
                   cc.J_of_lists(prob, lists, N_STEPS, **{name: base - e})) / (2 * e[label])
            for k, r in enumerate(res):
                err = abs(r[name][label] - num[k]) / abs(num[k])
                worst[name] = max(worst.get(name, 0.0), err)
                assert abs(num[k]) > 0 and err <= BAR, (name, label, k, r[name][label], num[k], err)
    if not deformed:
        for r in res:
            assert not any(np.any(r[k]) for k in ("gamma", "E", "nu"))
    p = np.random.default_rng(1).standard_normal(len(prob.points))
    if prob.dir_c is not None:
        p[prob.dir_c[0]] = 0.0
    h = 1e-5
    num = (cc.J_of_lists(prob, lists, N_STEPS, c0=prob.c0 + h * p) - cc.J_of_lists(prob, lists, N_STEPS, c0=prob.c0 - h * p)) / (2 * h)
    for k, r in enumerate(res):
        err = abs(r["c0"] @ p - num[k]) / abs(num[k])
        worst["c0"] = max(worst.get("c0", 0.0), err)
        assert err <= BAR, (k, r["c0"] @ p, num[k])
    print("dim %d%s: numpy gradient against central differences, the worst of %d lists: %s"
          % (prob.dim, " deformed" if deformed else "", len(lists), {k: "%.1e" % v for k, v in worst.items()}))


def test_fast_moments_equal_the_cell_loop(setting):
    prob, o, traj, lists, deformed = setting
    for t in [t for t in lists[0] if t["kind"] == cc.KIND and t["observable"] != "sharp"]:
        c = traj[t["step"]]
        u = o.mech_solve(c) if deformed else None
        (V, M), (Vf, Mf) = cc.moments(prob, t, c, u), cc.fast_moments(prob, t, c, u)
        assert abs(V - Vf) <= 1e-13 * abs(V) and np.abs(M - Mf).max() <= 1e-13 * np.abs(M).max()


def test_invariants_of_the_statement(setting):
    prob, o, traj, lists, deformed = setting
    N = N_STEPS
    c = traj[N]
    u = o.mech_solve(c) if deformed else None
    kw = dict(deformed=True, scale=0.7) if deformed else {}
    target = np.full(prob.dim, 0.45)
    # the centre of mass of a MASS term is homogeneous of degree 0 in c
    t = cc.com_term(N, "mass", target, weight=1.3, **kw)
    J, X, V, alpha, empty = cc.com_of(prob, t, c, u)
    g, gu = cc.com_parts(prob, t, c, u, alpha, X)
    assert np.abs(g).max() > 0 and abs(c @ g) <= 1e-12 * (np.abs(c) @ np.abs(g))
    # a SHARP term below every concentration measures the cells themselves: no c-gradient
    t = cc.com_term(N, "sharp", target, level=-1.0, **kw)
    J, X, V, alpha, empty = cc.com_of(prob, t, c, u)
    g, gu = cc.com_parts(prob, t, c, u, alpha, X)
    assert not np.any(g) and J > 0
    if deformed:
        # a translation moves the centre of mass with it: sum_n dX_a/du_n,b = scale delta_ab, so sum_n dJ/du_n = scale w r
        for kind, lv, sm in (("mass", 0.0, 1.0), ("smooth", 0.3, 0.08), ("sharp", otc.gap_level(c)[0], 1.0)):
            t = cc.com_term(N, kind, target, level=lv, smooth=sm, weight=1.3, **kw)
            J, X, V, alpha, empty = cc.com_of(prob, t, c, u)
            g, gu = cc.com_parts(prob, t, c, u, alpha, X)
            tot = gu.reshape(-1, prob.dim).sum(axis=0)
            want = 0.7 * 1.3 * (X - target)
            assert np.abs(tot - want).max() <= 1e-12 * np.abs(want).max(), (kind, tot, want)
    else:
        assert not np.any(gu)


def test_an_empty_measure_gives_nothing(setting):
    prob, o, traj, lists, deformed = setting
    empty = cc.com_term(N_STEPS, "sharp", np.full(prob.dim, 0.3), level=2.0 * max(c.max() for c in traj), weight=3.0)
    res = cc.evaluate(prob, o, traj, [empty])
    assert res["J"] == 0.0 and res["info"][0]["empty"] and not any(np.any(res[k]) for k in ("D", "rho", "gamma", "E", "nu", "c0"))


# ---- 2. the header on the host -------------------------------------------------------------------------------------------------
def _cases():
    """(d, kind, level, smooth, c, psi, tag): all three kinds, every in-count of SHARP with every vertex in every role (the
    2-in / 2-out prism among them), vertex ties"""
    rng = np.random.default_rng(3)
    cases = []
    for d in (2, 3):
        for perm in itertools.permutations(VALUES[d]):
            psi = rng.uniform(-1, 1, d + 1)
            for n_in, level in enumerate(LEVELS[d]):
                assert oc.in_count(perm, level) == n_in
                cases.append((d, "sharp", level, 1.0, perm, psi, "in%d" % n_in))
            for v in VALUES[d]:                                            # a tie: that vertex counts as in
                cases.append((d, "sharp", v, 1.0, perm, psi, "tie"))
            cases.append((d, "mass", 0.0, 1.0, perm, psi, "mass"))
            cases.append((d, "smooth", 0.45, 0.2, perm, psi, "smooth"))
            cases.append((d, "smooth", 0.8, 0.05, perm, psi, "smooth"))
        cases.append((d, "sharp", 0.3, 1.0, [0.3] * (d + 1), np.ones(d + 1), "all_equal"))
        cases.append((d, "sharp", 0.3, 1.0, [0.3, 0.3] + [0.1] * (d - 1), np.ones(d + 1), "two_ties"))
    return cases


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run([_compiler(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I",
                    os.path.join(ROOT, "glimslib_amd", "csrc"), os.path.join(ROOT, "tests", "observe_moment_grad_check.cpp"),
                    "-o", exe], check=True, timeout=180)
    return exe


def _run(exe, cases):
    lines = []
    for d, kind, level, smooth, c, psi, _ in cases:
        nums = [level, smooth] + [float(v) for v in c] + [float(v) for v in psi]
        lines.append("%d %d " % (d, oc.KIND_ID[kind]) + " ".join(repr(float(v)) for v in nums))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    rows = [np.array([float(v) for v in line.split()]) for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def _numpy_cell(d, kind, level, smooth, c, psi):
    """(b [d+2], g [d+1]) of the numpy statement in barycentric units: b from observe_cell on the unit simplex, g from the
    phi-weighted gradient on the well-shaped simplex of tests/test_observe_cpu.py divided by its |T| (phi_m = psi_m)."""
    p = SIMPLEX[d]
    T = abs(oc._vol(p.tolist()))
    nv = d + 1
    c, psi = np.asarray(c, dtype=np.float64), np.asarray(psi, dtype=np.float64)
    b = cc.unit_moments(c, kind, level, smooth)
    if kind == "mass":
        g = (psi.sum() + psi) / (nv * (nv + 1))
    elif kind == "smooth":
        lam, w = oc._rule(d)
        g = (w * otc.dthresh(lam @ c, level, smooth) * (lam @ psi)) @ lam
    else:
        g = cc.sharp_cell_weighted_grad(p, c, level, psi) / T
    return b, g


def test_moment_header_on_the_host_plain_and_under_the_sanitizers(tmp_path):
    """The first-moment templates against the numpy per-cell statement and against central differences of glims_oc_*'s own
    values (the program prints both sets of values).

    Tolerances.  tests/test_observe_cpu.py bounds the error of the b by 64 * 2^-52; the header's b must equal glims_oc_*'s to
    that.  g_i = sum_m psi_m d b[1+m] / d c_i with |psi| <= 1 is a sum of d+1 derivatives, each of the size and rounding of
    d b0 / d c_i of tests/test_observable_terms_cpu.py: 64 (d+1) 2^-52 / gap for SHARP (gap = the smallest c_a - c_o over the cut
    edges), 64 (d+1) 2^-52 / smooth for SMOOTH, 64 (d+1) 2^-52 for MASS.  Central differences of step h = 1e-6 on values with
    third derivatives of size 1 / gap^3 (1 / smooth^3) and rounding 2^-52 / h: 1e-7, on the cases whose in / out pattern the
    step cannot change.  The sanitizer build must run the same cases clean and print the same numbers."""
    cases = _cases()
    exe = _build(tmp_path, "observe_moment_grad_check")
    rows = _run(exe, cases)
    worst = {}
    fd_cases, fd_index = [], []
    h = 1e-6
    for k, ((d, kind, level, smooth, c, psi, tag), got) in enumerate(zip(cases, rows)):
        nv = d + 1
        b, g, n_in, o = got[:nv + 1], got[nv + 1:2 * nv + 1], int(got[2 * nv + 1]), got[2 * nv + 2:]
        assert np.abs(b - o).max() <= 64 * oc.EPS, (d, kind, level, c, tag, b, o)
        assert abs(b[1:].sum() - b[0]) <= 64 * oc.EPS
        want_b, want_g = _numpy_cell(d, kind, level, smooth, c, psi)
        assert np.abs(b - want_b).max() <= 64 * oc.EPS, (d, kind, level, c, tag, b, want_b)
        if kind == "sharp":
            assert n_in == oc.in_count(c, level)
            ins = [v for v in c if v >= level]
            outs = [v for v in c if not v >= level]
            gap = min((a - bb for a in ins for bb in outs), default=1.0)
            tol = 64 * nv * oc.EPS / gap
            if n_in in (0, nv):
                assert not np.any(g), (d, level, c, g)
        else:
            assert n_in == -1
            gap = smooth if kind == "smooth" else 1.0
            tol = 64 * nv * oc.EPS / gap
        err = np.abs(g - want_g).max()
        worst[(d, tag)] = max(worst.get((d, tag), 0.0), err / tol)
        assert err <= tol, (d, kind, level, c, tag, err / tol, g, want_g)
        if tag in ("tie", "all_equal", "two_ties"):
            continue                                                      # (a step changes the in / out pattern there)
        for i in range(nv):
            for s in (1.0, -1.0):
                cp = np.array(c, dtype=np.float64)
                cp[i] += s * h
                fd_cases.append((d, kind, level, smooth, cp, psi, tag))
            fd_index.append((k, i))
    fd_rows = _run(exe, fd_cases)
    for j, (k, i) in enumerate(fd_index):
        d, kind, level, smooth, c, psi, tag = cases[k]
        nv = d + 1
        up, dn = fd_rows[2 * j][2 * nv + 3:], fd_rows[2 * j + 1][2 * nv + 3:]
        num = (np.asarray(psi) @ up - np.asarray(psi) @ dn) / (2 * h)
        g = rows[k][nv + 1 + i]
        assert abs(g - num) <= 1e-7, (d, kind, level, c, tag, i, g, num)
    print({k: "%.3f of the bound" % v for k, v in sorted(worst.items())})
    san = _build(tmp_path, "observe_moment_grad_check_san", extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rows_san = _run(san, cases)
    for a, b in zip(rows, rows_san):
        assert np.allclose(a, b, rtol=1e-13, atol=1e-13)


# ---- 3. the surface ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_carry_the_struct_and_entry_points(tmp_path):
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _backend.load_library()
    assert lib.glims_abi_version() == _backend.ABI_VERSION == 6
    for name in ("glims_adjoint_observable_terms3", "glims_adjoint_observable_info3"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _backend.SIGNATURES
        assert hasattr(lib, name)
    assert "Not built: centre-of-mass" not in src
    body = re.search(r"typedef struct glims_observable_misfit3 \{(.*?)\} glims_observable_misfit3;", code, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*(?:\[\d+\])?\s*[,;]", body)
    assert fields == [f for f, _ in _backend.ObservableMisfit3._fields_]
    assert fields == ["step", "kind", "level", "smooth", "weight", "target", "labels", "deformed", "scale", "moment", "target_x"]
    assert _backend.SIGNATURES["glims_adjoint_observable_terms3"][1][-1] == C.POINTER(_backend.ObservableMisfit3)
    # sizeof and offsetof as the C compiler lays the header's struct out
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glims_hip.h"\nint main(void) {\n'
                    '  printf("%zu", sizeof(glims_observable_misfit3));\n' +
                    "".join('  printf(" %%zu", offsetof(glims_observable_misfit3, %s));\n' % f for f in fields) +
                    '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([_compiler(), "-x", "c", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe],
                   check=True, timeout=180)
    nums = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert nums[0] == C.sizeof(_backend.ObservableMisfit3) == 104
    assert nums[1:] == [getattr(_backend.ObservableMisfit3, f).offset for f in fields]


def test_distributed_handle_refuses_centre_of_mass_terms():
    from glimslib_amd.parallel import DistributedHandle
    dh = DistributedHandle.__new__(DistributedHandle)         # (no ranks needed: the refusal comes before anything else)
    t = cc.com_term(0, "mass", [0.5, 0.5])
    with pytest.raises(NotImplementedError):
        dh.set_observable_terms([t])
    with pytest.raises(NotImplementedError):
        dh.observable_term_info3(0)
    with pytest.raises(NotImplementedError):
        dh._local_terms([t])


class _StubSim:
    """What ReducedFunctional touches of a simulation: params with the initial-value Expression, the mesh points, run(), the
    backend's step count and adjoint_gradient -- here J = 1/2 |c0 - d|^2 of the nodal interpolant itself."""

    def __init__(self, iv, points, data):
        fs = types.SimpleNamespace(has_subspaces=True)
        self.params = types.SimpleNamespace(_functionspace=fs, get_iv=lambda sid: iv if sid == 1 else None, diffusion=0.1,
                                            proliferation=0.1, coupling=0.1)
        self.mesh = types.SimpleNamespace(points=points)
        self._backend = types.SimpleNamespace(stats=lambda: dict(steps=0))
        self.iv, self.data, self.runs = iv, data, 0

    def run(self, **kw):
        self.runs += 1

    def adjoint_gradient(self, terms):
        r = self.iv(self.mesh.points) - self.data
        z = np.zeros(1)
        return dict(J=0.5 * float(r @ r), diffusion=z, proliferation=z, coupling=z, c0=r)


def test_iv_controls_on_a_stub_simulation():
    """For the Gaussian exp(-a |x - x_seed|^2), dc0/dx0 by the central difference agrees with 2 a (x - x0) c0 to 1e-7: with
    h = 1e-6 the truncation h^2 |d3 c0 / dx0^3| / 6 <= 1e-12 and the rounding eps / h = 2e-10 are both below 1e-9."""
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.optimization import ReducedFunctional
    a, x0, y0 = 0.5, 0.3, -0.2
    iv = fenics.Expression('exp(-a*(pow(x[0]-x0,2)+pow(x[1]-y0,2)))', degree=1, a=a, x0=x0, y0=y0)
    pts = np.random.default_rng(0).uniform(-3, 3, (200, 2))
    data = np.exp(-a * ((pts[:, 0] - 0.8) ** 2 + (pts[:, 1] - 0.4) ** 2))
    sim = _StubSim(iv, pts, data)
    rf = ReducedFunctional(sim, 2, lambda s, n: [], names=("diffusion", "proliferation"), iv_controls=("x0", "y0"))
    c0 = iv(pts)
    for name, col, p in (("x0", 0, x0), ("y0", 1, y0)):
        d = rf.iv_derivative(name)
        assert np.abs(d - 2 * a * (pts[:, col] - p) * c0).max() <= 1e-7
        assert getattr(iv, name) == p                                  # left as it was
    m = np.array([0.1, 0.1, x0, y0])
    J = rf(m)
    dJ = rf.derivative(m)
    assert sim.runs == 1 and dJ.shape == (4,) and not np.any(dJ[:2])
    r = c0 - data
    assert J == pytest.approx(0.5 * r @ r, rel=1e-14)
    assert dJ[2] == pytest.approx(r @ (2 * a * (pts[:, 0] - x0) * c0), rel=1e-7)
    assert dJ[3] == pytest.approx(r @ (2 * a * (pts[:, 1] - y0) * c0), rel=1e-7)
    rf(np.array([0.1, 0.1, 0.5, 0.1]))                                 # the controls reach the Expression
    assert (iv.x0, iv.y0) == (0.5, 0.1) and sim.runs == 2
    with pytest.raises(NotImplementedError):
        rf.hessian_matrix(m)
    with pytest.raises(NotImplementedError):
        rf.hessian(m, np.ones(4))
    with pytest.raises(ValueError):
        rf(np.array([0.1, 0.1]))
    with pytest.raises(ValueError):
        ReducedFunctional(sim, 2, lambda s, n: [], names=("diffusion", "proliferation"), iv_controls=("x0", "z0"))
    with pytest.raises(ValueError):
        ReducedFunctional(sim, 2, lambda s, n: [], names=("diffusion", "proliferation"), iv_controls=("x0", "x0"))


# ---- 4. the numpy twin of the public-API fit ------------------------------------------------------------------------------------
def test_numpy_fit_of_seed_D_and_rho():
    """The setting of the public-API fit of tests/test_gpu_com_terms.py (com_terms_common.FIT: two SMOOTH volume series and two
    SMOOTH centre-of-mass series of the whole domain at five steps), run with the numpy statement and scipy's L-BFGS-B from the
    displaced first guess.  Recorded recovery: 19 iterations, errors (x0, y0 absolute; D, rho relative)
    (4.2e-13, 4.3e-13, 3.9e-12, 1.7e-12).  The bar B is the worst of them rounded up to the next power of ten:
    B = 1e-11 (com_terms_common.FIT["bar"]) -- the GPU fit uses the same B."""
    from scipy.optimize import minimize
    from glimslib_amd import fenics_local as fenics
    F = cc.FIT
    mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
    pts, cells = np.asarray(mesh.points), np.asarray(mesh.cells)
    truth = cc.fit_problem(pts, cells, F["truth"])
    traj = truth.trajectory(truth.oracle(), F["steps"])

    def make_volume(k, lv):
        t = otc.volume_term(k, "smooth", 0.0, level=lv, smooth=F["smooth"])
        t["target"] = cc.fast_moments(truth, t, traj[k])[0]
        return t

    def make_com(k, lv):
        t = cc.com_term(k, "smooth", np.zeros(2), level=lv, smooth=F["smooth"], weight=F["com_weight"])
        V, M = cc.fast_moments(truth, t, traj[k])
        t["target"] = M / V
        return t

    terms = cc.fit_terms(make_volume, make_com)
    path = []

    def fun(m):
        p = cc.fit_problem(pts, cells, m)
        o = p.oracle()
        r = cc.evaluate(p, o, p.trajectory(o, F["steps"]), terms, fast=True)
        c0 = p.c0
        dx = 2 * F["a"] * (pts[:, 0] - m[0]) * c0
        dy = 2 * F["a"] * (pts[:, 1] - m[1]) * c0
        path.append(np.array(m))
        return r["J"], np.array([r["c0"] @ dx, r["c0"] @ dy, r["D"].sum(), r["rho"].sum()])

    res = minimize(fun, np.array(F["start"]), jac=True, bounds=list(zip(F["lo_bounds"], F["hi_bounds"])), method="L-BFGS-B",
                   tol=F["tol"], options=dict(F["options"], disp=False))
    t = np.array(F["truth"])
    err = np.abs(res.x - t) / np.array([1.0, 1.0, t[2], t[3]])
    print("numpy fit of the seed: %d iterations, m = %s, error %s" % (res.nit, res.x, err))
    assert res.nit <= F["options"]["maxiter"]
    assert np.all(err <= F["bar"]), res
