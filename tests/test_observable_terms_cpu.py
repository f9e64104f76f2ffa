"""
Volume misfit terms (glims_adjoint_observable_terms), the parts that need no GPU:
  1. the numpy statement of tests/observable_terms_common.py -- the reference of the device path -- against central differences
     of its own J, with the step sizes and bars of tests/test_adjoint_image_cpu.py (h = 1e-5, relative 1e-6 for D, rho and a c0
     direction; eps = 1e-4, relative 1e-6 for the Hessian products of MASS and SMOOTH terms), in 2-D and 3-D;
  2. csrc/observe_grad.h, run on the host through tests/observe_grad_check.cpp (the host compiler alone, -Wall -Werror, and once
     more with the address and undefined-behaviour sanitizers), against the numpy per-cell derivative;
  3. the header declares the entry points, the ctypes table carries them, the library exports them, the ABI is still 6 and the
     ObservableMisfit mirror has the layout of the header's struct;
  4. the numpy twin of the public-API fit of tests/test_gpu_observable_terms.py.
"""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import observable_terms_common as otc
import observe_common as oc
from adjoint_common import Problem
from test_observe_cpu import LEVELS, SIMPLEX, VALUES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 4


def _problem(dim):
    prob = Problem(2, 9) if dim == 2 else Problem(3, 3)      # 100 and 64 nodes, two tissues, Dirichlet c on x = 1
    assert len(prob.points) <= 100
    return prob


@pytest.fixture(scope="module", params=[2, 3])
def setting(request):
    prob = _problem(request.param)
    o = prob.oracle()
    traj = prob.trajectory(o, N_STEPS)
    return prob, traj, otc.standard_terms(prob, traj, seed=request.param)


def _J(prob, terms, D=None, rho=None, c0=None):
    o = prob.oracle(D, rho)
    return otc.misfit(prob, o, prob.trajectory(o, N_STEPS, c0), terms)


def test_the_term_list_exercises_what_it_claims(setting):
    prob, traj, terms = setting
    vol = [t for t in terms if t["kind"] == otc.KIND]
    assert {t["observable"] for t in vol} == {"mass", "sharp", "smooth"} and {t["step"] for t in vol} == {0, N_STEPS // 2, N_STEPS}
    assert any(t["labels"] is None for t in vol) and any(t["labels"] is not None for t in vol)
    for t in vol:
        c = traj[t["step"]]
        assert 0 < otc.counted_cells(prob, t).sum() and otc.measure(prob, t, c) > 0
        if t["observable"] == "sharp":
            assert np.abs(c - t["level"]).min() >= 1e-2                      # the gap rule: no in / out pattern can change
            assert otc.cut_cells(prob, t, c) >= 1
            cut = set(np.unique(otc.in_counts(prob, t, c)[otc.counted_cells(prob, t)])) - {0, prob.dim + 1}
            assert cut, "no cut cell"


def test_numpy_adjoint_matches_central_differences(setting):
    prob, traj, terms = setting
    J, dD, drho, dc0 = otc.adjoint(prob, prob.oracle(), traj, terms)
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
        print("%d-D d%s: adjoint %s central differences %s" % (prob.dim, name, ad, num))
        assert np.linalg.norm(ad - num) <= 1e-6 * np.linalg.norm(num), (name, ad, num)
    p = np.random.default_rng(1).standard_normal(len(prob.points))
    h = 1e-5
    num = (_J(prob, terms, c0=prob.c0 + h * p) - _J(prob, terms, c0=prob.c0 - h * p)) / (2 * h)
    assert abs(dc0 @ p - num) <= 1e-6 * abs(num), (dc0 @ p, num)


@pytest.mark.parametrize("kind", ["mass", "sharp", "smooth"])
def test_each_kind_alone_matches_central_differences(setting, kind):
    """One kind carries the whole gradient (a wrong SHARP derivative cannot hide behind the larger MASS term)."""
    prob, traj, terms = setting
    only = [t for t in terms if t.get("observable") == kind]
    assert only
    J, dD, drho, dc0 = otc.adjoint(prob, prob.oracle(), traj, only)
    for name, ad in (("D", dD), ("rho", drho)):
        x0 = getattr(prob, name)
        num = np.zeros_like(x0)
        for i in range(len(x0)):
            e = np.zeros_like(x0)
            e[i] = 1e-5 * abs(x0[i])
            num[i] = (_J(prob, only, **{name: x0 + e}) - _J(prob, only, **{name: x0 - e})) / (2 * e[i])
        if all(t["step"] == 0 for t in only):
            assert not np.any(ad) and not np.any(num)
            continue
        assert np.linalg.norm(ad - num) <= 1e-6 * np.linalg.norm(num), (kind, name, ad, num)
    p = np.random.default_rng(2).standard_normal(len(prob.points))
    h = 1e-5
    num = (_J(prob, only, c0=prob.c0 + h * p) - _J(prob, only, c0=prob.c0 - h * p)) / (2 * h)
    assert abs(dc0 @ p - num) <= 1e-6 * abs(num), (kind, dc0 @ p, num)


def _direction(prob, seed):
    rng = np.random.default_rng(seed)
    return dict(D=prob.D * rng.uniform(-1, 1, prob.n_labels), rho=prob.rho * rng.uniform(-1, 1, prob.n_labels),
                c0=0.2 * rng.uniform(-1, 1, len(prob.points)) * (prob.c0 + 0.1))


def test_numpy_hessian_matches_central_differences_of_the_gradient(setting):
    prob, traj, terms = setting
    terms = [t for t in terms if t.get("observable") != "sharp"]          # MASS, SMOOTH and the nodal term
    assert {t.get("observable") for t in terms} == {"mass", "smooth", None}
    d = _direction(prob, 1)
    hv = otc.hessian(prob, prob.oracle(), traj, terms, [d])[4][0]
    ana = otc.flat(prob, hv)
    eps = 1e-4
    m = dict(D=prob.D, rho=prob.rho, c0=prob.c0)
    shift = lambda s: {k: m[k] + s * d[k] for k in m}
    num = (otc.gradient_at(prob, shift(eps), N_STEPS, terms)[1] - otc.gradient_at(prob, shift(-eps), N_STEPS, terms)[1]) / (2 * eps)
    L = prob.n_labels
    for what, sl in (("D", slice(0, L)), ("rho", slice(L, 2 * L)), ("c0", slice(2 * L, None))):
        err = np.linalg.norm(ana[sl] - num[sl]) / np.linalg.norm(num[sl])
        print("%d-D hv_%s: rel. difference to central differences %.3e" % (prob.dim, what, err))
        assert err <= 1e-6, (what, err, ana[sl][:4], num[sl][:4])


def test_numpy_hessian_is_symmetric(setting):
    prob, traj, terms = setting
    terms = [t for t in terms if t.get("observable") != "sharp"]
    L, n = prob.n_labels, len(prob.points)
    rng = np.random.default_rng(5)
    dirs = [{key: np.eye(L)[l]} for key in ("D", "rho") for l in range(L)] + [dict(c0=rng.uniform(-1, 1, n)) for _ in range(2)]
    hv = otc.hessian(prob, prob.oracle(), traj, terms, dirs)[4]
    V = np.array([otc.flat(prob, d) for d in dirs])
    H = np.array([[otc.flat(prob, hv[j]) @ V[i] for j in range(len(dirs))] for i in range(len(dirs))])
    assert np.abs(H - H.T).max() <= 1e-9 * np.abs(H).max(), H


def test_gap_rule_holds_on_the_problems_of_the_gpu_tests():
    """At the steps 0, N/2 and N the GPU tests observe (N = 4 on the 2-D meshes, N = 6 in 3-D) every nodal value is at least 1e-2
    from the level the gap rule picks.  (On Problem(2, 17) the widest gap narrows to 0.018 by step 6: its runs stop at N = 4.)"""
    for prob, N in ((Problem(2, 17), 4), (Problem(3, 6), 6), (Problem(2, 9), 4)):
        traj = prob.trajectory(prob.oracle(), N)
        for k in (0, N // 2, N):
            level, dist = otc.gap_level(traj[k])
            print("%d-D, %d nodes, step %d: level %.4f, nearest nodal value %.4f away" % (prob.dim, len(prob.points), k, level, dist))
            assert dist >= 1e-2


# ---- 2. the header on the host -------------------------------------------------------------------------------------------------
def _cases():
    """(d, kind, level, smooth, c, dc, tag)"""
    rng = np.random.default_rng(3)
    cases = []
    for d in (2, 3):
        for perm in itertools.permutations(VALUES[d]):
            dc = rng.uniform(-1, 1, d + 1)
            for n_in, level in enumerate(LEVELS[d]):
                assert oc.in_count(perm, level) == n_in
                cases.append((d, "sharp", level, 1.0, perm, dc, "in%d" % n_in))
            for v in VALUES[d]:                                            # a tie: that vertex counts as in
                cases.append((d, "sharp", v, 1.0, perm, dc, "tie"))
            cases.append((d, "mass", 0.0, 1.0, perm, dc, "mass"))
            cases.append((d, "smooth", 0.45, 0.2, perm, dc, "smooth"))
            cases.append((d, "smooth", 0.8, 0.05, perm, dc, "smooth"))
        cases.append((d, "sharp", 0.3, 1.0, [0.3] * (d + 1), np.ones(d + 1), "all_equal"))
        cases.append((d, "sharp", 0.3, 1.0, [0.3, 0.3] + [0.1] * (d - 1), np.ones(d + 1), "two_ties"))
        cases.append((d, "sharp", 0.3, 1.0, [0.3 + 1e-9, 0.3 - 1e-9] + [0.1] * (d - 1), np.ones(d + 1), "narrow"))
    return cases


def _compiler():
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    return cxx


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run([_compiler(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I",
                    os.path.join(ROOT, "glimslib_amd", "csrc"), os.path.join(ROOT, "tests", "observe_grad_check.cpp"), "-o", exe],
                   check=True, timeout=180)
    return exe


def _run(exe, cases):
    lines = []
    for d, kind, level, smooth, c, dc, _ in cases:
        nums = [level, smooth] + [float(v) for v in c] + [float(v) for v in dc]
        lines.append("%d %d " % (d, oc.KIND_ID[kind]) + " ".join(repr(float(v)) for v in nums))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    rows = [np.array([float(v) for v in line.split()]) for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def test_gradient_header_on_the_host_plain_and_under_the_sanitizers(tmp_path):
    """csrc/observe_grad.h against the numpy per-cell derivative, in units of the fraction b0 = V_T / |T| (the numpy figures,
    taken on a fixed well-shaped simplex, are divided by its |T|).  Every in-count 0 .. d+1 with every vertex in every role,
    vertex ties, all vertices at the level, two ties, and an in / out pair 2e-9 apart.

    Tolerance.  tests/test_observe_cpu.py bounds the error of b0 by 64 * 2^-52: a few dozen roundings of well-conditioned
    operations.  b0 is a polynomial in the edge parameters t = (c_a - level) / (c_a - c_b) in [0, 1], and its derivative by a
    vertex value is a sum of products of such factors times dt/dc = (1 - t | t) / (c_a - c_b): the same count of roundings,
    relative to a quantity of size at most 1 / min(c_a - c_b) over the cut edges.  Hence
        |d b0 / d c_i  (header) - (numpy)| <= 64 * 2^-52 / min over the cut edges of (c_a - c_b)
    for SHARP.  MASS is exact to one rounding; SMOOTH differentiates sum_q w_q h(v_q) with sum w = 1 and |h'| <= 1 / (2 smooth),
    |h''| <= 0.77 / smooth^2: 64 * 2^-52 / smooth for the gradient and 64 * 2^-52 max|dc| / smooth^2 for the product H dc.
    The same program, built with -fsanitize=address,undefined, must run the same cases clean and print the same numbers."""
    cases = _cases()
    exe = _build(tmp_path, "observe_grad_check")
    rows = _run(exe, cases)
    worst = {}
    for (d, kind, level, smooth, c, dc, tag), got in zip(cases, rows):
        p = SIMPLEX[d]
        T = abs(oc._vol(p.tolist()))
        nv = d + 1
        b0, g, Hd, n_in = got[0], got[1:1 + nv], got[1 + nv:1 + 2 * nv], int(got[-1])
        want_g, want_H = otc.cell_grad(p, c, kind, level, smooth, dc=None if kind == "sharp" else dc)
        want_b0 = oc.observe_cell(p, c, kind, level, smooth)[0] / T
        assert abs(b0 - want_b0) <= 64 * oc.EPS, (d, kind, level, c, tag, b0, want_b0)
        if kind == "sharp":
            assert n_in == oc.in_count(c, level)
            ins = [v for v in c if v >= level]
            outs = [v for v in c if not v >= level]
            gap = min((a - b for a in ins for b in outs), default=1.0)
            tol = 64 * oc.EPS / gap
            assert not np.any(Hd)
            if n_in in (0, nv):
                assert not np.any(g), (d, level, c, g)
        else:
            assert n_in == -1
            tol = 64 * oc.EPS / (smooth if kind == "smooth" else 1.0)
            tolH = 64 * oc.EPS * np.abs(dc).max() / smooth ** 2
            eH = np.abs(Hd - want_H / T).max()
            assert eH <= tolH, (d, kind, level, c, tag, eH / tolH)
            if kind == "mass":
                assert not np.any(Hd)
        err = np.abs(g - want_g / T).max()
        worst[(d, tag)] = max(worst.get((d, tag), 0.0), err / tol)
        assert err <= tol, (d, kind, level, c, tag, err / tol, g, want_g / T)
        # sum_i dV/dc_i = -dV/dlevel >= 0
        assert g.sum() >= -tol
    print({k: "%.3f of the bound" % v for k, v in sorted(worst.items())})
    san = _build(tmp_path, "observe_grad_check_san", extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rows_san = _run(san, cases)
    for a, b in zip(rows, rows_san):
        assert np.allclose(a, b, rtol=1e-13, atol=1e-13)


def test_sharp_gradient_sums_to_the_cross_section():
    """sum_i dV_T/dc_i = -dV_T/dlevel: central differences of the cell loop's own V in the level (numpy alone)."""
    for d in (2, 3):
        p = SIMPLEX[d]
        for perm in itertools.permutations(VALUES[d]):
            for level in LEVELS[d][1:-1]:
                g = otc.sharp_cell_grad(p, perm, level)
                h = 1e-6
                num = -(oc.observe_cell(p, perm, "sharp", level + h)[0] - oc.observe_cell(p, perm, "sharp", level - h)[0]) / (2 * h)
                assert abs(g.sum() - num) <= 1e-8 * max(1.0, abs(num)), (d, perm, level, g.sum(), num)


# ---- 3. the surface ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_carry_the_entry_points():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _backend.load_library()
    assert lib.glims_abi_version() == _backend.ABI_VERSION == 6
    for name in ("glims_adjoint_observable_terms", "glims_adjoint_observable_info"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _backend.SIGNATURES
        assert hasattr(lib, name)
    body = re.search(r"typedef struct glims_observable_misfit \{(.*?)\} glims_observable_misfit;", code, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert fields == [f for f, _ in _backend.ObservableMisfit._fields_]
    assert fields == ["step", "kind", "level", "smooth", "weight", "target", "labels"]

    class Mirror(C.Structure):   # the C layout, spelt out: int64, int (+ padding), 4 doubles, a pointer
        _fields_ = [("step", C.c_int64), ("kind", C.c_int), ("level", C.c_double), ("smooth", C.c_double),
                    ("weight", C.c_double), ("target", C.c_double), ("labels", C.c_void_p)]

    assert C.sizeof(_backend.ObservableMisfit) == C.sizeof(Mirror) == 56
    for f, _ in Mirror._fields_:
        assert getattr(_backend.ObservableMisfit, f).offset == getattr(Mirror, f).offset, f
    assert _backend.SIGNATURES["glims_adjoint_observable_terms"][1][-1] == C.POINTER(_backend.ObservableMisfit)


def test_distributed_handle_refuses_volume_terms():
    from glimslib_amd.parallel import DistributedHandle
    dh = DistributedHandle.__new__(DistributedHandle)         # (no ranks needed: the refusal comes before anything else)
    t = otc.volume_term(0, "mass", 1.0)
    with pytest.raises(NotImplementedError):
        dh.set_observable_terms([t])
    with pytest.raises(NotImplementedError):
        dh.observable_term_info(0)
    with pytest.raises(NotImplementedError):
        dh._local_terms([t])


# ---- 4. the numpy twin of the public-API fit ------------------------------------------------------------------------------------
def fit_volume_terms(prob, traj):
    """The T2- and T1-like SMOOTH volumes of the whole domain at FIT_VOLUMES' steps, as terms whose targets are the volumes of
    `traj`."""
    F = otc.FIT_VOLUMES
    terms = []
    for lv in F["levels"]:
        for k in F["steps"]:
            t = otc.volume_term(k, "smooth", 0.0, level=lv, smooth=F["smooth"])
            t["target"] = otc.measure(prob, t, traj[k])
            terms.append(t)
    return terms


def test_numpy_fit_to_two_volume_series_recovers_D_and_rho():
    """The setting of the public-API fit of tests/test_gpu_observable_terms.py (adjoint_image_common.FIT's mesh, model, start,
    bounds and options; the data are two SMOOTH volume series), run with the numpy statement and scipy's L-BFGS-B: it recovers
    (D, rho) to 1e-3 within the cap of 30 iterations, the bar of the image fit."""
    from scipy.optimize import minimize
    from glimslib_amd import fenics_local as fenics
    import adjoint_image_common as aic
    F = aic.FIT
    mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
    pts, cells = np.asarray(mesh.points), np.asarray(mesh.cells)
    truth = aic.fit_problem(pts, cells, *F["truth"])
    terms = fit_volume_terms(truth, truth.trajectory(truth.oracle(), F["steps"]))

    def fun(m):
        p = aic.fit_problem(pts, cells, m[0], m[1])
        o = p.oracle()
        J, dD, drho, _ = otc.adjoint(p, o, p.trajectory(o, F["steps"]), terms)
        return J, np.array([dD.sum(), drho.sum()])

    res = minimize(fun, np.array(F["start"]), jac=True, bounds=[F["bounds"]] * 2, method="L-BFGS-B", tol=F["tol"],
                   options=dict(F["options"], disp=False))
    err = np.abs(res.x - np.array(F["truth"])) / np.array(F["truth"])
    print("numpy fit to two volume series: %d iterations, m = %s, rel. error %s" % (res.nit, res.x, err))
    assert res.nit <= F["options"]["maxiter"]
    assert np.all(err <= 1e-3), res
