"""
Volume misfit terms in the deformed configuration (glims_adjoint_observable_terms2), the parts that need no GPU:
  1. the numpy statement of tests/deformed_volume_common.py -- the reference of the device path -- against central differences
     of its own J in D, rho, gamma, E, nu (every label) and a c0 direction, with the step and the bar of the project's adjoint
     tests (h = 1e-5 relative, agreement 1e-6), the terms together and each deformed term alone, in 2-D and 3-D;
  2. csrc/observe_grad.h's cofactors, run on the host through tests/observe_def_grad_check.cpp (the host compiler alone, -Wall
     -Werror, and once more with the address and undefined-behaviour sanitizers), against central differences of
     glims_oc_volume and the numpy minors;
  3. the surface: header, ctypes table, exported symbols, the struct mirror, the refusing DistributedHandle, volume_term;
  4. the numpy twin of the public-API fit of tests/test_gpu_deformed_volume.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deformed_volume_common as dvc
import observable_terms_common as otc
import observe_common as oc
from test_observable_terms_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 3
REL_STEP, BAR = 1e-5, 1e-6          # tests/test_adjoint_image_cpu.py, tests/test_adjoint_deformed_cpu.py


# ---- 1. the numpy statement ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[2, 3])
def setting(request):
    dim = request.param
    prob = dvc.clamped_problem(dim, 12 if dim == 2 else 5)
    o = dvc.oracle_of(prob)
    traj = prob.trajectory(o, N_STEPS)
    terms = dvc.standard_terms(prob, traj, o.mech_solve, seed=dim)
    deformed = [t for t in terms if dvc.is_deformed_volume(t)]
    lists = [terms] + [[t] for t in deformed]
    return prob, o, traj, lists


def test_the_term_list_exercises_what_it_claims(setting):
    prob, o, traj, lists = setting
    terms = lists[0]
    assert [(t.get("observable"), bool(t.get("deformed")), t["step"]) for t in terms] == \
        [("smooth", True, N_STEPS), ("sharp", True, 1), ("mass", True, N_STEPS), ("sharp", True, N_STEPS),
         ("smooth", False, N_STEPS), (None, False, N_STEPS)]
    assert terms[1]["scale"] == 0.5 and terms[3]["level"] == -1.0 and list(terms[3]["labels"]) == [0, 1]
    res = dvc.evaluate(prob, o, traj, terms)
    sharp, tissue = res["info"][1], res["info"][3]
    assert sharp["cut"] >= 1 and np.abs(traj[1] - terms[1]["level"]).min() >= 1e-2          # the gap rule
    assert tissue["cut"] == 0 and tissue["counted"] == int((prob.labels == 1).sum())
    u = o.mech_solve(traj[N_STEPS])
    ref = otc.measure(prob, terms[3], traj[N_STEPS])
    print("dim %d: tissue 1 has the volume %.6f undeformed and %.6f deformed; max |u| %.3f, smallest ratio %.3f"
          % (prob.dim, ref, tissue["V"], np.abs(u).max(), min(i["min_ratio"] for i in res["info"][:4])))
    assert abs(tissue["V"] - ref) > 1e-3 * ref, "no visible mass effect"
    assert all(i["folded"] == 0 and i["min_ratio"] > 0.3 for i in res["info"][:4])
    assert res["info"][4]["folded"] == -1 and np.isnan(res["info"][4]["min_ratio"])


def test_vectorised_statement_equals_the_cell_loop(setting):
    prob, o, traj, lists = setting
    for t in [t for t in lists[0] if dvc.is_deformed_volume(t)]:
        c = traj[t["step"]]
        u = o.mech_solve(c)
        a, b = dvc.deformed_parts(prob, t, c, u), dvc.deformed_parts_loop(prob, t, c, u)
        assert dvc.rel(a[0], b[0]) <= 1e-13 if np.any(b[0]) else not np.any(a[0])
        assert dvc.rel(a[1], b[1]) <= 1e-13 and a[2] == b[2]
    y = np.random.default_rng(0).uniform(-1, 1, (5, prob.dim + 1, prob.dim))
    for k in range(5):
        assert np.allclose(dvc.cofactors_all(y)[k], dvc.cofactors(y[k]), rtol=0, atol=1e-15)
        assert np.abs(dvc.cofactors(y[k]).sum(axis=0)).max() <= 1e-15


def test_numpy_adjoint_matches_central_differences(setting):
    prob, o, traj, lists = setting
    res = [dvc.evaluate(prob, o, traj, terms) for terms in lists]
    J0 = dvc.J_of_lists(prob, lists, N_STEPS)
    for r, j in zip(res, J0):
        assert r["J"] > 0 and r["J"] == pytest.approx(j, rel=1e-13)
    worst, smallest = {}, {}
    for name in ("D", "rho", "gamma", "E", "nu"):
        base = getattr(prob, name)
        for label in range(prob.n_labels):
            e = np.zeros_like(base)
            e[label] = REL_STEP * abs(base[label])
            num = (dvc.J_of_lists(prob, lists, N_STEPS, **{name: base + e}) -
                   dvc.J_of_lists(prob, lists, N_STEPS, **{name: base - e})) / (2 * e[label])
            for k, r in enumerate(res):
                err = abs(r[name][label] - num[k]) / abs(num[k])
                worst[name] = max(worst.get(name, 0.0), err)
                smallest[name] = min(smallest.get(name, np.inf), abs(num[k]))
                assert abs(num[k]) > 0 and err <= BAR, (name, label, k, r[name][label], num[k], err)
    p = np.random.default_rng(1).standard_normal(len(prob.points))
    if prob.dir_c is not None:
        p[prob.dir_c[0]] = 0.0
    h = 1e-5
    num = (dvc.J_of_lists(prob, lists, N_STEPS, c0=prob.c0 + h * p) - dvc.J_of_lists(prob, lists, N_STEPS, c0=prob.c0 - h * p)) \
        / (2 * h)
    for k, r in enumerate(res):
        err = abs(r["c0"] @ p - num[k]) / abs(num[k])
        worst["c0"] = max(worst.get("c0", 0.0), err)
        assert err <= BAR, (k, r["c0"] @ p, num[k])
    print("dim %d: numpy gradient against central differences, the worst of %d lists: %s; smallest derivative %s"
          % (prob.dim, len(lists), {k: "%.1e" % v for k, v in worst.items()}, {k: "%.1e" % v for k, v in smallest.items()}))


def test_reference_terms_give_gamma_E_and_nu_exact_zeros(setting):
    """What the deformed terms are for: the same terms with deformed=False see no displacement at all."""
    prob, o, traj, lists = setting
    flat = [{k: v for k, v in t.items() if k not in ("deformed", "scale")} for t in lists[0] if dvc.is_deformed_volume(t)]
    res = dvc.evaluate(prob, o, traj, flat)
    assert res["mech_steps"] == 0 and not any(np.any(res[k]) for k in ("gamma", "E", "nu")) and np.any(res["D"])
    only = dvc.evaluate(prob, o, traj, [t for t in lists[0] if dvc.is_deformed_volume(t)])
    assert only["mech_steps"] == 2 and all(np.all(only[k] != 0.0) for k in ("gamma", "E", "nu"))


# ---- 2. the header on the host ---------------------------------------------------------------------------------------------------
def _simplices():
    """(d, p, tag): a right-handed, a left-handed and a degenerate (zero-volume) cell in 2-D and 3-D, and random ones"""
    rng = np.random.default_rng(5)
    out = []
    for d in (2, 3):
        right = np.vstack([np.zeros(d), np.eye(d)]) + 0.2 * rng.uniform(-1, 1, (d + 1, d))
        left = right[[1, 0] + list(range(2, d + 1))]
        flat = right.copy()
        flat[d] = flat[:d].mean(axis=0)                       # the last vertex in the face (edge) of the others
        out += [(d, right, "right"), (d, left, "left"), (d, flat, "degenerate")]
        out += [(d, rng.uniform(-2, 2, (d + 1, d)), "random") for _ in range(6)]
    return out


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run([_compiler(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I",
                    os.path.join(ROOT, "glimslib_amd", "csrc"), os.path.join(ROOT, "tests", "observe_def_grad_check.cpp"),
                    "-o", exe], check=True, timeout=180)
    return exe


def _run(exe, cases, h):
    lines = ["%d %r " % (d, h) + " ".join(repr(float(v)) for v in np.ravel(p)) for d, p, _ in cases]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    rows = [np.array([float(v) for v in line.split()]) for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def test_cofactor_header_on_the_host_plain_and_under_the_sanitizers(tmp_path):
    """glims_og_volume_grad against a central difference of glims_oc_volume, for every vertex and component.

    Tolerance.  The volume is multilinear in the vertex coordinates, so the central difference has no truncation error: it
    differs from the derivative by the rounding of two volumes, each a sum of at most 6 products of d coordinate differences
    of size <= S = 2 max|p| + h -- at most 32 * 2^-52 S^d each --, divided by 2h.  The cofactors themselves (a sum of at most
    2 products of d - 1 differences) and the numpy minors carry a few roundings of S^(d-1): 32 * 2^-52 S^(d-1)."""
    cases = _simplices()
    h = 2.0 ** -10
    exe = _build(tmp_path, "observe_def_grad_check")
    rows = _run(exe, cases, h)
    for i, ((d, p, tag), row) in enumerate(zip(cases, rows)):
        n = (d + 1) * d
        vol, cof, num = row[0], row[1:1 + n].reshape(d + 1, d), row[1 + n:].reshape(d + 1, d)
        S = 2.0 * np.abs(p).max() + h
        assert abs(vol - oc._vol(p.tolist())) <= 32 * oc.EPS * S ** d
        tol_fd = 32 * oc.EPS * S ** d / h
        tol = 32 * oc.EPS * S ** (d - 1)
        assert np.abs(cof - num).max() <= tol_fd, (d, tag, np.abs(cof - num).max(), tol_fd)
        assert np.abs(cof - dvc.cofactors(p)).max() <= tol, (d, tag)
        assert np.abs(cof.sum(axis=0)).max() <= tol, (d, tag, cof.sum(axis=0))
        if tag == "degenerate":
            assert abs(vol) <= 32 * oc.EPS * S ** d and np.all(np.isfinite(cof)) and np.abs(cof).max() > 0.05
        if tag == "left":
            assert vol < 0 < rows[i - 1][0]
    san = _build(tmp_path, "observe_def_grad_check_san", extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for a, b in zip(rows, _run(san, cases, h)):
        assert np.allclose(a, b, rtol=1e-13, atol=1e-13)


# ---- 3. the surface ----------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_carry_the_new_entry_points_and_the_struct():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _backend.load_library()
    assert lib.glims_abi_version() == _backend.ABI_VERSION == 6
    for name in ("glims_adjoint_observable_terms2", "glims_adjoint_observable_info2"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _backend.SIGNATURES and hasattr(lib, name)
    assert "volumes of the deformed configuration" not in src
    body = re.search(r"typedef struct glims_observable_misfit2 \{(.*?)\} glims_observable_misfit2;", code, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert fields == [f for f, _ in _backend.ObservableMisfit2._fields_]
    assert fields == ["step", "kind", "level", "smooth", "weight", "target", "labels", "deformed", "scale"]

    class Mirror(C.Structure):   # the C layout, spelt out: the 56 bytes of glims_observable_misfit, int (+ padding), double
        _fields_ = [("step", C.c_int64), ("kind", C.c_int), ("level", C.c_double), ("smooth", C.c_double),
                    ("weight", C.c_double), ("target", C.c_double), ("labels", C.c_void_p), ("deformed", C.c_int),
                    ("scale", C.c_double)]

    assert C.sizeof(_backend.ObservableMisfit2) == C.sizeof(Mirror) == 72 and C.sizeof(_backend.ObservableMisfit) == 56
    for f, _ in Mirror._fields_:
        assert getattr(_backend.ObservableMisfit2, f).offset == getattr(Mirror, f).offset, f
    assert _backend.SIGNATURES["glims_adjoint_observable_terms2"][1][-1] == C.POINTER(_backend.ObservableMisfit2)
    assert len(_backend.SIGNATURES["glims_adjoint_observable_info2"][1]) == 5


def test_distributed_handle_refuses_deformed_volume_terms():
    from glimslib_amd.parallel import DistributedHandle
    dh = DistributedHandle.__new__(DistributedHandle)         # (no ranks needed: the refusal comes before anything else)
    t = dvc.volume_term(0, "mass", 1.0, deformed=True)
    with pytest.raises(NotImplementedError):
        dh.set_observable_terms([t])
    with pytest.raises(NotImplementedError):
        dh.observable_term_info2(0)
    with pytest.raises(NotImplementedError):
        dh._local_terms([t])


def _sim(mechanics):
    from glimslib_amd.simulation import TumorGrowth
    sim = TumorGrowth.__new__(TumorGrowth)                    # (volume_term reads these three and nothing else)
    sim._backend = None
    sim.solver = type("S", (), dict(mechanics=mechanics))()
    sim.subdomains = type("D", (), dict(tissue_id_name_map={1: 'A', 2: 'B'}))()
    sim._labels = lambda: np.array([1, 2, 2])
    return sim


def test_volume_term_dicts():
    sim = _sim(True)
    old = sim.volume_term(3, 1.5, threshold=0.4, kind='smooth', smooth=0.05, tissues=['b'], weight=2.0)
    assert set(old) == {"step", "kind", "observable", "level", "smooth", "target", "weight", "labels"}
    assert (old["step"], old["kind"], old["observable"], old["level"], old["smooth"], old["target"], old["weight"]) == \
        (3, "obs_volume", "smooth", 0.4, 0.05, 1.5, 2.0) and list(old["labels"]) == [0, 0, 1]
    same = sim.volume_term(3, 1.5, threshold=0.4, kind='smooth', smooth=0.05, tissues=['b'], weight=2.0, deformed=False, scale=3.0)
    assert set(same) == set(old) and all(np.array_equal(same[k], old[k]) for k in old)
    new = sim.volume_term(3, 1.5, threshold=-1.0, kind='sharp', tissues=['b'], deformed=True, scale=0.5)
    assert new["deformed"] is True and new["scale"] == 0.5 and set(new) == set(old) | {"deformed", "scale"}
    with pytest.raises(ValueError):
        _sim(False).volume_term(3, 1.5, deformed=True)
    assert "deformed" not in _sim(False).volume_term(3, 1.5)
    part = _sim(True)
    part._backend = object()                                  # not a single-GPU Handle: a partitioned run
    with pytest.raises(NotImplementedError):
        part.volume_term(3, 1.5, deformed=True)
    from glimslib_amd import _backend
    key = _backend.Handle._observable_key
    assert key(old) != key(dict(old, deformed=True)) and key(dict(old, deformed=True)) != key(dict(old, deformed=True, scale=2.0))
    assert key(old) == key(dict(old, scale=2.0))               # (scale means nothing to a reference term)


# ---- 4. the numpy twin of the public-API fit ------------------------------------------------------------------------------------
def test_numpy_fit_to_deformed_volume_series_recovers_the_coupling_and_D():
    """The setting of the public-API fit of tests/test_gpu_deformed_volume.py (deformed_volume_common.FIT), run with the numpy
    statement and scipy's L-BFGS-B from a start 30 % off: it recovers (coupling, D) to 1e-3, the bar of the volume and image
    fits, within the cap of 40 iterations.  The data do identify the coupling: without the deformed terms its gradient is 0."""
    from scipy.optimize import minimize
    from glimslib_amd import fenics_local as fenics
    F = dvc.FIT
    mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
    pts, cells = np.asarray(mesh.points), np.asarray(mesh.cells)
    lab = dvc.fit_labels(mesh)
    assert set(np.unique(lab)) == {1, 2}
    truth = dvc.fit_problem(pts, cells, lab, *F["truth"])
    o = dvc.oracle_of(truth)
    traj = truth.trajectory(o, F["steps"])
    tissue_B = np.array([0, 0, 1], dtype=np.uint8)
    terms = dvc.fit_terms(lambda k, kind, lv, sm, tissue, w: dvc.volume_term(k, kind, 0.0, level=lv, smooth=sm, weight=w,
                                                                            labels=tissue_B if tissue else None, deformed=True))
    for t in terms:
        t["target"] = dvc.measure(truth, t, traj[t["step"]], o.mech_solve(traj[t["step"]]))
    VB = [t["target"] for t in terms if t["observable"] == "sharp"]
    assert VB[0] > VB[-1] and VB[0] - VB[-1] > 0.1, "the tumour does not compress the neighbouring tissue"

    def fun(m):
        p = dvc.fit_problem(pts, cells, lab, m[0], m[1])
        po = dvc.oracle_of(p)
        r = dvc.evaluate(p, po, p.trajectory(po, F["steps"]), terms)
        return r["J"], np.array([r["gamma"].sum(), r["D"].sum()])

    res = minimize(fun, np.array(F["start"]), jac=True, bounds=[F["bounds"]] * 2, method="L-BFGS-B", tol=F["tol"],
                   options=dict(F["options"], disp=False))
    err = np.abs(res.x - np.array(F["truth"])) / np.array(F["truth"])
    print("numpy fit to deformed volume series: %d iterations, m = %s, rel. error %s" % (res.nit, res.x, err))
    assert res.nit <= F["options"]["maxiter"]
    assert np.all(err <= 1e-3), res
