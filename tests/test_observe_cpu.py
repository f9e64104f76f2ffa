"""
Tumour volumes and centres of mass per tissue (glims_observe), the parts that need no GPU:
  1. csrc/observe_clip.h, run on the host through tests/observe_clip_check.cpp (compiled with the host compiler alone), against
     the per-cell loop of tests/observe_common.py on fixed simplices: every in-count 0 .. d+1 in 2-D and 3-D with every vertex
     taking every role, vertex ties c_i == level, all vertices equal to the level, a negatively oriented simplex, in + out =
     the whole cell, MASS against the closed form, SMOOTH against the numpy rule.  Tolerance 64 * 2^-52 * |T| for the measure,
     times max|x| for the moments: a few dozen roundings of well-conditioned operations on identical inputs;
  2. the package's vectorised numpy statement (simulation_helpers/observables.py) against the same loop on the rectangle, the
     box and the brain-like mesh, reference and deformed;
  3. the header declares the entry points, the ctypes table carries them, the library exports them, the ABI is still 6 and
     the Observable mirror has the size of the header's struct.

Reference counterpart: compute_from_conc_for_each_time_step and compute_volume_thresholded / compute_com_all,
glimslib/optimization_workflow/image_based_optimization.py:1333-1397, :1262-1301.
"""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import observe_common as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIMPLEX = {2: np.array([[0.1, 0.2], [1.3, 0.4], [0.5, 1.1]]),
           3: np.array([[0.1, 0.2, 0.3], [1.2, 0.3, 0.1], [0.4, 1.3, 0.2], [0.5, 0.6, 1.4]])}
VALUES = {2: [0.1, 0.5, 0.9], 3: [0.1, 0.4, 0.7, 1.0]}
LEVELS = {2: [1.5, 0.7, 0.3, 0.05], 3: [1.5, 0.85, 0.55, 0.25, 0.05]}      # in-counts 0 .. d+1 of VALUES


def _cases():
    """(d, kind, level, smooth, p, c, tag)"""
    cases = []
    for d in (2, 3):
        p = SIMPLEX[d]
        assert oc._vol(p.tolist()) > 0.0
        flipped = p[[1, 0] + list(range(2, d + 1))]
        for perm in itertools.permutations(VALUES[d]):
            for n_in, level in enumerate(LEVELS[d]):
                assert oc.in_count(perm, level) == n_in
                cases.append((d, "sharp", level, 1.0, p, perm, "in%d" % n_in))
            for v in VALUES[d]:                                            # a tie: that vertex counts as in
                cases.append((d, "sharp", v, 1.0, p, perm, "tie"))
            cases.append((d, "mass", 0.0, 1.0, p, perm, "mass"))
            cases.append((d, "smooth", 0.45, 0.2, p, perm, "smooth"))
            cases.append((d, "smooth", 0.8, 0.05, p, perm, "smooth"))
        for level in LEVELS[d] + [VALUES[d][1]]:
            cases.append((d, "sharp", level, 1.0, flipped, VALUES[d], "flipped"))
        cases.append((d, "mass", 0.0, 1.0, flipped, VALUES[d], "flipped"))
        cases.append((d, "smooth", 0.45, 0.2, flipped, VALUES[d], "flipped"))
        for level in (0.3, 0.0, -0.25):                                    # all vertices equal to the level: the whole cell
            cases.append((d, "sharp", level, 1.0, p, [level] * (d + 1), "all_equal"))
        cases.append((d, "sharp", 0.3, 1.0, p, [0.3, 0.3] + [0.1] * (d - 1), "two_ties"))
    return cases


def _run_header(tmp_path, cases):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "observe_clip_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "observe_clip_check.cpp"), "-o", exe], check=True, timeout=120)
    lines = []
    for d, kind, level, smooth, p, c, _ in cases:
        nums = [level, smooth] + [float(v) for v in np.asarray(p).ravel()] + [float(v) for v in c]
        lines.append("%d %d " % (d, oc.KIND_ID[kind]) + " ".join(repr(float(v)) for v in nums))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [np.array([float(v) for v in line.split()]) for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def test_clip_header_on_the_host(tmp_path):
    cases = _cases()
    rows = _run_header(tmp_path, cases)
    worst = {}
    for (d, kind, level, smooth, p, c, tag), got in zip(cases, rows):
        want = oc.observe_cell(p, c, kind, level, smooth)
        T, xmax = abs(oc._vol(p.tolist())), np.abs(p).max()
        ev, em = abs(got[0] - want[0]) / T, np.abs(got[1:] - want[1:]).max() / (T * xmax)
        worst[(d, tag)] = max(worst.get((d, tag), 0.0), ev / oc.EPS, em / oc.EPS)
        assert ev <= 64 * oc.EPS and em <= 64 * oc.EPS, (d, kind, level, c, tag, ev / oc.EPS, em / oc.EPS)
        if tag == "all_equal":
            assert abs(got[0] - T) <= 64 * oc.EPS * T
        if tag == "flipped" and kind != "sharp":
            assert got[0] < 0.0                                           # the signed volume of the positions
    print({k: "%.1f eps" % v for k, v in sorted(worst.items())})


def test_in_plus_out_is_the_whole_cell(tmp_path):
    """[c >= L] + [-c >= -L] covers the cell (the level set itself has measure zero for these values)."""
    cases = []
    for d in (2, 3):
        for perm in itertools.permutations(VALUES[d]):
            for level in LEVELS[d]:
                cases.append((d, "sharp", level, 1.0, SIMPLEX[d], perm, "in"))
                cases.append((d, "sharp", -level, 1.0, SIMPLEX[d], [-v for v in perm], "out"))
    rows = _run_header(tmp_path, cases)
    for k in range(0, len(cases), 2):
        d, p = cases[k][0], cases[k][4]
        T, xmax = oc._vol(p.tolist()), np.abs(p).max()
        whole = np.concatenate([[T], T * p.mean(axis=0)])
        err = np.abs(rows[k] + rows[k + 1] - whole)
        assert err[0] <= 64 * oc.EPS * T and err[1:].max() <= 64 * oc.EPS * T * xmax, (cases[k], err / (oc.EPS * T))


# ---- 2. the package's numpy statement ------------------------------------------------------------------------------------------
problem, reference, queries = oc.problem, oc.reference, oc.queries


@pytest.mark.parametrize("deformed", [False, True])
@pytest.mark.parametrize("name", ["rect", "box", "brain"])
def test_numpy_statement_matches_the_loop(name, deformed):
    from glimslib_amd.simulation_helpers import observables
    mesh, lab, n_labels, c, u = problem(name)
    want, counts, sum_abs = reference(name, deformed)
    d = mesh.points.shape[1]
    qs = queries(name)
    for k, q in enumerate(qs):
        if q[0] == "sharp":
            assert counts[k] == set(range(d + 2)), (q, counts[k])
    got = observables.observe(mesh.points, mesh.cells, lab, c, qs, n_labels, u=u if deformed else None)
    assert got.shape == (len(qs), n_labels, 1 + d)
    assert np.all(got[:, 0] == 0.0)                                        # no cell carries label 0
    xmax = np.abs(mesh.points).max() + (np.abs(u).max() if deformed else 0.0)
    oc.assert_close(got, want, len(mesh.cells), sum_abs, xmax, "%s deformed=%s" % (name, deformed))


def test_totals_and_centre_of_mass():
    from glimslib_amd.simulation_helpers import observables
    mesh, lab, n_labels, c, u = problem("box")
    t = observables.observe(mesh.points, mesh.cells, lab, c, [("sharp", -1.0), ("sharp", 2.0)], n_labels)
    V, com = observables.totals_and_com(t)
    vol = np.abs(observables.signed_volumes(mesh.points[mesh.cells]))
    assert abs(V[0, 0] - 2 * 1 * 1.5) < 1e-13 and abs(V[0, 1]) == 0.0
    assert abs(V[0, 2] - vol[lab == 1].sum()) < 1e-13 and abs(V[0, 3] - vol[lab == 2].sum()) < 1e-13
    assert np.abs(com[0, 0] - [1.0, 0.5, 0.75]).max() < 1e-13
    assert np.isnan(com[0, 1]).all() and np.isnan(com[1]).all() and np.all(V[1] == 0.0)


# ---- 3. the surface ---------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_carry_the_entry_points():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _backend.load_library()
    for name in ("glims_observe", "glims_observe_info"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _backend.SIGNATURES
        assert hasattr(lib, name)
    macros = dict(re.findall(r"#define GLIMS_OBSERVE_([A-Z_]+) (\d+)", code))
    assert {k: int(v) for k, v in macros.items()} == {"MASS": 0, "SHARP": 1, "SMOOTH": 2, "MAX_QUERIES": 8}
    assert _backend.OBSERVE_KINDS == {"mass": 0, "sharp": 1, "smooth": 2} == oc.KIND_ID
    assert _backend.OBSERVE_MAX_QUERIES == 8
    body = re.search(r"typedef struct glims_observable \{(.*?)\} glims_observable;", code, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert fields == [f for f, _ in _backend.Observable._fields_] == ["kind", "level", "smooth"]
    assert ctypes.sizeof(_backend.Observable) == 24                        # int + padding, two doubles
    assert _backend.SIGNATURES["glims_observe"][1][-2] == ctypes.POINTER(_backend.Observable)
    assert lib.glims_abi_version() == _backend.ABI_VERSION == 6
