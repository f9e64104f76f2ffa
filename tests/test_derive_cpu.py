"""
Derived fields on the device (glims_derive), the parts that need no GPU:
  1. the numpy statement of the contract (tests/derive_common.py) against analytic answers (u = A x, c = c0, two labels that
     differ in E, nu, gamma, rho) in 2-D and 3-D, and against the right-hand-side builders of the PostProcess class (its
     np.add.at loops, with the device's mass solve replaced by a direct one) on random fields;
  2. the committed quadrature constants (csrc/derive_quadrature.h) through tests/derive_quadrature_check.cpp, compiled with the
     host compiler alone: weights, monomials up to degree 7, and the numbers themselves against simplex_quadrature(d, 4);
  3. the header declares the entry points and the ctypes table carries them.

Reference counterpart: the PostProcess classes, glimslib/simulation_helpers/helper_classes.py:1521-1972.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from glimslib_amd import fenics_local as fenics
from glimslib_amd.simulation_helpers.postprocess import PostProcess, simplex_quadrature
from oracle.glims_oracle import rel_l2

import derive_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mesh(dim):
    return (fenics.RectangleMesh((0, 0), (2, 1), 12, 9) if dim == 2 else fenics.BoxMesh((0, 0, 0), (2, 1, 1.5), 5, 4, 4))


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_reproduces_analytic_answers(dim):
    mesh = _mesh(dim)
    lab = dc.two_labels(mesh)
    assert set(np.unique(lab)) == {1, 2}
    ref = dc.DeriveReference(mesh.points, mesh.cells, lab, dc.TABLES)
    A = 0.01 * (np.arange(dim * dim).reshape(dim, dim) + 1.0)
    A[0, 0] += 0.03
    c0 = 0.35
    u = mesh.points @ A.T
    c = np.full(len(mesh.points), c0)
    eps = 0.5 * (A + A.T)
    jt = np.linalg.det(np.eye(dim) + A)
    assert np.abs(ref.field("strain_tensor", u=u) - eps).max() < 1e-12
    assert np.abs(ref.field("total_jacobian", u=u) - jt).max() < 1e-12
    # piecewise constant per label: compare the RIGHT-HAND SIDES (the projection of a discontinuous field is not the field)
    mu, lam = ref.lame()
    sig = 2.0 * mu[:, None, None] * eps + (lam * np.trace(eps))[:, None, None] * np.eye(dim)
    want = ref.project_cell(sig.reshape(-1, dim * dim)).reshape(-1, dim, dim)
    assert np.abs(ref.field("stress_tensor", u=u) - want).max() < 1e-12 * np.abs(want).max()
    assert np.abs(ref.field("pressure", u=u) - np.trace(want, axis1=1, axis2=2) / 3.0).max() < 1e-12 * np.abs(want).max()
    # one label over the whole mesh: every field is a constant the P1 space holds exactly
    one = dc.DeriveReference(mesh.points, mesh.cells, np.ones(len(mesh.cells), dtype=np.int32), dc.TABLES)
    E, nu, gamma, rho = (dc.TABLES[k][1] for k in ("E", "nu", "gamma", "rho"))
    m, l = E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))
    s1 = 2 * m * eps + l * np.trace(eps) * np.eye(dim)
    dev = s1 - np.trace(s1) / 3.0 * np.eye(dim)
    answers = {"stress_tensor": s1, "pressure": np.trace(s1) / 3.0, "van_mises_stress": np.sqrt(1.5 * (dev * dev).sum()),
               "log_growth": rho * c0 * (1 - c0), "mech_expansion": gamma * c0, "total_jacobian": jt,
               "growth_induced_jacobian": (1 + gamma * c0) ** dim,
               "concentration_deformed_config": c0 * (1 + gamma * c0) ** dim / jt}
    for kind, val in answers.items():
        got = one.field(kind, c=c, u=u)
        assert np.abs(got - val).max() < 1e-12 * max(1.0, np.abs(val).max()), kind
    # two labels, uniform c: the growth strain of the non-uniform branch is the projection of gamma_T c0
    want = ref.project_cell(ref.cell["gamma"] * c0)
    assert np.abs(ref.field("mech_expansion", c=c) - want).max() < 1e-12


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_matches_the_class_on_random_fields(dim):
    """The PostProcess class's own loops (np.add.at per quadrature point and vertex) with a direct mass solve."""
    mesh = _mesh(dim)
    lab = dc.two_labels(mesh)
    ref = dc.DeriveReference(mesh.points, mesh.cells, lab, dc.TABLES)
    c, u = dc.sample_fields(mesh.points, seed=dim)

    class _Results:
        def __init__(self, V):
            self._functionspace = V

        def get_solution_function(self, subspace_name=None, recording_step=None):
            return fenics.Function(mesh, {None: u if subspace_name == 'displacement' else c})

    class _Space:
        _mesh = mesh

    pp = PostProcess(_Results(_Space()), None, tables=dc.TABLES, labels=lab)
    pp._solve_mass = lambda rhs: ref.solve(rhs)
    getters = {"strain_tensor": pp.get_strain_tensor, "stress_tensor": pp.get_stress_tensor, "pressure": pp.get_pressure,
               "van_mises_stress": pp.get_van_mises_stress, "displacement_norm": pp.get_displacement_norm,
               "log_growth": pp.get_logistic_growth, "total_jacobian": pp.get_total_jacobian,
               "growth_induced_jacobian": pp.get_growth_induced_jacobian,
               "concentration_deformed_config": pp.get_concentration_deformed_configuration}
    for kind, get in getters.items():
        assert rel_l2(ref.field(kind, c=c, u=u), get().values()) < 1e-12, kind
    s = ref.field("mech_expansion", c=c)
    assert rel_l2(s[:, None, None] * np.eye(dim), pp.get_mech_expansion().values()) < 1e-12


def test_quadrature_header_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "derive_quadrature_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "derive_quadrature_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.splitlines()], dtype=object)
    for d in (2, 3):
        mine = np.array([row[2:] for row in rows if int(row[0]) == d], dtype=np.float64)
        lam, w = simplex_quadrature(d, 4)
        assert mine.shape == (4 ** d, d + 2)
        assert np.abs(mine[:, :d + 1] - lam).max() <= 1e-16
        assert np.abs(mine[:, d + 1] - w).max() <= 1e-16


def test_header_and_ctypes_carry_the_entry_points():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("glims_derive", "glims_derive_info"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _backend.SIGNATURES
        assert hasattr(_backend.load_library(), name)
    assert re.search(r"#define GLIMS_FIELD_DERIVED 4\b", code) and _backend.FIELD_DERIVED == 4
    assert re.search(r"#define GLIMS_DERIVE_CURRENT \(-1\)", code) and _backend.DERIVE_CURRENT == -1
    assert re.search(r"#define GLIMS_DERIVE_HOST \(-2\)", code) and _backend.DERIVE_HOST == -2
    for name, k in _backend.DERIVE_KINDS.items():
        assert name in dc.KINDS and dc.KINDS.index(name) == k
    macros = dict(re.findall(r"#define GLIMS_DERIVE_([A-Z_]+) (\d+)", code))
    assert [int(macros[m]) for m in ("STRAIN", "STRESS", "PRESSURE", "VON_MISES", "DISP_NORM", "LOG_GROWTH", "MECH_EXPANSION",
                                     "TOTAL_JACOBIAN", "GROWTH_JACOBIAN", "CONC_DEFORMED")] == list(range(10))
    assert _backend.SIGNATURES["glims_derive"][1][1:4] == [_backend.C.c_int, _backend.C.c_int64, _backend.C.POINTER(_backend.C.c_double)]
    assert _backend.ABI_VERSION == 6
