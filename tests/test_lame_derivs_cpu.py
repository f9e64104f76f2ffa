"""
The derivatives of the Lame pair on the host.  glimslib_amd/csrc/lame_derivs.h holds the first and second derivatives of
(m, l) = (E / (2 (1 + nu)), E nu / ((1 + nu)(1 - 2 nu))) in (E, nu) and the host combination of the elastic adjoint's per-label
sums into dJ/dE, dJ/dnu and their Hessian rows (glims_adjoint_gradient_full, glims_adjoint_hessian_full) in plain C++.
tests/lame_derivs_check.cpp checks the second derivatives by central differences of the first (<= 1e-7 relative, at nu in
{-0.3, 0, 0.1, 0.4, 0.49} and E in {1e-3, 1, 1e7}); it is compiled with the host compiler alone (no device code, no GPU) and
run here, and the first derivatives it prints are compared with the numpy reference's.

Reference counterpart: compute_mu / compute_lambda (simulation_helpers/math_linear_elasticity.py); the reference differentiates
them symbolically through dolfin-adjoint and has no closed forms of its own.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from adjoint_elastic_common import lame_derivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lame_second_derivatives_match_differences_and_first_match_numpy(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "lame_derivs_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lame_derivs_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = np.array([[float(x) for x in line.split()] for line in r.stdout.splitlines()])
    assert rows.shape == (15, 6)
    assert set(rows[:, 0]) == {1e-3, 1.0, 1e7} and set(rows[:, 1]) == {-0.3, 0.0, 0.1, 0.4, 0.49}
    ref = lame_derivatives(rows[:, 0], rows[:, 1])
    # the same closed forms in double on both sides: they differ by the rounding of a handful of operations
    for col, (key, k) in zip(range(2, 6), (("E", 0), ("E", 1), ("nu", 0), ("nu", 1))):
        want = np.broadcast_to(ref[key][k], rows[:, col].shape)
        assert np.all(np.abs(rows[:, col] - want) <= 1e-14 * np.abs(want)), (key, k, rows[:, col], want)


def test_numpy_second_derivatives_are_the_header_formulas():
    """tests/adjoint_hessian_elastic_common.lame_second_derivatives (what the numpy Hessian uses) against differences of
    lame_derivatives, as the host check does for the header."""
    from adjoint_hessian_elastic_common import lame_second_derivatives
    for E in (1e-3, 1.0, 1e7):
        for nu in (-0.3, 0.0, 0.1, 0.4, 0.49):
            d2 = lame_second_derivatives(E, nu)
            hn, hE = 3e-7, 1e-4 * E
            up, dn = lame_derivatives(E, nu + hn), lame_derivatives(E, nu - hn)
            eu, ed = lame_derivatives(E + hE, nu), lame_derivatives(E - hE, nu)
            for k in range(2):
                assert abs((up["nu"][k] - dn["nu"][k]) / (2 * hn) - d2["nunu"][k]) <= 1e-7 * abs(d2["nunu"][k])
                assert abs((up["E"][k] - dn["E"][k]) / (2 * hn) - d2["Enu"][k]) <= 1e-7 * abs(d2["Enu"][k])
                assert abs((eu["nu"][k] - ed["nu"][k]) / (2 * hE) - d2["Enu"][k]) <= 1e-7 * abs(d2["Enu"][k])
                assert d2["EE"][k] == 0.0 and abs(eu["E"][k] - ed["E"][k]) <= 1e-12 * abs(eu["E"][k])
