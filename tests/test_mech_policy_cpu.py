"""
The elasticity solve's policy on the host.  glimslib_amd/csrc/mech_policy.h holds the ring of stored solves (MechRing), the
least-squares fit that turns the solve history into an initial guess (mech_history_fit: trace-scaled ridge, elimination with
partial pivoting, fallback to the plain warm start) and every rule of gl_solve_mechanics that is a function of scalars -- when
the mixed-precision solve is used, when the verification loop ends, the refinement loop's tolerances -- in plain C++17.
tests/mech_policy_check.cpp asserts them as their comments state them; it is compiled with the host compiler alone (no device
code, no GPU) and run here.

Reference counterpart: none -- the reference solves its linear systems with a sparse LU factorisation (the SNES solver's default
direct solver, simulation_tumor_growth.py:126-131): it has no initial guess, no solve history and no iteration to control.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mech_policy_rules_hold_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "mech_policy_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mech_policy_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
