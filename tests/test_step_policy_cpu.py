"""
The RD time stepper's policy on the host.  glimslib_amd/csrc/step_policy.h holds what a run remembers between steps
(RunMemory) and every decision of gl_step that is a function of scalars -- the forcing term, sweep or cheap residual, PCG or
the dot-free iteration, the forcing-mode machine, the second-solve guess's continuity check and back-off -- in plain C++17.
tests/step_policy_check.cpp asserts the rules as their comments state them; it is compiled with the host compiler alone (no
device code, no GPU) and run here.

Reference counterpart: none -- the reference's Newton solver takes a fixed relative tolerance (simulation_tumor_growth.py:126-130).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_policy_rules_hold_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "step_policy_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_policy_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
