"""
Which instance of the incidence-list kernels a launch gets (glimslib_amd/csrc/sweep_instances.h): tests/sweep_instances_check.cpp
holds the policy as literal tables -- the bound ladder 16 / 20 / 24 / 32 / looped, the records per round trip of the sweep and of
the quadratic-term pass, the one 25-record instance, the refusals, the LDS bytes, 280 + 20 distinct instances -- and compares
them with the header over its whole input space, compiled with the host compiler alone.

Reference counterpart: none (a launch policy of this implementation).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_rules_hold_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "sweep_instances_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sweep_instances_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
