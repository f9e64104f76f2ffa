"""
The host side of the adjoint calls.  glimslib_amd/csrc/hessian_plan.h holds what sizes a gradient or Hessian call (HessShape and
the rules for its flags), the table of every device buffer the call allocates (hessian_buffers; the memory estimate
hessian_bytes is its sum, and adjoint.hip allocates from it), the per-label direction tables of a Hessian call (HessDirections),
the fold of the ranks' per-label sums in rank order (add_rows_in_rank_order, label_row_parts, scatter_row) and their combination
into the Hessian rows (hessian_label_rows) -- in plain C++17.  tests/hessian_plan_check.cpp asserts: the table's sum against the
formula it replaces (at least as large, larger by exactly the listed buffers that formula left out, every entry present exactly
when its flag says so), the layout and values of the direction tables, the rows against the formulas of lame_derivs.h written
out (a label with 2 mu + d lambda = 0 included, null outputs untouched between canaries) and the fold bit for bit.  It is
compiled with the host compiler alone (no device code, no GPU) and run here.

Reference counterpart: none -- the reference differentiates its forms symbolically and lets its adjoint library manage memory;
it has no buffer plan, no direction tables and no ranks to fold.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hessian_plan_holds_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.fail("no hipcc to compile the host-side check with")
    exe = str(tmp_path / "hessian_plan_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "glimslib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hessian_plan_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
