#!/usr/bin/env python3
"""
Cost of the deformed-configuration samplers -> profiles/deformed_sampler_cost.jsonl, one JSON object
per case.

  python tools/deformed_sampler_cost.py [--which lattice,brain] [--grids 128,256] [--out profiles/deformed_sampler_cost.jsonl]
      lattice  a 100^3-cell box lattice (1.03 M nodes)        brain  the 1 M-node brain-like mesh
  Per mesh and grid: creation of the undeformed sampler and of the deformed one from GLIMS_DERIVE_CURRENT (a smooth
  displacement put into U by set_state, no solve), ALTERNATED in one process, each the median of 5 after a warm-up, host clock
  around the call (which synchronises its stream before it returns); one warp (order 1, scalar source of the grid's own size)
  and one back map.  The expectation to compare with, not a gate: deformed creation = undeformed creation + two streaming
  passes (k_deform_xyz over the nodes, k_deform_cells over the cells).

  Kernel times come from a kernel trace of the same cases, one directory per case (as tools/sampler_cost.py):
      rocprofv3 --kernel-trace --output-format csv -d DIR/lattice -- python tools/deformed_sampler_cost.py --which lattice --no-write
      python tools/deformed_sampler_cost.py --which lattice --trace DIR
  adds the medians of k_deform_xyz, k_deform_cells and k_warp and the byte model's bytes over those times.  Without --trace the
  entry says "not measured".  --merge JSONL --trace DIR attaches the medians to records written earlier, without a GPU run.

  --parent-lib PATH: undeformed creation on this build next to another build of the library (the parent commit's), each in
  fresh child processes that alternate (new, parent, new, parent), through the same raw ctypes calls; the spread between two
  runs of the SAME library is reported next to the difference between the libraries.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
KERNELS = ("k_deform_xyz", "k_deform_cells", "k_deform_min", "k_warp", "k_claim_grid", "k_weights")


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), (max(ts) - min(ts))


def kernel_medians(trace_dir):
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if not any(k in name for k in KERNELS):
                    continue
                key = name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
                key += " @%s" % row.get("Grid_Size", row.get("Grid_Size_X", "?"))          # the two grids launch different sizes
                out.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(median_us=statistics.median(v), launches=len(v)) for k, v in out.items()}


def attach_trace(rec, trace_dir):
    """Kernel medians of the case's mesh from its trace directory, and the byte model's bytes over those times.  The two grids
    of one mesh share a trace: k_deform_* launch over nodes / cells (the same for both), a k_warp launch belongs to the grid
    whose point count its launch size matches."""
    if not trace_dir or not glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rec["kernel_medians_us"] = "not measured (no kernel trace given)"
        return
    med = kernel_medians(trace_dir)
    blocks = (rec["n_points"] + 255) // 256
    # the same kernels with every gathered array counted ONCE (what DRAM has to deliver at least): coordinates per node, the
    # source image (of the grid's own size here) per voxel
    d = 3 if rec["case"].endswith("^3 grid") else 2
    nv = d + 1
    once = {"k_deform_xyz": rec["model_bytes"]["k_deform_xyz"],
            "k_deform_cells": rec["n_cells"] * 4 * nv + rec["n_nodes"] * 2 * 8 * d,
            "k_warp": rec["n_points"] * (4 + 8) + rec["n_found"] * nv * 12 + rec["n_nodes"] * 8 * d + rec["n_points"] * 8}
    rec["compulsory_bytes"] = {k: int(v) for k, v in once.items()}
    keep, rate, rate_once = {}, {}, {}
    for k, v in med.items():
        name, size = k.split(" @")
        base = name.split("<")[0]
        if base in ("k_warp", "k_weights") and size.isdigit() and int(size) not in (blocks, blocks * 256):
            continue
        keep[k] = v
        if base in rec["model_bytes"]:
            rate[name] = rec["model_bytes"][base] / (v["median_us"] * 1e-6) / 1e12
            rate_once[name] = once[base] / (v["median_us"] * 1e-6) / 1e12
    rec["kernel_medians_us"] = keep
    rec["model_bytes_over_time_TBs"] = rate
    rec["compulsory_bytes_over_time_TBs"] = rate_once


def mesh_of(which, n_points):
    from glimslib_amd import workloads
    from glimslib_amd.mesh import BoxMesh
    if which == "lattice":
        n = max(2, int(round(n_points ** (1.0 / 3.0))))
        m = BoxMesh((0., 0., 0.), (1., 1., 1.), n, n, n)
        return m.points, m.cells
    wl = workloads.config_brain_like(n_points, isolate=True)
    return wl.mesh.points, wl.mesh.cells


def smooth_u(pts, amp=0.03):
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    t = (pts - lo) / (hi - lo)
    d = pts.shape[1]
    return np.stack([amp * (hi - lo)[a] * np.sin(np.pi * t[:, (a + 1) % d]) * np.cos(0.5 * np.pi * t[:, a]) for a in range(d)],
                    axis=1)


def grid_over(pts, n):
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    size = (n,) * pts.shape[1]
    return lo - 0.02 * (hi - lo), 1.04 * (hi - lo) / (n - 1), size


def cases(which, pts, cells, grids, trace):
    from glimslib_amd import _backend
    d = pts.shape[1]
    nv = d + 1
    h = _backend.Handle(pts, cells, np.zeros(len(cells), dtype=np.int32))
    h.set_materials([0.1], [0.1], [0.1], [1.0], [0.3])
    h.set_options(dt=1.0, mech_precond=0)                      # (no multigrid hierarchy: the displacement is given, not solved)
    h.setup(True)
    u = smooth_u(pts)
    h.set_state(np.zeros(len(pts)), u.reshape(-1))
    recs = []
    for n in grids:
        origin, spacing, size = grid_over(pts + u, n)
        made = []

        def create(**kw):
            for s in made:
                s.close()
            made.clear()
            made.append(h.sampler_grid(origin, spacing, size, **kw))

        # alternated: undeformed, deformed, undeformed, ... -- the medians see the same drift
        create()
        create(deformed_by='current')
        tu, td = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            create()
            tu.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            create(deformed_by='current')
            td.append((time.perf_counter() - t0) * 1e3)
        s = made[0]
        img = np.random.default_rng(0).standard_normal(tuple(reversed(size)))
        rec = dict(case="%s, %d^%d grid" % (which, n, d), n_nodes=int(len(pts)), n_cells=int(len(cells)),
                   n_points=int(s.n_points), n_found=int(s.n_found), n_inverted=int(s.n_inverted), min_jacobian=s.min_jacobian,
                   ms_create_undeformed=statistics.median(tu), ms_create_undeformed_spread=max(tu) - min(tu),
                   ms_create_deformed=statistics.median(td), ms_create_deformed_spread=max(td) - min(td),
                   ms_warp_linear_1=median_ms(lambda: s.warp(img, origin, spacing))[0],
                   ms_back_map=median_ms(lambda: s.back_map())[0],
                   note="wall times of the C-ABI calls, host <-> device copies of their arguments and results included")
        by = {"k_deform_xyz": len(pts) * 24 * d, "k_deform_cells": len(cells) * (4 * nv + 2 * nv * 8 * d),
              "k_warp": s.n_points * 4 + s.n_found * (nv * 12 + nv * 8 * d + (1 << d) * 8) + s.n_points * 8}
        rec["model_bytes"] = {k: int(v) for k, v in by.items()}
        rec["model_note"] = ("k_deform_cells and k_warp count their gathers (coordinates, voxels) once per use; through the "
                             "caches the DRAM traffic is smaller")
        attach_trace(rec, trace)
        for s in made:
            s.close()
        recs.append(rec)
    h.close()
    return recs


# ---- undeformed creation on two builds of the library, raw ctypes in a child process -------------------------------------------
def raw_child(lib_path, which, n_points, n):
    pts, cells = mesh_of(which, n_points)
    lib = C.CDLL(lib_path)
    dp, ip, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    lib.glims_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int64, C.c_int64, C.c_int64, dp, i32, i32, C.c_int]
    lib.glims_sampler_create_grid.argtypes = [C.c_void_p, dp, dp, ip, C.c_int, ip]
    lib.glims_sampler_destroy.argtypes = [C.c_void_p, C.c_int64]
    lib.glims_destroy.argtypes = [C.c_void_p]
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    cl = np.ascontiguousarray(cells, dtype=np.int32)
    lab = np.zeros(len(cl), dtype=np.int32)
    h = C.c_void_p()
    st = lib.glims_create(C.byref(h), pts.shape[1], len(pts), len(pts), len(cl), pts.ctypes.data_as(dp), cl.ctypes.data_as(i32),
                          lab.ctypes.data_as(i32), 0)
    assert st == 0, st
    origin, spacing, size = grid_over(pts + smooth_u(pts), n)
    o, sp = np.ascontiguousarray(origin), np.ascontiguousarray(spacing)
    sz = np.ascontiguousarray(size, dtype=np.int64)

    def create():
        sid = C.c_int64(-1)
        assert lib.glims_sampler_create_grid(h, o.ctypes.data_as(dp), sp.ctypes.data_as(dp), sz.ctypes.data_as(ip), 0,
                                             C.byref(sid)) == 0
        lib.glims_sampler_destroy(h, sid.value)

    med, spread = median_ms(create)
    lib.glims_destroy(h)
    print(json.dumps(dict(lib=os.path.relpath(lib_path, ROOT), ms_create_undeformed=med, spread_ms=spread)), flush=True)


def parent_comparison(parent_lib, which, n_points, grids):
    from glimslib_amd import _backend
    recs = []
    for n in grids:
        runs = {"this": [], "parent": []}
        for _ in range(2):
            for name, path in (("this", _backend.LIB_PATH), ("parent", parent_lib)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--raw-lib", path, "--which", which,
                                      "--points", str(n_points), "--grids", str(n)], capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    raise RuntimeError(out.stderr[-2000:])
                runs[name].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_create_undeformed"])
        same = max(abs(runs[k][0] - runs[k][1]) for k in runs)
        diff = statistics.mean(runs["this"]) - statistics.mean(runs["parent"])
        recs.append(dict(case="undeformed creation, this build vs the parent's: %s, %d^3 grid" % (which, n),
                         ms_this=runs["this"], ms_parent=runs["parent"], ms_difference_of_means=diff,
                         ms_run_to_run_spread_same_library=same, within_spread=bool(abs(diff) <= same)))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="lattice,brain")
    ap.add_argument("--grids", default="128,256")
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deformed_sampler_cost.jsonl"))
    ap.add_argument("--trace", default=None)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--raw-lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--merge", default=None, metavar="JSONL",
                    help="no GPU run: read the records of JSONL, attach the kernel medians of --trace, write --out")
    a = ap.parse_args()
    grids = [int(v) for v in a.grids.split(",")]
    if a.merge:
        recs = [json.loads(line) for line in open(a.merge) if line.strip()]
        for r in recs:
            if "model_bytes" in r:
                attach_trace(r, os.path.join(a.trace, r["case"].split(",")[0]))
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
        return
    if a.raw_lib:
        raw_child(a.raw_lib, a.which, a.points, grids[0])
        return
    recs = []
    for which in a.which.split(","):
        pts, cells = mesh_of(which, a.points)
        for r in cases(which, pts, cells, grids, a.trace and os.path.join(a.trace, which)):
            recs.append(r)
            print(json.dumps(r), flush=True)
    if a.parent_lib:
        for r in parent_comparison(a.parent_lib, "lattice", a.points, grids):
            recs.append(r)
            print(json.dumps(r), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
