#!/usr/bin/env python3
"""
Cost of the samplers -> profiles/sampler_cost.jsonl, one JSON object per case.

  python tools/sampler_cost.py [--which bl,c3,host] [--out profiles/sampler_cost.jsonl]
      bl    the 1.04 M-node brain-like mesh under a 240 x 240 x 155 grid of 1 mm voxels
      c3    config C3 under its own vertex grid
      host  for scale: the host evaluation the package had before (fenics_local.Function.__call__) on a size it can finish,
            32^3 points on the 6 k-node brain-like mesh, next to the sampler on the same points (ratio reported, not asserted)
  Per case: sampler creation, one apply with 1 and with 3 components, one apply_t -- each the median of 5 calls after a
  warm-up; every call ends with a stream synchronise inside the library, i.e. inside the timed window, and includes the host
  <-> device copies of its arguments.  Algorithmic bytes per kernel from the shapes, and the share of 8 TB/s they would be at
  the measured KERNEL median when a trace is given:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/bl -- python tools/sampler_cost.py --which bl --no-write
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/c3 -- python tools/sampler_cost.py --which c3 --no-write
  python tools/sampler_cost.py --which bl,c3,host --trace DIR   # adds kernel medians from DIR/<case>/**/*_kernel_trace.csv
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_medians(trace_dir):
    """{kernel name prefix: median us} over the sampler kernels of a rocprofv3 --kernel-trace CSV."""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "k_sample" not in name and "k_claim" not in name and "k_weights" not in name:
                    continue
                key = name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
                out.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(median_us=statistics.median(v), launches=len(v)) for k, v in out.items()}


# kernel (as the trace names it, without its dimension argument) -> entry of the byte table
BYTES_OF = {"k_sample<%d, 1>": "k_sample_1", "k_sample<%d, 3>": "k_sample_3", "k_claim_grid<%d>": "k_claim_grid",
            "k_weights<%d>": "k_weights", "k_sample_t_cells<%d>": "k_sample_t_cells_1", "k_sample_t<%d>": "k_sample_t_1"}


def case(name, pts, cells, origin, spacing, size, trace):
    from glimslib_amd import _backend
    d = pts.shape[1]
    nv = d + 1
    h = _backend.Handle(pts, cells, np.zeros(len(cells), dtype=np.int32))
    made = []

    def create():
        for s in made:
            s.close()
        made.clear()
        made.append(h.sampler_grid(origin, spacing, size))

    t_create = median_ms(create)
    s = made[0]
    f1 = np.random.default_rng(0).standard_normal(len(pts))
    f3 = np.random.default_rng(1).standard_normal((len(pts), 3))
    r1 = np.random.default_rng(2).standard_normal(s.n_points)
    rec = dict(case=name, n_nodes=int(len(pts)), n_cells=int(len(cells)), n_points=int(s.n_points), n_found=int(s.n_found),
               ms_create=t_create, ms_apply_1=median_ms(lambda: s.apply(f1)), ms_apply_3=median_ms(lambda: s.apply(f3)),
               ms_apply_t_1=median_ms(lambda: s.apply_t(r1)),
               note="wall times of the C-ABI calls, host <-> device copies of the arguments included")
    # algorithmic bytes: apply reads (4 + 8) B per vertex of a found point, writes 8 ncomp B per point, and reads the nodal
    # field once; location reads each cell's geometry (vertex ids + coordinates) once and 4 B per claimed point
    by = {}
    for k in (1, 3):
        by["k_sample_%d" % k] = s.n_found * nv * 12 + s.n_points * (4 + 8 * k) + len(pts) * 8 * k
    by["k_claim_grid"] = len(cells) * nv * (4 + 8 * d) + s.n_found * 4
    by["k_weights"] = s.n_points * (4 + nv * 12) + s.n_found * nv * (4 + 8 * d)
    n_lists = min(len(cells), s.n_found)                    # cells that hold a point: one chunk each, or a few
    by["k_sample_t_cells_1"] = s.n_found * (4 + nv * 8 + 8) + n_lists * nv * 8
    # pass 2: a node's incidence records (cell 4 B, slots 4 B), two chunk offsets per record, one q entry per held cell
    by["k_sample_t_1"] = len(cells) * nv * (4 + 4 + 8) + n_lists * nv * 8 + len(pts) * (8 + 1 + 16)
    rec["algorithmic_bytes"] = {k: int(v) for k, v in by.items()}
    if trace:
        med = kernel_medians(trace)
        rec["kernel_medians_us"] = med
        rec["share_of_8TBs"] = {}
        for pat, b in BYTES_OF.items():
            k = pat % (nv if "k_sample" in pat else d)
            if k in med:
                rec["share_of_8TBs"][k] = by[b] / (med[k]["median_us"] * 1e-6) / PEAK
    else:
        rec["kernel_medians_us"] = "not measured (no --trace given)"
    h.close()
    return rec


def host_case():
    from glimslib_amd import _backend, fenics_local as fenics, workloads
    wl = workloads.config_brain_like(5000, isolate=True)
    pts, cells = wl.mesh.points, wl.mesh.cells
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    size = (32, 32, 32)
    spacing = (hi - lo) / (np.array(size) - 1)
    f = np.random.default_rng(0).standard_normal(len(pts))
    fn = fenics.Function(wl.mesh, {None: f})
    ax = [lo[a] + np.arange(size[a]) * spacing[a] for a in range(3)]
    g = np.stack(np.meshgrid(*ax[::-1], indexing='ij')[::-1], axis=-1).reshape(-1, 3)
    t0 = time.perf_counter()
    host = np.asarray(fn(g))
    t_host = (time.perf_counter() - t0) * 1e3
    h = _backend.Handle(pts, cells, np.zeros(len(cells), dtype=np.int32))
    t0 = time.perf_counter()
    s = h.sampler_grid(lo, spacing, size)
    dev = s.apply(f)
    t_dev = (time.perf_counter() - t0) * 1e3
    ok = ~np.isnan(dev)
    rec = dict(case="host path for scale: 32^3 points, %d nodes" % len(pts), ms_host_function_call=t_host,
               ms_sampler_create_plus_apply=t_dev, ratio=t_host / t_dev, n_found=int(ok.sum()),
               max_abs_difference=float(np.abs(dev[ok] - host[ok]).max()))
    h.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="bl,c3,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_cost.jsonl"))
    ap.add_argument("--trace", default=None)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--bl-points", type=int, default=1000000)
    a = ap.parse_args()
    from glimslib_amd import workloads
    recs = []
    for which in a.which.split(","):
        if which == "bl":
            wl = workloads.config_brain_like(a.bl_points, isolate=True)
            pts = wl.mesh.points
            lo = pts.min(axis=0)
            recs.append(case("brain-like mesh, 240 x 240 x 155 grid of 1 mm voxels", pts, wl.mesh.cells, lo + 0.5,
                             (1.0, 1.0, 1.0), (240, 240, 155), a.trace and os.path.join(a.trace, "bl")))
        elif which == "c3":
            from glimslib_amd.utils.data_io import get_measures_from_structured_mesh
            wl = workloads.config_c3()
            origin, size, spacing, _, _ = get_measures_from_structured_mesh(wl.mesh)
            recs.append(case("C3 under its own vertex grid", wl.mesh.points, wl.mesh.cells, origin, spacing, size,
                             a.trace and os.path.join(a.trace, "c3")))
        elif which == "host":
            recs.append(host_case())
        print(json.dumps(recs[-1]), flush=True)
    if not a.no_write:
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
