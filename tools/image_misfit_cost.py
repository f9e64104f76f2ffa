#!/usr/bin/env python3
"""
Cost of the image-space misfit terms (DESIGN.md sections 13 and 14) -> profiles/image_misfit_cost.jsonl, one JSON object.

  python tools/image_misfit_cost.py [--points 1000000] [--steps 2] [--out profiles/image_misfit_cost.jsonl]
      The 1.04 M-node brain-like mesh under a 240 x 240 x 155 grid of 1 mm voxels (the case of tools/sampler_cost.py), a
      recording of --steps steps, a threshold image of the last state as the target.
      (a) median wall time of a gradient call with ONE img_thresh term, of the same call with a nodal c_thresh term in its
          place, and their difference: what observing in image space costs per evaluation;
      (b) in the same process the host composition the term replaces: sampler.apply -> numpy -> sampler.apply_t.
      The one pass condition is (a)'s difference < (b) ("device_path_cheaper_than_host_composition").
  Kernel medians come from a kernel trace of their own (one gradient and one 1-direction Hessian call; the mesh must come
  from GLIMS_MESH_CACHE, filled by the first command, because a profiled process may not start the mesh builder's children):

  GLIMS_MESH_CACHE=DIR/mesh python tools/image_misfit_cost.py
  GLIMS_MESH_CACHE=DIR/mesh rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- \\
      python tools/image_misfit_cost.py --trace-run
  python tools/image_misfit_cost.py --merge DIR/trace     # no GPU: adds kernel medians and shares of 8 TB/s to the record
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
KERNELS = ("k_img_misfit_dir", "k_img_misfit", "k_img_sum", "k_sample_t_cells", "k_sample_t")


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_medians(trace_dir):
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "").replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
                base = name.split("<")[0]
                if base in KERNELS:
                    out.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(median_us=statistics.median(v), launches=len(v)) for k, v in out.items()}


def thresh(x, level, smooth):
    return 0.5 * (np.tanh((x - level) / smooth) + 1.0)


def build(n_points, n_steps):
    from glimslib_amd import _backend, workloads
    wl = workloads.config_brain_like(n_points, isolate=True)
    pts, cells = wl.mesh.points, wl.mesh.cells
    t = {k: np.asarray(v, dtype=np.float64) for k, v in wl.tables.items()}
    h = _backend.Handle(pts, cells, np.asarray(wl.cell_label, dtype=np.int32))
    h.set_materials(t["D"], t["rho"], t["gamma"], t["E"], t["nu"])
    h.set_options(dt=wl.dt)
    h.setup(with_mechanics=False)
    h.set_state(wl.c0)
    h.adjoint_record(True)
    assert h.step(n_steps) == 0
    s = h.sampler_grid(pts.min(axis=0) + 0.5, (1.0, 1.0, 1.0), (240, 240, 155))
    return h, s, pts, cells


def measure(a):
    level, smooth = 0.3, 0.1
    h, s, pts, cells = build(a.points, a.steps)
    nv = pts.shape[1] + 1
    c = h.get_state(want_u=False)[0]
    target = thresh(1.1 * s.apply('c'), level, smooth)            # NaN outside the mesh: not observed
    img = [dict(step=a.steps, kind="img_thresh", level=level, smooth=smooth, sampler=s, target=target)]
    nod = [dict(step=a.steps, kind="c_thresh", level=level, smooth=smooth, target=thresh(1.1 * c, level, smooth))]
    if a.trace_run:   # what the kernel trace needs: the two new kernels and both transpose launches, a few times each
        for _ in range(5):
            h.adjoint_gradient(img, want_dc0=False)
        h.adjoint_hessian(img, [dict(D=np.ones(h.n_labels))])
        h.close()
        return None
    ms_img = median_ms(lambda: h.adjoint_gradient(img, want_dc0=False))
    n_obs = h.image_term_info(0)[2]
    ms_nod = median_ms(lambda: h.adjoint_gradient(nod, want_dc0=False))

    def host():
        v = s.apply('c')                                            # the state after the last step
        th = np.tanh((v - level) / smooth)
        r = np.where(np.isnan(target), 0.0, 0.5 * (1.0 - th * th) / smooth * (0.5 * (th + 1.0) - target))
        return s.apply_t(np.nan_to_num(r))

    ms_host = median_ms(host)
    n, nn, ne = s.n_points, len(pts), len(cells)
    n_lists = min(ne, s.n_found)
    by = {"k_img_misfit<%d>" % nv: n_obs * nv * 12 + n * (8 + 8) + nn * 8,
          "k_img_misfit_dir<%d>" % nv: n_obs * nv * 12 + n * (8 + 8) + nn * 8 * 2,      # one direction
          "k_sample_t_cells<%d>" % nv: s.n_found * (4 + nv * 8 + 8) + n_lists * nv * 8,
          "k_sample_t<%d>" % nv: ne * nv * (4 + 4 + 8) + n_lists * nv * 8 + nn * (8 + 8 + 1 + 16)}
    rec = dict(case="brain-like mesh, 240 x 240 x 155 grid of 1 mm voxels, %d recorded steps" % a.steps, n_nodes=int(nn),
               n_cells=int(ne), n_points=int(n), n_found=int(s.n_found), n_observed=int(n_obs),
               ms_gradient_one_img_thresh=ms_img, ms_gradient_one_c_thresh=ms_nod, ms_image_term_extra=ms_img - ms_nod,
               ms_host_apply_numpy_apply_t=ms_host,
               device_path_cheaper_than_host_composition=bool(ms_img - ms_nod < ms_host),
               algorithmic_bytes={k: int(v) for k, v in by.items()},
               bytes_per_point_model="NV (4 + 8) + 8 (t) + 8 (q, if present) + 8 (r); no q in this case",
               kernel_medians_us="not measured (no --merge of a kernel trace yet)",
               note="wall times are medians of 5 calls after a warm-up, host <-> device copies of the arguments included")
    h.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_misfit_cost.jsonl"))
    ap.add_argument("--trace-run", action="store_true", help="only issue the calls a kernel trace needs; writes nothing")
    ap.add_argument("--merge", default=None, metavar="DIR", help="add the kernel medians of the trace under DIR to --out")
    a = ap.parse_args()
    if a.merge:
        with open(a.out) as f:
            rec = json.loads(f.readline())
        med = kernel_medians(a.merge)
        rec["kernel_medians_us"] = med
        rec["share_of_8TBs"] = {k: rec["algorithmic_bytes"][k] / (med[k]["median_us"] * 1e-6) / PEAK
                                for k in rec["algorithmic_bytes"] if k in med}
    else:
        rec = measure(a)
        if rec is None:
            return
    print(json.dumps(rec), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
