#!/usr/bin/env python3
"""
Cost of an image term in the DEFORMED configuration ("Image terms in the deformed configuration")
-> profiles/deformed_term_cost.jsonl, one JSON object per run (appended).

  python tools/deformed_term_cost.py [--points 1000000] [--steps 2] [--grid 128] [--out profiles/deformed_term_cost.jsonl]
      The brain-like mesh (clamped exterior, mechanics on) under a --grid^3 voxel grid over its bounding box, a recording of
      --steps steps, a threshold image of the last state as the target.  In ONE process, on ONE handle, median wall time of
        (a) a gradient call with the term FIXED (glims_adjoint_image_terms on a sampler of the grid: the parent's path, no
            elastic solve), and
        (b) the same call with the term DEFORMED (glims_adjoint_deformed_image_terms: u_k and mu_k solved, the grid located in
            the displaced mesh, the misfit kernel, two transposes),
      and (c) the same call with the fixed term plus a u_l2 term on the step, which pays the two elastic solves without the
      location -- (b) - (c) is what the location and the new kernel cost, (c) - (a) what the solves cost.
      No ratio is promised: the record is the measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def thresh(x, level, smooth):
    return 0.5 * (np.tanh((x - level) / smooth) + 1.0)


def measure(a):
    from glimslib_amd import _backend, workloads
    from oracle.glims_oracle import boundary_facets
    wl = workloads.config_brain_like(a.points, isolate=True)
    pts, cells = np.asarray(wl.mesh.points, dtype=np.float64), wl.mesh.cells
    t = {k: np.asarray(v, dtype=np.float64) for k, v in wl.tables.items()}
    h = _backend.Handle(pts, cells, np.asarray(wl.cell_label, dtype=np.int32))
    h.set_materials(t["D"], t["rho"], t["gamma"], t["E"], t["nu"])
    h.set_options(dt=wl.dt)
    xb = np.unique(boundary_facets(cells)[0])
    h.set_dirichlet_u((xb[:, None] * 3 + np.arange(3)[None]).ravel(), np.zeros(len(xb) * 3))
    h.setup(with_mechanics=True)
    h.set_state(wl.c0)
    h.adjoint_record(True)
    assert h.step(a.steps) == 0
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    size = (a.grid,) * 3
    spacing = (hi - lo) / a.grid
    origin = lo + 0.5 * spacing
    s = h.sampler_grid(origin, spacing, size)
    level, smooth = 0.3, 0.1
    target = thresh(1.1 * s.apply('c'), level, smooth)            # NaN outside the mesh: not observed
    base = dict(step=a.steps, kind="img_thresh", level=level, smooth=smooth, target=target)
    fixed = [dict(base, sampler=s)]
    moving = [dict(base, deformed=True, scale=1.0, grid=(origin, spacing, size))]
    with_u = fixed + [dict(step=a.steps, kind="u_l2", target=np.zeros(len(pts) * 3))]
    L = h.n_labels
    ms_fixed = median_ms(lambda: h.adjoint_gradient(fixed, L, want_dc0=False, elastic=True), a.reps)
    ms_fixed_u = median_ms(lambda: h.adjoint_gradient(with_u, L, want_dc0=False, elastic=True), a.reps)
    st0 = h.adjoint_stats()
    ms_moving = median_ms(lambda: h.adjoint_gradient(moving, L, want_dc0=False, elastic=True), a.reps)
    st1 = h.adjoint_stats()
    info = h.deformed_image_term_info(0)
    calls = st1["gradients"] - st0["gradients"]
    rec = dict(case="brain-like mesh, clamped exterior, %d^3 grid over its bounding box, %d recorded steps" % (a.grid, a.steps),
               n_nodes=int(len(pts)), n_cells=int(len(cells)), n_points=int(s.n_points), n_found_fixed=int(s.n_found),
               deformed_info=info,
               ms_gradient_term_fixed=ms_fixed, ms_gradient_term_fixed_plus_u_l2=ms_fixed_u, ms_gradient_term_deformed=ms_moving,
               ms_location_and_kernel=ms_moving - ms_fixed_u, ms_two_elastic_solves=ms_fixed_u - ms_fixed,
               elastic_solves_per_deformed_call=(st1["mech_solves"] - st0["mech_solves"]) / max(1, calls),
               elastic_pcg_its_per_deformed_call=(st1["mech_its"] - st0["mech_its"]) / max(1, calls),
               bytes_per_point_model="4 (cell) + NV (4 + 8) + 8 (t) + 8 (q, if present) + 8 (r) + 8 D (S); no q in this case; "
                                     "16 D NV of coordinates and 8 NV of c gathered through the caches",
               note="wall times are medians of %d calls after a warm-up, on one handle in one process" % a.reps)
    h.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deformed_term_cost.jsonl"))
    a = ap.parse_args()
    rec = measure(a)
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
