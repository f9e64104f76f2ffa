#!/usr/bin/env python
"""
What a stored displacement-image misfit term (glims_adjoint_displacement_image_terms) costs next to the elastic solve of the
step it observes, on the brain-like unstructured mesh with mechanics on and the exterior clamped: a `--grid`^3 voxel grid over
the mesh's bounding box, its target the sampled displacement of the recorded step times 0.9, with a mask.  From the library's
own HIP event pairs (GLIMS_UIMG_TIMING; they synchronise the stream): the misfit kernel with its sum, and the transpose into
the elastic adjoint's load; from the host clock around it: the u_k solve of the step.  Medians of `--reps` gradient calls after
one warm-up, with the algorithmic bytes of the kernel.

    python tools/displacement_image_cost.py [--nodes 1000000] [--grid 128] [--steps 2] [--reps 5]

Writes one JSON line to profiles/displacement_image_cost.jsonl (or --out).
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_calls(h, terms, n_labels, reps):
    """per call after one warm-up: (misfit ms, transpose ms, u_k solve ms, its)"""
    os.environ["GLIMS_UIMG_TIMING"] = "1"
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 1):
                h.adjoint_gradient(terms, n_labels, want_dc0=False)
                os.write(2, b"glims displacement image terms: end of call\n")
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["GLIMS_UIMG_TIMING"]
        tmp.seek(0)
        calls, cur = [], [None, None, None, None]
        for line in tmp.read().decode().splitlines():
            if "end of call" in line:
                calls.append(cur)
                cur = [None, None, None, None]
            m = re.search(r"misfit ([0-9.]+) ms\s+transpose ([0-9.]+) ms", line)
            if m:
                cur[0], cur[1] = float(m.group(1)), float(m.group(2))
            m = re.search(r"u_k solve ([0-9.]+) ms\s+(\d+) iterations", line)
            if m:
                cur[2], cur[3] = float(m.group(1)), int(m.group(2))
    return calls[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "displacement_image_cost.jsonl"))
    args = ap.parse_args()
    from glimslib_amd import _backend, workloads
    from oracle.glims_oracle import boundary_facets
    w = workloads.config_brain_like(args.nodes, isolate=True)   # (the mesh builder forks: not from this process)
    mesh, d = w.mesh, w.mesh.points.shape[1]
    pts = np.asarray(mesh.points, dtype=np.float64)
    n_labels = len(w.tables["D"])
    h = _backend.Handle(pts, mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[w.tables[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=w.dt)
    xb = np.unique(boundary_facets(mesh.cells)[0])
    h.set_dirichlet_u((xb[:, None] * d + np.arange(d)[None]).ravel(), np.zeros(len(xb) * d))
    h.setup(with_mechanics=True)
    h.set_state(w.c0)
    h.adjoint_record(True)
    assert h.step(args.steps) == _backend.GLIMS_OK
    assert h.solve_mechanics() == _backend.GLIMS_OK
    u = h.get_state()[1]
    size = np.full(d, args.grid)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    spacing = (hi - lo) / (size - 1) * 0.999
    origin = lo + 0.0005 * (hi - lo)
    t0 = time.perf_counter()
    sampler = h.sampler_grid(origin, spacing, size)
    locate_s = time.perf_counter() - t0
    target = 0.9 * sampler.apply(np.asarray(u).reshape(-1, d), fill=np.nan)
    rng = np.random.default_rng(0)
    mask = np.where(rng.random(len(target)) < 0.1, 0.0, 1.0)
    term = dict(step=args.steps, kind="img_u_l2", sampler=sampler, target=target, pweight=mask, weight=1.0)
    walls = []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        J = h.adjoint_gradient([term], n_labels, want_dc0=False)[0]
        walls.append(time.perf_counter() - t0)
    calls = timed_calls(h, [term], n_labels, args.reps)
    med = lambda k: round(float(np.median([c[k] for c in calls])), 4)
    sid, n_points, n_obs = h.displacement_image_term_info(0)
    rec = dict(config="displacement_image_grid_%d" % args.grid, workload=w.name, n_nodes=int(mesh.num_vertices()),
               n_cells=int(mesh.num_cells()), steps=args.steps, n_points=n_points, n_observed=n_obs, J=float(J),
               locate_s=round(locate_s, 4), gradient_wall_s=round(float(np.median(walls[1:])), 5),
               misfit_ms=med(0), transpose_ms=med(1), u_solve_ms=med(2), u_solve_iterations=int(np.median([c[3] for c in calls])),
               # ids and weights, the target planes, the mask, R; u_k gathered through the caches
               model_bytes_misfit=int(n_points * ((d + 1) * 12 + 8 * d + 8 + 8 * d)))
    rec["misfit_gb_s"] = round(rec["model_bytes_misfit"] / (rec["misfit_ms"] * 1e-3) / 1e9, 1) if rec["misfit_ms"] else None
    rec["term_over_u_solve"] = round((rec["misfit_ms"] + rec["transpose_ms"]) / rec["u_solve_ms"], 5)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    h.close()


if __name__ == "__main__":
    main()
