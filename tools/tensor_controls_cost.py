#!/usr/bin/env python3
"""
Cost of tangent fields ("Tangent fields") in a gradient call on the ~1 M-node brain-like mesh: one
recorded run of `--steps` steps with the random SPD field of tools/anisotropic_cost.py, then `--repeat` gradient calls each
without tangents, with K = 1 and with K = 4 random symmetric tangent fields.  One JSON line per K on stdout with the median,
the smallest and the largest call (their spread is the run-to-run spread of the figure) and the time of the set call
(profiles/anisotropic_cost.jsonl holds the lines of the run recorded in DESIGN.md).

    python tools/tensor_controls_cost.py [--steps 20] [--nodes 1000000] [--repeat 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import _backend, workloads  # noqa: E402
from anisotropic_cost import random_spd  # noqa: E402


def random_tangents(n_cells, dim, K, seed=0):
    A = np.random.default_rng(seed).standard_normal((K, n_cells, dim, dim))
    return 0.5 * (A + np.swapaxes(A, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()
    w = workloads.config_brain_like(a.nodes, isolate=not os.environ.get("GLIMS_MESH_CACHE"))
    t = w.tables
    nc = len(w.mesh.cells)
    h = _backend.Handle(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[np.asarray(t[k], dtype=np.float64) for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=float(w.dt))
    h.set_diffusion_tensor(random_spd(nc, 3, seed=1))
    h.setup(with_mechanics=False)
    h.set_state(w.c0)
    assert h.step(2) == 0          # warm-up: preconditioner decision, spectral interval
    h.set_state(w.c0)
    h.adjoint_record(True)
    assert h.step(a.steps) == 0
    c = h.get_state(want_u=False)[0]
    terms = [dict(step=a.steps, kind="c_thresh", level=0.8, smooth=0.1, target=(c > 0.8).astype(float)),
             dict(step=a.steps, kind="c_thresh", level=0.16, smooth=0.1, target=(c > 0.16).astype(float))]
    n_labels = len(t["D"])
    h.adjoint_gradient(terms, n_labels)   # first call builds the vertex table
    for K in (0, 1, 4):
        t0 = time.perf_counter()
        h.set_diffusion_tensor_tangents(random_tangents(nc, 3, K, seed=2) if K else None)
        set_ms = 1e3 * (time.perf_counter() - t0)
        ms = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            g = h.adjoint_gradient(terms, n_labels)
            ms.append(1e3 * (time.perf_counter() - t0))
        tg = h.adjoint_tensor_gradient() if K else np.zeros((0, n_labels))
        print(json.dumps(dict(workload=w.name, nodes=len(c), cells=nc, steps=a.steps, field=True, tangents=K,
                              set_tangents_ms=round(set_ms, 2), gradient_ms=round(float(np.median(ms)), 2),
                              gradient_ms_min=round(min(ms), 2), gradient_ms_max=round(max(ms), 2), calls=a.repeat,
                              tangent_bytes_per_cell=48 * K, J=float(g[0]),
                              tensor_gradient_norm=float(np.linalg.norm(tg)))), flush=True)
    h.close()


if __name__ == "__main__":
    main()
