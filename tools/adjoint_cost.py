#!/usr/bin/env python3
"""
Cost of the discrete adjoint next to the forward run: forward ms/step of glims_step with recording on,
backward ms/step of glims_adjoint_gradient, adjoint PCG iterations per backward step, for config C3 (1 M-node lattice) and
the 1.04 M-node brain-like mesh.  One JSON line per workload on stdout.

    python tools/adjoint_cost.py [--steps 20] [--which c3,brain_like]

Kernel medians of the sensitivity pass (k_sens) and the G^T pass come from a separate kernel-trace run of this script, e.g.
rocprofv3 --kernel-trace --stats -d <dir> -- python tools/adjoint_cost.py --which c3 --steps 10 --mechanics
(GLIMS_MESH_CACHE must hold the brain-like mesh beforehand when that workload runs under the profiler).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import _backend, workloads  # noqa: E402


def measure(w, n_steps, mechanics):
    t = w.tables
    h = _backend.Handle(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[np.asarray(t[k], dtype=np.float64) for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=float(w.dt))
    if mechanics and w.dirichlet_nodes is not None:
        d = w.mesh.points.shape[1]
        nodes = np.asarray(w.dirichlet_nodes, dtype=np.int64)
        h.set_dirichlet_u((nodes[:, None] * d + np.arange(d)[None]).ravel(), 0.0)
    h.setup(with_mechanics=mechanics)
    h.set_state(w.c0)
    assert h.step(2) == 0          # warm-up: preconditioner decision, spectral interval
    h.set_state(w.c0)
    h.adjoint_record(True)
    h.reset_stats()
    t0 = time.perf_counter()
    assert h.step(n_steps) == 0
    fwd_ms = 1e3 * (time.perf_counter() - t0) / n_steps
    st = h.stats()
    c = h.get_state(want_u=False)[0]
    n = len(c)
    terms = [dict(step=n_steps, kind="c_thresh", level=0.8, smooth=0.1, target=(c > 0.8).astype(float)),
             dict(step=n_steps, kind="c_thresh", level=0.16, smooth=0.1, target=(c > 0.16).astype(float))]
    if mechanics:
        terms.append(dict(step=n_steps, kind="u_l2", target=np.zeros(n * w.mesh.points.shape[1])))
    n_labels = len(t["D"])
    h.adjoint_gradient(terms, n_labels)   # first call builds the vertex table
    a0 = h.adjoint_stats()
    t0 = time.perf_counter()
    h.adjoint_gradient(terms, n_labels)
    bwd_ms = 1e3 * (time.perf_counter() - t0) / n_steps
    a1 = h.adjoint_stats()
    out = dict(workload=w.name, nodes=n, steps=n_steps, mechanics=mechanics, forward_ms_per_step=round(fwd_ms, 3),
               forward_device_ms_per_step=round(st["ms_steps"] / n_steps, 3), backward_ms_per_step=round(bwd_ms, 3),
               ratio=round(bwd_ms / fwd_ms, 3), forward_krylov_its_per_step=st["cg_its"] / n_steps,
               adjoint_pcg_its_per_step=(a1["pcg_its"] - a0["pcg_its"]) / n_steps,
               rd_precond=int(st["rd_precond_used"]))
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--which", default="c3,brain_like")
    ap.add_argument("--mechanics", action="store_true")
    a = ap.parse_args()
    for name in a.which.split(","):
        if name == "c3":
            w = workloads.config_c3(mechanics=a.mechanics)
        elif name == "brain_like":
            w = workloads.config_brain_like(mechanics=a.mechanics, isolate=not os.environ.get("GLIMS_MESH_CACHE"))
        else:
            raise SystemExit("unknown workload " + name)
        print(json.dumps(measure(w, a.steps, a.mechanics)), flush=True)


if __name__ == "__main__":
    main()
