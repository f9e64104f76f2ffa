#!/usr/bin/env python3
"""
Cost of a diffusion-tensor field ("Anisotropic diffusion") on the ~1 M-node brain-like mesh: glims_setup time,
device time per step, the rd_lin_slices / cheb_coded_passes / rd_scode_* statistics and the time of one gradient call, without a
field and with a random SPD field of eigenvalue ratio up to 10.  One JSON line per run on stdout (profiles/anisotropic_cost.jsonl
holds the lines of the run recorded in DESIGN.md).

    python tools/anisotropic_cost.py [--steps 20] [--nodes 1000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import _backend, workloads  # noqa: E402


def random_spd(n_cells, dim, seed=0, max_ratio=10.0):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n_cells, dim, dim)))[0]
    l = np.exp(rng.uniform(-0.5, 0.5, (n_cells, dim)) * rng.uniform(0.0, np.log(max_ratio), n_cells)[:, None])
    T = np.einsum('nak,nk,nbk->nab', Q, l, Q)
    return 0.5 * (T + np.swapaxes(T, 1, 2))


def measure(w, n_steps, T):
    t = w.tables
    h = _backend.Handle(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[np.asarray(t[k], dtype=np.float64) for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=float(w.dt))
    t0 = time.perf_counter()
    if T is not None:
        h.set_diffusion_tensor(T)
    set_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    h.setup(with_mechanics=False)
    setup_ms = 1e3 * (time.perf_counter() - t0)
    h.set_state(w.c0)
    assert h.step(2) == 0          # warm-up: preconditioner decision, spectral interval
    h.set_state(w.c0)
    h.adjoint_record(True)
    h.reset_stats()
    t0 = time.perf_counter()
    assert h.step(n_steps) == 0
    wall_ms = 1e3 * (time.perf_counter() - t0) / n_steps
    st = h.stats()
    c = h.get_state(want_u=False)[0]
    terms = [dict(step=n_steps, kind="c_thresh", level=0.8, smooth=0.1, target=(c > 0.8).astype(float)),
             dict(step=n_steps, kind="c_thresh", level=0.16, smooth=0.1, target=(c > 0.16).astype(float))]
    n_labels = len(t["D"])
    h.adjoint_gradient(terms, n_labels)   # first call builds the vertex table
    t0 = time.perf_counter()
    h.adjoint_gradient(terms, n_labels)
    grad_ms = 1e3 * (time.perf_counter() - t0)
    info = h.diffusion_tensor_info()
    out = dict(workload=w.name, nodes=len(c), cells=len(w.mesh.cells), steps=n_steps, field=T is not None,
               max_ratio=round(info["max_ratio"], 4), set_tensor_ms=round(set_ms, 2), setup_ms=round(setup_ms, 2),
               step_wall_ms=round(wall_ms, 3), step_device_ms=round(st["ms_steps"] / n_steps, 3),
               gradient_ms=round(grad_ms, 2), min_c=float(c.min()),
               **{k: int(st[k]) for k in ("rd_lin_slices", "cheb_coded_passes", "rd_scode_slices", "rd_scode_uncoded_slices",
                                          "cheb_solves", "cheb_its", "cg_its", "newton_its")})
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=1000000)
    a = ap.parse_args()
    w = workloads.config_brain_like(a.nodes, isolate=not os.environ.get("GLIMS_MESH_CACHE"))
    for T in (None, random_spd(len(w.mesh.cells), 3, seed=1)):
        print(json.dumps(measure(w, a.steps, T)), flush=True)


if __name__ == "__main__":
    main()
