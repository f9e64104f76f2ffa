#!/usr/bin/env python3
"""
Cost of the second-order adjoint ("Second order"): the wall ms of glims_adjoint_hessian with P
directions (the five brain controls: D and rho of the two tissues, the coupling; repeated beyond 5), as the call reports it
(stats ms, synchronised), next to glims_adjoint_gradient on the same recorded trajectory (its glims_adjoint_stats ms):
median, min and max of --reps calls after one warm-up, with the tangent-linear and second-order PCG iterations per step and
direction, for config C3 (1 M-node lattice) and the 1.04 M-node brain-like mesh.  One JSON line per workload on stdout.

    python tools/adjoint_hessian_cost.py [--steps 20] [--which c3,brain_like] [--dirs 1,2,5] [--reps 5]

Kernel medians of k_spmm<P> (and k_spmv) come from a kernel-trace run of this script, e.g.
rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/adjoint_hessian_cost.py --which c3 --steps 10
--dirs 1,2,4,8 --reps 1, reduced by tools/spmm_medians.py.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import _backend, workloads  # noqa: E402


def measure(w, n_steps, dirs, reps):
    t = w.tables
    h = _backend.Handle(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[np.asarray(t[k], dtype=np.float64) for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=float(w.dt))
    h.setup(with_mechanics=False)
    h.set_state(w.c0)
    assert h.step(2) == 0          # warm-up: preconditioner decision, spectral interval
    h.set_state(w.c0)
    h.adjoint_record(True)
    assert h.step(n_steps) == 0
    st = h.stats()
    c = h.get_state(want_u=False)[0]
    terms = [dict(step=n_steps, kind="c_thresh", level=0.8, smooth=0.1, target=(c > 0.8).astype(float)),
             dict(step=n_steps, kind="c_thresh", level=0.16, smooth=0.1, target=(c > 0.16).astype(float))]
    L = len(t["D"])
    tis = [int(l) for l in np.nonzero(np.asarray(t["D"]) != 0)[0][:2]]
    unit = lambda l: np.eye(L)[l]
    five = [dict(D=unit(tis[0])), dict(D=unit(tis[-1])), dict(rho=unit(tis[0])), dict(rho=unit(tis[-1])),
            dict(gamma=np.ones(L))]
    h.adjoint_gradient(terms, L)   # first call builds the vertex table
    spread = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(np.min(v)), 2),
                            max=round(float(np.max(v)), 2))
    g_ms = []
    for _ in range(reps):   # the call's own wall time (glims_adjoint_stats ms, synchronised on return)
        a0 = h.adjoint_stats()["ms_backward"]
        h.adjoint_gradient(terms, L)
        g_ms.append(h.adjoint_stats()["ms_backward"] - a0)
    out = dict(workload=w.name, nodes=len(c), nnz=int(st["nnz"]), steps=n_steps, rd_precond=int(st["rd_precond_used"]),
               reps=reps, gradient_ms=spread(g_ms))
    for P in dirs:
        h.adjoint_hessian(terms, five[:P] + five[:max(0, P - 5)], L)   # warm-up
        ms, r = [], None
        for _ in range(reps):
            r = h.adjoint_hessian(terms, five[:P] + five[:max(0, P - 5)], L)
            ms.append(r["stats"]["ms"])
        out["hessian_P%d_ms" % P] = spread(ms)
        out["hessian_P%d_over_gradient" % P] = round(float(np.median(ms) / np.median(g_ms)), 3)
        out["hessian_P%d_tlm_its_per_step" % P] = round(r["stats"]["tlm_pcg_its"] / (n_steps * P), 2)
        out["hessian_P%d_soa_its_per_step" % P] = round(r["stats"]["soa_pcg_its"] / (n_steps * P), 2)
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--which", default="c3,brain_like")
    ap.add_argument("--dirs", default="1,2,5", help="direction counts (1..8; beyond 5 the five repeat)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dirs = [int(x) for x in a.dirs.split(",")]
    for name in a.which.split(","):
        if name == "c3":
            w = workloads.config_c3()
        elif name == "brain_like":
            w = workloads.config_brain_like(isolate=not os.environ.get("GLIMS_MESH_CACHE"))
        else:
            raise SystemExit("unknown workload " + name)
        print(json.dumps(measure(w, a.steps, dirs, a.reps)), flush=True)


if __name__ == "__main__":
    main()
