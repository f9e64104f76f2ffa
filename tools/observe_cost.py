#!/usr/bin/env python
"""
What the tumour volumes and centres of mass of a recorded run cost: ONE glims_observe call over the snapshots of a run with the
two reference thresholds (SHARP at T2 = 0.12 and T1 = 0.80), on the 3-D lattice workload and on the brain-like unstructured mesh,
  * on the device: the time per source from the library's own HIP event pair around each source's pass (GLIMS_OBSERVE_TIMING),
    median of `--reps` calls after one warm-up, and the wall time of the whole call, and
  * by the only way to the same numbers without it: glims_snapshot_load of each step, then the numpy statement
    (simulation_helpers/observables.py), timed on `--numpy-steps` of the steps,
next to the algorithmic bytes of the pass: per cell its vertex ids and label, per node c once, and the positions of the nodes of
the cells that can contribute (the others are not read).

    python tools/observe_cost.py --case lattice:1000000 --case brain:1000000 [--snapshots 20]

Writes one JSON line per case to profiles/observe_cost.jsonl (or --out).
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

QUERIES = [("sharp", 0.12), ("sharp", 0.80)]


def build(case):
    from glimslib_amd import workloads
    kind, n = case.split(":")
    n = int(n)
    if kind == "lattice":
        return workloads._brain_box(max(2, int(round(n ** (1.0 / 3.0))) - 1), False, 1, "lattice %d" % n)
    if kind == "brain":
        return workloads.config_brain_like(n, mechanics=False, isolate=True)   # (the mesh builder forks: not from this process)
    raise SystemExit("unknown case %r" % case)


def timed_calls(h, ids, reps):
    """(per-source ms of every timed call [reps][n_src], wall seconds per call [reps]) -- call 0 is the warm-up"""
    os.environ["GLIMS_OBSERVE_TIMING"] = "1"
    walls = []
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 1):
                t0 = time.perf_counter()
                h.observe(QUERIES, snapshots=ids)
                walls.append(time.perf_counter() - t0)
                os.write(2, b"glims observe: end of call\n")
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["GLIMS_OBSERVE_TIMING"]
        tmp.seek(0)
        calls, cur = [], []
        for line in tmp.read().decode().splitlines():
            if "end of call" in line:
                calls.append(cur)
                cur = []
                continue
            m = re.match(r"glims observe: source (-?\d+)\s+pass ([0-9.]+) ms", line)
            if m:
                cur.append(float(m.group(2)))
    return calls[1:], walls[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[])
    ap.add_argument("--snapshots", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-steps", type=int, default=2, help="steps the host baseline is timed on (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "observe_cost.jsonl"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("observe_cost.py: no GPU visible", file=sys.stderr)
        return 3
    from glimslib_amd import _backend
    from glimslib_amd.simulation_helpers import observables
    lines = []
    for case in args.case or ["lattice:100000"]:
        w = build(case)
        mesh, d = w.mesh, w.mesh.points.shape[1]
        labels = np.asarray(w.cell_label)
        n_labels = len(w.tables["D"])
        h = _backend.Handle(mesh.points, mesh.cells, labels)
        h.set_materials(*[w.tables[k] for k in ("D", "rho", "gamma", "E", "nu")])
        h.set_options(dt=w.dt)
        h.setup(False)
        h.set_state(w.c0)
        ids = []
        for _ in range(args.snapshots):
            assert h.step(1) == _backend.GLIMS_OK
            ids.append(h.snapshot_save())
        calls, walls = timed_calls(h, ids, args.reps)
        per_src = float(np.median([np.median(c) for c in calls]))
        table = h.observe(QUERIES, snapshots=ids)
        # the bytes: connectivity + label per cell, c per node, positions of the nodes of cells that can contribute (last snapshot)
        c_last = h.snapshot_load(ids[-1])
        live = c_last[mesh.cells].max(axis=1) >= min(q[1] for q in QUERIES)
        n_cells, n_nodes = int(mesh.num_cells()), int(mesh.num_vertices())
        live_nodes = int(len(np.unique(mesh.cells[live])))
        model = n_cells * (4 * (d + 1) + 1) + n_nodes * 8 + live_nodes * 8 * d
        rec = dict(case=case, workload=w.name, n_nodes=n_nodes, n_cells=n_cells, n_labels=n_labels, snapshots=len(ids),
                   queries=QUERIES, pass_ms_per_source=round(per_src, 4),
                   pass_ms_per_source_by_call=[round(float(np.median(c)), 4) for c in calls],
                   call_wall_s=round(float(np.median(walls)), 5), live_cell_fraction=round(float(live.mean()), 4),
                   model_bytes_per_cell=round(model / n_cells, 2), model_bytes=int(model),
                   model_TBps=round(model / (per_src * 1e-3) / 1e12, 3) if per_src > 0 else None,
                   observe_info=h.observe_info())
        if args.numpy_steps > 0:
            loads, nps = [], []
            for k, sid in enumerate(ids[-args.numpy_steps:]):
                t0 = time.perf_counter()
                c = h.snapshot_load(sid)
                t1 = time.perf_counter()
                t = observables.observe(mesh.points, mesh.cells, labels, c, QUERIES, n_labels)
                t2 = time.perf_counter()
                loads.append(t1 - t0)
                nps.append(t2 - t1)
                ref = table[len(ids) - args.numpy_steps + k]
                rec["numpy_vs_device_max_abs"] = max(rec.get("numpy_vs_device_max_abs", 0.0), float(np.abs(t - ref).max()))
            rec.update(host_snapshot_load_s_per_step=round(float(np.median(loads)), 4),
                       host_numpy_s_per_step=round(float(np.median(nps)), 4))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
