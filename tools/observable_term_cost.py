#!/usr/bin/env python
"""
What stored volume misfit terms (glims_adjoint_observable_terms) add to a gradient call, on the brain-like unstructured mesh:
  * the wall time of adjoint_gradient of a recorded run with one nodal term and NO stored volume term -- the behaviour before the
    terms existed, the baseline -- median of `--reps` calls after one warm-up,
  * the same call with 1, 8 and 16 SMOOTH terms and with 8 SHARP terms on the last step (16 terms: two cell passes), and
  * per pass the time of the cell pass (k_observe_grad_cells + its block sums) and of the row-owned gather
    (k_observe_grad_rows), from the library's own HIP event pairs (GLIMS_OBSERVABLE_TIMING; measured in a separate run of calls:
    the event pairs synchronise the stream),
next to the algorithmic bytes of a pass: per cell its vertex ids, label and volume, per node c once, and the planes of vertex
partials written by the cell pass and read back by the gather (8 (d+1) bytes per cell and term, each way).

    python tools/observable_term_cost.py [--nodes 1000000] [--steps 10] [--reps 5]

Writes one JSON line per configuration to profiles/observable_term_cost.jsonl (or --out).

    python tools/observable_term_cost.py --deformed [--nodes 1000000] [--steps 10] [--reps 5]

What the DEFORMED configuration adds (glims_adjoint_observable_terms2), on the same mesh with mechanics on and the exterior
clamped: in ONE process, alternating call by call, (a) the gradient call with 1 and with 8 SMOOTH terms in the reference
configuration plus a u_l2 term on the same step -- so that both sides pay the step's two elastic solves -- and (b) the same call
with the volume terms deformed; medians of `--reps` after a warm-up.  Per pass, from the library's event pairs: the DEF = 1 cell
pass with its sum, the gather of the c-partials, the load kernel (k_observe_def_load_cells) and the D-component gather into the
elastic adjoint's load, with the algorithmic bytes of each.  APPENDS its lines (config "deformed_*") to the same file.

    python tools/observable_term_cost.py --com [--nodes 1000000] [--steps 10] [--reps 5]

What CENTRE-OF-MASS terms cost (glims_adjoint_observable_terms3), on the same mesh with mechanics on: eight SMOOTH and eight SHARP
terms on the last step, in the reference and in the deformed configuration, once as volume terms and once as centre-of-mass
terms, in ONE process.  Per pass, from the library's event pairs: the moments pass (k_observe_mom_cells + its sum; centre of
mass only), the gradient cell pass with its sum, the gather, and for deformed terms the load kernel and the u-gather.  The
figure of merit is (moments + cells) of the centre-of-mass batch over cells of the volume batch.  APPENDS its lines (config
"com_*" / "vol_*") to profiles/com_term_cost.jsonl (or --out).
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

CONFIGS = [("none", None, 0), ("smooth_1", "smooth", 1), ("smooth_8", "smooth", 8), ("smooth_16", "smooth", 16),
           ("sharp_8", "sharp", 8)]


def pass_times(h, nodal, n_labels, reps):
    """[(terms, cells ms, gather ms)] of every pass of `reps` gradient calls after one warm-up"""
    os.environ["GLIMS_OBSERVABLE_TIMING"] = "1"
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 1):
                h.adjoint_gradient(nodal, n_labels, want_dc0=False)
                os.write(2, b"glims observable terms: end of call\n")
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["GLIMS_OBSERVABLE_TIMING"]
        tmp.seek(0)
        calls, cur = [], []
        for line in tmp.read().decode().splitlines():
            if "end of call" in line:
                calls.append(cur)
                cur = []
                continue
            m = re.match(r"glims observable terms: step (\d+)\s+terms (\d+)\s+cells ([0-9.]+) ms\s+gather ([0-9.]+) ms", line)
            if m:
                cur.append((int(m.group(2)), float(m.group(3)), float(m.group(4))))
    return calls[1:]


def deformed_pass_times(h, terms, n_labels, reps):
    """[(terms, cells ms, gather ms, load ms, u-gather ms)] of every pass of `reps` gradient calls after one warm-up (the load
    figures are None for a pass without a deformed term)"""
    os.environ["GLIMS_OBSERVABLE_TIMING"] = "1"
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 1):
                h.adjoint_gradient(terms, n_labels, want_dc0=False)
                os.write(2, b"glims observable terms: end of call\n")
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["GLIMS_OBSERVABLE_TIMING"]
        tmp.seek(0)
        calls, cur = [], []
        for line in tmp.read().decode().splitlines():
            if "end of call" in line:
                calls.append(cur)
                cur = []
                continue
            m = re.match(r"glims observable terms: step (\d+)\s+terms (\d+)\s+cells ([0-9.]+) ms\s+gather ([0-9.]+) ms", line)
            if m:
                cur.append([int(m.group(2)), float(m.group(3)), float(m.group(4)), None, None])
            m = re.match(r"glims observable terms: step (\d+)\s+deformed pass\s+load ([0-9.]+) ms\s+u-gather ([0-9.]+) ms", line)
            if m and cur:
                cur[-1][3:] = [float(m.group(2)), float(m.group(3))]
    return calls[1:]


def com_pass_times(h, terms, n_labels, reps):
    """[[terms, cells ms, gather ms, load ms, u-gather ms, moments ms]] of every pass of `reps` gradient calls after a warm-up"""
    os.environ["GLIMS_OBSERVABLE_TIMING"] = "1"
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 1):
                h.adjoint_gradient(terms, n_labels, want_dc0=False)
                os.write(2, b"glims observable terms: end of call\n")
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["GLIMS_OBSERVABLE_TIMING"]
        tmp.seek(0)
        calls, cur = [], []
        for line in tmp.read().decode().splitlines():
            if "end of call" in line:
                calls.append(cur)
                cur = []
                continue
            m = re.match(r"glims observable terms: step (\d+)\s+terms (\d+)\s+cells ([0-9.]+) ms\s+gather ([0-9.]+) ms", line)
            if m:
                cur.append([int(m.group(2)), float(m.group(3)), float(m.group(4)), 0.0, 0.0, 0.0])
            m = re.match(r"glims observable terms: step (\d+)\s+deformed pass\s+load ([0-9.]+) ms\s+u-gather ([0-9.]+) ms", line)
            if m and cur:
                cur[-1][3:5] = [float(m.group(2)), float(m.group(3))]
            m = re.match(r"glims observable terms: step (\d+)\s+moments pass ([0-9.]+) ms", line)
            if m and cur:
                cur[-1][5] = float(m.group(2))
    return calls[1:]


def main_com(args):
    from glimslib_amd import _backend, workloads
    from oracle.glims_oracle import boundary_facets
    w = workloads.config_brain_like(args.nodes, isolate=True)   # (the mesh builder forks: not from this process)
    mesh, d = w.mesh, w.mesh.points.shape[1]
    pts = np.asarray(mesh.points, dtype=np.float64)
    n_labels = len(w.tables["D"])
    n_cells, n_nodes = int(mesh.num_cells()), int(mesh.num_vertices())
    h = _backend.Handle(pts, mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[w.tables[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=w.dt)
    xb = np.unique(boundary_facets(mesh.cells)[0])
    h.set_dirichlet_u((xb[:, None] * d + np.arange(d)[None]).ravel(), np.zeros(len(xb) * d))
    h.setup(with_mechanics=True)
    h.set_state(w.c0)
    h.adjoint_record(True)
    assert h.step(args.steps) == _backend.GLIMS_OK
    c_last = h.get_state(want_u=False)[0]
    centre = pts.mean(axis=0)
    n = 8
    levels = np.linspace(0.12, 0.80, n) * min(1.0, float(c_last.max()))
    lines = []
    for kind in ("smooth", "sharp"):
        for deformed in (False, True):
            vol_ms = None
            for what in ("vol", "com"):
                terms = [dict(step=args.steps, kind="obs_volume" if what == "vol" else "obs_com", observable=kind,
                              level=float(lv), smooth=0.05, target=0.0 if what == "vol" else centre, weight=1.0,
                              deformed=deformed, scale=1.0) for lv in levels]
                h.set_observable_terms(terms)
                walls = []
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    J = h.adjoint_gradient([], n_labels, want_dc0=False)[0]
                    walls.append(time.perf_counter() - t0)
                calls = com_pass_times(h, [], n_labels, args.reps)
                per_pass = [p for c in calls for p in c]
                med = lambda k: round(float(np.median([p[k] for p in per_pass])), 4)
                info = h.observable_term_info(0)
                rec = dict(config="%s_%s%s_%d" % (what, "deformed_" if deformed else "", kind, n), workload=w.name,
                           n_nodes=n_nodes, n_cells=n_cells, steps=args.steps, kind=kind, n_terms=n, deformed=deformed,
                           J=float(J), gradient_wall_s=round(float(np.median(walls[1:])), 5), passes_per_call=len(calls[0]),
                           moments_ms_per_pass=med(5), cells_ms_per_pass=med(1), gather_ms_per_pass=med(2),
                           load_ms_per_pass=med(3), u_gather_ms_per_pass=med(4), V_first=info["V"], cut_first=info["cut"])
                if what == "vol":
                    vol_ms = rec
                else:
                    rec["com_first"] = [float(v) for v in info["com"]]
                    rec["cell_passes_over_volume_batch"] = round((rec["moments_ms_per_pass"] + rec["cells_ms_per_pass"]) /
                                                                 vol_ms["cells_ms_per_pass"], 3)
                    rec["gather_over_volume_batch"] = round(rec["gather_ms_per_pass"] / vol_ms["gather_ms_per_pass"], 3)
                    # the moments pass: vertex ids, label and volume per cell, c and X (and u_k) once per node
                    rec["model_bytes_moments"] = int(n_cells * (4 * (d + 1) + 1 + 8) + n_nodes * 8 * (1 + d * (2 if deformed else 1)))
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    h.set_observable_terms([])
    h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


def main_deformed(args):
    from glimslib_amd import _backend, workloads
    from oracle.glims_oracle import boundary_facets
    w = workloads.config_brain_like(args.nodes, isolate=True)   # (the mesh builder forks: not from this process)
    mesh, d = w.mesh, w.mesh.points.shape[1]
    pts = np.asarray(mesh.points, dtype=np.float64)
    n_labels = len(w.tables["D"])
    n_cells, n_nodes = int(mesh.num_cells()), int(mesh.num_vertices())
    h = _backend.Handle(pts, mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[w.tables[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=w.dt)
    xb = np.unique(boundary_facets(mesh.cells)[0])
    h.set_dirichlet_u((xb[:, None] * d + np.arange(d)[None]).ravel(), np.zeros(len(xb) * d))
    h.setup(with_mechanics=True)
    h.set_state(w.c0)
    h.adjoint_record(True)
    assert h.step(args.steps) == _backend.GLIMS_OK
    c_last = h.get_state(want_u=False)[0]
    u_l2 = dict(step=args.steps, kind="u_l2", target=np.zeros(n_nodes * d))
    lines = []
    for n in (1, 8):
        levels = np.linspace(0.12, 0.80, n) * min(1.0, float(c_last.max()))
        lists = {}
        for name, deformed in (("reference", False), ("deformed", True)):
            lists[name] = [dict(step=args.steps, kind="obs_volume", observable="smooth", level=float(lv), smooth=0.05,
                                         target=0.0, weight=1.0, deformed=deformed, scale=1.0) for lv in levels]
        # (the stored list is replaced outside the timed call; the call itself then allocates the passes' planes anew, on both
        #  sides alike but for the deformed side's b0 and load planes)
        walls = {name: [] for name in lists}
        its = {name: [] for name in lists}                        # PCG iterations of the call's two elastic solves
        J, st0 = {}, h.adjoint_stats()
        for rep in range(args.reps + 1):                          # alternating: drift hits both sides alike
            for name, terms in lists.items():
                h.set_observable_terms(terms)
                before = h.adjoint_stats()
                t0 = time.perf_counter()
                J[name] = h.adjoint_gradient([u_l2], n_labels, want_dc0=False)[0]
                walls[name].append(time.perf_counter() - t0)
                after = h.adjoint_stats()
                its[name].append((after["mech_its"] - before["mech_its"], after["pcg_its"] - before["pcg_its"]))
        st1 = h.adjoint_stats()
        calls = deformed_pass_times(h, [u_l2], n_labels, args.reps)   # (the deformed list is the stored one)
        info = h.observable_term_info2(0)
        per_pass = [p for c in calls for p in c]
        med = lambda k: round(float(np.median([p[k] for p in per_pass])), 4)
        plane = 8 * (d + 1) * n_cells * n
        rec = dict(config="deformed_smooth_%d" % n, workload=w.name, n_nodes=n_nodes, n_cells=n_cells, steps=args.steps,
                   kind="smooth", n_terms=n, with_u_l2=True,
                   J_reference=float(J["reference"]), J_deformed=float(J["deformed"]),
                   reference_wall_s=round(float(np.median(walls["reference"][1:])), 5),
                   deformed_wall_s=round(float(np.median(walls["deformed"][1:])), 5),
                   reference_wall_s_by_call=[round(float(v), 5) for v in walls["reference"][1:]],
                   deformed_wall_s_by_call=[round(float(v), 5) for v in walls["deformed"][1:]],
                   reference_elastic_and_rd_pcg_its=[int(v) for v in np.median(its["reference"][1:], axis=0)],
                   deformed_elastic_and_rd_pcg_its=[int(v) for v in np.median(its["deformed"][1:], axis=0)],
                   elastic_solves_per_call=(st1["mech_solves"] - st0["mech_solves"]) / (2.0 * (args.reps + 1)),
                   passes_per_call=len(calls[0]), cells_ms_per_pass=med(1), gather_ms_per_pass=med(2),
                   load_ms_per_pass=med(3), u_gather_ms_per_pass=med(4),
                   # the DEF = 1 cell pass: vertex ids, label and volume per cell, c, X and u_k once per node, the c-planes and the
                   # b0 planes written; the load kernel: vertex ids, X, u_k, the b0 planes read, the (d+1) d load planes
                   # written; the D-component gather: per incidence the cell id, the cell's vertex ids and d plane entries, per
                   # node its d sums read and written
                   model_bytes_cells=int(n_cells * (4 * (d + 1) + 1 + 8) + n_nodes * 8 * (1 + 2 * d) + plane + 8 * n_cells * n),
                   model_bytes_gather=int(n_cells * (d + 1) * (4 + 4 * (d + 1)) + plane + 16 * n_nodes),
                   model_bytes_load=int(n_cells * 4 * (d + 1) + n_nodes * 16 * d + 8 * n_cells * n + 8 * (d + 1) * d * n_cells),
                   model_bytes_u_gather=int(n_cells * (d + 1) * (4 + 4 * (d + 1) + 8 * d) + 16 * d * n_nodes),
                   V_first=info["V"], folded_first=info["folded"], min_ratio_first=info["min_ratio"])
        rec["added_wall_s"] = round(rec["deformed_wall_s"] - rec["reference_wall_s"], 5)
        for k in ("cells", "gather", "load", "u_gather"):
            rec["achieved_TBps_" + k] = round(rec["model_bytes_" + k] / (rec[k + "_ms_per_pass"] * 1e-3) / 1e12, 3)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    h.set_observable_terms([])
    h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deformed", action="store_true", help="the deformed-configuration comparison (appends to --out)")
    ap.add_argument("--com", action="store_true", help="centre-of-mass terms against volume terms (appends to --out)")
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "com_term_cost.jsonl" if args.com else "observable_term_cost.jsonl")
    import torch
    if not torch.cuda.is_available():
        print("observable_term_cost.py: no GPU visible", file=sys.stderr)
        return 3
    if args.com:
        return main_com(args)
    if args.deformed:
        return main_deformed(args)
    from glimslib_amd import _backend, workloads
    w = workloads.config_brain_like(args.nodes, mechanics=False, isolate=True)   # (the mesh builder forks: not from this process)
    mesh, d = w.mesh, w.mesh.points.shape[1]
    labels = np.asarray(w.cell_label)
    n_labels = len(w.tables["D"])
    n_cells, n_nodes = int(mesh.num_cells()), int(mesh.num_vertices())
    h = _backend.Handle(mesh.points, mesh.cells, labels)
    h.set_materials(*[w.tables[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=w.dt)
    h.setup(False)
    h.set_state(w.c0)
    h.adjoint_record(True)
    assert h.step(args.steps) == _backend.GLIMS_OK
    c_last = h.get_state(want_u=False)[0]
    nodal = [dict(step=args.steps, kind="c_l2", target=0.9 * c_last)]
    lines = []
    for name, kind, n in CONFIGS:
        # levels spread over the reference's T2 .. T1 thresholds, as fractions of the run's largest c where the short run stays
        # below 1 (a level above every nodal value would cut no cell); target 0, so that every term pulls
        levels = np.linspace(0.12, 0.80, max(n, 1)) * min(1.0, float(c_last.max()))
        h.set_observable_terms([dict(step=args.steps, kind="obs_volume", observable=kind, level=float(lv), smooth=0.05,
                                     target=0.0, weight=1.0) for lv in levels[:n]])
        walls = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            J = h.adjoint_gradient(nodal, n_labels, want_dc0=False)[0]
            walls.append(time.perf_counter() - t0)
        rec = dict(config=name, workload=w.name, n_nodes=n_nodes, n_cells=n_cells, steps=args.steps, kind=kind, n_terms=n,
                   J=float(J), gradient_wall_s=round(float(np.median(walls[1:])), 5),
                   gradient_wall_s_by_call=[round(float(v), 5) for v in walls[1:]])
        if n:
            calls = pass_times(h, nodal, n_labels, args.reps)
            per_pass = [p for c in calls for p in c]
            rec.update(passes_per_call=len(calls[0]), terms_per_pass=[p[0] for p in calls[0]],
                       cells_ms_per_pass=round(float(np.median([p[1] for p in per_pass])), 4),
                       gather_ms_per_pass=round(float(np.median([p[2] for p in per_pass])), 4),
                       cells_ms_by_pass=[round(float(np.median([c[k][1] for c in calls])), 4) for k in range(len(calls[0]))],
                       gather_ms_by_pass=[round(float(np.median([c[k][2] for c in calls])), 4) for k in range(len(calls[0]))])
            nt = calls[0][0][0]
            plane = 8 * (d + 1) * n_cells * nt
            rec.update(model_bytes_cells=int(n_cells * (4 * (d + 1) + 1 + 8) + n_nodes * 8 + plane),
                       model_bytes_gather=int(n_cells * (d + 1) * (4 + 4 * (d + 1)) + plane + 16 * n_nodes),
                       V_first=h.observable_term_info(0)["V"], cut_first=h.observable_term_info(0)["cut"])
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    base = lines[0]["gradient_wall_s"]
    for rec in lines[1:]:
        rec["added_wall_s"] = round(rec["gradient_wall_s"] - base, 5)
    h.set_observable_terms([])
    h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
