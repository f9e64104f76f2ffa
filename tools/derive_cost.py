#!/usr/bin/env python
"""
What the derived fields of ONE recorded step cost: the field set that PostProcess.save_all writes (pressure, von Mises stress,
total and growth-induced Jacobian, concentration in the deformed configuration, logistic growth), computed
  * by the numpy path (PostProcess(device=False): right-hand sides integrated on the host, mass solves through glims_project), and
  * by the device path (Handle.derive: csrc/derive.hip),
on the 3-D lattice workload and on the brain-like unstructured mesh; plus the times of the two derive kernels alone (cell pass,
gather; HIP events inside the library, GLIMS_DERIVE_TIMING), median of 5 after a warm-up, next to their byte models.

    python tools/derive_cost.py --case lattice:100000 --case lattice:1000000 --case brain:1000000 [--numpy-max-nodes N]

Writes one JSON line per (case, path) and per (case, integrand) to profiles/derive_cost.jsonl (or --out).  The displacement of
the step is solved before either path is timed (its time is reported separately): both paths then start from the same device
state, the numpy path with c and u already on the host.
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

FIELDS = (("pressure", "get_pressure"), ("van_mises_stress", "get_van_mises_stress"), ("total_jacobian", "get_total_jacobian"),
          ("growth_induced_jacobian", "get_growth_induced_jacobian"),
          ("concentration_deformed_config", "get_concentration_deformed_configuration"), ("log_growth", "get_logistic_growth"))
INTEGRANDS = {0: "strain", 1: "stress", 2: "total_jacobian", 3: "van_mises", 4: "displacement_norm", 5: "log_growth",
              6: "gamma_c", 7: "growth_jacobian", 8: "conc_deformed"}


class _Solver:
    _mech_current = False


class _Components(dict):
    _solver = _Solver()


class _Field:
    def __init__(self, c, u, sid):
        self.components = _Components({0: u, 1: c})
        if sid is not None:
            self.snapshot_id = sid


class _Obs:
    def __init__(self, field):
        self._field = field

    def get_field(self):
        return self._field


class _Space:
    def __init__(self, mesh):
        self._mesh = mesh


class _Results:
    """One recorded step, as the PostProcess class reads it."""

    def __init__(self, mesh, field):
        from glimslib_amd.fenics_local import Function
        self._functionspace, self._field, self._Function = _Space(mesh), field, Function

    def get_recording_steps(self):
        return [1]

    def get_result(self, recording_step):
        return _Obs(self._field)

    def get_solution_function(self, subspace_name=None, subspace_id=None, recording_step=None):
        k = 0 if subspace_name == 'displacement' else 1
        return self._Function(self._functionspace._mesh, {None: self._field.components[k]})


def build(case):
    from glimslib_amd import workloads
    kind, n = case.split(":")
    n = int(n)
    if kind == "lattice":
        w = workloads._brain_box(max(2, int(round(n ** (1.0 / 3.0))) - 1), True, 1, "lattice %d" % n)
    elif kind == "brain":
        w = workloads.config_brain_like(n, mechanics=True, isolate=True)   # (the mesh builder forks: not from this process)
    else:
        raise SystemExit("unknown case %r" % case)
    return w


def kernel_times(h, sid, reps=5):
    """Median ms of the cell pass and the gather per integrand, from the library's own event pairs."""
    kinds = ("strain_tensor", "stress_tensor", "total_jacobian", "van_mises_stress", "displacement_norm", "log_growth",
             "growth_induced_jacobian", "concentration_deformed_config")
    os.environ["GLIMS_DERIVE_TIMING"] = "1"
    seen = {}
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            for rep in range(reps + 1):
                for k in kinds:
                    h.derive(k, snapshot=sid, fetch=False)
                    if k == "stress_tensor":
                        h.snapshot_mechanics(sid)   # a new displacement generation: the next call projects the stress again
                os.write(2, b"glims derive: end of repetition\n")
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["GLIMS_DERIVE_TIMING"]
        tmp.seek(0)
        rep = 0
        for line in tmp.read().decode().splitlines():
            if "end of repetition" in line:
                rep += 1
                continue
            m = re.match(r"glims derive: integrand (\d+)\s+cell pass ([0-9.]+) ms\s+gather ([0-9.]+) ms", line)
            if m and rep >= 1:   # repetition 0 is the warm-up
                seen.setdefault(int(m.group(1)), []).append((float(m.group(2)), float(m.group(3))))
    return {k: (float(np.median([a for a, _ in v])), float(np.median([b for _, b in v])), len(v)) for k, v in seen.items()}


def byte_model(ck, d, n_cells, n_nodes, n_inc):
    """(cell pass, gather) bytes: streams only -- the gathered vertex values mostly hit the caches."""
    nv, ns = d + 1, d * (d + 1) // 2
    rec = (1 + nv * d) * 8 + 4 * nv + 1
    const = ck in (0, 1, 2)
    planes = (1 if ck == 2 else ns) if const else nv
    cells = n_cells * (rec + 8 * planes)
    ncomp = planes if const else 1
    rows = n_inc * (4 + 8 * ncomp + (0 if const else 4 * nv)) + n_nodes * 8 * ncomp
    return cells, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", default=[])
    ap.add_argument("--numpy-max-nodes", type=int, default=2000000, help="skip the numpy path above this many nodes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derive_cost.jsonl"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--paths", default="device,numpy", help="which paths to time (the kernels are timed with 'device')")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("derive_cost.py: no GPU visible", file=sys.stderr)
        return 3
    from glimslib_amd import _backend
    from glimslib_amd.simulation_helpers.postprocess import PostProcess
    lines = []
    for case in args.case or ["lattice:100000"]:
        w = build(case)
        mesh, d = w.mesh, w.mesh.points.shape[1]
        h = _backend.Handle(mesh.points, mesh.cells, w.cell_label)
        h.set_materials(*[w.tables[k] for k in ("D", "rho", "gamma", "E", "nu")])
        h.set_options(dt=w.dt)
        dofs = (np.asarray(w.dirichlet_nodes)[:, None] * d + np.arange(d)).ravel()
        h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
        h.setup(True)
        h.set_state(w.c0)
        assert h.step(2) == _backend.GLIMS_OK
        sid = h.snapshot_save()
        t0 = time.perf_counter()
        u, st = h.snapshot_mechanics(sid)
        t_mech = time.perf_counter() - t0
        c = h.snapshot_load(sid)
        st_ = h.stats()
        base = dict(case=case, workload=w.name, n_nodes=int(mesh.num_vertices()), n_cells=int(mesh.num_cells()),
                    n_incidences=int(st_["n_corners"]), elastic_solve_s=round(t_mech, 4), elastic_status=int(st))
        paths = [("device", _Field(None, None, sid), None)] if "device" in args.paths else []
        if "numpy" in args.paths and mesh.num_vertices() <= args.numpy_max_nodes:
            paths.append(("numpy", _Field(c, u.reshape(-1, d), None), False))
        for name, field, device in paths:
            pp = PostProcess(_Results(mesh, field), None, backend=h, tables=w.tables, labels=w.cell_label, device=device)
            if name == "device":
                for _, get in FIELDS:   # warm-up: allocations, the cell -> vertex map
                    getattr(pp, get)(1)
                h.snapshot_mechanics(sid)   # (a new displacement generation: the timed pass projects the stress itself)
            i0 = h.derive_info()
            per = {}
            t_all = time.perf_counter()
            for key, get in FIELDS:
                t0 = time.perf_counter()
                getattr(pp, get)(1).values()
                per[key] = round(time.perf_counter() - t0, 4)
            total = time.perf_counter() - t_all
            i1 = h.derive_info()
            lines.append(dict(base, record="field_set", path=name, seconds=round(total, 4), per_field_s=per,
                              derive_info={k: i1[k] - i0[k] for k in i1}))
            print(json.dumps(lines[-1]), flush=True)
        for ck, (ms_c, ms_r, n) in sorted(kernel_times(h, sid).items() if "device" in args.paths else []):
            bc, br = byte_model(ck, d, base["n_cells"], base["n_nodes"], base["n_incidences"])
            lines.append(dict(case=case, record="kernels", integrand=INTEGRANDS[ck], samples=n,
                              cell_pass_ms=round(ms_c, 4), cell_pass_model_bytes=int(bc),
                              cell_pass_model_TBps=round(bc / (ms_c * 1e-3) / 1e12, 3) if ms_c > 0 else None,
                              gather_ms=round(ms_r, 4), gather_model_bytes=int(br),
                              gather_model_TBps=round(br / (ms_r * 1e-3) / 1e12, 3) if ms_r > 0 else None))
            print(json.dumps(lines[-1]), flush=True)
        h.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
