#!/usr/bin/env python3
"""
Cost of the second-order adjoint ("Second order"): the wall ms of glims_adjoint_hessian with P
directions (the five brain controls: D and rho of the two tissues, the coupling; repeated beyond 5), as the call reports it
(stats ms, synchronised), next to glims_adjoint_gradient on the same recorded trajectory (its glims_adjoint_stats ms):
median, min and max of --reps calls after one warm-up, with the tangent-linear and second-order PCG iterations per step and
direction, for config C3 (1 M-node lattice) and the 1.04 M-node brain-like mesh.  One JSON line per workload on stdout.

    python tools/adjoint_hessian_cost.py [--steps 20] [--which c3,brain_like] [--dirs 1,2,5] [--reps 5]
                                         [--lib path/to/libglimship.so --build NAME]   # another build of the library, named

--elastic measures what directions in E / nu add ("Second order in E and nu"): the handle is set up with
mechanics (u = 0 on the workload's Dirichlet nodes), one u_l2 term observes the last step, and glims_adjoint_hessian_full with
P directions that include dE / dnu runs next to glims_adjoint_hessian -- the call as it was -- with the D / rho / gamma part of
the same P directions, in the same process on the same trajectory (so both make the same RD solves).  --pure-columns puts
pure dE / dnu columns in place of the D / rho ones instead (no RD solve for them: the full call is then the cheaper one).  Both make 2 P elastic solves (asserted): the difference is the row pass
k_dkel_rows, one more cell and row pass of dG^T mu and the sum kernel k_hesens.  Their kernel medians come from a kernel-trace
run of this script (rocprofv3 --kernel-trace --stats ... -- python tools/adjoint_hessian_cost.py --elastic --reps 1).

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


def measure_elastic(w, n_steps, dirs, reps, pure=False):
    t = w.tables
    d = w.mesh.points.shape[1]
    h = _backend.Handle(w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32))
    h.set_materials(*[np.asarray(t[k], dtype=np.float64) for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=float(w.dt))
    nodes = np.asarray(w.dirichlet_nodes, dtype=np.int64)
    dofs = (nodes[:, None] * d + np.arange(d)[None]).ravel()
    h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
    h.setup(with_mechanics=True)
    h.set_state(w.c0)
    h.adjoint_record(True)
    assert h.step(n_steps) == 0
    assert h.solve_mechanics() == 0
    st = h.stats()
    c, u = h.get_state()
    terms = [dict(step=n_steps, kind="u_l2", weight=1.0, target=0.5 * u)]
    L = len(t["D"])
    tis = [int(l) for l in np.nonzero(np.asarray(t["D"]) != 0)[0][:2]]
    unit = lambda l: np.eye(L)[l]
    old = [dict(D=unit(tis[0])), dict(gamma=np.ones(L)), dict(rho=unit(tis[0])), dict(D=unit(tis[-1])), dict(rho=unit(tis[-1]))]
    # the same columns with a dE or dnu added: the RD solves of both calls are the same, the difference is the E / nu work
    extra = [dict(E=unit(tis[0])), dict(nu=unit(tis[-1])), dict(nu=unit(tis[0])), dict(E=unit(tis[-1])), dict(E=np.ones(L))]
    new = [dict(o, **e) for o, e in zip(old, extra)]
    if pure:   # --pure-columns: dE / dnu alone (dc = 0: those columns make no RD solve); the coupling column stays
        new = [e if "gamma" not in o else o for o, e in zip(old, extra)]
    h.adjoint_gradient(terms, L, elastic=True)
    spread = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(np.min(v)), 2),
                            max=round(float(np.max(v)), 2))
    out = dict(workload=w.name, elastic=True, nodes=len(c), nnz=int(st["nnz"]), steps=n_steps, reps=reps,
               directions="hessian: D / rho / gamma columns; hessian_full: " +
               ("pure dE / dnu columns in their place (the coupling column stays)" if pure else
                "the same columns with dE or dnu added"))
    for P in dirs:
        res = {}
        for name, call, dd in (("hessian", h.adjoint_hessian, old[:P]), ("hessian_full", h.adjoint_hessian_full, new[:P])):
            call(terms, dd, L)   # warm-up
            ms, r = [], None
            for _ in range(reps):
                r = call(terms, dd, L)
                ms.append(r["stats"]["ms"])
            res[name] = (ms, r)
            out["%s_P%d_ms" % (name, P)] = spread(ms)
            out["%s_P%d_mech_solves" % (name, P)] = r["stats"]["mech_solves"]
        assert res["hessian"][1]["stats"]["mech_solves"] == res["hessian_full"][1]["stats"]["mech_solves"] == 2 * P
        out["full_minus_hessian_P%d_ms" % P] = round(float(np.median(res["hessian_full"][0]) - np.median(res["hessian"][0])), 2)
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--which", default="c3,brain_like")
    ap.add_argument("--dirs", default="1,2,5", help="direction counts (1..8; beyond 5 the five repeat)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--elastic", action="store_true", help="glims_adjoint_hessian_full with dE / dnu directions next to "
                    "glims_adjoint_hessian, one u_l2 term (see above)")
    ap.add_argument("--pure-columns", action="store_true", help="with --elastic: the full call's columns are dE / dnu alone "
                    "instead of dE / dnu added to the D / rho columns")
    ap.add_argument("--lib", help="measure this build of libglimship.so instead of the tree's (A/B of two builds in one session)")
    ap.add_argument("--build", help="a name for the build, added to every JSON line as 'build'")
    a = ap.parse_args()
    if a.lib:
        _backend.LIB_PATH = os.path.abspath(a.lib)
    tag = (lambda d: dict(d, build=a.build)) if a.build else (lambda d: d)
    dirs = [int(x) for x in a.dirs.split(",")]
    for name in a.which.split(","):
        if name == "c3":
            w = workloads.config_c3(mechanics=a.elastic)
        elif name == "brain_like":
            w = workloads.config_brain_like(mechanics=a.elastic, isolate=not os.environ.get("GLIMS_MESH_CACHE"))
        else:
            raise SystemExit("unknown workload " + name)
        if a.elastic:
            print(json.dumps(tag(measure_elastic(w, a.steps, dirs, a.reps, a.pure_columns))), flush=True)
        else:
            print(json.dumps(tag(measure(w, a.steps, dirs, a.reps))), flush=True)


if __name__ == "__main__":
    main()
