#!/usr/bin/env python3
"""
Threaded-rank rehearsal of the collective second-order adjoint (glims_adjoint_hessian_spmd; DESIGN.md section 13, "Second
order", "Partitioned handles"): the brain-like 26 588-node mesh, --steps recorded steps, P directions (the five brain controls),
on 1, 2 and 4 ranks that are THREADS of one process sharing one GPU (parallel.ThreadedTransport: every all-reduce is a host
barrier, every exchange a host copy).  It exercises the code path and counts its collectives; it says nothing about RCCL
between devices.  Per rank count and P one JSON line: the slowest rank's call ms, the gradient's ms on the same handles and
their ratio, the tangent-linear and second-order PCG iterations (sums over the columns, the same on every rank), and the
all-reduces and ghost exchanges of the call per PCG iteration (iterations of a P-column solve taken as its / P).

    python tools/adjoint_hessian_partitioned_cost.py [--steps 6] [--dirs 1,2,5] [--ranks 1,2,4] [--nodes 24000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  (before libglimship: the transport's libamdhip64 must be the runtime the library uses)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import _backend, workloads  # noqa: E402
from glimslib_amd.parallel import ThreadedTransport, ThreadGroup  # noqa: E402
from glimslib_amd.partition import partition_mesh  # noqa: E402


class CountingTransport(ThreadedTransport):
    def __init__(self, group, rank):
        self.n_halo = self.n_allreduce = 0
        super().__init__(group, rank)

    def _halo(self, *a):
        self.n_halo += 1
        return super()._halo(*a)

    def _allreduce(self, *a):
        self.n_allreduce += 1
        return super()._allreduce(*a)


def rank_body(w, world, rank, tr, n_steps, dirs):
    t = w.tables
    pts, cells, lab = w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32)
    n = len(pts)
    if world > 1:
        part = partition_mesh(pts, cells, world, rank)
        gid = part.global_ids
        h = _backend.Handle(part.points, part.cells, lab[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(pts.min(axis=0), pts.max(axis=0))
    else:
        gid = np.arange(n)
        h = _backend.Handle(pts, cells, lab)
    h.set_materials(*[np.asarray(t[k], dtype=np.float64) for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=float(w.dt))
    h.setup(with_mechanics=False)
    h.set_state(np.asarray(w.c0, float)[gid])
    h.adjoint_record(True)
    assert h.step(n_steps) == 0
    rng = np.random.default_rng(11)
    terms = [dict(step=n_steps, kind="c_thresh", level=0.3, smooth=0.1, target=rng.uniform(0, 1, n)[gid]),
             dict(step=max(1, n_steps // 2), kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, n)[gid])]
    L = len(t["D"])
    tis = [int(l) for l in np.nonzero(np.asarray(t["D"]) != 0)[0][:2]]
    unit = lambda l: np.eye(L)[l]
    five = [dict(D=unit(tis[0])), dict(D=unit(tis[-1])), dict(rho=unit(tis[0])), dict(rho=unit(tis[-1])),
            dict(gamma=np.ones(L))]
    h.adjoint_gradient(terms, L)   # builds the vertex table
    a0 = h.adjoint_stats()["ms_backward"]
    h.adjoint_gradient(terms, L)
    out = dict(gradient_ms=h.adjoint_stats()["ms_backward"] - a0)
    for P in dirs:
        h.adjoint_hessian(terms, five[:P], L, collective=True)   # warm-up
        c0 = (tr.n_allreduce, tr.n_halo) if tr is not None else (0, 0)
        r = h.adjoint_hessian(terms, five[:P], L, collective=True)
        c1 = (tr.n_allreduce, tr.n_halo) if tr is not None else (0, 0)
        out[P] = dict(ms=r["stats"]["ms"], tlm=r["stats"]["tlm_pcg_its"], soa=r["stats"]["soa_pcg_its"],
                      allreduces=c1[0] - c0[0], exchanges=c1[1] - c0[1])
    h.close()
    if tr is not None and tr.failed is not None:
        raise tr.failed
    return out


def run_ranks(world, fn):
    """parallel.run_threaded_ranks with the counting transport"""
    import threading
    if world == 1:
        return [fn(0, None)]
    group = ThreadGroup(world)
    res, err = [None] * world, [None] * world

    def body(r):
        try:
            res[r] = fn(r, CountingTransport(group, r))
        except BaseException as e:   # noqa: BLE001
            err[r] = e
            group.barrier.abort()

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in err:
        if e is not None:
            raise e
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--dirs", default="1,2,5")
    ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--nodes", type=int, default=24000)
    a = ap.parse_args()
    dirs = [int(x) for x in a.dirs.split(",")]
    w = workloads.config_brain_like(a.nodes, isolate=True)
    for world in [int(x) for x in a.ranks.split(",")]:
        res = run_ranks(world, lambda r, tr: rank_body(w, world, r, tr, a.steps, dirs))
        g_ms = max(r["gradient_ms"] for r in res)
        for P in dirs:
            its = res[0][P]["tlm"] + res[0][P]["soa"]
            assert all(r[P]["tlm"] + r[P]["soa"] == its for r in res)
            ms = max(r[P]["ms"] for r in res)
            per = max(1.0, its / P)
            print(json.dumps(dict(workload=w.name, nodes=int(len(w.mesh.points)), steps=a.steps, ranks=world, P=P,
                                  transport="threads of one process, one GPU", hessian_ms=round(ms, 2),
                                  gradient_ms=round(g_ms, 2), hessian_over_gradient=round(ms / g_ms, 3),
                                  tlm_pcg_its=res[0][P]["tlm"], soa_pcg_its=res[0][P]["soa"],
                                  allreduces_per_iteration=round(res[0][P]["allreduces"] / per, 2),
                                  exchanges_per_iteration=round(res[0][P]["exchanges"] / per, 2))), flush=True)


if __name__ == "__main__":
    main()
