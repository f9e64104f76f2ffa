#!/usr/bin/env python3
"""
Cost of the image-space misfit terms on partitioned handles (DESIGN.md sections 13 and 14) ->
profiles/image_misfit_partitioned.jsonl, one JSON object.

  python tools/image_misfit_partitioned_cost.py [--points 24000] [--world 4] [--grid 32] [--steps 6] [--out FILE]

The brain-like mesh (26 588 nodes at --points 24000) under a --grid^3 voxel grid, `--world` ranks as THREADS of one process
that share one GPU through the host-staged threaded transport: a rehearsal of the code path, not of RCCL -- the times say what
the calls cost in this setting and nothing about a run with one GPU per rank.
  (a) wall time of glims_sampler_resolve (median over fresh samplers of the same grid, the slowest rank of each round);
  (b) median wall time of a gradient call with ONE img_thresh term on the last step, and of the same call with a nodal
      c_thresh term in its place (the slowest rank), with the adjoint PCG iterations of each call: the two right-hand sides
      differ, every iteration of a partitioned solve is an all-reduce through the transport, and the difference of the two
      times carries the difference of the iteration counts as well as the image term's own work.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--world", type=int, default=4)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_misfit_partitioned.jsonl"))
    a = ap.parse_args()
    import torch  # noqa: F401  (before libglimship: one HIP runtime for the library and the transport's ctypes calls)
    from glimslib_amd import _backend as B, workloads
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    wl = workloads.config_brain_like(a.points, isolate=True)
    pts, cells = wl.mesh.points, wl.mesh.cells
    lab = np.asarray(wl.cell_label, dtype=np.int32)
    t = {k: np.asarray(v, dtype=np.float64) for k, v in wl.tables.items()}
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    size = (a.grid,) * 3
    spacing = (hi - lo) * 1.1 / (a.grid - 1)
    origin = lo - 0.05 * (hi - lo)
    level, smooth = 0.3, 0.1
    rng = np.random.default_rng(0)
    target_img = rng.uniform(0, 1, a.grid ** 3)
    target_nod = rng.uniform(0, 1, len(pts))

    def body(rank, tr):
        part = partition_mesh(pts, cells, a.world, rank)
        h = B.Handle(part.points, part.cells, lab[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, a.world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(lo, hi)
        h.set_materials(t["D"], t["rho"], t["gamma"], t["E"], t["nu"])
        h.set_options(dt=wl.dt)
        h.setup(with_mechanics=False)
        h.set_state(np.asarray(wl.c0, float)[part.global_ids])
        h.adjoint_record(True)
        assert h.step(a.steps) == 0
        ms_resolve = []
        for _ in range(a.reps + 1):
            s = h.sampler_grid(origin, spacing, size)
            t0 = time.perf_counter()
            s.resolve(part.cell_ids)                 # (ends in a device synchronise)
            ms_resolve.append((time.perf_counter() - t0) * 1e3)
        img = [dict(step=a.steps, kind="img_thresh", level=level, smooth=smooth, sampler=s, target=target_img)]
        nod = [dict(step=a.steps, kind="c_thresh", level=level, smooth=smooth, target=target_nod[part.global_ids])]

        def timed(terms):
            out = []
            for _ in range(a.reps + 1):
                its0 = h.adjoint_stats()["pcg_its"]
                t0 = time.perf_counter()
                J = h.adjoint_gradient(terms, want_dc0=False)[0]
                out.append((time.perf_counter() - t0) * 1e3)
            return out[1:], J, h.adjoint_stats()["pcg_its"] - its0

        ms_img, J_img, its_img = timed(img)
        n_obs = h.image_term_info(0)[2]
        ms_nod, _, its_nod = timed(nod)
        res = dict(ms_resolve=ms_resolve[1:], ms_img=ms_img, ms_nod=ms_nod, J=J_img, n_obs=n_obs, n_kept=s.n_found,
                   n_own=part.n_own, n_local=len(part.global_ids), its_img=its_img, its_nod=its_nod)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return res

    res = run_threaded_ranks(a.world, body)
    assert all(r["J"] == res[0]["J"] for r in res)
    slowest = lambda key: statistics.median([max(r[key][k] for r in res) for k in range(a.reps)])
    rec = dict(case="brain-like mesh, %d^3 grid, %d recorded steps, %d threaded ranks on ONE GPU (host-staged transport): a "
                    "rehearsal, not a multi-GPU measurement" % (a.grid, a.steps, a.world),
               n_nodes=int(len(pts)), n_cells=int(len(cells)), n_points=int(a.grid ** 3), world=a.world,
               n_observed=int(sum(r["n_obs"] for r in res)), n_kept_per_rank=[int(r["n_kept"]) for r in res],
               n_own_per_rank=[int(r["n_own"]) for r in res], n_local_per_rank=[int(r["n_local"]) for r in res],
               ms_sampler_resolve=slowest("ms_resolve"), ms_gradient_one_img_thresh=slowest("ms_img"),
               ms_gradient_one_c_thresh=slowest("ms_nod"),
               ms_image_term_extra=slowest("ms_img") - slowest("ms_nod"),
               adjoint_pcg_its_img_thresh=int(res[0]["its_img"]), adjoint_pcg_its_c_thresh=int(res[0]["its_nod"]),
               note="wall times: per round the slowest rank, then the median of %d rounds after a warm-up round; every call "
                    "ends in a device synchronise; transport = device -> host -> thread barrier -> device" % a.reps)
    print(json.dumps(rec), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
