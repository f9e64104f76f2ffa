#!/usr/bin/env python3
"""
The elasticity solve, solve by solve, on a handful of small problems, for a bit-for-bit comparison of two BUILDS of the library
(a refactoring of gl_solve_mechanics in csrc/solver.hip, or of solve_elastic in csrc/adjoint.hip, must move neither a bit nor a
count).  The problems are those of tests/test_gpu_mechanics.py, test_gpu_multirank.py and test_gpu_adjoint_elastic.py at their
sizes, a few seconds each:

  * _c5_reduced(16), 12 coupled steps (step(1) + solve_mechanics()): the defaults (multigrid, history depth 8: the ring wraps),
    mech_history 0 and 2, block-Jacobi, mech_mixed = 2 with either preconditioner, mg_smooth = 1;
  * the depth sequence 2 -> 8 -> 3 of test_changing_the_history_depth_restarts_the_ring;
  * calls between solves, mid-run: set_materials + setup(True), set_dirichlet_u with another node set, set_mech_load, and
    set_state(c, None) -- the solves after the latter also against a fresh handle brought to the same state;
  * a 2-D RectangleMesh with inhomogeneous clamp values and a body load, the body pinned at six dofs, and no Dirichlet dofs at
    all (a uniform concentration: the right-hand side is self-equilibrated);
  * snapshot_mechanics of two saved snapshots and then a solve of the state; one derive that solves a snapshot's displacement;
  * adjoint_gradient(elastic=True) with dJ/dE and dJ/dnu at the smallest case of test_gpu_adjoint_elastic.py, either
    preconditioner (solve_elastic shares the preconditioner's preparation with gl_solve_mechanics);
  * two threaded ranks with the framed multigrid and the default history.

Per problem: U and c at the end and, after every step(1) + solve_mechanics(), every integer counter of glims_stats, the two
statuses and last_mech_res.

    python tools/mech_dump.py out.npz [--lib path/to/libglimship.so]   # run once per build (default: the tree's library)
    python tools/mech_dump.py --compare a.npz b.npz                    # np.array_equal of every array; exit status 1 on a difference
                                                                       # (and, per file, the restarted run against the fresh handle)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_dump import ROOT, compare, int_keys, open_handle   # noqa: E402  (step_dump puts ROOT and tests/ on sys.path)


class MechRecorder:
    def __init__(self, out, tag):
        self.out, self.tag, self.ints, self.floats, self.keys = out, tag, [], [], None

    def note(self, h, *statuses):
        st = h.stats()
        if self.keys is None:
            self.keys = int_keys(st)
        self.ints.append([int(st[k]) for k in self.keys] + [int(s) for s in statuses])
        self.floats.append(float(st["last_mech_res"]))

    def solves(self, h, n, before=None):
        for k in range(n):
            if before is not None:
                before(h, k)
            status = h.step(1)
            self.note(h, status, h.solve_mechanics())
        return self

    def finish(self, h, own=None, **extra):
        c, u = h.get_state()
        d = h.dim
        self.out[self.tag + "/c"] = np.asarray(c if own is None else c[:own])
        self.out[self.tag + "/U"] = np.asarray(u if own is None else u[:own * d])
        self.out[self.tag + "/counters"] = np.array(self.ints, dtype=np.int64)
        self.out[self.tag + "/counter_names"] = np.array(self.keys + ["step_status", "mech_status"])
        self.out[self.tag + "/residuals"] = np.array(self.floats, dtype=np.float64)
        for k, v in extra.items():
            self.out[self.tag + "/" + k] = np.asarray(v)
        h.close()
        print("%-28s done" % self.tag, flush=True)


def all_dofs(nodes, d):
    return (np.asarray(nodes)[:, None] * d + np.arange(d)).ravel()


def mech_handle(B, w, dofs=None, vals=None, mload=None, c0=None, **opts):
    """open_handle with the clamp (default: u = 0 on the workload's Dirichlet nodes), glims_setup(with_mechanics) and the state."""
    h = open_handle(B, w, setup=False, **opts)
    if dofs is None:
        dofs = all_dofs(w.dirichlet_nodes, w.mesh.points.shape[1])
    if len(dofs):
        h.set_dirichlet_u(dofs, np.zeros(len(dofs)) if vals is None else vals)
    if mload is not None:
        h.set_mech_load(mload)
    h.setup(True)
    h.set_state(w.c0 if c0 is None else c0)
    return h


def ranks_case(B, out, tag, w, world, solves):
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    pts, cells = w.mesh.points, w.mesh.cells
    parts = partition_mesh(pts, cells, world)
    outs = [dict() for _ in range(world)]

    def rank_body(rank, tr):
        part = parts[rank]
        h = B.Handle(part.points, part.cells, w.cell_label[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(pts.min(axis=0), pts.max(axis=0))
        t = w.tables
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        h.set_options(dt=w.dt)                                # defaults: multigrid, history depth 8
        g2l = np.full(len(pts), -1, dtype=np.int64)
        g2l[part.global_ids[:part.n_own]] = np.arange(part.n_own)
        nodes = g2l[np.asarray(w.dirichlet_nodes)]
        dofs = all_dofs(nodes[nodes >= 0], 3)
        h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
        h.setup(True)
        h.set_state(w.c0[part.global_ids])
        MechRecorder(outs[rank], "%s/rank%d" % (tag, rank)).solves(h, solves).finish(h, own=part.n_own)
        if tr.failed is not None:
            raise tr.failed

    run_threaded_ranks(world, rank_body)
    for o in outs:
        out.update(o)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        raise SystemExit(compare(sys.argv[2], sys.argv[3], restarted="restarted", fresh="fresh_from_solve6"))
    if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4 and sys.argv[2] != "--lib"):
        raise SystemExit(__doc__)
    import torch  # noqa: F401  (before the library loads: the threaded transport's HIP runtime is the library's)
    from glimslib_amd import workloads, _backend as B
    from glimslib_amd.mesh import BoxMesh, RectangleMesh
    import test_gpu_mechanics as tgm
    import test_gpu_adjoint_elastic as tae
    if len(sys.argv) == 4:
        B.LIB_PATH = os.path.abspath(sys.argv[3])
    out = {}

    def case(tag, h, n, **kw):
        MechRecorder(out, tag).solves(h, n, **kw).finish(h)

    w = tgm._c5_reduced(16)
    variants = dict(default={}, history0=dict(mech_history=0), history2=dict(mech_history=2),
                    block_jacobi=dict(mech_precond=B.PRECOND_BLOCK_JACOBI),
                    mixed_mg=dict(mech_mixed=2), mixed_block_jacobi=dict(mech_mixed=2, mech_precond=B.PRECOND_BLOCK_JACOBI),
                    mg_smooth1=dict(mg_smooth=1))
    for name, kw in variants.items():
        case("c5_16/" + name, mech_handle(B, w, **kw), 12)

    depth = {3: 8, 7: 3}   # (before solve k: the new depth)
    case("depth_2_8_3", mech_handle(B, w, mech_history=2), 9,
         before=lambda h, k: h.set_options(mech_history=depth[k]) if k in depth else None)

    # calls between solves: the ring holds six solves (and the hint a count) when they come
    t2 = dict(w.tables, E=[1.5 * e for e in w.tables['E']], nu=[0.9 * v for v in w.tables['nu']])

    def new_materials(h, k):
        if k == 6:
            h.set_materials(t2['D'], t2['rho'], t2['gamma'], t2['E'], t2['nu'])
            h.setup(True)
    case("mid_run/set_materials", mech_handle(B, w), 10, before=new_materials)

    d = 3
    nodes = np.asarray(w.dirichlet_nodes)
    half = all_dofs(nodes[w.mesh.points[nodes, 0] < w.mesh.points[:, 0].mean()], d)
    case("mid_run/set_dirichlet_u", mech_handle(B, w), 10,
         before=lambda h, k: h.set_dirichlet_u(half, 1e-3 * np.cos(np.arange(len(half)))) if k == 6 else None)
    mload = 1e-6 * np.random.default_rng(3).standard_normal(w.mesh.num_vertices() * d)
    case("mid_run/set_mech_load", mech_handle(B, w), 10, before=lambda h, k: h.set_mech_load(mload) if k == 6 else None)

    # set_state(c, None) after six solves: the solves after it against a fresh handle started from the same state
    h = mech_handle(B, w)
    MechRecorder({}, "first_half").solves(h, 6)
    c6 = h.get_state(want_u=False)[0]
    h.set_state(c6)
    h.reset_stats()
    case("restarted", h, 4)
    h = mech_handle(B, w, c0=c6)
    h.reset_stats()
    case("fresh_from_solve6", h, 4)

    # 2-D, inhomogeneous clamp values on the left half of the hull, two tissues, a body load
    mesh = RectangleMesh((-5, -5), (5, 5), 60, 52)
    lab = (1 + (mesh.cell_midpoints()[:, 0] > mesh.points[:, 0].mean())).astype(np.int32)
    tabs = dict(D=[0, .1, .02], rho=[0, .1, .05], gamma=[0, .2, .1], E=[1.0, 1e-3, 3e-3], nu=[.3, .40, .45])
    f = mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    bn = bn[mesh.points[bn, 0] < mesh.points[:, 0].mean()]
    c0 = np.exp(-0.2 * ((mesh.points - mesh.points.mean(0)) ** 2).sum(1))
    w2 = workloads.Workload("rectangle", mesh, lab, tabs, c0, 1.0, 8, False)
    dofs2 = all_dofs(bn, 2)
    for name, pre in (("mg", B.PRECOND_MULTIGRID), ("block_jacobi", B.PRECOND_BLOCK_JACOBI)):
        case("rectangle_2d/" + name,
             mech_handle(B, w2, dofs=dofs2, vals=1e-3 * np.cos(np.arange(len(dofs2))),
                         mload=1e-6 * np.random.default_rng(2).standard_normal(mesh.num_vertices() * 2), mech_precond=pre), 6)

    # the body pinned at six dofs, and with no Dirichlet dofs at all (test_unclamped_body_and_single_pinned_node)
    mesh = BoxMesh((0, 0, 0), (4.0, 3.0, 2.0), 12, 10, 8)
    tabs = dict(D=[0, .1], rho=[0, .1], gamma=[0, .15], E=[1.0, 2e-3], nu=[.3, .4])
    p = mesh.points
    ix = int(np.flatnonzero((p[:, 1] == 0) & (p[:, 2] == 0) & (p[:, 0] > 0))[0])
    iy = int(np.flatnonzero((p[:, 0] == 0) & (p[:, 2] == 0) & (p[:, 1] > 0))[0])
    pins = np.array([0, 1, 2, 3 * ix + 1, 3 * ix + 2, 3 * iy + 2])
    w3 = workloads.Workload("box", mesh, np.ones(mesh.num_cells(), np.int32), tabs, np.full(mesh.num_vertices(), 0.6), 1.0, 0,
                            False)
    case("pinned_body", mech_handle(B, w3, dofs=pins), 4)
    case("no_dirichlet", mech_handle(B, w3, dofs=np.zeros(0, dtype=np.int64)), 4)

    # other entry points into the solve: snapshots' displacements, then the state's; a derive that solves one
    h = mech_handle(B, w)
    rec = MechRecorder(out, "snapshots")
    sids = []
    for _ in range(2):
        rec.solves(h, 2)
        sids.append(h.snapshot_save())
    rec.solves(h, 1)
    extra = {}
    for sid in sids:
        u, st = h.snapshot_mechanics(sid)
        rec.note(h, 0, st)
        extra["u_snapshot%d" % sid] = u
    rec.note(h, 0, h.solve_mechanics())
    extra["von_mises_snapshot%d" % sids[0]] = h.derive("van_mises_stress", snapshot=sids[0])
    rec.note(h, 0, h.last_derive_status)
    extra["derive_info"] = np.array([v for _, v in sorted(h.derive_info().items())], dtype=np.int64)
    rec.finish(h, **extra)

    # the E / nu adjoint: solve_elastic for u_k and mu_k
    for dim in (2,):
        prob = tae._problem(dim)
        terms = tae._terms(prob, 3)
        for name, pre in (("mg", B.PRECOND_MULTIGRID), ("block_jacobi", B.PRECOND_BLOCK_JACOBI)):
            g = tae._rank(prob, 1, 0, None, 3, terms, opts=dict(mech_precond=pre))
            tag = "adjoint_elastic_%dd/%s" % (dim, name)
            for k in ("J", "dD", "drho", "dgamma", "dc0", "dE", "dnu"):
                out[tag + "/" + k] = np.asarray(g[k])
            adj = g["adj"]
            names = int_keys(adj)
            out[tag + "/counters"] = np.array([[int(adj[k]) for k in names]], dtype=np.int64)
            out[tag + "/counter_names"] = np.array(names)
            print("%-28s done" % tag, flush=True)

    ranks_case(B, out, "ranks2", tgm._c5_reduced(24), 2, 5)
    print("ranks2 done", flush=True)

    np.savez(sys.argv[1], **out)
    print("%d arrays -> %s" % (len(out), sys.argv[1]))


if __name__ == "__main__":
    main()
