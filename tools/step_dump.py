#!/usr/bin/env python3
"""
The RD time stepper step by step on a handful of small problems, for a bit-for-bit comparison of two BUILDS of the library (a
refactoring of gl_step in csrc/solver.hip must move neither a bit nor a count).  The problems are those of the GPU tests at
their sizes, a few seconds each:

  * _c3_reduced(24), 40 steps (an age-32 relearn, forcing modes 0 -> 1): default flags, FULL_NEWTON, FIXED_FORCING,
    EXTRAPOLATE_GUESS, NO_FUSED_GUESS, FP32_JACOBIAN set, WARM_START cleared; rd_linear PCG and CHEBYSHEV;
  * the take-back case of test_gpu_chebyshev.py (GLIMS_CHEB_TEST_SCALE_HI = 0.45);
  * the strong-nonlinearity cases of test_gpu_newton_quadratic.py (rebase events);
  * the cg_atol case of test_a_solve_whose_tolerance_is_met_leaves_the_state_alone, with and without the warm start;
  * a stiff case with the RD multigrid, and `auto` switching to it mid-run on the Delaunay mesh of test_gpu_rd_multigrid.py;
  * new Dirichlet values between steps;
  * a jittered-lattice and a random-point mesh of about 2000 nodes;
  * two and three threaded ranks, with and without the take-back hook;
  * a run restarted with set_state after 8 steps, and a fresh handle started from the state of step 8.

Per problem: the final field and, after every step(1), every integer counter of glims_stats plus last_newton_res, last_cg_res,
cheb_lmin and cheb_lmax.

    python tools/step_dump.py out.npz [--lib path/to/libglimship.so]   # run once per build (default: the tree's library)
    python tools/step_dump.py --compare a.npz b.npz                    # np.array_equal of every array; exit status 1 on a difference
                                                                       # (and, per file, the restarted run against the fresh handle)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOATS = ("last_newton_res", "last_cg_res", "cheb_lmin", "cheb_lmax")


def compare(pa, pb, restarted="restarted", fresh="fresh_from_step8"):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("%-44s only in one file" % k)
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
        print("%-44s %-14s %s" % (k, a[k].shape, "equal" if same else "DIFFERENT"))
        if not same:
            bad.append(k)
            if k.endswith("/counters") and a[k].shape == b[k].shape and (k[:-8] + "counter_names") in a.files:
                names = a[k[:-8] + "counter_names"]
                for j in np.flatnonzero((a[k] != b[k]).any(axis=0)):
                    print("    %-28s %s | %s" % (names[j], a[k][-1, j], b[k][-1, j]))
    print("%d arrays, %d differ" % (len(set(a.files) | set(b.files)), len(bad)))
    # within each file: the run restarted with set_state against the fresh handle started from the same state (printed, not
    # part of the verdict; files without such a pair have nothing to print)
    for path, f in ((pa, a), (pb, b)):
        for k in sorted(k[len(restarted) + 1:] for k in f.files if k.startswith(restarted + "/") and not k.endswith("_names")):
            if fresh + "/" + k not in f.files:
                continue
            x, y = f[restarted + "/" + k], f[fresh + "/" + k]
            print("%-24s %s/%-10s vs %s/%-10s %s" % (os.path.basename(path), restarted, k, fresh, k,
                                                     "equal" if x.shape == y.shape and np.array_equal(x, y) else "DIFFERENT"))
    return 1 if bad else 0


def int_keys(st):
    return [k for k in sorted(st) if isinstance(st[k], (int, np.integer)) and not isinstance(st[k], bool)]


class Recorder:
    def __init__(self, out, tag):
        self.out, self.tag, self.ints, self.floats, self.keys = out, tag, [], [], None

    def steps(self, h, n, expect=0, before=None):
        for k in range(n):
            if before is not None:
                before(h, k)
            status = h.step(1)
            st = h.stats()
            if self.keys is None:
                self.keys = int_keys(st)
            self.ints.append([int(st[k]) for k in self.keys] + [int(status)])
            self.floats.append([float(st[k]) for k in FLOATS])
            if status != 0:
                assert status == expect, (self.tag, k, status)
                break
        return self

    def finish(self, h, own=None):
        c = h.get_state(want_u=False)[0]
        self.out[self.tag + "/c"] = np.asarray(c if own is None else c[:own])
        self.out[self.tag + "/counters"] = np.array(self.ints, dtype=np.int64)
        self.out[self.tag + "/counter_names"] = np.array(self.keys + ["status"])
        self.out[self.tag + "/residuals"] = np.array(self.floats, dtype=np.float64)
        h.close()


def open_handle(B, w, tables=None, flags_or=0, flags_andnot=0, dirichlet=None, setup=True, **opts):
    h = B.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
    t = tables or w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    opts.setdefault('dt', w.dt)
    h.set_options(flags=(h.options.flags | flags_or) & ~flags_andnot, **opts)
    if dirichlet is not None:
        h.set_dirichlet_c(*dirichlet)
    if setup:
        h.setup(False)
        h.set_state(w.c0)
    return h


def ranks_case(B, out, tag, w, world, steps):
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import node_owners, build_local_part
    pts, cells = w.mesh.points, w.mesh.cells
    owner = node_owners(pts, world, cells, method='rcb')
    parts = [build_local_part(pts, cells, owner, r, world) for r in range(world)]
    outs = [dict() for _ in range(world)]

    def rank_body(rank, tr):
        part = parts[rank]
        h = B.Handle(part.points, part.cells, w.cell_label[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(pts.min(axis=0), pts.max(axis=0))
        t = w.tables
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        h.set_options(dt=w.dt, mech_history=0)
        h.setup(False)
        h.set_state(w.c0[part.global_ids])
        Recorder(outs[rank], "%s/rank%d" % (tag, rank)).steps(h, steps).finish(h, own=part.n_own)
        if tr.failed is not None:
            raise tr.failed

    run_threaded_ranks(world, rank_body)
    for o in outs:
        out.update(o)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        raise SystemExit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4 and sys.argv[2] != "--lib"):
        raise SystemExit(__doc__)
    import torch  # noqa: F401  (before the library loads: the threaded transport's HIP runtime is the library's)
    from glimslib_amd import workloads, _backend as B
    from glimslib_amd.mesh import RectangleMesh
    import test_gpu_rd_multigrid as trm
    if len(sys.argv) == 4:
        B.LIB_PATH = os.path.abspath(sys.argv[3])
    out = {}

    def c3_reduced(n):
        w = workloads.config_c3(n)
        hx = 240.0 / n
        w.c0 = np.exp(-((w.mesh.points - np.array([118.0, -109.0, 72.0])) ** 2).sum(axis=1) / (2.0 * (2.5 * hx) ** 2))
        return w

    def case(tag, h, steps, **kw):
        Recorder(out, tag).steps(h, steps, **kw).finish(h)
        print("%-28s done" % tag, flush=True)

    w = c3_reduced(24)
    variants = dict(default={}, full_newton=dict(flags_or=B.FLAG_FULL_NEWTON), fixed_forcing=dict(flags_or=B.FLAG_FIXED_FORCING),
                    extrapolate=dict(flags_or=B.FLAG_EXTRAPOLATE_GUESS), no_fused_guess=dict(flags_or=B.FLAG_NO_FUSED_GUESS),
                    fp32_jacobian=dict(flags_or=B.FLAG_FP32_JACOBIAN), no_warm_start=dict(flags_andnot=B.FLAG_WARM_START),
                    pcg=dict(rd_linear=B.RD_LINEAR_PCG), chebyshev=dict(rd_linear=B.RD_LINEAR_CHEBYSHEV))
    for name, kw in variants.items():
        case("c3_24/" + name, open_handle(B, w, **kw), 40)

    os.environ["GLIMS_CHEB_TEST_SCALE_HI"] = "0.45"   # (read when a handle is created)
    case("take_back", open_handle(B, w), 10)
    del os.environ["GLIMS_CHEB_TEST_SCALE_HI"]

    w16 = c3_reduced(16)
    case("strong_3d", open_handle(B, w16, tables=dict(w16.tables, rho=[12.0 * r for r in w16.tables['rho']])), 8)
    mesh = RectangleMesh((0.0, 0.0), (10.0, 8.0), 60, 48)
    tables = dict(D=[0.0, 0.05], rho=[0.0, 0.6], gamma=[0.0, 0.1], E=[1.0, 3e-3], nu=[0.3, 0.45])
    c0 = 0.9 * np.exp(-0.2 * ((mesh.points - np.array([5.0, 4.0])) ** 2).sum(axis=1))
    w2 = workloads.Workload("square", mesh, np.ones(mesh.num_cells(), dtype=np.int32), tables, c0, 1.0, 8, False)
    case("strong_2d", open_handle(B, w2), 8)

    for name, kw in (("warm", {}), ("cold", dict(flags_andnot=B.FLAG_WARM_START))):
        h = open_handle(B, w, **kw)
        rec = Recorder(out, "cg_atol/" + name).steps(h, 10)
        ca = h.get_state(want_u=False)[0]
        h.set_options(cg_atol=10.0 * np.linalg.norm(h.rd_residual(ca, ca)))
        rec.steps(h, 3, expect=B.GLIMS_NOT_CONVERGED).finish(h)

    smesh, lab, tabs, left, sc0 = trm._stiff_problem(3, 22)
    vals = 0.2 + 0.1 * np.cos(5.0 * smesh.points[left, 1])
    ws = workloads.Workload("stiff", smesh, lab, tabs, sc0, 1.0, 0, False)
    case("stiff_mg", open_handle(B, ws, dirichlet=(left, vals), rd_precond=B.RD_PRECOND_MULTIGRID), 4)
    wu = workloads.config_unstructured(30000)
    # (D x 20 000: the Jacobi count of the first step is above `auto`'s break-even where its prediction is not -- the switch)
    case("stiff_auto", open_handle(B, wu, tables=dict(wu.tables, D=[2e4 * d for d in wu.tables['D']]), dt=1.0), 4)

    f = w.mesh.facets()
    bn = np.unique(f['vertices'][f['exterior']])
    case("new_dirichlet", open_handle(B, w, dirichlet=(bn, np.full(len(bn), 0.01))), 12,
         before=lambda h, k: h.set_dirichlet_c(bn, np.full(len(bn), 0.01 + 0.002 * (k // 3))) if k % 3 == 2 else None)

    case("jittered_2000", open_handle(B, workloads.config_brain_like(2000, isolate=True)), 12)
    case("random_2000", open_handle(B, workloads.config_unstructured(2000)), 12)

    for world in (2, 3):
        ranks_case(B, out, "ranks%d" % world, w, world, 8)
        os.environ["GLIMS_CHEB_TEST_SCALE_HI"] = "0.45"
        ranks_case(B, out, "ranks%d_take_back" % world, w, world, 8)
        del os.environ["GLIMS_CHEB_TEST_SCALE_HI"]
        print("ranks%d done" % world, flush=True)

    # the second half of the restarted run counts from the restart, like the fresh handle started from the state of step 8
    h = open_handle(B, w)
    Recorder({}, "first_half").steps(h, 8)
    c8 = h.get_state(want_u=False)[0]
    h.set_state(c8)
    h.reset_stats()
    case("restarted", h, 8)
    w8 = c3_reduced(24)
    w8.c0 = c8
    h = open_handle(B, w8)
    h.reset_stats()
    case("fresh_from_step8", h, 8)

    np.savez(sys.argv[1], **out)
    print("%d arrays -> %s" % (len(out), sys.argv[1]))


if __name__ == "__main__":
    main()
