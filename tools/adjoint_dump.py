#!/usr/bin/env python3
"""
Every output of the discrete adjoint on a handful of small problems, for a bit-for-bit comparison of two BUILDS of the library
(a refactoring of csrc/adjoint.hip must not move a bit).  The problems are those of the GPU tests at their sizes, a few seconds
in total:

  * Problem(2, 16) and Problem(3, 6) with terms(6, smooth=0.1): c_l2, c_thresh and u_l2 terms, Dirichlet c, clamped u;
  * the stiff case of test_gpu_adjoint.py with the multigrid RD preconditioner;
  * 9 and 17 tissues (more than the 8 labels of one sensitivity launch), as test_label_chunks;
  * stored image terms (the hessian_case of test_gpu_adjoint_image.py);
  * a 2-rank threaded-transport gradient with dJ/dE and dJ/dnu; the same with 9 tissues (the ranks' rows are [L][3] + [L][2]
    with L beyond one sensitivity launch);
  * adjoint_hessian_full on the first two problems: 1 and 4 directions with parts in E and nu, and one call without a direction
    in E / nu (hv_E, hv_nu still asked for: the E / nu sums run without the dK passes);
  * a Hessian with stored volume terms (the small case of test_gpu_observable_terms.py, 2-D);
  * the collective Hessian on two threaded ranks with displacement terms and a gamma direction (the case of
    test_gpu_adjoint_hessian_partitioned.py);
  * a gradient with deformed image terms (the 2-D case of test_gpu_adjoint_deformed.py).

Per problem: adjoint_gradient with and without elastic=True (where the handle has mechanics), adjoint_hessian with 1 and 4
directions (J, the gradient, every hv_*), their iteration counts, and adjoint_stats() without its wall time.

    python tools/adjoint_dump.py out.npz [--lib path/to/libglimship.so]   # run once per build (default: the tree's library)
    python tools/adjoint_dump.py --compare a.npz b.npz   # np.array_equal of every array; exit status 1 on a difference
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("%-44s only in one file" % k)
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
        print("%-44s %-14s %s" % (k, a[k].shape, "equal" if same else "DIFFERENT"))
        if not same:
            bad.append(k)
    print("%d arrays, %d differ" % (len(set(a.files) | set(b.files)), len(bad)))
    return 1 if bad else 0


def handle(B, prob, mechanics=True, **opts):
    h = B.Handle(prob.points, prob.cells, prob.labels)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12, **opts)
    if prob.dir_c is not None:
        h.set_dirichlet_c(prob.dir_c[0], prob.dir_c[1])
    if mechanics:
        h.set_dirichlet_u(prob.dir_u[0], prob.dir_u[1])
    h.setup(with_mechanics=mechanics)
    h.set_state(prob.c0)
    return h


def directions(prob, seed, count, scale=None):
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    sD, srho, sgam = scale if scale is not None else (prob.D, prob.rho, prob.gamma)
    out = []
    for k in range(count):
        d = dict(D=sD * rng.uniform(-1, 1, L), rho=srho * rng.uniform(-1, 1, L), gamma=sgam * rng.uniform(-1, 1, L))
        if k % 2 == 0:
            d["c0"] = 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
        out.append(d)
    return out


def stats_of(h):
    st = h.adjoint_stats()
    return np.array([st[k] for k in sorted(st) if k != "ms_backward"], dtype=np.int64)


def put_hessian(out, prefix, r):
    for k, v in r.items():
        if k == "stats":
            out[prefix + "/its"] = np.array([v[s] for s in sorted(v) if s != "ms"], dtype=np.float64)
        else:
            out[prefix + "/" + k] = np.asarray(v)


def dump_case(out, tag, h, prob, n_steps, terms, dirs, elastic, full_dirs=None, record=True):
    if record:
        h.adjoint_record(True)
        assert h.step(n_steps) == 0
    names = ("J", "dD", "drho", "dgamma", "dc0", "dE", "dnu")
    for full in ((False, True) if elastic else (False,)):
        g = h.adjoint_gradient(terms, prob.n_labels, elastic=full)
        for k, v in zip(names, g):
            out["%s/gradient%s/%s" % (tag, "_full" if full else "", k)] = np.asarray(v)
    for P in (1, 4) if dirs else ():
        put_hessian(out, "%s/hessian_P%d" % (tag, P), h.adjoint_hessian(terms, dirs[:P]))
    if full_dirs:
        for P in (1, 4):
            put_hessian(out, "%s/hessian_full_P%d" % (tag, P), h.adjoint_hessian_full(terms, full_dirs[:P]))
        put_hessian(out, tag + "/hessian_full_rows_only", h.adjoint_hessian_full(terms, dirs[:2]))   # el_sums without el_dirs
    out[tag + "/adjoint_stats"] = stats_of(h)
    h.close()
    print("%-20s done" % tag, flush=True)


def elastic_directions(prob, seed, dirs):
    """dirs with parts in E and nu: every second one in both, the others in one of them."""
    rng = np.random.default_rng(seed)
    out = []
    for k, d in enumerate(dirs):
        d = dict(d)
        if k % 2 == 0 or k % 4 == 1:
            d["E"] = prob.E * rng.uniform(-1, 1, prob.n_labels)
        if k % 2 == 0 or k % 4 == 3:
            d["nu"] = 0.1 * rng.uniform(-1, 1, prob.n_labels)
        out.append(d)
    return out


def put_ranks(out, tag, res, keys=("J", "dD", "drho", "dgamma", "dc0", "dE", "dnu")):
    for r, g in enumerate(res):
        for k in keys:
            out["%s/rank%d/%s" % (tag, r, k)] = np.asarray(g[k])
        out["%s/rank%d/adjoint_stats" % (tag, r)] = np.array([g["adj"][k] for k in sorted(g["adj"]) if k != "ms_backward"],
                                                             dtype=np.int64)
    print("%-20s done" % tag, flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        raise SystemExit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) not in (2, 4) or (len(sys.argv) == 4 and sys.argv[2] != "--lib"):
        raise SystemExit(__doc__)
    import torch  # noqa: F401  (before the library loads: the threaded transport's HIP runtime is the library's)
    import adjoint_image_common as aic
    from adjoint_common import Problem, many_tissues
    from glimslib_amd import _backend as B
    if len(sys.argv) == 4:
        B.LIB_PATH = os.path.abspath(sys.argv[3])
    out = {}
    for dim, n in ((2, 16), (3, 6)):
        prob = Problem(dim, n)
        dirs = directions(prob, 13, 4)
        dump_case(out, "basic_%dd" % dim, handle(B, prob), prob, 6, prob.terms(6, smooth=0.1), dirs, True,
                  full_dirs=elastic_directions(prob, 17, dirs))
    prob = Problem(3, 10, dt=1.0, D=(0.1, 0.2), rho=(0.05, 0.1), dirichlet_c=None)
    h = handle(B, prob, rd_precond=B.RD_PRECOND_MULTIGRID)
    dump_case(out, "stiff_mg", h, prob, 4, prob.terms(4, with_u=False), directions(prob, 14, 4), True)
    for dim, L, n, empty, zero in ((2, 9, 16, 3, 5), (3, 17, 6, 12, 9)):
        prob = many_tissues(dim, L, n=n, empty=(empty,), zero=(zero,), zero_gamma=(zero,), seed=L)
        dump_case(out, "labels_%d" % L, handle(B, prob), prob, 5, prob.terms(5), directions(prob, L, 4, (0.03, 0.4, 0.15)),
                  True)
    prob = Problem(2, 16)
    terms, grid, xp = aic.standard_terms(prob, 5, seed=9)
    h = handle(B, prob, mechanics=False)
    sg, sp = h.sampler_grid(*grid), h.sampler_points(xp)
    for t in terms:
        if t.get("where"):
            t["sampler"] = sg if t["where"] == "grid" else sp
    dirs = [{k: v for k, v in d.items() if k != "gamma"} for d in directions(prob, 13, 4)]
    dump_case(out, "image", h, prob, 5, terms, dirs, False)
    # two ranks as threads of this process (the per-label sums cross the ranks in rank order)
    import test_gpu_adjoint_elastic as te
    from glimslib_amd.parallel import run_threaded_ranks
    # (u clamped on the whole exterior, as the partitioned tests have it: every rank must own constrained dofs, or none)
    prob = te._clamp_all_exterior(te._problem(2), 0.02)
    terms = te._terms(prob, 3)
    put_ranks(out, "ranks2", run_threaded_ranks(2, lambda r, tr: te._rank(prob, 2, r, tr, 3, terms)))
    prob = te._clamp_all_exterior(many_tissues(2, 9, n=12, empty=(3,), zero_gamma=(1,), mech_load=0.5, seed=15), 0.02)
    terms = te._terms(prob, 3)
    put_ranks(out, "ranks2_labels_9", run_threaded_ranks(2, lambda r, tr: te._rank(prob, 2, r, tr, 3, terms)))
    # the collective Hessian on two ranks: displacement terms, a gamma direction
    import test_gpu_adjoint_hessian_partitioned as thp
    from adjoint_common import u_terms
    prob = te._clamp_all_exterior(many_tissues(2, 3, n=16, mech_load=1.0, seed=22), 0.02)
    terms = u_terms(prob, [1, 3], seed=21) + [dict(step=3, kind="c_l2", weight=1.0, target=np.full(len(prob.points), 0.2))]
    dirs = thp._directions(prob, 13, 2, gamma=True)
    res = run_threaded_ranks(2, lambda r, tr: thp._hess_rank(prob, 2, r, tr, 3, terms, dirs, [(0, 1)], mech=True))
    for r, g in enumerate(res):
        for k, v in zip(("J", "dD", "drho", "dgamma", "dc0"), g["grad"]):
            out["ranks2_hessian/rank%d/gradient/%s" % (r, k)] = np.asarray(v)
        put_hessian(out, "ranks2_hessian/rank%d/hessian_P2" % r, g["res"][0])
    print("%-20s done" % "ranks2_hessian", flush=True)
    # stored volume terms: a Hessian through gl_observable_terms_of_step
    import observable_terms_common as otc
    import test_gpu_observable_terms as tot
    from test_gpu_adjoint import _record
    from test_gpu_adjoint_image import _handle as image_handle
    prob, N = tot._problem(2)
    h = image_handle(B, prob)
    traj = _record(h, N)
    terms = [t for t in otc.standard_terms(prob, traj, seed=12) if t.get("observable") != "sharp"]
    dump_case(out, "volume_terms", h, prob, N, terms, tot._directions(prob, 13, 4), False, record=False)
    # deformed image terms: the gradient through the location (no second order)
    import adjoint_deformed_common as adc
    import test_gpu_adjoint_deformed as tad
    from test_gpu_adjoint import _handle as mech_handle
    prob = adc.clamped_problem(2, 16)
    terms = tad._std_terms(prob, 6)
    h = mech_handle(B, prob)
    tad._attach(h, terms)
    dump_case(out, "deformed", h, prob, 6, terms, None, True)
    np.savez(sys.argv[1], **out)
    print("%d arrays -> %s" % (len(out), sys.argv[1]))


if __name__ == "__main__":
    main()
