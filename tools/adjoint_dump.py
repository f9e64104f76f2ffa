#!/usr/bin/env python3
"""
Every output of the discrete adjoint on a handful of small problems, for a bit-for-bit comparison of two BUILDS of the library
(a refactoring of csrc/adjoint.hip must not move a bit).  The problems are those of the GPU tests at their sizes, a few seconds
in total:

  * Problem(2, 16) and Problem(3, 6) with terms(6, smooth=0.1): c_l2, c_thresh and u_l2 terms, Dirichlet c, clamped u;
  * the stiff case of test_gpu_adjoint.py with the multigrid RD preconditioner;
  * 9 and 17 tissues (more than the 8 labels of one sensitivity launch), as test_label_chunks;
  * stored image terms (the hessian_case of test_gpu_adjoint_image.py);
  * a 2-rank threaded-transport gradient with dJ/dE and dJ/dnu.

Per problem: adjoint_gradient with and without elastic=True (where the handle has mechanics), adjoint_hessian with 1 and 4
directions (J, the gradient, every hv_*), their iteration counts, and adjoint_stats() without its wall time.

    python tools/adjoint_dump.py out.npz                 # run once per build of glimslib_amd/libglimship.so
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


def dump_case(out, tag, h, prob, n_steps, terms, dirs, elastic):
    h.adjoint_record(True)
    assert h.step(n_steps) == 0
    names = ("J", "dD", "drho", "dgamma", "dc0", "dE", "dnu")
    for full in ((False, True) if elastic else (False,)):
        g = h.adjoint_gradient(terms, prob.n_labels, elastic=full)
        for k, v in zip(names, g):
            out["%s/gradient%s/%s" % (tag, "_full" if full else "", k)] = np.asarray(v)
    for P in (1, 4):
        r = h.adjoint_hessian(terms, dirs[:P])
        for k, v in r.items():
            if k == "stats":
                out["%s/hessian_P%d/its" % (tag, P)] = np.array([v[s] for s in sorted(v) if s != "ms"], dtype=np.float64)
            else:
                out["%s/hessian_P%d/%s" % (tag, P, k)] = np.asarray(v)
    out[tag + "/adjoint_stats"] = stats_of(h)
    h.close()


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        raise SystemExit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    import torch  # noqa: F401  (before the library loads: the threaded transport's HIP runtime is the library's)
    import adjoint_image_common as aic
    from adjoint_common import Problem, many_tissues
    from glimslib_amd import _backend as B
    out = {}
    for dim, n in ((2, 16), (3, 6)):
        prob = Problem(dim, n)
        dump_case(out, "basic_%dd" % dim, handle(B, prob), prob, 6, prob.terms(6, smooth=0.1), directions(prob, 13, 4), True)
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
    prob = te._problem(2)
    terms = te._terms(prob, 3)
    res = run_threaded_ranks(2, lambda r, tr: te._rank(prob, 2, r, tr, 3, terms))
    for r, g in enumerate(res):
        for k in ("J", "dD", "drho", "dgamma", "dc0", "dE", "dnu"):
            out["ranks2/rank%d/%s" % (r, k)] = np.asarray(g[k])
        out["ranks2/rank%d/adjoint_stats" % r] = np.array([g["adj"][k] for k in sorted(g["adj"]) if k != "ms_backward"],
                                                          dtype=np.int64)
    np.savez(sys.argv[1], **out)
    print("%d arrays -> %s" % (len(out), sys.argv[1]))


if __name__ == "__main__":
    main()
