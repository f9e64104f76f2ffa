"""
Numpy statement of the image-space misfit terms (include/glims_hip.h, "image-space misfit terms") -- the
CPU reference of glims_adjoint_image_terms, independent of the code under test.

    J_img = 1/2 w sum_p q_p (h((P c_k)_p) - t_p)^2      over the OBSERVED points: found in the mesh, t_p not NaN, q_p != 0

with P, P^T of tests/sampler_common.py (locate / apply / apply_t) and h = identity ('img_l2') or the tanh threshold of
tests/adjoint_common.py ('img_thresh').  adjoint_common's and adjoint_hessian_common's recursions have no hook for a new kind,
so this file carries a first- and second-order recursion of its own for the concentration kinds ('c_l2', 'c_thresh', 'img_l2',
'img_thresh'; no displacement terms).  tests/test_adjoint_image_cpu.py checks it by central differences.

An image term is a dict {step, kind, level, smooth, weight, target [n_points], pweight [n_points] or None, loc = (cell, w) of
sampler_common.locate for its points}; the device tests add sampler = the library's Sampler of the same points.
"""
import numpy as np
import scipy.sparse.linalg as spla

import sampler_common as sc
from adjoint_common import dthresh, thresh
from adjoint_hessian_common import _Cells, _direction, d2thresh

IMAGE_KINDS = ("img_l2", "img_thresh")


def image_term(prob, x, step, kind, target, pweight=None, level=0.0, smooth=1.0, weight=1.0):
    """Locates the points x [n, dim] in prob's mesh (asserting that no decision sits on the rounding edge)."""
    cell, w, margin, _ = sc.locate(prob.points, prob.cells, x)
    sc.assert_decisive(margin)
    return dict(step=step, kind=kind, level=level, smooth=smooth, weight=weight, target=target, pweight=pweight,
                loc=(cell, w))


def observed(t):
    cell = t["loc"][0]
    q = np.ones(len(cell)) if t.get("pweight") is None else np.asarray(t["pweight"], dtype=np.float64).reshape(-1)
    return (cell >= 0) & ~np.isnan(np.asarray(t["target"], dtype=np.float64).reshape(-1)) & (q != 0.0), q


def _h(t, v):
    if t["kind"] in ("img_thresh", "c_thresh"):
        lv, s = t["level"], t["smooth"]
        return thresh(v, lv, s), dthresh(v, lv, s), d2thresh(v, lv, s)
    return v, np.ones_like(v), np.zeros_like(v)


def _image_parts(prob, t, c):
    """(ok, q, e = h(v) - t, h', h'') at the observed points of an image term (values elsewhere are not to be read)."""
    cell, w = t["loc"]
    ok, q = observed(t)
    v = sc.apply(prob.cells, cell, w, c, fill=0.0)
    hv, hp, h2 = _h(t, v)
    e = np.zeros(len(v))
    e[ok] = hv[ok] - np.asarray(t["target"], dtype=np.float64).reshape(-1)[ok]
    return ok, q, e, hp, h2


def misfit(prob, o, traj, terms):
    J = 0.0
    for t in terms:
        c = traj[t["step"]]
        if t["kind"] in IMAGE_KINDS:
            ok, q, e, _, _ = _image_parts(prob, t, c)
            J += 0.5 * t["weight"] * np.sum(q[ok] * e[ok] ** 2)
        else:
            e = _h(t, c)[0] - t["target"]
            J += 0.5 * t["weight"] * e @ (o.M @ e)
    return J


def hessian(prob, o, traj, terms, directions=()):
    """(J, dD, drho, dc0, hv): J and its gradient by the discrete adjoint and, per direction (a dict {'D', 'rho' [n_labels],
    'c0' [n_nodes]}, missing keys 0), the Hessian-vector product {'D', 'rho', 'c0'}.  Per step the nodal terms in list order,
    then the image terms in list order (the order of the device sweep)."""
    assert all(t["kind"] in ("c_l2", "c_thresh") + IMAGE_KINDS for t in terms)
    lab, L = prob.labels, prob.n_labels
    geo = _Cells(prob)
    n, N, dt, M = geo.n, len(traj) - 1, prob.dt, o.M
    free = o._free_mask_c()
    rho = prob.rho[lab]
    dirs = [_direction(prob, dd) for dd in directions]
    P = len(dirs)

    def rd_solver(c):
        lu = spla.splu(o.rd_jacobian(c)[free][:, free].tocsc())

        def solve(b):
            x = np.zeros(n)
            x[free] = lu.solve(b[free])
            return x
        return solve

    # tangent-linear sweep
    dc = [[dirs[p][3].copy()] for p in range(P)]
    for k in range(1, N + 1):
        c = traj[k]
        solve = rd_solver(c)
        for p in range(P):
            D_p, r_p = dirs[p][0][lab], dirs[p][1][lab]
            src = -dt * geo.scatter(D_p[:, None] * geo.K(c) + r_p[:, None] * (geo.T(c, c) - geo.Mv(c)))
            dc[p].append(solve(M @ dc[p][k - 1] + src))
    J = misfit(prob, o, traj, terms)
    dD, drho, dc0 = np.zeros(L), np.zeros(L), None
    hv = [dict(D=np.zeros(L), rho=np.zeros(L), c0=None) for _ in range(P)]
    lam_next = np.zeros(n)
    nu_next = [np.zeros(n) for _ in range(P)]
    for k in range(N, -1, -1):
        c = traj[k]
        g = np.zeros(n)
        dg = [np.zeros(n) for _ in range(P)]
        here = [t for t in terms if t["step"] == k]
        for t in [t for t in here if t["kind"] not in IMAGE_KINDS]:
            hc, hp, h2 = _h(t, c)
            Me = M @ (hc - t["target"])
            g += t["weight"] * hp * Me
            for p in range(P):
                dg[p] += t["weight"] * (hp * (M @ (hp * dc[p][k])) + h2 * Me * dc[p][k])
        for t in [t for t in here if t["kind"] in IMAGE_KINDS]:
            cell, w = t["loc"]
            ok, q, e, hp, h2 = _image_parts(prob, t, c)
            r = np.zeros(len(cell))
            r[ok] = t["weight"] * q[ok] * hp[ok] * e[ok]
            g += sc.apply_t(prob.cells, cell, w, r, n)
            for p in range(P):
                Pd = sc.apply(prob.cells, cell, w, dc[p][k], fill=0.0)
                r2 = np.zeros(len(cell))
                r2[ok] = t["weight"] * q[ok] * (hp[ok] ** 2 + h2[ok] * e[ok]) * Pd[ok]
                dg[p] += sc.apply_t(prob.cells, cell, w, r2, n)
        if k == 0:
            dc0 = M @ lam_next + g
            for p in range(P):
                hv[p]["c0"] = M @ nu_next[p] + dg[p]
            break
        solve = rd_solver(c)
        lam = solve(g + M @ lam_next)
        dD += -dt * np.bincount(lab, geo.gg(lam, c), minlength=L)
        drho += -dt * np.bincount(lab, geo.xyz(lam, c, c) - geo.xy(lam, c), minlength=L)
        for p in range(P):
            D_p, r_p, dcp = dirs[p][0][lab], dirs[p][1][lab], dc[p][k]
            soa = 2.0 * rho[:, None] * geo.T(dcp, lam) + D_p[:, None] * geo.K(lam) + \
                r_p[:, None] * (2.0 * geo.T(c, lam) - geo.Mv(lam))
            nu_k = solve(M @ nu_next[p] + dg[p] - dt * geo.scatter(soa))
            hv[p]["D"] += -dt * np.bincount(lab, geo.gg(nu_k, c) + geo.gg(lam, dcp), minlength=L)
            hv[p]["rho"] += -dt * np.bincount(lab, geo.xyz(nu_k, c, c) - geo.xy(nu_k, c) +
                                               2.0 * geo.xyz(lam, c, dcp) - geo.xy(lam, dcp), minlength=L)
            nu_next[p] = nu_k
        lam_next = lam
    return J, dD, drho, dc0, hv


def adjoint(prob, o, traj, terms):
    """(J, dJ/dD [labels], dJ/drho, dJ/dc0)."""
    return hessian(prob, o, traj, terms)[:4]


def flat(prob, d):
    """[D, rho, c0] of a direction or product dict as one vector."""
    D, r, _, c0 = _direction(prob, d)
    return np.concatenate([D, r, c0])


def gradient_at(prob, m, n_steps, terms):
    """(J, flat gradient [D, rho, c0]) at m = dict(D, rho, c0)."""
    o = prob.oracle(D=m["D"], rho=m["rho"])
    traj = prob.trajectory(o, n_steps, c0=m["c0"])
    J, dD, drho, dc0 = adjoint(prob, o, traj, terms)
    return J, np.concatenate([dD, drho, dc0])


def standard_terms(prob, n_steps, seed=0, grid_size=None, n_pts=150):
    """The term list of the gradient tests: on the last step an img_thresh term on an overhanging grid (NaN targets, a
    pweight with zeros and non-unit values), an img_l2 term on a point set and a nodal c_thresh term; an image term midway;
    an image term at step 0.  Returns (terms, grid = (origin, spacing, size), points)."""
    rng = np.random.default_rng(seed)
    d = prob.dim
    # (in 3-D the outermost layer of an overhanging grid is a large share of it: more points per axis, a smaller overhang)
    size = np.asarray(grid_size if grid_size is not None else ([19, 17] if d == 2 else [17, 15, 13]))
    origin, spacing = sc.overhanging_grid(prob.points, size, overhang=0.05 if d == 2 else 0.03)
    xg = sc.grid_points(origin, spacing, size)
    lo, hi = prob.points.min(axis=0), prob.points.max(axis=0)
    xp = lo + (hi - lo) * rng.uniform(-0.04, 1.04, (n_pts, d))
    ng = len(xg)
    tg = rng.uniform(0, 1, ng)
    tg[rng.random(ng) < 0.1] = np.nan
    qg = rng.uniform(0.5, 2.0, ng)
    qg[rng.random(ng) < 0.05] = 0.0
    tp = rng.uniform(0, 0.6, n_pts)
    tp[rng.random(n_pts) < 0.1] = np.nan
    tm = rng.uniform(0, 0.6, ng)
    tm[rng.random(ng) < 0.1] = np.nan
    mid = max(1, n_steps // 2) if n_steps else 0
    terms = [image_term(prob, xg, n_steps, "img_thresh", tg, qg, level=0.25, smooth=0.1, weight=1.5),
             image_term(prob, xp, n_steps, "img_l2", tp, None, weight=2.0),
             dict(step=n_steps, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5,
                  target=rng.uniform(0, 1, len(prob.points))),
             image_term(prob, xg, mid, "img_l2", tm, None, weight=0.7),
             image_term(prob, xp, 0, "img_thresh", rng.uniform(0, 1, n_pts), rng.uniform(0.5, 2.0, n_pts), level=0.4,
                        smooth=0.15, weight=0.8)]
    for t, where in zip(terms, ("grid", "points", None, "grid", "points")):
        if where:
            t["where"] = where
    return terms, (origin, spacing, size), xp


# ---- the (D, rho) fit to two threshold images: one setting for the numpy fit (CPU test) and the public-API fit (GPU test) ----
FIT = dict(lo=-5.0, hi=5.0, n=24, steps=10, dt=1.0, truth=(0.1, 0.1), start=(0.05, 0.2), smooth=0.1, levels=(0.2, 0.4),
           # voxels of about half the mesh width (10 / 24 = 0.4167) on a grid that does not align with the mesh lines
           origin=(-5.07, -5.04), spacing=(0.211, 0.213), size=(49, 48),
           options={"maxiter": 30, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16, bounds=(0.005, 0.5))


def fit_problem(points, cells, D, rho):
    """The fit's model on the given mesh: two tissues (1: x >= 0, 2: x < 0; id 0 carried by no cell) with one D and one rho,
    no Dirichlet data on c, the Gaussian seed of the public-API fits."""
    from adjoint_common import Problem
    x = np.asarray(points, dtype=np.float64)
    lab = np.where(x[np.asarray(cells)].mean(axis=1)[:, 0] >= 0.0, 1, 2).astype(np.int32)
    c0 = np.exp(-((x[:, 0] - 1.0) ** 2 + (x[:, 1] - 0.5) ** 2) / 2.0)
    one = np.ones(3)
    return Problem.from_mesh(x, cells, lab, D * one, rho * one, 0.1 * one, 0.001 * one, 0.4 * one, c0, dt=FIT["dt"])


def fit_image_terms(prob, c_true):
    """The two threshold images of c_true on FIT's grid (NaN outside the mesh) as volume-weighted img_thresh terms."""
    size = np.asarray(FIT["size"])
    x = sc.grid_points(FIT["origin"], FIT["spacing"], size)
    cell, w, margin, _ = sc.locate(prob.points, prob.cells, x)
    sc.assert_decisive(margin)
    v = sc.apply(prob.cells, cell, w, c_true)                      # NaN outside
    vol = float(np.prod(FIT["spacing"]))
    return [dict(step=FIT["steps"], kind="img_thresh", level=lv, smooth=FIT["smooth"], weight=vol,
                 target=thresh(v, lv, FIT["smooth"]), pweight=None, loc=(cell, w)) for lv in FIT["levels"]]
