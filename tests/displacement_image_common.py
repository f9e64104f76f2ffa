"""
Numpy statement of the DISPLACEMENT-IMAGE misfit terms (include/glims_hip.h, "displacement-image misfit terms"; DESIGN.md section
13) -- the CPU reference of glims_adjoint_displacement_image_terms, independent of the code under test.  With P the operator of
a fixed sampler (sampler_common.locate on the REFERENCE mesh), u_k = K_el^-1 (G c_k + f) the oracle's mech_solve of step k,

    J      = 1/2 w sum_p q_p sum_a kappa_a (s (P u_k)_p,a - d_p,a)^2       over the OBSERVED points,
    dJ/du_k = P^T R,     R_p,a  = w q_p kappa_a s (s (P u_k)_p,a - d_p,a),
    d(dJ/du_k) . du = P^T R2,   R2_p,a = w q_p kappa_a s^2 (P du)_p,a.

A point is observed iff it was found, q_p != 0 and d_p,a is not NaN for every component with kappa_a != 0.  dJ/du_k joins the
load of the step's u_l2 terms: one mu_k = K_el^-1 dJ/du_k per step, then G^T mu_k, the gamma sums and the E / nu derivatives
mu^T (d_p G c - d_p K u) from ASSEMBLED d_p K, d_p G (as adjoint_elastic_common / adjoint_hessian_elastic_common), and for the
products the sweep of adjoint_hessian_elastic_common.hessian_full with  K dmu = sum w M_vec du + sum P^T R2(du) - dK mu.
The recursion knows 'c_l2', 'c_thresh', 'u_l2', the fixed image terms of adjoint_image_common ('img_l2' / 'img_thresh' with
`loc`) and 'img_u_l2'.  tests/test_displacement_image_cpu.py checks it by central differences of its own J and gradient.
"""
import copy

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sampler_common as sc
from adjoint_common import dthresh, thresh
from adjoint_deformed_common import clamped_problem, oracle_of   # noqa: F401  (the problems of the tests)
from adjoint_elastic_common import lame_derivatives
from adjoint_hessian_common import _Cells, _direction, d2thresh
from adjoint_hessian_elastic_common import _label_dir, lame_second_derivatives
from oracle.glims_oracle import assemble_coupling, assemble_elasticity, compute_lambda, compute_mu

KIND = "img_u_l2"
KEYS = ("D", "rho", "gamma", "E", "nu")
IMAGE_KINDS = ("img_l2", "img_thresh")


def displacement_term(prob, x, step, target, pweight=None, weight=1.0, scale=1.0, cweight=None, grid=None):
    """A displacement image term on the points x [n, dim] (grid = (origin, spacing, size) when x are that grid's points),
    located in prob's reference mesh; no decision of the location sits on the rounding edge."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    cell, w, margin, _ = sc.locate(prob.points, prob.cells, x)
    sc.assert_decisive(margin)
    cw = np.ones(prob.dim) if cweight is None else np.asarray(cweight, dtype=np.float64)
    return dict(step=step, kind=KIND, target=np.ascontiguousarray(target, dtype=np.float64).reshape(len(x), prob.dim),
                pweight=pweight, weight=weight, scale=scale, cweight=cw, x=x, grid=grid, loc=(cell, w))


def observed(t):
    """(ok [n] bool, q [n]) of a displacement image term."""
    cell = t["loc"][0]
    q = np.ones(len(cell)) if t.get("pweight") is None else np.asarray(t["pweight"], dtype=np.float64).reshape(-1)
    ok = (cell >= 0) & (q != 0.0)
    for a, k in enumerate(t["cweight"]):
        if k != 0.0:
            ok &= ~np.isnan(t["target"][:, a])
    return ok, q


def _residual(prob, t, u):
    """(ok, q, e [n, dim]): e_a = s (P u)_a - d_a at the observed points and the components with kappa_a != 0, else 0."""
    cell, w = t["loc"]
    ok, q = observed(t)
    Pu = sc.apply(prob.cells, cell, w, np.reshape(u, prob.points.shape), fill=0.0)
    e = np.zeros_like(Pu)
    for a, k in enumerate(t["cweight"]):
        if k != 0.0:
            e[ok, a] = t["scale"] * Pu[ok, a] - t["target"][ok, a]
    return ok, q, e


def term_J(prob, t, u):
    ok, q, e = _residual(prob, t, u)
    return 0.5 * t["weight"] * np.sum(q[ok, None] * t["cweight"][None] * e[ok] ** 2)


def term_load(prob, t, u):
    """dJ/du = P^T R, flat [n_nodes * dim]."""
    cell, w = t["loc"]
    ok, q, e = _residual(prob, t, u)
    R = t["weight"] * t["scale"] * q[:, None] * t["cweight"][None] * e
    R[~ok] = 0.0
    return sc.apply_t(prob.cells, cell, w, R, len(prob.points)).reshape(-1)


def term_second(prob, t, du):
    """d(dJ/du) . du = P^T R2, flat."""
    cell, w = t["loc"]
    ok, q = observed(t)
    Pdu = sc.apply(prob.cells, cell, w, np.reshape(du, prob.points.shape), fill=0.0)
    R2 = t["weight"] * t["scale"] ** 2 * q[:, None] * t["cweight"][None] * Pdu
    R2[~ok] = 0.0
    R2[:, t["cweight"] == 0.0] = 0.0
    return sc.apply_t(prob.cells, cell, w, R2, len(prob.points)).reshape(-1)


def _h(t, v):
    if t["kind"] in ("img_thresh", "c_thresh"):
        lv, s = t["level"], t["smooth"]
        return thresh(v, lv, s), dthresh(v, lv, s), d2thresh(v, lv, s)
    return v, np.ones_like(v), np.zeros_like(v)


def _image_parts(prob, t, c):
    cell, w = t["loc"]
    q = np.ones(len(cell)) if t.get("pweight") is None else np.asarray(t["pweight"], dtype=np.float64).reshape(-1)
    tg = np.asarray(t["target"], dtype=np.float64).reshape(-1)
    ok = (cell >= 0) & ~np.isnan(tg) & (q != 0.0)
    hv, hp, h2 = _h(t, sc.apply(prob.cells, cell, w, c, fill=0.0))
    e = np.zeros(len(cell))
    e[ok] = hv[ok] - tg[ok]
    return ok, q, e, hp, h2


def needs_u(t):
    return t["kind"] in ("u_l2", KIND)


def misfit(prob, o, traj, terms):
    d = prob.dim
    Mvec = sp.kron(o.M, sp.eye(d)).tocsr()
    J = 0.0
    for t in terms:
        c = traj[t["step"]]
        if t["kind"] == KIND:
            J += term_J(prob, t, o.mech_solve(c))
        elif t["kind"] == "u_l2":
            e = o.mech_solve(c) - np.ravel(t["target"])
            J += 0.5 * t["weight"] * e @ (Mvec @ e)
        elif t["kind"] in IMAGE_KINDS:
            ok, q, e, _, _ = _image_parts(prob, t, c)
            J += 0.5 * t["weight"] * np.sum(q[ok] * e[ok] ** 2)
        else:
            e = _h(t, c)[0] - t["target"]
            J += 0.5 * t["weight"] * e @ (o.M @ e)
    return J


def sweep(prob, o, traj, terms, directions=()):
    """(J, g, hv): g = {'D', 'rho', 'gamma', 'E', 'nu' [labels], 'c0'}, hv one such dict per direction (a dict of the same keys,
    labels or a scalar, missing keys 0).  prob's own tables must be those of the oracle o."""
    lab, d, L = prob.labels, prob.dim, prob.n_labels
    pts, cells_ = prob.points, prob.cells
    geo = _Cells(prob)
    cells, n = geo.cells, geo.n
    N, dt, M = len(traj) - 1, prob.dt, o.M
    Mvec = sp.kron(M, sp.eye(d)).tocsr()
    free = o._free_mask_c()
    rho = prob.rho[lab]
    dirs = [_direction(prob, dd) for dd in directions]
    dEs = [_label_dir(prob, dd, "E") for dd in directions]
    dnus = [_label_dir(prob, dd, "nu") for dd in directions]
    P = len(dirs)
    g = dict(D=np.zeros(L), rho=np.zeros(L), gamma=np.zeros(L), E=np.zeros(L), nu=np.zeros(L), c0=None)
    hv = [dict(D=np.zeros(L), rho=np.zeros(L), gamma=np.zeros(L), E=np.zeros(L), nu=np.zeros(L), c0=None) for _ in range(P)]
    J = 0.0
    if any(needs_u(t) for t in terms):
        Kel, G = o._mech_setup()
        free_u = np.ones(n * d, bool)
        if prob.dir_u is not None:
            free_u[np.asarray(prob.dir_u[0], dtype=np.int64)] = False
        Kff = spla.splu(Kel[free_u][:, free_u].tocsc())
        mu_c, lam_c, gam_c = compute_mu(prob.E[lab], prob.nu[lab]), compute_lambda(prob.E[lab], prob.nu[lab]), prob.gamma[lab]
        d1 = lame_derivatives(prob.E, prob.nu)            # per label
        d2 = lame_second_derivatives(prob.E, prob.nu)
        present = [t for t in range(L) if (lab == t).any()]
        masks = {t: (lab == t).astype(float) for t in present}
        dK1, dG1 = {}, {}
        for p in ("E", "nu"):
            mp, lp = d1[p]
            for t in present:
                dK1[p, t] = assemble_elasticity(pts, cells_, mp[lab] * masks[t], lp[lab] * masks[t])
                dG1[p, t] = assemble_coupling(pts, cells_, mp[lab] * masks[t], lp[lab] * masks[t], gam_c)
        dK, dG, dK2, dG2, dGg = [], [], [], [], []
        for j in range(P):
            dE, dnu, dga = dEs[j], dnus[j], dirs[j][2]
            dm = dE * d1["E"][0] + dnu * d1["nu"][0]
            dl = dE * d1["E"][1] + dnu * d1["nu"][1]
            dK.append(assemble_elasticity(pts, cells_, dm[lab], dl[lab]))
            dG.append(assemble_coupling(pts, cells_, mu_c, lam_c, dga[lab]) + assemble_coupling(pts, cells_, dm[lab], dl[lab], gam_c))
            k2, g2, gg = {}, {}, {}
            for t in present:
                gg[t] = assemble_coupling(pts, cells_, dm[lab] * masks[t], dl[lab] * masks[t], 1.0)
                for p, (a, b) in (("E", ("EE", "Enu")), ("nu", ("Enu", "nunu"))):
                    dmp = dE * d2[a][0] + dnu * d2[b][0]
                    dlp = dE * d2[a][1] + dnu * d2[b][1]
                    mp, lp = d1[p]
                    k2[p, t] = assemble_elasticity(pts, cells_, dmp[lab] * masks[t], dlp[lab] * masks[t])
                    g2[p, t] = assemble_coupling(pts, cells_, dmp[lab] * masks[t], dlp[lab] * masks[t], gam_c) + \
                        assemble_coupling(pts, cells_, mp[lab] * masks[t], lp[lab] * masks[t], dga[lab])
            dK2.append(k2)
            dG2.append(g2)
            dGg.append(gg)
        cG = (2.0 * mu_c + d * lam_c) * geo.vol / (d + 1)   # G_T with gamma = 1

        def solve_u(b):
            x = np.zeros(n * d)
            x[free_u] = Kff.solve(b[free_u])
            return x

        def div(v):
            return np.einsum('mad,mad->m', v.reshape(n, d)[cells], geo.grads)

    def rd_solver(c):
        lu = spla.splu(o.rd_jacobian(c)[free][:, free].tocsc())

        def solve(b):
            x = np.zeros(n)
            x[free] = lu.solve(b[free])
            return x
        return solve

    dc = [[dirs[p][3].copy()] for p in range(P)]
    for k in range(1, N + 1):
        c = traj[k]
        solve = rd_solver(c) if P else None
        for p in range(P):
            D_p, r_p = dirs[p][0][lab], dirs[p][1][lab]
            src = -dt * geo.scatter(D_p[:, None] * geo.K(c) + r_p[:, None] * (geo.T(c, c) - geo.Mv(c)))
            dc[p].append(solve(M @ dc[p][k - 1] + src))
    lam_next = np.zeros(n)
    nu_next = [np.zeros(n) for _ in range(P)]
    for k in range(N, -1, -1):
        c = traj[k]
        here = [t for t in terms if t["step"] == k]
        gk = np.zeros(n)
        dg = [np.zeros(n) for _ in range(P)]
        have_u = any(needs_u(t) for t in here)
        if have_u:
            u = o.mech_solve(c)                # with its Dirichlet values
            gu = np.zeros(n * d)
        for t in here:
            w = t["weight"]
            if t["kind"] == "u_l2":
                e = u - np.ravel(t["target"])
                J += 0.5 * w * e @ (Mvec @ e)
                gu += w * (Mvec @ e)
            elif t["kind"] == KIND:
                J += term_J(prob, t, u)
                gu += term_load(prob, t, u)
            elif t["kind"] in IMAGE_KINDS:
                cell, wt = t["loc"]
                ok, q, e, hp, h2 = _image_parts(prob, t, c)
                J += 0.5 * w * np.sum(q[ok] * e[ok] ** 2)
                r = np.zeros(len(cell))
                r[ok] = w * q[ok] * hp[ok] * e[ok]
                gk += sc.apply_t(prob.cells, cell, wt, r, n)
                for p in range(P):
                    r2 = np.zeros(len(cell))
                    r2[ok] = (w * q * (hp * hp + h2 * e) * sc.apply(prob.cells, cell, wt, dc[p][k], fill=0.0))[ok]
                    dg[p] += sc.apply_t(prob.cells, cell, wt, r2, n)
            else:
                h, hp, h2 = _h(t, c)
                Me = M @ (h - t["target"])
                J += 0.5 * w * (h - t["target"]) @ Me
                gk += w * hp * Me
                for p in range(P):
                    dg[p] += w * (hp * (M @ (hp * dc[p][k])) + h2 * Me * dc[p][k])
        if have_u:
            mu = solve_u(gu)
            gk += G.T @ mu
            Sc = c[cells].sum(axis=1)
            g["gamma"] += np.bincount(lab, cG * div(mu) * Sc, minlength=L)
            for t in present:
                for key in ("E", "nu"):
                    g[key][t] += mu @ (dG1[key, t] @ c - dK1[key, t] @ u)
            for p in range(P):
                dcp = dc[p][k]
                du = solve_u(G @ dcp + dG[p] @ c - dK[p] @ u)
                load = -(dK[p] @ mu)
                for t in here:
                    if t["kind"] == "u_l2":
                        load += t["weight"] * (Mvec @ du)
                    elif t["kind"] == KIND:
                        load += term_second(prob, t, du)
                dmu = solve_u(load)
                dg[p] += G.T @ dmu + dG[p].T @ mu
                hv[p]["gamma"] += np.bincount(lab, cG * div(dmu) * Sc, minlength=L) + \
                    np.bincount(lab, cG * div(mu) * dcp[cells].sum(axis=1), minlength=L)
                for t in present:
                    hv[p]["gamma"][t] += mu @ (dGg[p][t] @ c)
                    for key in ("E", "nu"):
                        hv[p][key][t] += dmu @ (dG1[key, t] @ c - dK1[key, t] @ u) + \
                            mu @ (dG1[key, t] @ dcp - dK1[key, t] @ du) + mu @ (dG2[p][key, t] @ c - dK2[p][key, t] @ u)
        if k == 0:
            g["c0"] = M @ lam_next + gk
            for p in range(P):
                hv[p]["c0"] = M @ nu_next[p] + dg[p]
            break
        solve = rd_solver(c)
        lam = solve(gk + M @ lam_next)
        g["D"] += -dt * np.bincount(lab, geo.gg(lam, c), minlength=L)
        g["rho"] += -dt * np.bincount(lab, geo.xyz(lam, c, c) - geo.xy(lam, c), minlength=L)
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
    return J, g, hv


# ---- parameters as one dict m = {D, rho, gamma, E, nu [labels], c0} -------------------------------------------------------------
def base(prob):
    return dict(D=prob.D, rho=prob.rho, gamma=prob.gamma, E=prob.E, nu=prob.nu, c0=prob.c0)


def problem_at(prob, m):
    """A copy of the problem with the tables and the start of m, and its oracle."""
    p2 = copy.copy(prob)
    for k in KEYS:
        setattr(p2, k, np.array(m[k], dtype=np.float64))
    p2.c0 = np.array(m["c0"], dtype=np.float64)
    return p2, oracle_of(p2)


def J_at(prob, m, n_steps, terms):
    p2, o = problem_at(prob, m)
    return misfit(p2, o, p2.trajectory(o, n_steps), terms)


def gradient_at(prob, m, n_steps, terms):
    """(J, flat gradient [D, rho, gamma, E, nu, c0]) at m."""
    p2, o = problem_at(prob, m)
    J, g, _ = sweep(p2, o, p2.trajectory(o, n_steps), terms)
    return J, flat(prob, g)


def flat(prob, d):
    """[D, rho, gamma, E, nu, c0] of a gradient, a direction or a product (missing keys 0)."""
    D, rho, gam, c0 = _direction(prob, d)
    return np.concatenate([D, rho, gam, _label_dir(prob, d, "E"), _label_dir(prob, d, "nu"), c0])


def random_direction(prob, seed):
    """Every block at once, on every label (as tests/test_adjoint_hessian_elastic_cpu.py::_direction)."""
    rng = np.random.default_rng(seed)
    L, n = prob.n_labels, len(prob.points)
    return dict(D=0.03 * rng.uniform(-1, 1, L), rho=0.4 * rng.uniform(-1, 1, L), gamma=0.15 * rng.uniform(-1, 1, L),
                E=prob.E * rng.uniform(-1, 1, L), nu=0.1 * rng.uniform(-1, 1, L), c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1))


# ---- the term list of the tests ---------------------------------------------------------------------------------------------------
def standard_terms(prob, n_steps, seed=0):
    """A grid term at the last step whose mask has zeros (and voxels overhanging the mesh); a point-set term midway with NaN
    targets and points outside the mesh; a term with cweight = (1, 0[, 0]) at the last step whose ignored components hold NaNs;
    a term with scale = -2.5 at step 1; one c_thresh and one u_l2 term at the last step (the shared u_k / mu_k solves).
    The targets are a perturbed multiple of the displacement at prob's own parameters (a registration of the truth plus noise):
    J > 0 and no derivative vanishes."""
    rng = np.random.default_rng(seed)
    d, n = prob.dim, len(prob.points)
    o = oracle_of(prob)
    traj = prob.trajectory(o, n_steps)
    size = np.asarray([17, 15] if d == 2 else [9, 8, 7])
    # a grid that aligns with no mesh line and whose last layer along every axis lies outside the mesh
    lo, ext = prob.points.min(axis=0), np.ptp(prob.points, axis=0)
    origin, spacing = lo + 0.0138 * ext, 1.04 * ext / (size - 1)
    xg = sc.grid_points(origin, spacing, size)
    n_pts = 120
    xp = 0.5 + 0.56 * rng.uniform(-1.0, 1.0, (n_pts, d))            # about a fifth of them outside the unit box
    mid = max(1, n_steps // 2)

    def warp(x, step, factor, noise):
        cell, w, _, _ = sc.locate(prob.points, prob.cells, x)
        u = o.mech_solve(traj[step]).reshape(n, d)
        v = sc.apply(prob.cells, cell, w, u, fill=0.0)
        return factor * v + noise * np.abs(u).max() * rng.standard_normal(v.shape)

    mask = rng.uniform(0.5, 2.0, len(xg))
    mask[rng.random(len(xg)) < 0.2] = 0.0
    tp = warp(xp, mid, 0.8, 0.2)
    tp[rng.random(n_pts) < 0.1, rng.integers(0, d, 1)[0]] = np.nan
    tc = warp(xg, n_steps, 1.3, 0.2)
    tc[rng.random(len(xg)) < 0.3, 1:] = np.nan                      # NaNs in the ignored components only
    cw = np.zeros(d)
    cw[0] = 1.0
    qs = rng.uniform(0.5, 1.5, n_pts)
    terms = [displacement_term(prob, xg, n_steps, warp(xg, n_steps, 0.7, 0.3), mask, weight=1.5,
                               grid=(origin, spacing, size)),
             displacement_term(prob, xp, mid, tp, None, weight=2.0),
             displacement_term(prob, xg, n_steps, tc, None, weight=0.8, cweight=cw, grid=(origin, spacing, size)),
             displacement_term(prob, xp, 1, warp(xp, 1, -2.5 * 0.6, 0.5), qs, weight=0.6, scale=-2.5),
             dict(step=n_steps, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5, target=rng.uniform(0, 1, n)),
             dict(step=n_steps, kind="u_l2", weight=10.0, target=0.01 * rng.standard_normal(n * d))]
    return terms


def displacement_terms(terms):
    return [t for t in terms if t["kind"] == KIND]


# ---- the public-API fit and its numpy twin ---------------------------------------------------------------------------------------
# (coupling, D) of the model of deformed_volume_common.fit_problem (two tissues, the whole boundary clamped, the 24 x 24 mesh of
# the sibling fits) from two images of the last step of a truth run on adjoint_image_common.FIT's grid, which aligns with no mesh
# line: the T2-like threshold image of the concentration and the displacement image with a disc around the seed masked out (where
# a registration is unreliable).  u_weight puts the displacement image (|u| about 0.1) on the scale of the threshold image.
# bar: the recovery error of the numpy twin (tests/test_displacement_image_cpu.py::test_numpy_fit_of_coupling_and_D) rounded up
# to the next power of ten.
FIT = dict(lo=-5.0, hi=5.0, n=24, steps=10, dt=1.0, truth=(0.3, 0.1), start=(0.39, 0.07), level=0.2, smooth=0.1,
           origin=(-5.07, -5.04), spacing=(0.211, 0.213), size=(49, 48), seed=(1.0, 0.5), mask_radius=1.5, u_weight=100.0,
           bounds=(0.005, 0.5), options={"maxiter": 40, "gtol": 1e-14, "ftol": 1e-18}, tol=1e-18, bar=1e-12)


def fit_mask(x):
    """[n_points]: 0 inside the disc around the seed, 1 elsewhere."""
    r2 = ((np.asarray(x) - np.asarray(FIT["seed"])[None]) ** 2).sum(axis=1)
    return np.where(r2 < FIT["mask_radius"] ** 2, 0.0, 1.0)


def fit_terms(prob, c_true, u_true):
    """The two terms of the fit for numpy: the volume-weighted img_thresh term of c_true and the masked, volume-weighted
    displacement image of u_true (NaN outside the mesh in both)."""
    size = np.asarray(FIT["size"])
    x = sc.grid_points(FIT["origin"], FIT["spacing"], size)
    cell, w, margin, _ = sc.locate(prob.points, prob.cells, x)
    sc.assert_decisive(margin)
    vol = float(np.prod(FIT["spacing"]))
    v = sc.apply(prob.cells, cell, w, c_true)                                     # NaN outside
    d = sc.apply(prob.cells, cell, w, np.reshape(u_true, prob.points.shape))
    t_c = dict(step=FIT["steps"], kind="img_thresh", level=FIT["level"], smooth=FIT["smooth"], weight=vol,
               target=thresh(v, FIT["level"], FIT["smooth"]), pweight=None, loc=(cell, w))
    t_u = dict(step=FIT["steps"], kind=KIND, target=d, pweight=fit_mask(x), weight=FIT["u_weight"] * vol, scale=1.0,
               cweight=np.ones(prob.dim), x=x, grid=(FIT["origin"], FIT["spacing"], size), loc=(cell, w))
    return [t_c, t_u]
