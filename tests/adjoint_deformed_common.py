"""
Numpy statement of the image terms in the DEFORMED configuration (include/glims_hip.h, "image terms in the deformed
configuration") -- the CPU reference of glims_adjoint_deformed_image_terms, independent of the code under
test.  A deformed term observing step k locates its points x_p in the mesh at  y = X + scale u_k,  u_k = K_el^-1 (G c_k + f),
with deformed_common.locate, and with the winner's weights

    v_p = sum_a w_p,a c_k,a,   J = 1/2 w sum_p q_p (h(v_p) - t_p)^2   over the OBSERVED points (found now, t_p not NaN, q_p != 0),
    dJ/dc_k = P^T r,           r_p = w q_p h'(v_p) (h(v_p) - t_p),
    dJ/du_k = P^T S,           S_p = -scale r_p grad_y c_k|T(p)        (0 for a winner whose determinant ratio is not > 0).

dJ/du_k joins the displacement terms' load of the same step: one mu_k = K_el^-1 dJ/du_k per observed step, then G^T mu_k and the
gamma sums as in adjoint_common.adjoint, and the E / nu derivatives from the assembled dK/dp, dG/dp as in
adjoint_elastic_common.elastic_adjoint.  The recursion below knows every kind: 'c_l2', 'c_thresh', 'u_l2', the fixed image
terms of adjoint_image_common (a dict with `loc`) and the deformed ones (a dict with `x` and `scale`, no `loc`).
tests/test_adjoint_deformed_cpu.py checks it by central differences of its own J.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import deformed_common as dc
import sampler_common as sc
from adjoint_common import Problem, dthresh, thresh
from adjoint_elastic_common import lame_derivatives
from oracle.glims_oracle import (OracleTumorGrowth, assemble_coupling, assemble_elasticity, compute_lambda, compute_mu,
                                 p1_geometry, reference_mass, reference_triple)

IMAGE_KINDS = ("img_l2", "img_thresh")
MARGIN = 1e-3            # decisive_mask: the smallest barycentric weight an observed point may have at the base parameters
MAX_DROPPED = 0.05       # ... and the share of the found points the mask may drop
MIN_MOVED = 0.20         # every problem: at least this share of the found points lies in another cell than undeformed
MIN_RATIO = 0.3          # ... and no cell is compressed below this determinant ratio


def clamped_problem(dim, n, gamma=None, E=(1.0, 2.0), nu=(0.3, 0.4), **kw):
    """adjoint_common.Problem with the WHOLE outer boundary clamped (no point enters or leaves the mesh) and a coupling
    strong enough to push the tissue across cells: gamma = (2, 1.4) on the 2-D meshes, (4, 3) on the coarser 3-D ones
    (displacements up to about 0.13 on the unit square / cube; displacement_matters asserts what that buys)."""
    if gamma is None:
        gamma = (2.0, 1.4) if dim == 2 else (4.0, 3.0)
    prob = Problem(dim, n, gamma=gamma, E=E, nu=nu, **kw)
    x = prob.points
    b = np.nonzero((np.isclose(x, 0.0) | np.isclose(x, 1.0)).any(axis=1))[0]
    prob.dir_u = ((b[:, None] * dim + np.arange(dim)[None]).ravel(), np.zeros(len(b) * dim))
    return prob


def oracle_of(prob, D=None, rho=None, gamma=None, E=None, nu=None):
    lab = prob.labels
    pick = lambda a, b: np.asarray(b if a is None else a, dtype=np.float64)[lab]
    return OracleTumorGrowth(prob.points, prob.cells, pick(D, prob.D), pick(rho, prob.rho), pick(gamma, prob.gamma),
                             pick(E, prob.E), pick(nu, prob.nu), prob.dt, dirichlet_u=prob.dir_u, dirichlet_c=prob.dir_c,
                             rd_load=prob.rd_load, mech_load=prob.mech_load)


def deformed_term(x, step, kind, target, pweight=None, level=0.0, smooth=1.0, weight=1.0, scale=1.0, grid=None):
    """A deformed image term on the points x [n, dim]; grid = (origin, spacing, size) when x are that grid's points.  The
    dict is also what Handle.adjoint_gradient takes (deformed=True with `grid`, or with `points`)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return dict(step=step, kind=kind, level=level, smooth=smooth, weight=weight, scale=scale, target=target, pweight=pweight,
                x=x, grid=grid, points=None if grid is not None else x, deformed=True)


def is_deformed(t):
    return t["kind"] in IMAGE_KINDS and "loc" not in t


def locate_term(prob, t, u):
    """(cell, w, margin, n_accept) of the term's points in the mesh at X + scale u."""
    return dc.locate(prob.points, prob.cells, np.reshape(u, prob.points.shape), t["scale"], t["x"])


def decisive_mask(loc, margin=MARGIN):
    """q [n_points]: 0 for every found point whose smallest barycentric weight is below `margin`, 1 elsewhere.  With it as (a
    factor of) the pweight, every observed point sits at least `margin` inside its cell at the base parameters, so both ends of
    a central difference and the device pick the same cell.  Asserts that at most MAX_DROPPED of the found points go."""
    cell, w = loc[0], loc[1]
    found = cell >= 0
    drop = found & (w.min(axis=1) < margin)
    assert found.any() and drop.sum() <= MAX_DROPPED * found.sum(), \
        "the decisive mask drops %d of %d found points" % (drop.sum(), found.sum())
    return np.where(drop, 0.0, 1.0)


def displacement_matters(prob, t, u):
    """Asserts MIN_MOVED and MIN_RATIO for term t at the displacement u; returns (moved share, smallest ratio)."""
    cell = locate_term(prob, t, u)[0]
    cell0 = sc.locate(prob.points, prob.cells, t["x"])[0]
    found = cell >= 0
    moved = float(((cell != cell0) & found).sum()) / max(1, found.sum())
    ratio = dc.cell_ratios(prob.points, prob.cells, np.reshape(u, prob.points.shape), t["scale"]).min()
    assert moved >= MIN_MOVED, "only %.1f %% of the found points change their cell" % (100 * moved)
    assert ratio > MIN_RATIO, "smallest cell ratio %.3f" % ratio
    return moved, ratio


def _h(t, v):
    if t["kind"] in ("img_thresh", "c_thresh"):
        return thresh(v, t["level"], t["smooth"]), dthresh(v, t["level"], t["smooth"])
    return v, np.ones_like(v)


def _point_parts(prob, t, c, cell, w):
    """(ok, q, e = h(v) - t, h') of an image term with the location (cell, w)."""
    q = np.ones(len(cell)) if t.get("pweight") is None else np.asarray(t["pweight"], dtype=np.float64).reshape(-1)
    tg = np.asarray(t["target"], dtype=np.float64).reshape(-1)
    ok = (cell >= 0) & ~np.isnan(tg) & (q != 0.0)
    v = sc.apply(prob.cells, cell, w, c, fill=0.0)
    hv, hp = _h(t, v)
    e = np.zeros(len(v))
    e[ok] = hv[ok] - tg[ok]
    return ok, q, e, hp


def evaluate(prob, o, traj, terms, gradient=True):
    """J and, with `gradient`, dJ/dD, dJ/drho, dJ/dgamma, dJ/dE, dJ/dnu [labels] and dJ/dc0 of the term list; `info`: per
    deformed term (list order) a dict n_points, found, observed, folded (cells of the displaced mesh), min_ratio, cell, w.
    Per step: the nodal terms, the fixed image terms, the deformed image terms, each in list order."""
    pts, lab, d = prob.points, prob.labels, prob.dim
    cells = np.asarray(prob.cells, dtype=np.int64)
    L, n, N, dt, M = prob.n_labels, len(pts), len(traj) - 1, prob.dt, o.M
    Mv = sp.kron(M, sp.eye(d)).tocsr()
    out = dict(J=0.0, info=[None] * sum(is_deformed(t) for t in terms))
    slot = {id(t): i for i, t in enumerate([t for t in terms if is_deformed(t)])}
    needs_u = lambda t: t["kind"] == "u_l2" or is_deformed(t)
    if any(needs_u(t) for t in terms):
        Kel, G = o._mech_setup()
        free_u = np.ones(n * d, bool)
        if prob.dir_u is not None:
            free_u[np.asarray(prob.dir_u[0], dtype=np.int64)] = False
        Kff = spla.splu(Kel[free_u][:, free_u].tocsc()) if gradient else None
    if gradient:
        vol, grads = p1_geometry(pts, cells)
        Mr, Tr = reference_mass(d), reference_triple(d)
        free = o._free_mask_c()
        cG = (2.0 * compute_mu(o.E, o.nu) + d * compute_lambda(o.E, o.nu)) * vol / (d + 1)   # G_T with gamma = 1
    dD, drho, dgam = np.zeros(L), np.zeros(L), np.zeros(L)
    lam_next = np.zeros(n)
    obs = []                                  # (c_k, u_k, mu_k) of every step with a load on u
    for k in range(N, -1, -1):
        c = traj[k]
        here = [t for t in terms if t["step"] == k]
        if not here and not gradient:
            continue
        g, gu = np.zeros(n), np.zeros(n * d)
        have_u = any(needs_u(t) for t in here)
        u = o.mech_solve(c) if have_u else None
        for t in [t for t in here if t["kind"] not in IMAGE_KINDS]:
            if t["kind"] == "u_l2":
                e = u - np.ravel(t["target"])
                out["J"] += 0.5 * t["weight"] * e @ (Mv @ e)
                gu += t["weight"] * (Mv @ e)
            else:
                hv, hp = _h(t, c)
                Me = M @ (hv - t["target"])
                out["J"] += 0.5 * t["weight"] * (hv - t["target"]) @ Me
                g += t["weight"] * hp * Me
        for t in [t for t in here if t["kind"] in IMAGE_KINDS and not is_deformed(t)]:
            cell, w = t["loc"]
            ok, q, e, hp = _point_parts(prob, t, c, cell, w)
            out["J"] += 0.5 * t["weight"] * np.sum(q[ok] * e[ok] ** 2)
            r = np.zeros(len(cell))
            r[ok] = t["weight"] * q[ok] * hp[ok] * e[ok]
            g += sc.apply_t(prob.cells, cell, w, r, n)
        for t in [t for t in here if is_deformed(t)]:
            s = t["scale"]
            y = dc.deformed_points(pts, u, s)
            cell, w, margin, _ = sc.locate(y, prob.cells, t["x"])
            ok, q, e, hp = _point_parts(prob, t, c, cell, w)
            out["J"] += 0.5 * t["weight"] * np.sum(q[ok] * e[ok] ** 2)
            ratios = dc.cell_ratios(pts, prob.cells, np.reshape(u, pts.shape), s)
            out["info"][slot[id(t)]] = dict(n_points=len(cell), found=int((cell >= 0).sum()), observed=int(ok.sum()),
                                            folded=dc.n_inverted(ratios), min_ratio=float(ratios.min()), cell=cell, w=w,
                                            margin=margin)
            if not gradient:
                continue
            r = np.zeros(len(cell))
            r[ok] = t["weight"] * q[ok] * hp[ok] * e[ok]
            g += sc.apply_t(prob.cells, cell, w, r, n)
            gy = p1_geometry(y, cells)[1]                                          # grad_y lambda_a on the deformed cells
            gc = np.einsum('ma,mad->md', c[cells], gy)                             # grad_y c_k, constant per cell
            good = (ratios > 0) & np.isfinite(ratios)
            S = np.zeros((len(cell), d))
            use = ok & good[np.maximum(cell, 0)]
            S[use] = -s * r[use, None] * gc[cell[use]]
            gu += sc.apply_t(prob.cells, cell, w, S, n).reshape(-1)
        if not gradient:
            continue
        if have_u:
            mu = np.zeros(n * d)
            mu[free_u] = Kff.solve(gu[free_u])
            g += G.T @ mu
            div = np.einsum('mad,mad->m', mu.reshape(n, d)[cells], grads)
            dgam += np.bincount(lab, weights=cG * div * c[cells].sum(axis=1), minlength=L)
            obs.append((c, u, mu))
        if k == 0:
            out["c0"] = M @ lam_next + g
            break
        A = o.rd_jacobian(c)
        lam = np.zeros(n)
        lam[free] = spla.splu(A[free][:, free].tocsc()).solve((g + M @ lam_next)[free])
        cl, ll = c[cells], lam[cells]
        gc, gl = np.einsum('ma,mad->md', cl, grads), np.einsum('ma,mad->md', ll, grads)
        dD += -dt * np.bincount(lab, weights=vol * (gl * gc).sum(axis=1), minlength=L)
        lNc = np.einsum('ijk,mi,mj,mk->m', Tr, ll, cl, cl, optimize=True)
        lMc = np.einsum('ij,mi,mj->m', Mr, ll, cl)
        drho += -dt * np.bincount(lab, weights=vol * (lNc - lMc), minlength=L)
        lam_next = lam
    if not gradient:
        return out
    out.update(D=dD, rho=drho, gamma=dgam)
    der = lame_derivatives(o.E, o.nu)                                              # per cell
    for p in ("E", "nu"):
        mp, lp = der[p]
        gp = np.zeros(L)
        for t in range(L):
            m = (lab == t).astype(float)
            if not obs or not m.any():
                continue
            dK = assemble_elasticity(pts, prob.cells, mp * m, lp * m)
            dG = assemble_coupling(pts, prob.cells, mp * m, lp * m, o.gamma)
            gp[t] = sum(mu @ (dG @ c - dK @ u) for c, u, mu in obs)
        out[p] = gp
    return out


def J_at(prob, terms, n_steps, c0=None, **params):
    """(J, [cell arrays of the deformed terms]) at per-label parameter tables D, rho, gamma, E, nu and the start c0."""
    o = oracle_of(prob, **params)
    res = evaluate(prob, o, prob.trajectory(o, n_steps, c0=c0), terms, gradient=False)
    return res["J"], [i["cell"] for i in res["info"]]


def standard_terms(prob, n_steps, seed=0, masked=False):
    """The term list of the gradient tests (the GPU test's case 1): a deformed img_thresh GRID term at the last step with NaN
    targets, zero and non-unit pweights and voxels overhanging the mesh; a deformed img_l2 POINT-SET term midway with scale =
    0.5; a fixed image term; a u_l2 and a c_thresh term at the last step.  masked: the pweights of the two deformed terms
    carry the decisive mask at prob's own parameters (for central differences)."""
    import adjoint_image_common as aic
    rng = np.random.default_rng(seed)
    d, n = prob.dim, len(prob.points)
    # an irrational-looking origin and spacing: the grid aligns with no mesh line
    size = np.asarray([23, 21] if d == 2 else [15, 14, 13])
    origin, spacing = sc.overhanging_grid(prob.points, size, overhang=0.04)
    xg = sc.grid_points(origin, spacing, size)
    n_pts = 180
    xp = 0.5 + 0.47 * rng.uniform(-1.0, 1.0, (n_pts, d))
    ng = len(xg)
    tg = rng.uniform(0, 1, ng)
    tg[rng.random(ng) < 0.1] = np.nan
    qg = rng.uniform(0.5, 2.0, ng)
    qg[rng.random(ng) < 0.05] = 0.0
    tp = rng.uniform(0, 0.6, n_pts)
    tp[rng.random(n_pts) < 0.1] = np.nan
    mid = max(1, n_steps // 2)
    grid_t = deformed_term(xg, n_steps, "img_thresh", tg, qg, level=0.25, smooth=0.1, weight=1.5, scale=1.0,
                           grid=(origin, spacing, size))
    pts_t = deformed_term(xp, mid, "img_l2", tp, None, weight=2.0, scale=0.5)
    terms = [grid_t, pts_t,
             aic.image_term(prob, xg, mid, "img_l2", rng.uniform(0, 0.6, ng), None, weight=0.7),
             dict(step=n_steps, kind="u_l2", weight=10.0, target=0.01 * rng.standard_normal(n * d)),
             dict(step=n_steps, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5, target=rng.uniform(0, 1, n))]
    if masked:
        o = oracle_of(prob)
        traj = prob.trajectory(o, n_steps)
        for t in (grid_t, pts_t):
            loc = locate_term(prob, t, o.mech_solve(traj[t["step"]]))
            q = decisive_mask(loc)
            t["pweight"] = q if t["pweight"] is None else t["pweight"] * q
    return terms
