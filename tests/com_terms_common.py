"""
Numpy statement of the centre-of-mass misfit terms (include/glims_hip.h, "CENTRE-OF-MASS terms") -- the CPU
reference of glims_adjoint_observable_terms3, independent of csrc/observe_grad.h.  A term that observes step k with the query
(observable, level, smooth), a label mask and the positions p = X, or p = y = X + scale u_k when deformed:

    V = sum_T V_T,  M = sum_T M_T  (observe_common.observe_mesh, summed over the counted labels),  X = M / V,
    J = 1/2 w |X - target|^2,   alpha = w (X - target) / V,   phi(x) = alpha . (x - X)   (a linear function of the position)

With alpha and X frozen J's first variation is that of the phi-weighted measure  F = sum_T int_T q(c_h) phi dx:
  mass    dF_T/dc_i = T int lam_i phi = T (sum_m phi_m + phi_i) / ((d+1)(d+2)),   phi_m = phi(p_m)
  smooth  dF_T/dc_i = T sum_q w_q h'(v_q) lam_qi phi(x_q)                          (the rule observe_common integrates with)
  sharp   dF_T/dc_i = int_Gamma lam_i phi dS / |grad c_h|:  Gamma = the level set inside the cell, a flat segment (2-D), triangle
          or quadrilateral (3-D) whose corners are the EXPLICIT cut points of the edges (as observable_terms_common
          .sharp_cell_grad); lam_i phi is quadratic on a flat piece: Simpson's rule on a segment and the edge-midpoint rule on a
          triangle integrate it exactly.  Lengths, areas and grad c_h are taken from the vertex positions.
T = |vol(X)| in the reference configuration and sigma vol(y) in the deformed one (a folded cell counts negatively).
  dF/du_n = scale sum_{T, n = vertex m of T} sigma_T (B_T cof_m(y_T) + vol(y_T) b_{1+m,T} alpha),  B_T = int_T q phi dx / vol(y_T)
          = alpha . (M_T - X V_T) / vol(y_T), with V_T, M_T from observe_common.observe_cell at y, the cofactors of
          deformed_volume_common and b_{1+m} = the first moments observe_cell gives on the UNIT simplex (p_0 = 0, p_k = e_k).
If V is not > 0 the term is EMPTY: J = 0 and no gradient at that evaluation.

evaluate() is deformed_volume_common.evaluate's recursion (which has no hook for a new kind) with the kind 'obs_com' added: per
step the nodal terms, the deformed image terms, then the volume and centre-of-mass terms in list order.
tests/test_com_terms_cpu.py checks it by central differences of its own J.

A centre-of-mass term is the dict the backend takes: observable_terms_common.volume_term's keys with kind='obs_com' and
target = [x, y(, z)], plus deformed=True and scale for the deformed configuration.
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import adjoint_deformed_common as adc
import deformed_common as dc
import deformed_volume_common as dvc
import observable_terms_common as otc
import observe_common as oc
import sampler_common as sc
from adjoint_elastic_common import lame_derivatives
from oracle.glims_oracle import (assemble_coupling, assemble_elasticity, compute_lambda, compute_mu, p1_geometry,
                                 reference_mass, reference_triple)

KIND = "obs_com"
VOLUME = otc.KIND
rel = dvc.rel


def com_term(step, observable, target, level=0.0, smooth=1.0, weight=1.0, labels=None, deformed=False, scale=1.0):
    t = otc.volume_term(step, observable, 0.0, level=level, smooth=smooth, weight=weight, labels=labels)
    t.update(kind=KIND, target=np.asarray(target, dtype=np.float64).reshape(-1).copy())
    if deformed:
        t.update(deformed=True, scale=float(scale))
    return t


def is_deformed(t):
    return t["kind"] in (KIND, VOLUME) and bool(t.get("deformed"))


def moments(prob, t, c, u=None):
    """(V, M [d]) of a term at (c, u): observe_mesh over the counted labels, in the term's configuration"""
    kw = dict(u=np.reshape(u, prob.points.shape), scale=t["scale"]) if t.get("deformed") else {}
    tab, _, _ = oc.observe_mesh(prob.points, prob.cells, prob.labels, c, [(t["observable"], t["level"], t["smooth"])],
                                prob.n_labels, **kw)
    mask = np.ones(prob.n_labels, dtype=bool) if t.get("labels") is None else np.asarray(t["labels"], dtype=bool)
    tot = sum(tab[0, l] for l in range(prob.n_labels) if mask[l])
    return float(tot[0]), np.asarray(tot[1:], dtype=np.float64)


def com_of(prob, t, c, u=None):
    """(J, X, V, alpha, empty) of a term"""
    V, M = moments(prob, t, c, u)
    d = prob.dim
    if not V > 0.0:
        return 0.0, np.full(d, np.nan), V, np.zeros(d), True
    X = M / V
    r = X - t["target"]
    return 0.5 * t["weight"] * float(r @ r), X, V, t["weight"] * r / V, False


def unit_moments(c, kind, level, smooth):
    """b[0 .. d+1] of one cell from observe_common.observe_cell on the unit simplex p_0 = 0, p_k = e_k (volume 1 / d!)"""
    nv = len(c)
    d = nv - 1
    p = np.vstack([np.zeros(d), np.eye(d)])
    out = oc.observe_cell(p, c, kind, level, smooth) * math.factorial(d)
    return np.concatenate([[out[0], out[0] - out[1:].sum()], out[1:]])


def sharp_cell_weighted_grad(p, c, level, phi):
    """dF_T/dc_i of one simplex for q = H(c_h - level): the surface integral of lam_i phi over the level set (see the module
    docstring); p [d+1, d] positions, phi [d+1] the weight at the vertices"""
    p, c, phi = np.asarray(p, dtype=np.float64), np.asarray(c, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    nv, d = p.shape
    ins = [i for i in range(nv) if c[i] >= level]
    outs = [i for i in range(nv) if not c[i] >= level]
    if not ins or not outs:
        return np.zeros(nv)
    grad = np.linalg.solve(p[1:] - p[0], c[1:] - c[0])

    def cut(a, b):                       # barycentric coordinates of the cut point on the edge a (in) -> b (out)
        t = (c[a] - level) / (c[a] - c[b])
        lam = np.zeros(nv)
        lam[a], lam[b] = 1.0 - t, t
        return lam

    if len(ins) == 1:
        corners = [cut(ins[0], b) for b in outs]
    elif len(outs) == 1:
        corners = [cut(a, outs[0]) for a in ins]
    else:                                # 3-D, two in (a, b), two out (e, f): neighbours in this cycle share a face of the cell
        (a, b), (e, f) = ins, outs
        corners = [cut(a, e), cut(a, f), cut(b, f), cut(b, e)]
    lam = np.array(corners)
    x = lam @ p
    g = np.zeros(nv)
    if d == 2:
        mid = 0.5 * (lam[0] + lam[1])
        length = np.linalg.norm(x[1] - x[0])
        g += length / 6.0 * (lam[0] * (lam[0] @ phi) + 4.0 * mid * (mid @ phi) + lam[1] * (lam[1] @ phi))
    else:
        for tri in ([0, 1, 2], [0, 2, 3])[:len(corners) - 2]:
            area = 0.5 * np.linalg.norm(np.cross(x[tri[1]] - x[tri[0]], x[tri[2]] - x[tri[0]]))
            for i, j in ((0, 1), (1, 2), (2, 0)):
                mid = 0.5 * (lam[tri[i]] + lam[tri[j]])
                g += area / 3.0 * mid * (mid @ phi)
    return g / np.linalg.norm(grad)


def com_parts(prob, t, c, u, alpha, X):
    """(g [n_nodes] = dJ/dc_k, gu [n_nodes * d] = dJ/du_k (zeros for a reference term)) of a centre-of-mass term with alpha and
    X frozen.  MASS and SMOOTH for all cells at once, SHARP cell by cell over the cut cells."""
    pts = np.asarray(prob.points, dtype=np.float64)
    cells = np.asarray(prob.cells, dtype=np.int64)
    n, d = pts.shape
    nv = d + 1
    deformed = bool(t.get("deformed"))
    s = t["scale"] if deformed else 0.0
    y = pts + s * np.reshape(u, pts.shape) if deformed else pts
    on = otc.counted_cells(prob, t)
    vX, vY = dvc.signed_volumes(pts, cells), dvc.signed_volumes(y, cells)
    sigma = np.where(vX >= 0.0, 1.0, -1.0)
    T = sigma * vY if deformed else np.abs(vX)
    kind, level, smooth = t["observable"], t["level"], t["smooth"]
    cv = np.asarray(c, dtype=np.float64)[cells]
    P = y[cells]                                                               # [m, nv, d]
    phi = (P - X) @ alpha                                                      # [m, nv]
    gc, b1 = np.zeros((len(cells), nv)), np.zeros((len(cells), nv))
    if kind == "mass":
        b1[on] = ((cv.sum(axis=1)[:, None] + cv) / (nv * (nv + 1)))[on]
        gc[on] = (T[:, None] * (phi.sum(axis=1)[:, None] + phi) / (nv * (nv + 1)))[on]
    elif kind == "smooth":
        lam, w = oc._rule(d)
        v = cv @ lam.T
        b1[on] = ((w * 0.5 * (np.tanh((v - level) / smooth) + 1.0)) @ lam)[on]
        gc[on] = (T[:, None] * ((w * otc.dthresh(v, level, smooth) * (phi @ lam.T)) @ lam))[on]
    else:
        n_in = (cv >= level).sum(axis=1)
        b1[on & (n_in == nv)] = 1.0 / nv
        for e in np.nonzero(on & (n_in > 0) & (n_in < nv))[0]:
            b1[e] = unit_moments(cv[e], kind, level, smooth)[1:]
            gc[e] = np.sign(T[e]) * sharp_cell_weighted_grad(P[e], cv[e], level, phi[e])
    g = np.bincount(cells.ravel(), weights=gc.ravel(), minlength=n)
    gu = np.zeros((n, d))
    if deformed:
        B = (b1 * phi).sum(axis=1)
        load = s * ((sigma * B)[:, None, None] * dvc.cofactors_all(P) + (T[:, None] * b1)[:, :, None] * alpha[None, None, :])
        for k in range(d):
            gu[:, k] = np.bincount(cells.ravel(), weights=load[:, :, k].ravel(), minlength=n)
    return g, gu.reshape(-1)


def fast_moments(prob, t, c, u=None):
    """moments() of a MASS or SMOOTH term without the Python loop over the cells (the fit's statement; the CPU test holds it
    against moments())"""
    assert t["observable"] in ("mass", "smooth")
    pts = np.asarray(prob.points, dtype=np.float64)
    cells = np.asarray(prob.cells, dtype=np.int64)
    d = pts.shape[1]
    nv = d + 1
    deformed = bool(t.get("deformed"))
    y = pts + t["scale"] * np.reshape(u, pts.shape) if deformed else pts
    on = otc.counted_cells(prob, t)
    vX = dvc.signed_volumes(pts, cells)
    T = np.where(vX >= 0.0, 1.0, -1.0) * dvc.signed_volumes(y, cells) if deformed else np.abs(vX)
    cv = np.asarray(c, dtype=np.float64)[cells]
    if t["observable"] == "mass":
        b1 = (cv.sum(axis=1)[:, None] + cv) / (nv * (nv + 1))
    else:
        lam, w = oc._rule(d)
        b1 = (w * 0.5 * (np.tanh((cv @ lam.T - t["level"]) / t["smooth"]) + 1.0)) @ lam
    Tb = (T[:, None] * b1)[on]
    return float(Tb.sum()), np.einsum('ma,mad->d', Tb, y[cells][on])


def needs_u(t):
    return t["kind"] == "u_l2" or adc.is_deformed(t) or is_deformed(t)


def evaluate(prob, o, traj, terms, gradient=True, fast=False):
    """dict J and, with `gradient`, D, rho, gamma, E, nu [labels] and c0; `info`: per volume / centre-of-mass term (list order)
    a dict with V and, for a centre-of-mass term, com, empty and J."""
    pts, lab, d = prob.points, prob.labels, prob.dim
    cells = np.asarray(prob.cells, dtype=np.int64)
    L, n, N, dt, M = prob.n_labels, len(pts), len(traj) - 1, prob.dt, o.M
    Mv = sp.kron(M, sp.eye(d)).tocsr()
    obs_terms = [t for t in terms if t["kind"] in (KIND, VOLUME)]
    slot = {id(t): i for i, t in enumerate(obs_terms)}
    out = dict(J=0.0, info=[None] * len(obs_terms), mech_steps=0)
    assert all(t["kind"] in ("c_l2", "c_thresh", "u_l2", KIND, VOLUME) or adc.is_deformed(t) for t in terms)
    mech = any(needs_u(t) for t in terms)
    if mech:
        Kel, G = o._mech_setup()
        free_u = np.ones(n * d, bool)
        if prob.dir_u is not None:
            free_u[np.asarray(prob.dir_u[0], dtype=np.int64)] = False
        Kff = spla.splu(Kel[free_u][:, free_u].tocsc()) if gradient else None
    if gradient:
        vol, grads = p1_geometry(pts, cells)
        Mr, Tr = reference_mass(d), reference_triple(d)
        free = o._free_mask_c()
        geo = otc._Cells(prob)
        if mech:
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
        out["mech_steps"] += int(have_u)
        for t in [t for t in here if t["kind"] in ("c_l2", "c_thresh", "u_l2")]:
            if t["kind"] == "u_l2":
                e = u - np.ravel(t["target"])
                out["J"] += 0.5 * t["weight"] * e @ (Mv @ e)
                gu += t["weight"] * (Mv @ e)
            else:
                hv, hp = adc._h(t, c)
                Me = M @ (hv - t["target"])
                out["J"] += 0.5 * t["weight"] * (hv - t["target"]) @ Me
                g += t["weight"] * hp * Me
        for t in [t for t in here if adc.is_deformed(t)]:
            s = t["scale"]
            y = dc.deformed_points(pts, u, s)
            cell, w, _, _ = sc.locate(y, prob.cells, t["x"])
            ok, q, e, hp = adc._point_parts(prob, t, c, cell, w)
            out["J"] += 0.5 * t["weight"] * np.sum(q[ok] * e[ok] ** 2)
            if not gradient:
                continue
            ratios = dc.cell_ratios(pts, prob.cells, np.reshape(u, pts.shape), s)
            r = np.zeros(len(cell))
            r[ok] = t["weight"] * q[ok] * hp[ok] * e[ok]
            g += sc.apply_t(prob.cells, cell, w, r, n)
            gcl = np.einsum('ma,mad->md', c[cells], p1_geometry(y, cells)[1])
            good = (ratios > 0) & np.isfinite(ratios)
            S = np.zeros((len(cell), d))
            use = ok & good[np.maximum(cell, 0)]
            S[use] = -s * r[use, None] * gcl[cell[use]]
            gu += sc.apply_t(prob.cells, cell, w, S, n).reshape(-1)
        for t in [t for t in here if t["kind"] in (KIND, VOLUME)]:
            if t["kind"] == KIND:
                if fast:
                    V, Mo = fast_moments(prob, t, c, u)
                    if V > 0.0:
                        X = Mo / V
                        r = X - t["target"]
                        Jt, alpha, empty = 0.5 * t["weight"] * float(r @ r), t["weight"] * r / V, False
                    else:
                        Jt, X, alpha, empty = 0.0, np.full(d, np.nan), np.zeros(d), True
                else:
                    Jt, X, V, alpha, empty = com_of(prob, t, c, u)
                out["J"] += Jt
                out["info"][slot[id(t)]] = dict(V=V, com=X, empty=empty, J=Jt)
                if gradient and not empty:
                    gv, guv = com_parts(prob, t, c, u, alpha, X)
                    g += gv
                    gu += guv
                continue
            V = dvc.measure(prob, t, c, u)
            res = V - t["target"]
            out["J"] += 0.5 * t["weight"] * res ** 2
            out["info"][slot[id(t)]] = dict(V=V)
            if not gradient:
                continue
            if dvc.is_deformed_volume(t):
                gv, guv, _ = dvc.deformed_parts(prob, t, c, u)
                g += t["weight"] * res * gv
                gu += t["weight"] * res * guv
            else:
                g += t["weight"] * res * otc.nodal_grad(prob, geo, t, c)[0]
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
        gcl, gl = np.einsum('ma,mad->md', cl, grads), np.einsum('ma,mad->md', ll, grads)
        dD += -dt * np.bincount(lab, weights=vol * (gl * gcl).sum(axis=1), minlength=L)
        lNc = np.einsum('ijk,mi,mj,mk->m', Tr, ll, cl, cl, optimize=True)
        lMc = np.einsum('ij,mi,mj->m', Mr, ll, cl)
        drho += -dt * np.bincount(lab, weights=vol * (lNc - lMc), minlength=L)
        lam_next = lam
    if not gradient:
        return out
    out.update(D=dD, rho=drho, gamma=dgam)
    for p in ("E", "nu"):
        gp = np.zeros(L)
        if obs:
            mp, lp = lame_derivatives(o.E, o.nu)[p]
            for t in range(L):
                m = (lab == t).astype(float)
                if not m.any():
                    continue
                dK = assemble_elasticity(pts, prob.cells, mp * m, lp * m)
                dG = assemble_coupling(pts, prob.cells, mp * m, lp * m, o.gamma)
                gp[t] = sum(mu @ (dG @ c - dK @ u) for c, u, mu in obs)
        out[p] = gp
    return out


def J_of_lists(prob, lists, n_steps, c0=None, **params):
    """J of every term list of `lists` on ONE trajectory at the per-label tables D, rho, gamma, E, nu and the start c0"""
    o = dvc.oracle_of(prob, **params)
    traj = prob.trajectory(o, n_steps, c0=c0)
    return np.array([evaluate(prob, o, traj, terms, gradient=False)["J"] for terms in lists])


def diameter(prob):
    pts = np.asarray(prob.points)
    return float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))


def standard_terms(prob, traj, u_of=None, seed=0, deformed=False):
    """The mixed list of the gradient tests, on an N-step trajectory: on the last step a SMOOTH centre-of-mass term over the
    whole domain, a MASS one on label 1 and a volume term and a nodal c_thresh term; a SHARP centre-of-mass term at a gap_level
    on the middle step (scale 0.5 when deformed); a MASS centre-of-mass term over the whole domain at the last step.
    deformed: the centre-of-mass terms and the volume term measure X + scale u (u_of(c): the displacement of a state).
    Targets: the centre of mass itself displaced by 0.03 .. 0.06 of the domain's diameter in a random direction, so that
    |X - target| >= 1e-2 diameter and no bar is met by cancellation."""
    rng = np.random.default_rng(seed)
    N, L = len(traj) - 1, prob.n_labels
    only1 = np.zeros(L, dtype=np.uint8)
    only1[1] = 1
    mid = max(1, N // 2)
    lv, dist = otc.gap_level(traj[mid])
    assert dist >= 1e-2, dist
    diam = diameter(prob)
    specs = [(N, "smooth", 0.3, 0.08, None, 2.0, 1.0), (mid, "sharp", lv, 1.0, None, 1.2, 0.5),
             (N, "mass", 0.0, 1.0, only1, 0.7, 1.0), (N, "mass", 0.0, 1.0, None, 1.5, 1.0)]
    terms = []
    for step, kind, level, smooth, lab, weight, scale in specs:
        t = com_term(step, kind, np.zeros(prob.dim), level=level, smooth=smooth, weight=weight, labels=lab, deformed=deformed,
                     scale=scale)
        _, X, V, _, empty = com_of(prob, t, traj[step], u_of(traj[step]) if deformed else None)
        assert not empty and V > 0
        e = rng.standard_normal(prob.dim)
        t["target"] = X + rng.uniform(0.03, 0.06) * diam * e / np.linalg.norm(e)
        terms.append(t)
    v = dvc.volume_term(N, "smooth", 0.0, level=0.25, smooth=0.1, weight=0.9, deformed=deformed, scale=1.0)
    v["target"] = float(rng.uniform(0.5, 0.9) * dvc.measure(prob, v, traj[N], u_of(traj[N]) if deformed else None))
    terms.insert(3, v)
    terms.append(dict(step=N, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5, target=rng.uniform(0, 1, len(prob.points))))
    return terms


# ---- the (x0, y0, D, rho) fit: one setting for the numpy fit (CPU test) and the public-API fit (GPU test), the one of
# examples/adjoint_fit_seed_2D.py at test size ---------------------------------------------------------------------------------
# Mesh, model and rate bounds of adjoint_image_common.FIT ([-5, 5]^2, 24 x 24, two tissues with one D and one rho); the seed
# exp(-a |x - x_seed|^2) with the seed position as two further controls.  The data, at five steps of a truth run: the T2- /
# T1-like SMOOTH volumes and centres of mass of the whole domain.  The centre of mass moves by tenths while the volumes change
# by tens: com_weight makes both kinds of datum count.
FIT = dict(lo=-5.0, hi=5.0, n=24, steps=10, dt=1.0, a=0.5, truth=(0.8, 0.4, 0.1, 0.1), start=(0.2, -0.3, 0.05, 0.2),
           levels=(0.2, 0.4), smooth=0.1, obs_steps=(2, 4, 6, 8, 10), com_weight=100.0,
           lo_bounds=(-2.0, -2.0, 0.005, 0.005), hi_bounds=(2.0, 2.0, 0.5, 0.5),
           options={"maxiter": 60, "gtol": 1e-14, "ftol": 1e-18}, tol=1e-18,
           bar=1e-11)     # (the recovery of the numpy twin rounded up to the next power of ten: tests/test_com_terms_cpu.py)


def fit_c0(points, x0, y0):
    x = np.asarray(points, dtype=np.float64)
    return np.exp(-FIT["a"] * ((x[:, 0] - x0) ** 2 + (x[:, 1] - y0) ** 2))


def fit_problem(points, cells, m):
    """The fit's model on the given mesh at m = (x0, y0, D, rho): adjoint_image_common.fit_problem with the seed at (x0, y0)"""
    from adjoint_common import Problem
    x0, y0, D, rho = m
    x = np.asarray(points, dtype=np.float64)
    lab = np.where(x[np.asarray(cells)].mean(axis=1)[:, 0] >= 0.0, 1, 2).astype(np.int32)
    one = np.ones(3)
    return Problem.from_mesh(x, cells, lab, D * one, rho * one, 0.1 * one, 0.001 * one, 0.4 * one, fit_c0(x, x0, y0),
                             dt=FIT["dt"])


def fit_terms(make_volume, make_com):
    """The fit's term list in its fixed order; make_volume(step, level) / make_com(step, level) build one term each (the caller
    fills in the targets)."""
    out = []
    for k in FIT["obs_steps"]:
        for lv in FIT["levels"]:
            out.append(make_volume(k, lv))
            out.append(make_com(k, lv))
    return out
