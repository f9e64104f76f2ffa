"""
Numpy statement of the volume misfit terms (include/glims_hip.h, "volume misfit terms") -- the CPU reference
of glims_adjoint_observable_terms, independent of csrc/observe_grad.h.

    J_obs = 1/2 w (V - target)^2,   V = sum over the cells of the counted labels of V_T(c_k)

V comes from the cell loop of tests/observe_common.py.  Its derivative by the vertex values is stated WITHOUT the edge-parameter
products of the header:

  mass    dV_T/dc_i = |T| / (d+1)
  smooth  dV_T/dc_i = |T| sum_q w_q h'(v_q) lam_qi,  d2V_T/dc_i dc_j = |T| sum_q w_q h''(v_q) lam_qi lam_qj  with the rule
          simplex_quadrature(d, 4) of the package (what observe_common integrates with)
  sharp   V_T = int_T H(c_h - level) dx, so dV_T/dc_i = int_T delta(c_h - level) lam_i dx = int_Gamma lam_i dS / |grad c_h|:
          Gamma = the level set inside the cell, a flat segment (2-D), triangle or quadrilateral (3-D) whose corners are the cut
          points of the edges; lam_i is linear, so each flat piece contributes its measure times lam_i at its centroid.  Lengths
          and areas are taken from the vertex POSITIONS, grad c_h from the P1 geometry.

adjoint_common's and adjoint_image_common's recursions have no hook for a new kind, so this file carries a first- and
second-order recursion of its own for the kinds 'c_l2', 'c_thresh' and 'obs_volume' (per step: the nodal terms in list order,
then the volume terms in list order -- the order of the device sweep).  tests/test_observable_terms_cpu.py checks it by central
differences.

A volume term is the dict the backend takes: {step, kind='obs_volume', observable ('mass' | 'sharp' | 'smooth'), level, smooth,
target, weight, labels (a mask [n_labels] or None = every label)}.
"""
import numpy as np
import scipy.sparse.linalg as spla

import observe_common as oc
from adjoint_common import dthresh, thresh
from adjoint_hessian_common import _Cells, _direction, d2thresh

KIND = "obs_volume"


def volume_term(step, observable, target, level=0.0, smooth=1.0, weight=1.0, labels=None):
    return dict(step=int(step), kind=KIND, observable=observable, level=float(level), smooth=float(smooth),
                target=float(target), weight=float(weight),
                labels=None if labels is None else np.asarray(labels, dtype=np.uint8))


def counted_cells(prob, t):
    """bool [n_cells]: the cells the term counts"""
    if t.get("labels") is None:
        return np.ones(len(prob.cells), dtype=bool)
    return np.asarray(t["labels"], dtype=bool)[np.asarray(prob.labels)]


# ---- one cell ------------------------------------------------------------------------------------------------------------------
def sharp_cell_grad(p, c, level):
    """dV_T/dc_i of one simplex as the surface integral over the level set (see the module docstring)"""
    p, c = np.asarray(p, dtype=np.float64), np.asarray(c, dtype=np.float64)
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
        g += np.linalg.norm(x[1] - x[0]) * lam.mean(axis=0)
    else:
        for tri in ([0, 1, 2], [0, 2, 3])[:len(corners) - 2]:
            area = 0.5 * np.linalg.norm(np.cross(x[tri[1]] - x[tri[0]], x[tri[2]] - x[tri[0]]))
            g += area * lam[tri].mean(axis=0)
    return g / np.linalg.norm(grad)


def cell_grad(p, c, kind, level=0.0, smooth=1.0, dc=None):
    """(dV_T/dc [d+1], H_T dc [d+1] or None) of one simplex with positions p and the volume |T| of p"""
    p, c = np.asarray(p, dtype=np.float64), np.asarray(c, dtype=np.float64)
    nv, d = p.shape
    T = abs(oc._vol(p.tolist()))
    Hd = None if dc is None else np.zeros(nv)
    if kind == "mass":
        return np.full(nv, T / nv), Hd
    if kind == "sharp":
        return sharp_cell_grad(p, c, level), None
    lam, w = oc._rule(d)
    v = lam @ c
    g = T * (w * dthresh(v, level, smooth)) @ lam
    if dc is not None:
        Hd = T * (w * d2thresh(v, level, smooth) * (lam @ np.asarray(dc, dtype=np.float64))) @ lam
    return g, Hd


# ---- the mesh ------------------------------------------------------------------------------------------------------------------
def measure(prob, t, c):
    """V of a term at the nodal field c: the loop of observe_common over the counted labels, added in label order"""
    tab, _, _ = oc.observe_mesh(prob.points, prob.cells, prob.labels, c, [(t["observable"], t["level"], t["smooth"])],
                                prob.n_labels)
    mask = np.ones(prob.n_labels, dtype=bool) if t.get("labels") is None else np.asarray(t["labels"], dtype=bool)
    return float(sum(tab[0, l, 0] for l in range(prob.n_labels) if mask[l]))


def in_counts(prob, t, c):
    """in-count of every cell for the term's level"""
    return (np.asarray(c)[np.asarray(prob.cells)] >= t["level"]).sum(axis=1)


def cut_cells(prob, t, c):
    """the counted cells the level set cuts (a SHARP term's glims_adjoint_observable_info figure)"""
    n = in_counts(prob, t, c)
    return int(((n > 0) & (n < prob.dim + 1) & counted_cells(prob, t)).sum())


def nodal_grad(prob, geo, t, c, dc=None):
    """(g [n_nodes] = dV/dc, H dc [n_nodes] or None)"""
    cells = geo.cells
    on = counted_cells(prob, t)
    kind = t["observable"]
    nv = prob.dim + 1
    vol = np.abs(geo.vol)
    gc = np.zeros((len(cells), nv))
    Hc = None if dc is None else np.zeros((len(cells), nv))
    if kind == "mass":
        gc[on] = (vol[on] / nv)[:, None]
    elif kind == "smooth":
        lam, w = oc._rule(prob.dim)
        v = c[cells] @ lam.T                                             # [m, nq]
        gc[on] = (vol[:, None] * ((w * dthresh(v, t["level"], t["smooth"])) @ lam))[on]
        if dc is not None:
            dv = dc[cells] @ lam.T
            Hc[on] = (vol[:, None] * ((w * d2thresh(v, t["level"], t["smooth"]) * dv) @ lam))[on]
    else:
        assert dc is None, "no second order for a sharp volume term"
        n = in_counts(prob, t, c)
        for e in np.nonzero(on & (n > 0) & (n < nv))[0]:
            gc[e] = sharp_cell_grad(prob.points[cells[e]], c[cells[e]], t["level"])
    return geo.scatter(gc), (None if dc is None else geo.scatter(Hc))


def _h(t, v):
    if t["kind"] == "c_thresh":
        lv, s = t["level"], t["smooth"]
        return thresh(v, lv, s), dthresh(v, lv, s), d2thresh(v, lv, s)
    return v, np.ones_like(v), np.zeros_like(v)


def misfit(prob, o, traj, terms):
    J = 0.0
    for t in terms:
        c = traj[t["step"]]
        if t["kind"] == KIND:
            J += 0.5 * t["weight"] * (measure(prob, t, c) - t["target"]) ** 2
        else:
            e = _h(t, c)[0] - t["target"]
            J += 0.5 * t["weight"] * e @ (o.M @ e)
    return J


def hessian(prob, o, traj, terms, directions=()):
    """(J, dD, drho, dc0, hv): J and its gradient by the discrete adjoint and, per direction (a dict {'D', 'rho' [n_labels],
    'c0' [n_nodes]}, missing keys 0), the Hessian-vector product {'D', 'rho', 'c0'}."""
    assert all(t["kind"] in ("c_l2", "c_thresh", KIND) for t in terms)
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
        for t in [t for t in here if t["kind"] != KIND]:
            hc, hp, h2 = _h(t, c)
            Me = M @ (hc - t["target"])
            g += t["weight"] * hp * Me
            for p in range(P):
                dg[p] += t["weight"] * (hp * (M @ (hp * dc[p][k])) + h2 * Me * dc[p][k])
        for t in [t for t in here if t["kind"] == KIND]:
            r = measure(prob, t, c) - t["target"]
            gv, _ = nodal_grad(prob, geo, t, c)
            g += t["weight"] * r * gv
            for p in range(P):
                _, Hd = nodal_grad(prob, geo, t, c, dc[p][k])
                dg[p] += t["weight"] * (gv * (gv @ dc[p][k]) + r * Hd)
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


# ---- the level of a SHARP term: the gap rule -------------------------------------------------------------------------------
def gap_level(c):
    """The midpoint of the widest gap between sorted nodal values within [0.2, 0.8] max c, and the distance of the nearest
    nodal value from it (half that gap): with every value at least 1e-2 away, no perturbation of the tests changes a cell's
    in / out pattern."""
    c = np.asarray(c, dtype=np.float64)
    lo, hi = 0.2 * c.max(), 0.8 * c.max()
    v = np.sort(c[(c >= lo) & (c <= hi)])
    if len(v) < 2:
        # a mesh so coarse that the range holds fewer than two nodal values (the 64-node cube): the gaps of ALL sorted values,
        # clipped to the range
        s = np.sort(c)
        a, b = np.clip(s[:-1], lo, hi), np.clip(s[1:], lo, hi)
        k = int(np.argmax(b - a))
        level = 0.5 * (a[k] + b[k])
    else:
        k = int(np.argmax(np.diff(v)))
        level = 0.5 * (v[k] + v[k + 1])
    return level, float(np.abs(c - level).min())


def standard_terms(prob, traj, seed=0, empty_label=None):
    """The list of the gradient tests: on the last step a SHARP term over the whole domain, a SMOOTH term on label 1, a MASS
    term over the whole domain and a nodal c_thresh term; a SHARP term on label 1 at N/2; a MASS term at step 0; with
    empty_label (a label id that no cell carries) a SMOOTH term on that label at the last step.  SHARP levels by the gap rule;
    targets are a fraction of the measure itself, so that V - target is of the size of V."""
    rng = np.random.default_rng(seed)
    N = len(traj) - 1
    L = prob.n_labels
    only1 = np.zeros(L, dtype=np.uint8)
    only1[1] = 1
    lvN, distN = gap_level(traj[N])
    lvM, distM = gap_level(traj[N // 2])
    assert distN >= 1e-2 and distM >= 1e-2, (distN, distM)
    specs = [(N, "sharp", lvN, 1.0, None, 1.5), (N, "smooth", 0.3, 0.08, only1, 2.0), (N, "mass", 0.0, 1.0, None, 0.7),
             (N // 2, "sharp", lvM, 1.0, only1, 1.2), (0, "mass", 0.0, 1.0, only1, 0.9)]
    terms = []
    for step, kind, level, smooth, labels, weight in specs:
        t = volume_term(step, kind, 0.0, level=level, smooth=smooth, weight=weight, labels=labels)
        t["target"] = float(rng.uniform(0.5, 0.9) * measure(prob, t, traj[step]))
        terms.append(t)
    terms.insert(3, dict(step=N, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5,
                         target=rng.uniform(0, 1, len(prob.points))))
    if empty_label is not None:
        m = np.zeros(L, dtype=np.uint8)
        m[empty_label] = 1
        terms.append(volume_term(N, "smooth", 0.37, level=0.3, smooth=0.08, weight=1.3, labels=m))
    return terms


# ---- the (D, rho) fit to two SMOOTH volume series: one setting for the numpy fit (CPU test) and the public-API fit (GPU test) ----
# (mesh, model, start, bounds and optimiser options of adjoint_image_common.FIT; the data are the T2- and T1-like volumes of the
#  whole domain at these steps)
FIT_VOLUMES = dict(levels=(0.2, 0.4), smooth=0.1, steps=(2, 4, 6, 8, 10))
