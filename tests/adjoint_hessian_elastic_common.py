"""
Numpy statement of the exact Hessian-vector products in the per-label Young's modulus and Poisson ratio (DESIGN.md section 13,
"Second order in E and nu"): the CPU reference of glims_adjoint_hessian_full.  It restates the sweep of
tests/adjoint_hessian_common.hessian with directions dm = (dD, drho, dgamma, dE, dnu [labels], dc0):

    K du_k = G dc_k + dG c_k - dK u_k,     K dmu_k = w M_vec du_k - dK mu_k,     dg_k += G^T dmu_k + dG^T mu_k,
    (H dm)_{p_t} = sum_k dmu_k^T (d_p G c_k - d_p K u_k) + mu_k^T (d_p G dc_k - d_p K du_k) + mu_k^T (d(d_p G) c_k - d(d_p K) u_k)

for p = E_t, nu_t.  d_p K, d_p G and their changes along the direction are ASSEMBLED by the oracle's assemble_elasticity /
assemble_coupling from label-masked Lame derivatives (as tests/adjoint_elastic_common.py does for first order): independent of
the per-cell sums (A_t, B_t, C_t) that the device combines.
"""
import copy

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adjoint_common import adjoint, dthresh, thresh
from adjoint_elastic_common import elastic_adjoint, lame_derivatives
from adjoint_hessian_common import _Cells, _direction, d2thresh, gradient_at
from oracle.glims_oracle import assemble_coupling, assemble_elasticity, compute_lambda, compute_mu

KEYS = ("D", "rho", "gamma", "E", "nu")


def lame_second_derivatives(E, nu):
    """{'EE', 'Enu', 'nunu'}: (m'', l'') of the Lame pair m = E / (2 (1 + nu)), l = E nu / q, q = (1 + nu)(1 - 2 nu)."""
    E, nu = np.asarray(E, float), np.asarray(nu, float)
    q = (1.0 + nu) * (1.0 - 2.0 * nu)
    z = np.zeros_like(E * nu)
    return {"EE": (z, z),
            "Enu": (-1.0 / (2.0 * (1.0 + nu) ** 2) + z, (1.0 + 2.0 * nu * nu) / (q * q) + z),
            "nunu": (E / (1.0 + nu) ** 3, 2.0 * E * (1.0 + 6.0 * nu + 4.0 * nu ** 3) / q ** 3)}


def _label_dir(prob, d, key):
    L = prob.n_labels
    return np.broadcast_to(np.asarray(d[key], dtype=np.float64), (L,)).copy() if d.get(key) is not None else np.zeros(L)


def hessian_full(prob, o, traj, terms, directions):
    """(J, g, hv): g = {'D', 'rho', 'gamma', 'E', 'nu' [labels], 'c0'} the numpy adjoint's gradient, hv one dict of the same
    keys per direction (a dict {'D', 'rho', 'gamma', 'E', 'nu' [labels or scalar], 'c0' [nodes]}, missing keys 0)."""
    lab, d, L = prob.labels, prob.dim, prob.n_labels
    pts, cells_ = prob.points, prob.cells
    geo = _Cells(prob)
    cells, n = geo.cells, geo.n
    N, dt = len(traj) - 1, prob.dt
    M = o.M
    Mvec = sp.kron(M, sp.eye(d)).tocsr()
    free = o._free_mask_c()
    rho = prob.rho[lab]
    dirs = [_direction(prob, dd) for dd in directions]
    dEs = [_label_dir(prob, dd, "E") for dd in directions]
    dnus = [_label_dir(prob, dd, "nu") for dd in directions]
    P = len(dirs)
    any_u = any(t["kind"] == "u_l2" for t in terms)
    J, dD, drho, dgam, dc0 = adjoint(prob, o, traj, terms)
    gE, gnu = elastic_adjoint(prob, o, traj, terms)
    g = dict(D=dD, rho=drho, gamma=dgam, E=gE, nu=gnu, c0=dc0)
    if any_u:
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
        # d_p K, d_p G per label (direction-independent), and G_t per unit coefficient with the direction's Lame change
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
                # the gamma row's extra term: d/dgamma_t of the E / nu part of dG
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
        A = o.rd_jacobian(c)
        lu = spla.splu(A[free][:, free].tocsc())

        def solve(b):
            x = np.zeros(n)
            x[free] = lu.solve(b[free])
            return x
        return solve

    # tangent-linear sweep (the concentration does not depend on E or nu)
    dc = [[dirs[p][3].copy()] for p in range(P)]
    for k in range(1, N + 1):
        c = traj[k]
        solve = rd_solver(c)
        for p in range(P):
            D_p, r_p = dirs[p][0][lab], dirs[p][1][lab]
            src = -dt * geo.scatter(D_p[:, None] * geo.K(c) + r_p[:, None] * (geo.T(c, c) - geo.Mv(c)))
            dc[p].append(solve(M @ dc[p][k - 1] + src))
    hv = [dict(D=np.zeros(L), rho=np.zeros(L), gamma=np.zeros(L), E=np.zeros(L), nu=np.zeros(L), c0=None) for _ in range(P)]
    lam_next = np.zeros(n)
    nu_next = [np.zeros(n) for _ in range(P)]
    for k in range(N, -1, -1):
        c = traj[k]
        gk = np.zeros(n)
        dg = [np.zeros(n) for _ in range(P)]
        gu = np.zeros(n * d)
        wu = 0.0
        for t in terms:
            if t["step"] != k:
                continue
            w = t["weight"]
            if t["kind"] == "u_l2":
                gu += w * (Mvec @ (o.mech_solve(c) - np.ravel(t["target"])))
                wu += w
                continue
            if t["kind"] == "c_thresh":
                lv, s = t["level"], t["smooth"]
                h, hp, h2 = thresh(c, lv, s), dthresh(c, lv, s), d2thresh(c, lv, s)
            else:
                h, hp, h2 = c, np.ones(n), np.zeros(n)
            Me = M @ (h - t["target"])
            gk += w * hp * Me
            for p in range(P):
                dg[p] += w * (hp * (M @ (hp * dc[p][k])) + h2 * Me * dc[p][k])
        if wu:
            u = o.mech_solve(c)                # with its Dirichlet values
            mu = solve_u(gu)
            gk += G.T @ mu
            Sc = c[cells].sum(axis=1)
            for p in range(P):
                dcp = dc[p][k]
                du = solve_u(G @ dcp + dG[p] @ c - dK[p] @ u)
                dmu = solve_u(wu * (Mvec @ du) - dK[p] @ mu)
                dg[p] += G.T @ dmu + dG[p].T @ mu
                hv[p]["gamma"] += np.bincount(lab, cG * div(dmu) * Sc, minlength=L) + \
                    np.bincount(lab, cG * div(mu) * dcp[cells].sum(axis=1), minlength=L)
                for t in present:
                    hv[p]["gamma"][t] += mu @ (dGg[p][t] @ c)
                    for key in ("E", "nu"):
                        hv[p][key][t] += dmu @ (dG1[key, t] @ c - dK1[key, t] @ u) + \
                            mu @ (dG1[key, t] @ dcp - dK1[key, t] @ du) + mu @ (dG2[p][key, t] @ c - dK2[p][key, t] @ u)
        if k == 0:
            for p in range(P):
                hv[p]["c0"] = M @ nu_next[p] + dg[p]
            break
        solve = rd_solver(c)
        lam = solve(gk + M @ lam_next)
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


def with_elastic(prob, E=None, nu=None):
    """A copy of the problem with its per-label E / nu tables replaced."""
    p2 = copy.copy(prob)
    if E is not None:
        p2.E = np.array(E, dtype=np.float64)
    if nu is not None:
        p2.nu = np.array(nu, dtype=np.float64)
    return p2


def full_gradient_at(prob, m, n_steps, terms):
    """The numpy adjoint's (J, flat gradient [D, rho, gamma, E, nu, c0]) at m = dict(D, rho, gamma, E, nu, c0):
    adjoint_hessian_common.gradient_at for the first three and c0, adjoint_elastic_common.elastic_adjoint for E and nu."""
    p2 = with_elastic(prob, m["E"], m["nu"])
    J, g = gradient_at(p2, m, n_steps, terms)
    L = prob.n_labels
    o = p2.oracle(D=m["D"], rho=m["rho"], gamma=m["gamma"])
    p3 = copy.copy(p2)
    p3.D, p3.rho, p3.gamma = (np.array(m[k], dtype=np.float64) for k in ("D", "rho", "gamma"))
    traj = p3.trajectory(o, n_steps, c0=m["c0"])
    gE, gnu = elastic_adjoint(p3, o, traj, terms)
    return J, np.concatenate([g[:3 * L], gE, gnu, g[3 * L:]])


def flat_full(prob, d):
    """[D, rho, gamma, E, nu, c0] of a direction or a product (missing keys 0)."""
    D, rho, gam, c0 = _direction(prob, d)
    return np.concatenate([D, rho, gam, _label_dir(prob, d, "E"), _label_dir(prob, d, "nu"), c0])


def unit_directions(prob, keys=KEYS, labels=None):
    """One direction per (key, label): the unit vectors of the per-label block of the Hessian."""
    L = prob.n_labels
    out = []
    for key in keys:
        for l in (range(L) if labels is None else labels):
            e = np.zeros(L)
            e[l] = 1.0
            out.append({key: e})
    return out
