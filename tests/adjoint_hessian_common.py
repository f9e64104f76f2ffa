"""
Numpy tangent-linear + second-order adjoint of the oracle's backward-Euler / Newton scheme ("Second
order"): Hessian-vector products of J, the CPU reference of glims_adjoint_hessian.  tests/test_adjoint_hessian_cpu.py checks it
by central differences of the numpy adjoint gradient of tests/adjoint_common.py, by symmetry and by a Taylor test.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adjoint_common import adjoint, dthresh, thresh
from oracle.glims_oracle import compute_lambda, compute_mu, p1_geometry, reference_mass, reference_triple


def d2thresh(c, level, smooth):
    t = np.tanh((c - level) / smooth)
    return -t * (1.0 - t * t) / smooth ** 2


class _Cells:
    """Per-cell P1 integrals, exact (the f3 / f2 factorial formulas of the device kernels)."""

    def __init__(self, prob):
        self.cells = np.asarray(prob.cells, dtype=np.int64)
        self.n = len(prob.points)
        self.vol, self.grads = p1_geometry(prob.points, self.cells)
        self.Mr, self.Tr = reference_mass(prob.dim), reference_triple(prob.dim)
        self.GG = np.einsum('mad,mbd->mab', self.grads, self.grads)

    def scatter(self, v):            # [M, nv] cell shares -> node vector
        return np.bincount(self.cells.ravel(), weights=v.ravel(), minlength=self.n)

    def K(self, x):                  # int_T grad x . grad phi_a
        return self.vol[:, None] * np.einsum('mab,mb->ma', self.GG, x[self.cells])

    def T(self, x, y):               # int_T x y phi_a
        return self.vol[:, None] * np.einsum('abk,mb,mk->ma', self.Tr, x[self.cells], y[self.cells], optimize=True)

    def Mv(self, x):                 # int_T x phi_a
        return self.vol[:, None] * np.einsum('ab,mb->ma', self.Mr, x[self.cells])

    def gg(self, x, y):              # int_T grad x . grad y
        return self.vol * np.einsum('mab,ma,mb->m', self.GG, x[self.cells], y[self.cells])

    def xyz(self, x, y, z):          # int_T x y z
        return self.vol * np.einsum('abk,ma,mb,mk->m', self.Tr, x[self.cells], y[self.cells], z[self.cells], optimize=True)

    def xy(self, x, y):              # int_T x y
        return self.vol * np.einsum('ab,ma,mb->m', self.Mr, x[self.cells], y[self.cells])


def _direction(prob, d):
    L, n = prob.n_labels, len(prob.points)
    get = lambda k, size: np.broadcast_to(np.asarray(d.get(k, 0.0), dtype=np.float64), (size,)).copy() \
        if d.get(k) is not None else np.zeros(size)
    return get("D", L), get("rho", L), get("gamma", L), get("c0", n)


def hessian(prob, o, traj, terms, directions):
    """(J, dD, drho, dgamma, dc0, hv): the numpy adjoint's J and gradient, and per direction (a dict {'D', 'rho', 'gamma'
    [n_labels], 'c0' [n_nodes]}, missing keys 0) the Hessian-vector product {'D', 'rho', 'gamma', 'c0'}."""
    lab, d, L = prob.labels, prob.dim, prob.n_labels
    geo = _Cells(prob)
    cells, n = geo.cells, geo.n
    N, dt = len(traj) - 1, prob.dt
    M = o.M
    Mvec = sp.kron(M, sp.eye(d)).tocsr()
    free = o._free_mask_c()
    rho = prob.rho[lab]
    dirs = [_direction(prob, dd) for dd in directions]
    P = len(dirs)
    any_u = any(t["kind"] == "u_l2" for t in terms)
    if any_u:
        Kel, G = o._mech_setup()
        free_u = np.ones(n * d, bool)
        if prob.dir_u is not None:
            free_u[np.asarray(prob.dir_u[0], dtype=np.int64)] = False
        Kff = spla.splu(Kel[free_u][:, free_u].tocsc())
        E, nu = prob.E[lab], prob.nu[lab]
        cG = (2.0 * compute_mu(E, nu) + d * compute_lambda(E, nu)) * geo.vol / (d + 1)   # G_T with gamma = 1

        def solve_u(b):
            x = np.zeros(n * d)
            x[free_u] = Kff.solve(b[free_u])
            return x

        def div(v):
            return np.einsum('mad,mad->m', v.reshape(n, d)[cells], geo.grads)

        def G_of(wcell, x):          # sum_t w_t G_t x
            out = np.zeros((n, d))
            np.add.at(out, cells, (wcell * cG * x[cells].sum(axis=1))[:, None, None] * geo.grads)
            return out.ravel()

        def GT_of(wcell, v):         # sum_t w_t G_t^T v
            return geo.scatter(np.repeat((wcell * cG * div(v))[:, None], d + 1, axis=1))

    def rd_solver(c):
        A = o.rd_jacobian(c)
        lu = spla.splu(A[free][:, free].tocsc())

        def solve(b):
            x = np.zeros(n)
            x[free] = lu.solve(b[free])
            return x
        return solve

    J, dD, drho, dgam, dc0 = adjoint(prob, o, traj, terms)
    # tangent-linear sweep
    dc = [[dirs[p][3].copy()] for p in range(P)]
    for k in range(1, N + 1):
        c = traj[k]
        solve = rd_solver(c)
        for p in range(P):
            D_p, r_p = dirs[p][0][lab], dirs[p][1][lab]
            src = -dt * geo.scatter(D_p[:, None] * geo.K(c) + r_p[:, None] * (geo.T(c, c) - geo.Mv(c)))
            dc[p].append(solve(M @ dc[p][k - 1] + src))
    # second-order adjoint sweep
    hv = [dict(D=np.zeros(L), rho=np.zeros(L), gamma=np.zeros(L), c0=None) for _ in range(P)]
    lam_next = np.zeros(n)
    nu_next = [np.zeros(n) for _ in range(P)]
    for k in range(N, -1, -1):
        c = traj[k]
        g = np.zeros(n)
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
            g += w * hp * Me
            for p in range(P):
                dg[p] += w * (hp * (M @ (hp * dc[p][k])) + h2 * Me * dc[p][k])
        if wu:
            mu = solve_u(gu)
            g += G.T @ mu
            Sc = c[cells].sum(axis=1)
            for p in range(P):
                dgam_c = dirs[p][2][lab]
                du = solve_u(G @ dc[p][k] + G_of(dgam_c, c))
                dmu = solve_u(wu * (Mvec @ du))
                dg[p] += G.T @ dmu + GT_of(dgam_c, mu)
                hv[p]["gamma"] += np.bincount(lab, cG * div(dmu) * Sc, minlength=L) + \
                    np.bincount(lab, cG * div(mu) * dc[p][k][cells].sum(axis=1), minlength=L)
        if k == 0:
            for p in range(P):
                hv[p]["c0"] = M @ nu_next[p] + dg[p]
            break
        solve = rd_solver(c)
        lam = solve(g + M @ lam_next)
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
    return J, dD, drho, dgam, dc0, hv


def gradient_at(prob, m, n_steps, terms):
    """The numpy adjoint's (J, flat gradient [D, rho, gamma, c0]) at m = dict(D, rho, gamma, c0)."""
    o = prob.oracle(D=m["D"], rho=m["rho"], gamma=m["gamma"])
    traj = prob.trajectory(o, n_steps, c0=m["c0"])
    J, dD, drho, dgam, dc0 = adjoint(prob, o, traj, terms)
    return J, np.concatenate([dD, drho, dgam, dc0])


def flat(prob, d):
    return np.concatenate(_direction(prob, d))
