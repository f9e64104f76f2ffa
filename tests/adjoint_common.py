"""
Numpy discrete adjoint of the oracle's backward-Euler / Newton scheme -- the CPU reference the device adjoint is checked
against (tests/test_adjoint_cpu.py validates it by central finite differences of the oracle's rd_step loop).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.glims_oracle import (OracleTumorGrowth, assemble_coupling, assemble_mass, assemble_stiffness,
                                 assemble_weighted_mass_p1, box_mesh, rectangle_mesh)


def thresh(c, level, smooth):
    return 0.5 * (np.tanh((c - level) / smooth) + 1.0)


def dthresh(c, level, smooth):
    t = np.tanh((c - level) / smooth)
    return 0.5 * (1.0 - t * t) / smooth


class Problem:
    """Two-tissue mesh (label 1 right of x = 0.5), Gaussian seed, Dirichlet c on the nodes at x = 1, u = 0 at x = 0."""

    def __init__(self, dim, n, dt=0.05, D=(0.02, 0.05), rho=(0.4, 0.6), gamma=(0.2, 0.1), E=(1.0, 2.0), nu=(0.3, 0.4),
                 dirichlet_c=0.05):
        if dim == 2:
            self.points, self.cells = rectangle_mesh([0.0, 0.0], [1.0, 1.0], n, n)
        else:
            self.points, self.cells = box_mesh([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], n, n, n)
        self.dim, self.dt = dim, dt
        self.labels = (self.points[self.cells].mean(axis=1)[:, 0] > 0.5).astype(np.int32)
        self.n_labels = 2
        self.D, self.rho, self.gamma = np.array(D, float), np.array(rho, float), np.array(gamma, float)
        self.E, self.nu = np.array(E, float), np.array(nu, float)
        x = self.points
        self.c0 = 0.8 * np.exp(-((x - 0.35) ** 2).sum(axis=1) / 0.04)
        xc = np.nonzero(np.isclose(x[:, 0], 1.0))[0]
        self.dir_c = (xc, np.full(len(xc), dirichlet_c)) if dirichlet_c is not None else None
        xu = np.nonzero(np.isclose(x[:, 0], 0.0))[0]
        self.dir_u = ((xu[:, None] * dim + np.arange(dim)[None]).ravel(), np.zeros(len(xu) * dim))

    def oracle(self, D=None, rho=None, gamma=None):
        lab = self.labels
        D = self.D if D is None else np.asarray(D)
        rho = self.rho if rho is None else np.asarray(rho)
        gamma = self.gamma if gamma is None else np.asarray(gamma)
        return OracleTumorGrowth(self.points, self.cells, D[lab], rho[lab], gamma[lab], self.E[lab], self.nu[lab],
                                 self.dt, dirichlet_u=self.dir_u, dirichlet_c=self.dir_c)

    def trajectory(self, o, n_steps, c0=None):
        c = [np.array(self.c0 if c0 is None else c0, dtype=np.float64)]
        for _ in range(n_steps):
            c.append(o.rd_step(c[-1], rtol=1e-14, atol=1e-16)[0])
        return c

    def terms(self, n_steps, seed=0, with_u=True, smooth=0.1):
        """T2-like + T1-like threshold terms at the last step, a plain L2 term midway, a displacement term at the last step."""
        rng = np.random.default_rng(seed)
        n = len(self.points)
        t = [dict(step=n_steps, kind="c_thresh", level=0.25, smooth=smooth, weight=1.0, target=rng.uniform(0, 1, n)),
             dict(step=n_steps, kind="c_thresh", level=0.6, smooth=smooth, weight=0.5, target=rng.uniform(0, 1, n)),
             dict(step=max(1, n_steps // 2), kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, n))]
        if with_u:
            t.append(dict(step=n_steps, kind="u_l2", weight=10.0, target=0.01 * rng.standard_normal(n * self.dim)))
        return t


def _u_solve(o, c):
    return o.mech_solve(c)


def misfit(prob, o, traj, terms):
    M = o.M
    Mv = sp.kron(M, sp.eye(prob.dim)).tocsr()
    J = 0.0
    for t in terms:
        c = traj[t["step"]]
        if t["kind"] == "u_l2":
            e = _u_solve(o, c) - np.ravel(t["target"])
            J += 0.5 * t["weight"] * e @ (Mv @ e)
        else:
            h = thresh(c, t["level"], t["smooth"]) if t["kind"] == "c_thresh" else c
            e = h - t["target"]
            J += 0.5 * t["weight"] * e @ (M @ e)
    return J


def adjoint(prob, o, traj, terms):
    """(J, dJ/dD [labels], dJ/drho, dJ/dgamma, dJ/dc0) of J(c_0 .. c_N) by the discrete adjoint."""
    pts, cells, lab, d = prob.points, prob.cells, prob.labels, prob.dim
    L = prob.n_labels
    n = len(pts)
    N = len(traj) - 1
    dt = prob.dt
    M = o.M
    Mv = sp.kron(M, sp.eye(d)).tocsr()
    Kel, G = o._mech_setup()
    free = o._free_mask_c()
    free_u = np.ones(n * d, bool)
    free_u[prob.dir_u[0]] = False
    Kt = [assemble_stiffness(pts, cells, (lab == t).astype(float)) for t in range(L)]
    Mt = [assemble_mass(pts, cells, (lab == t).astype(float)) for t in range(L)]
    Gt = [assemble_coupling(pts, cells, o.mu, o.lam, (lab == t).astype(float)) for t in range(L)]
    J = misfit(prob, o, traj, terms)
    dD, drho, dgam = np.zeros(L), np.zeros(L), np.zeros(L)
    lam_next = np.zeros(n)
    Kff = spla.splu(Kel[free_u][:, free_u].tocsc())
    dc0 = None
    for k in range(N, -1, -1):
        c = traj[k]
        g = np.zeros(n)
        gu = np.zeros(n * d)
        have_u = False
        for t in terms:
            if t["step"] != k:
                continue
            if t["kind"] == "u_l2":
                e = _u_solve(o, c) - np.ravel(t["target"])
                gu += t["weight"] * (Mv @ e)
                have_u = True
            elif t["kind"] == "c_thresh":
                e = thresh(c, t["level"], t["smooth"]) - t["target"]
                g += t["weight"] * dthresh(c, t["level"], t["smooth"]) * (M @ e)
            else:
                g += t["weight"] * (M @ (c - t["target"]))
        if have_u:
            mu = np.zeros(n * d)
            mu[free_u] = Kff.solve(gu[free_u])
            g += G.T @ mu
            for t in range(L):
                dgam[t] += mu @ (Gt[t] @ c)
        if k == 0:
            dc0 = M @ lam_next + g
            break
        rhs = g + M @ lam_next
        A = o.rd_jacobian(c)
        lam = np.zeros(n)
        lam[free] = spla.splu(A[free][:, free].tocsc()).solve(rhs[free])
        for t in range(L):
            Nt = assemble_weighted_mass_p1(pts, cells, c, (lab == t).astype(float))
            dD[t] += -dt * lam @ (Kt[t] @ c)
            drho[t] += -dt * lam @ (Nt @ c - Mt[t] @ c)
        lam_next = lam
    return J, dD, drho, dgam, dc0


def make_problem(dim):
    return Problem(2, 8) if dim == 2 else Problem(3, 4)
