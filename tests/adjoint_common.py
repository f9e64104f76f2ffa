"""
Numpy discrete adjoint of the oracle's backward-Euler / Newton scheme -- the CPU reference the device adjoint is checked
against (tests/test_adjoint_cpu.py validates it by central finite differences of the oracle's rd_step loop).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.glims_oracle import (OracleTumorGrowth, box_mesh, compute_lambda, compute_mu, lumped_load, p1_geometry,
                                 rectangle_mesh, reference_mass, reference_triple)


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
        self.rd_load = self.mech_load = None

    @classmethod
    def from_mesh(cls, points, cells, labels, D, rho, gamma, E, nu, c0, dt=0.05, dir_c=None, dir_u=None, rd_load=None,
                  mech_load=None):
        """Any mesh and numbering, L = len(D) tissues (label ids that no cell carries allowed), Dirichlet c (nodes, values)
        and u (interleaved dofs, values, non-zero allowed), an RD load (already times dt) and a mechanical load."""
        self = cls.__new__(cls)
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.cells = np.ascontiguousarray(cells, dtype=np.int32)
        self.dim = self.points.shape[1]
        self.dt = dt
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.D, self.rho, self.gamma = np.array(D, float), np.array(rho, float), np.array(gamma, float)
        self.E, self.nu = np.array(E, float), np.array(nu, float)
        self.n_labels = len(self.D)
        assert self.labels.max() < self.n_labels
        assert all(len(a) == self.n_labels for a in (self.rho, self.gamma, self.E, self.nu))
        self.c0 = np.array(c0, dtype=np.float64)
        self.dir_c, self.dir_u, self.rd_load, self.mech_load = dir_c, dir_u, rd_load, mech_load
        return self

    def oracle(self, D=None, rho=None, gamma=None):
        lab = self.labels
        D = self.D if D is None else np.asarray(D)
        rho = self.rho if rho is None else np.asarray(rho)
        gamma = self.gamma if gamma is None else np.asarray(gamma)
        return OracleTumorGrowth(self.points, self.cells, D[lab], rho[lab], gamma[lab], self.E[lab], self.nu[lab],
                                 self.dt, dirichlet_u=self.dir_u, dirichlet_c=self.dir_c, rd_load=self.rd_load,
                                 mech_load=self.mech_load)

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


def _cell_sums(labels, L, x):
    return np.bincount(labels, weights=x, minlength=L)


def adjoint(prob, o, traj, terms):
    """(J, dJ/dD [labels], dJ/drho, dJ/dgamma, dJ/dc0) of J(c_0 .. c_N) by the discrete adjoint.  The per-label sensitivities
    are per-cell integrals (exact for P1) summed over each label's cells."""
    pts, lab, d = prob.points, prob.labels, prob.dim
    cells = np.asarray(prob.cells, dtype=np.int64)
    L = prob.n_labels
    n = len(pts)
    N = len(traj) - 1
    dt = prob.dt
    M = o.M
    Mv = sp.kron(M, sp.eye(d)).tocsr()
    vol, grads = p1_geometry(pts, cells)
    Mr, Tr = reference_mass(d), reference_triple(d)
    free = o._free_mask_c()
    any_u = any(t["kind"] == "u_l2" for t in terms)
    if any_u:
        Kel, G = o._mech_setup()
        free_u = np.ones(n * d, bool)
        if prob.dir_u is not None:
            free_u[np.asarray(prob.dir_u[0], dtype=np.int64)] = False
        Kff = spla.splu(Kel[free_u][:, free_u].tocsc())
        E, nu = prob.E[lab], prob.nu[lab]
        cG = (2.0 * compute_mu(E, nu) + d * compute_lambda(E, nu)) * vol / (d + 1)   # G_T with gamma = 1
    J = misfit(prob, o, traj, terms)
    dD, drho, dgam = np.zeros(L), np.zeros(L), np.zeros(L)
    lam_next = np.zeros(n)
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
            div = np.einsum('mad,mad->m', mu.reshape(n, d)[cells], grads)          # div mu_h on each cell
            dgam += _cell_sums(lab, L, cG * div * c[cells].sum(axis=1))           # mu^T G_t c
        if k == 0:
            dc0 = M @ lam_next + g
            break
        rhs = g + M @ lam_next
        A = o.rd_jacobian(c)
        lam = np.zeros(n)
        lam[free] = spla.splu(A[free][:, free].tocsc()).solve(rhs[free])
        cl, ll = c[cells], lam[cells]
        gc, gl = np.einsum('ma,mad->md', cl, grads), np.einsum('ma,mad->md', ll, grads)
        dD += -dt * _cell_sums(lab, L, vol * (gl * gc).sum(axis=1))                 # lam^T K_t c
        lNc = np.einsum('ijk,mi,mj,mk->m', Tr, ll, cl, cl, optimize=True)   # lam^T N_t(c) c / |T|
        lMc = np.einsum('ij,mi,mj->m', Mr, ll, cl)
        drho += -dt * _cell_sums(lab, L, vol * (lNc - lMc))
        lam_next = lam
    return J, dD, drho, dgam, dc0


def renumber(points, cells, seed):
    """The same mesh under a random permutation of its node ids: returns (points, cells, perm) with new node i = old perm[i]."""
    perm = np.random.default_rng(seed).permutation(len(points))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return np.ascontiguousarray(points[perm]), np.ascontiguousarray(inv[cells], dtype=np.int32), perm


def many_tissues(dim, L, n=None, mesh=None, empty=(), zero=(), zero_gamma=(), u_clamp=0.0, mech_load=0.0, rd_load=0.0,
                 dt=0.05, seed=0):
    """L tissues on the unit square / cube (n per axis) or on ``mesh`` = (points, cells) scaled into it.  Cells go to labels in
    scrambled bands of x + 0.61 y (+ 0.37 z), skipping the ids in ``empty``; tissues in ``zero`` get D = rho = 0, those in
    ``zero_gamma`` gamma = 0.  Dirichlet c = 0.05 on x = 1 (x >= 0.97 on a mesh without a face there), u clamped on x = 0 to
    u_clamp times a smooth non-zero field, a mechanical load of size mech_load and an RD source (times dt) of size rd_load."""
    rng = np.random.default_rng(seed)
    if mesh is None:
        points, cells = rectangle_mesh([0.0, 0.0], [1.0, 1.0], n, n) if dim == 2 else \
            box_mesh([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], n, n, n)
    else:
        points, cells = np.asarray(mesh[0], dtype=np.float64), np.asarray(mesh[1])
        lo, hi = points.min(axis=0), points.max(axis=0)
        points = (points - lo) / (hi - lo)
    ids = rng.permutation([l for l in range(L) if l not in empty])
    xm = points[cells].mean(axis=1)
    s = xm @ np.array([1.0, 0.61, 0.37][:dim])
    band = np.floor((s - s.min()) / (np.ptp(s) * (1 + 1e-12)) * 2 * len(ids)).astype(np.int64) % len(ids)
    labels = ids[band].astype(np.int32)
    D, rho = rng.uniform(0.01, 0.06, L), rng.uniform(0.2, 0.7, L)
    gamma, E, nu = rng.uniform(0.05, 0.25, L), rng.uniform(1.0, 3.0, L), rng.uniform(0.25, 0.4, L)
    D[list(zero)] = 0.0
    rho[list(zero)] = 0.0
    gamma[list(zero_gamma)] = 0.0
    x = points
    c0 = 0.8 * np.exp(-((x - 0.35) ** 2).sum(axis=1) / 0.04)
    tol = 1e-9 if mesh is None else 0.03
    xc = np.nonzero(x[:, 0] >= 1.0 - tol)[0]
    xu = np.nonzero(x[:, 0] <= tol)[0]
    dofs = (xu[:, None] * dim + np.arange(dim)[None]).ravel()
    uval = u_clamp * (np.sin(3.0 * x[xu, 1:2] + 1.0) * (1.0 + np.arange(dim))[None]).ravel()
    ml = mech_load * rng.standard_normal(len(x) * dim) * np.repeat(lumped_load(points, cells), dim) if mech_load else None
    src = np.exp(-((x - 0.6) ** 2).sum(axis=1) / 0.02)
    rl = rd_load * dt * lumped_load(points, cells) * src if rd_load else None
    return Problem.from_mesh(points, cells, labels, D, rho, gamma, E, nu, c0, dt=dt, dir_c=(xc, np.full(len(xc), 0.05)),
                             dir_u=(dofs, uval), rd_load=rl, mech_load=ml)


def u_terms(prob, steps, seed=0, weight=10.0):
    """One u_l2 term per entry of ``steps`` (repeats allowed) with random targets of the size of the displacement."""
    rng = np.random.default_rng(seed)
    n = len(prob.points)
    return [dict(step=k, kind="u_l2", weight=weight * (1 + i), target=0.01 * rng.standard_normal(n * prob.dim))
            for i, k in enumerate(steps)]


def make_problem(dim):
    return Problem(2, 8) if dim == 2 else Problem(3, 4)
