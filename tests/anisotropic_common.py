"""
The numpy statement of the anisotropic model ("Anisotropic diffusion"): the flux of cell T with label t is
D_t * TT_T grad c with a symmetric positive-definite tensor TT_T per cell.

  * aniso_oracle: an OracleTumorGrowth whose attributes K and S are replaced by
        K = scatter(vol * D[lab] * einsum(grads, TT, grads)),   S = M - dt * Mrho + dt * K
    (rd_residual reads K, rd_jacobian reads S: the oracle's own Newton loop then steps the anisotropic model);
  * adjoint / hessian: copies of the first- and second-order statements of tests/adjoint_common.py and
    tests/adjoint_hessian_common.py with TT in the three gradient forms -- everything else (rho, gamma, the misfit terms, the
    mechanics) is theirs, line by line.  The Dirichlet rows are eliminated on o._free_mask_c() as there;
  * the tensor fields of the tests: random SPD tensors with a log-uniform eigenvalue ratio up to 10 in random frames, and the
    uniform diag(a^2, 1 ...) of the stretch identity.

tests/test_anisotropic_cpu.py validates these statements by finite differences and by the stretch identity.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adjoint_common import dthresh, misfit, thresh
from adjoint_hessian_common import _direction, d2thresh
from oracle.glims_oracle import (_scatter_scalar, compute_lambda, compute_mu, p1_geometry, reference_mass,
                                 reference_triple)


# ---- tensor fields ---------------------------------------------------------------------------------------------------------
def random_spd(n_cells, dim, seed=0, max_ratio=10.0):
    """[n_cells, d, d]: Q diag(l) Q^T with Q a random rotation (QR of a Gaussian matrix) and eigenvalues l = exp(uniform) such
    that lambda_max / lambda_min is log-uniform in [1, max_ratio] and the geometric mean of the extremes is 1."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n_cells, dim, dim)))[0]
    half = 0.5 * rng.uniform(0.0, np.log(max_ratio), n_cells)
    l = np.empty((n_cells, dim))
    l[:, 0], l[:, -1] = np.exp(half), np.exp(-half)
    for k in range(1, dim - 1):
        l[:, k] = np.exp(rng.uniform(-half, half))
    T = np.einsum('nak,nk,nbk->nab', Q, l, Q)
    return 0.5 * (T + np.swapaxes(T, 1, 2))


def uniform_stretch(n_cells, dim, a=2.0):
    """[n_cells, d, d]: diag(a^2, 1, ...) in every cell."""
    T = np.eye(dim)
    T[0, 0] = a * a
    return np.broadcast_to(T, (n_cells, dim, dim)).copy()


def identity_field(n_cells, dim):
    return np.broadcast_to(np.eye(dim), (n_cells, dim, dim)).copy()


def pack(T):
    """[n, d, d] -> [n, d (d + 1) / 2], the upper triangle row by row."""
    iu = np.triu_indices(T.shape[1])
    return np.ascontiguousarray(T[:, iu[0], iu[1]])


def max_ratio(T):
    w = np.linalg.eigvalsh(T)
    return float((w[:, -1] / w[:, 0]).max())


# ---- the operators ---------------------------------------------------------------------------------------------------------
def stiffness(points, cells, Dcell, T):
    vol, grads = p1_geometry(points, cells)
    local = (vol * Dcell)[:, None, None] * np.einsum('mad,mde,mbe->mab', grads, T, grads)
    return _scatter_scalar(np.asarray(cells), local, len(points))


def aniso_oracle(prob, T, D=None, rho=None, gamma=None):
    """prob.oracle(...) with K and S of the tensor field T [n_cells, d, d] (None: the oracle as it is)."""
    o = prob.oracle(D=D, rho=rho, gamma=gamma)
    if T is not None:
        o.K = stiffness(o.points, o.cells, o.D, np.asarray(T, dtype=np.float64))
        o.S = (o.M - o.dt * o.Mrho + o.dt * o.K).tocsr()
    return o


class _Cells:
    """adjoint_hessian_common._Cells with GG = grads TT grads^T."""

    def __init__(self, prob, T):
        self.cells = np.asarray(prob.cells, dtype=np.int64)
        self.n = len(prob.points)
        self.vol, self.grads = p1_geometry(prob.points, self.cells)
        self.Mr, self.Tr = reference_mass(prob.dim), reference_triple(prob.dim)
        self.GG = np.einsum('mad,mde,mbe->mab', self.grads, T, self.grads)

    def scatter(self, v):
        return np.bincount(self.cells.ravel(), weights=v.ravel(), minlength=self.n)

    def K(self, x):                  # int_T grad phi_a^T TT grad x
        return self.vol[:, None] * np.einsum('mab,mb->ma', self.GG, x[self.cells])

    def T(self, x, y):
        return self.vol[:, None] * np.einsum('abk,mb,mk->ma', self.Tr, x[self.cells], y[self.cells], optimize=True)

    def Mv(self, x):
        return self.vol[:, None] * np.einsum('ab,mb->ma', self.Mr, x[self.cells])

    def gg(self, x, y):              # int_T grad x^T TT grad y
        return self.vol * np.einsum('mab,ma,mb->m', self.GG, x[self.cells], y[self.cells])

    def xyz(self, x, y, z):
        return self.vol * np.einsum('abk,ma,mb,mk->m', self.Tr, x[self.cells], y[self.cells], z[self.cells], optimize=True)

    def xy(self, x, y):
        return self.vol * np.einsum('ab,ma,mb->m', self.Mr, x[self.cells], y[self.cells])


# ---- first order -----------------------------------------------------------------------------------------------------------
def adjoint(prob, o, traj, terms, T):
    """adjoint_common.adjoint with dJ/dD_t = -dt sum_{T in t} |T| grad lam^T TT grad c; o is aniso_oracle(prob, T)."""
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
        cG = (2.0 * compute_mu(E, nu) + d * compute_lambda(E, nu)) * vol / (d + 1)
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
                e = o.mech_solve(c) - np.ravel(t["target"])
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
            div = np.einsum('mad,mad->m', mu.reshape(n, d)[cells], grads)
            dgam += np.bincount(lab, weights=cG * div * c[cells].sum(axis=1), minlength=L)
        if k == 0:
            dc0 = M @ lam_next + g
            break
        rhs = g + M @ lam_next
        A = o.rd_jacobian(c)
        lam = np.zeros(n)
        lam[free] = spla.splu(A[free][:, free].tocsc()).solve(rhs[free])
        cl, ll = c[cells], lam[cells]
        gc, gl = np.einsum('ma,mad->md', cl, grads), np.einsum('ma,mad->md', ll, grads)
        dD += -dt * np.bincount(lab, weights=vol * np.einsum('md,mde,me->m', gl, T, gc), minlength=L)   # lam^T K_t c
        lNc = np.einsum('ijk,mi,mj,mk->m', Tr, ll, cl, cl, optimize=True)
        lMc = np.einsum('ij,mi,mj->m', Mr, ll, cl)
        drho += -dt * np.bincount(lab, weights=vol * (lNc - lMc), minlength=L)
        lam_next = lam
    return J, dD, drho, dgam, dc0


# ---- second order ----------------------------------------------------------------------------------------------------------
def hessian(prob, o, traj, terms, directions, T):
    """adjoint_hessian_common.hessian with TT in int grad c . grad phi_i, int grad lam . grad phi_i and
    int grad nu . grad c + grad lam . grad dc; o is aniso_oracle(prob, T)."""
    lab, d, L = prob.labels, prob.dim, prob.n_labels
    geo = _Cells(prob, T)
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
        cG = (2.0 * compute_mu(E, nu) + d * compute_lambda(E, nu)) * geo.vol / (d + 1)

        def solve_u(b):
            x = np.zeros(n * d)
            x[free_u] = Kff.solve(b[free_u])
            return x

        def div(v):
            return np.einsum('mad,mad->m', v.reshape(n, d)[cells], geo.grads)

        def G_of(wcell, x):
            out = np.zeros((n, d))
            np.add.at(out, cells, (wcell * cG * x[cells].sum(axis=1))[:, None, None] * geo.grads)
            return out.ravel()

        def GT_of(wcell, v):
            return geo.scatter(np.repeat((wcell * cG * div(v))[:, None], d + 1, axis=1))

    def rd_solver(c):
        A = o.rd_jacobian(c)
        lu = spla.splu(A[free][:, free].tocsc())

        def solve(b):
            x = np.zeros(n)
            x[free] = lu.solve(b[free])
            return x
        return solve

    J, dD, drho, dgam, dc0 = adjoint(prob, o, traj, terms, T)
    dc = [[dirs[p][3].copy()] for p in range(P)]
    for k in range(1, N + 1):
        c = traj[k]
        solve = rd_solver(c)
        for p in range(P):
            D_p, r_p = dirs[p][0][lab], dirs[p][1][lab]
            src = -dt * geo.scatter(D_p[:, None] * geo.K(c) + r_p[:, None] * (geo.T(c, c) - geo.Mv(c)))
            dc[p].append(solve(M @ dc[p][k - 1] + src))
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


def gradient_at(prob, m, n_steps, terms, T):
    """(J, flat gradient [D, rho, gamma, c0]) of the numpy adjoint at m = dict(D, rho, gamma, c0)."""
    o = aniso_oracle(prob, T, D=m["D"], rho=m["rho"], gamma=m["gamma"])
    traj = prob.trajectory(o, n_steps, c0=m["c0"])
    J, dD, drho, dgam, dc0 = adjoint(prob, o, traj, terms, T)
    return J, np.concatenate([dD, drho, dgam, dc0])


def J_at(prob, D, n_steps, terms, T):
    o = aniso_oracle(prob, T, D=D)
    return misfit(prob, o, prob.trajectory(o, n_steps), terms)


# ---- the example's fit (examples/anisotropic_growth_2D.py), shared by its scipy twin (CPU) and the device test -------------
FIT = dict(n=16, half=5.0, steps=5, dt=1.0, D=0.1, rho=0.1, ratio=6.0, start=(0.05, 0.2), seed=(1.0, 0.5), levels=(0.16, 0.8))


def fit_tensor(centroids, labels):
    """Horizontal fibres of ratio FIT['ratio'], trace-normalised, in tissue 1 (x >= 0); the identity in tissue 2."""
    from glimslib_amd.utils.data_io import tensor_from_fibres
    T = identity_field(len(centroids), 2)
    e = np.zeros((int((labels == 1).sum()), 2))
    e[:, 0] = 1.0
    T[labels == 1] = tensor_from_fibres(e, FIT["ratio"])
    return T


def make_fit_sim(D, rho, with_tensor=True):
    """The example's simulation through the public API (no device is touched before run())."""
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.simulation import TumorGrowth

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    F = FIT
    mesh = fenics.RectangleMesh(fenics.Point(-F["half"], -F["half"]), fenics.Point(F["half"], F["half"]), F["n"], F["n"])
    labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1), fenics.FunctionSpace(mesh, "DG", 1))
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    u0 = fenics.Expression('exp(-(pow(x[0]-%r,2)+pow(x[1]-%r,2))/2.0)' % F["seed"], degree=1)
    tensor = (lambda xm: fit_tensor(xm, sim._labels())) if with_tensor else None
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                               proliferation=rho, E=0.001, poisson=0.4, sim_time=F["steps"] * F["dt"], sim_time_step=F["dt"],
                               diffusion_tensor=tensor)
    return sim


def fit_problem():
    """The example's problem as a numpy Problem on the simulation's own mesh and labels: tissues 1 and 2, one D and one rho
    for both, a Gaussian seed, no Dirichlet data on c.  Returns (prob, T)."""
    from adjoint_common import Problem
    sim = make_fit_sim(FIT["D"], FIT["rho"])
    pts, cells = np.asarray(sim.mesh.points, dtype=np.float64), np.asarray(sim.mesh.cells, dtype=np.int32)
    labels = np.asarray(sim._labels(), dtype=np.int32)
    c0 = np.exp(-((pts[:, 0] - FIT["seed"][0]) ** 2 + (pts[:, 1] - FIT["seed"][1]) ** 2) / 2.0)
    three = lambda v: np.array([0.0, v, v])
    prob = Problem.from_mesh(pts, cells, labels, three(FIT["D"]), three(FIT["rho"]), three(0.1), np.full(3, 0.001),
                             np.full(3, 0.4), c0, dt=FIT["dt"])
    return prob, fit_tensor(pts[cells].mean(axis=1), labels)


def fit_terms(c_end, n_steps):
    """T2-like and T1-like smoothed-threshold images of the final concentration."""
    return [dict(step=n_steps, kind="c_thresh", level=lv, target=thresh(c_end, lv, 0.1), smooth=0.1, weight=1.0)
            for lv in FIT["levels"]]


def second_moment_ratio(points, lumped, c):
    """Largest / smallest principal second moment of the concentration c about its centre of mass (nodal quadrature)."""
    w = lumped * c
    x = points - (w[:, None] * points).sum(axis=0) / w.sum()
    C = np.einsum('n,na,nb->ab', w, x, x) / w.sum()
    ev = np.linalg.eigvalsh(C)
    return float(ev[-1] / ev[0]), C
