"""
Numpy reference of dJ/dE and dJ/dnu per tissue label: the displacement misfit terms see E and nu
through u_k = K_el^-1 (G c_k + f), so with mu_k = K_el^-1 dJ/du_k (0 on the constrained dofs)

    dJ/dp_t = sum_k mu_k^T (dG/dp c_k - dK/dp u_k)        (u_k with its Dirichlet values)

summed over the steps that a displacement term observes.  dK/dp and dG/dp are assembled by the oracle's assemble_elasticity
/ assemble_coupling from the per-cell Lame derivatives masked to label t: independent of the per-cell algebra (A_t, B_t, C_t)
the device pass uses, which `formula_gradient` restates for comparison.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adjoint_common import misfit
from oracle.glims_oracle import OracleTumorGrowth, assemble_coupling, assemble_elasticity, p1_geometry


def lame_derivatives(E, nu):
    """{'E': (mu', lam'), 'nu': (mu', lam')}: derivatives of the Lame pair of (E, nu) (math_linear_elasticity.py)."""
    E, nu = np.asarray(E, float), np.asarray(nu, float)
    q = (1.0 + nu) * (1.0 - 2.0 * nu)
    return {"E": (1.0 / (2.0 * (1.0 + nu)), nu / q),
            "nu": (-E / (2.0 * (1.0 + nu) ** 2), E * (1.0 + 2.0 * nu * nu) / (q * q))}


def oracle_with(prob, E=None, nu=None):
    """prob.oracle() with per-label E / nu tables replaced."""
    lab = prob.labels
    E = prob.E if E is None else np.asarray(E, float)
    nu = prob.nu if nu is None else np.asarray(nu, float)
    return OracleTumorGrowth(prob.points, prob.cells, prob.D[lab], prob.rho[lab], prob.gamma[lab], E[lab], nu[lab], prob.dt,
                             dirichlet_u=prob.dir_u, dirichlet_c=prob.dir_c, rd_load=prob.rd_load, mech_load=prob.mech_load)


def observed(prob, o, traj, terms):
    """[(c_k, u_k, mu_k)] for every step k a displacement term observes."""
    n, d = len(prob.points), prob.dim
    Kel, _ = o._mech_setup()
    Mv = sp.kron(o.M, sp.eye(d)).tocsr()
    free = np.ones(n * d, bool)
    if prob.dir_u is not None:
        free[np.asarray(prob.dir_u[0], dtype=np.int64)] = False
    Kff = spla.splu(Kel[free][:, free].tocsc())
    out = []
    for k in sorted({t["step"] for t in terms if t["kind"] == "u_l2"}):
        c = traj[k]
        u = o.mech_solve(c)
        gu = np.zeros(n * d)
        for t in terms:
            if t["step"] == k and t["kind"] == "u_l2":
                gu += t["weight"] * (Mv @ (u - np.ravel(t["target"])))
        mu = np.zeros(n * d)
        mu[free] = Kff.solve(gu[free])
        out.append((c, u, mu))
    return out


def elastic_adjoint(prob, o, traj, terms):
    """(dJ/dE [labels], dJ/dnu [labels]) from the assembled derivatives of K_el and G."""
    lab, L = prob.labels, prob.n_labels
    obs = observed(prob, o, traj, terms)
    der = lame_derivatives(prob.E[lab], prob.nu[lab])
    out = []
    for p in ("E", "nu"):
        mp, lp = der[p]
        g = np.zeros(L)
        for t in range(L):
            m = (lab == t).astype(float)
            if not obs or not m.any():
                continue
            dK = assemble_elasticity(prob.points, prob.cells, mp * m, lp * m)
            dG = assemble_coupling(prob.points, prob.cells, mp * m, lp * m, prob.gamma[lab])
            g[t] = sum(mu @ (dG @ c - dK @ u) for c, u, mu in obs)
        out.append(g)
    return out[0], out[1]


def formula_gradient(prob, o, traj, terms):
    """The same two arrays through the per-label sums of the device pass: A_t = sum int_t eps(mu):eps(u),
    B_t = sum int_t div mu div u, C_t = sum int_t 1/(d+1) div mu sum_a c_a, and
    dJ/dp_t = gamma_t (2 mu' + d lam') C_t - (2 mu' A_t + lam' B_t)."""
    lab, L, d = prob.labels, prob.n_labels, prob.dim
    cells = np.asarray(prob.cells, dtype=np.int64)
    n = len(prob.points)
    vol, grads = p1_geometry(prob.points, cells)
    A, B, Cs = np.zeros(L), np.zeros(L), np.zeros(L)
    for c, u, mu in observed(prob, o, traj, terms):
        gm = np.einsum('mvb,mva->mab', mu.reshape(n, d)[cells], grads)    # grad mu_h [a][b] = d_a mu_b
        gu = np.einsum('mvb,mva->mab', u.reshape(n, d)[cells], grads)
        em, eu = 0.5 * (gm + gm.transpose(0, 2, 1)), 0.5 * (gu + gu.transpose(0, 2, 1))
        dm, du = np.trace(gm, axis1=1, axis2=2), np.trace(gu, axis1=1, axis2=2)
        A += np.bincount(lab, vol * (em * eu).sum(axis=(1, 2)), minlength=L)
        B += np.bincount(lab, vol * dm * du, minlength=L)
        Cs += np.bincount(lab, vol / (d + 1) * dm * c[cells].sum(axis=1), minlength=L)
    out = []
    for p in ("E", "nu"):
        mp, lp = lame_derivatives(prob.E, prob.nu)[p]
        out.append(prob.gamma * (2.0 * mp + d * lp) * Cs - (2.0 * mp * A + lp * B))
    return out[0], out[1]


def misfit_of(prob, traj, terms, E=None, nu=None):
    """J for per-label E / nu tables (the concentration trajectory does not depend on them)."""
    return misfit(prob, oracle_with(prob, E, nu), traj, terms)


def central_differences(prob, traj, terms, rel_step=1e-5):
    """(dJ/dE, dJ/dnu) per label by central differences of the oracle's J."""
    out = []
    for key in ("E", "nu"):
        base = getattr(prob, key)
        g = np.zeros(prob.n_labels)
        for t in range(prob.n_labels):
            h = rel_step * abs(base[t])
            hi, lo = base.copy(), base.copy()
            hi[t] += h
            lo[t] -= h
            kw_hi, kw_lo = {key: hi}, {key: lo}
            g[t] = (misfit_of(prob, traj, terms, **kw_hi) - misfit_of(prob, traj, terms, **kw_lo)) / (2.0 * h)
        out.append(g)
    return out[0], out[1]
