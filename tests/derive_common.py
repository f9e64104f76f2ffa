"""
The derived fields of a step (glims_derive; csrc/derive.hip) stated in numpy, without a GPU.

Every field is the L2 projection  M p = int f phi_i dx  of an integrand f onto the P1 space:
  * per cell, either the cell's constant q_T times |T| / (d+1) for each of its vertices, or the local load vector
    loc[e][a] = |T| sum_q w_q lambda_qa f_q with the conical-product Gauss-Jacobi rule simplex_quadrature(d, 4);
  * per node, the sum of its cells' shares -- here ONE sparse incidence matrix B [N x M(d+1)] applied to the flattened local
    vectors (no np.add.at loops: this file is written independently of simulation_helpers/postprocess.py);
  * the mass systems solved directly (scipy spsolve on oracle.glims_oracle.assemble_mass).
Two-stage kinds follow the PostProcess class: von Mises stress from the PROJECTED (P1) stress, the growth-induced Jacobian
from the P1 growth strain, pressure as nodal algebra on the projected stress.

Tensors are returned as [N, d, d]; SYM[d] lists the (a, b) pairs of the symmetric components in the order the device keeps
and samples them: xx, yy, (zz,) xy, (xz, yz).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from glimslib_amd.simulation_helpers.postprocess import simplex_quadrature
from oracle.glims_oracle import assemble_mass, p1_geometry

KINDS = ("strain_tensor", "stress_tensor", "pressure", "van_mises_stress", "displacement_norm", "log_growth",
         "mech_expansion", "total_jacobian", "growth_induced_jacobian", "concentration_deformed_config")
NEEDS_U = {"strain_tensor", "stress_tensor", "pressure", "van_mises_stress", "displacement_norm", "total_jacobian",
           "concentration_deformed_config"}
NEEDS_C = {"log_growth", "mech_expansion", "growth_induced_jacobian", "concentration_deformed_config"}
SYM = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]}


def sym_components(t):
    """[N, d, d] -> [N, d(d+1)/2] in the device's component order."""
    d = t.shape[-1]
    return np.stack([t[:, a, b] for a, b in SYM[d]], axis=1)


class DeriveReference:
    def __init__(self, points, cells, labels, tables):
        self.points = np.asarray(points, dtype=np.float64)
        self.cells = np.asarray(cells, dtype=np.int64)
        self.d = self.points.shape[1]
        self.N, self.M = len(self.points), len(self.cells)
        lab = np.asarray(labels)
        self.cell = {k: np.asarray(tables[k], dtype=np.float64)[lab] for k in ("rho", "gamma", "E", "nu")}
        self.vol, self.grad = p1_geometry(self.points, self.cells)            # [M], [M, d+1, d]
        nv = self.d + 1
        self.B = sp.csr_matrix((np.ones(self.M * nv), (self.cells.ravel(), np.arange(self.M * nv))),
                               shape=(self.N, self.M * nv))
        self.lu = spla.splu(assemble_mass(self.points, self.cells).tocsc())
        self.lam, self.w = simplex_quadrature(self.d, 4)                     # [Q, d+1], [Q]

    # -- the two right-hand sides and the solve -------------------------------------------------------------------------
    def solve(self, rhs):
        return self.lu.solve(rhs)

    def rhs_cell(self, q):
        """q [M] or [M, k] cell-wise constant -> right-hand side(s) [N] / [N, k]"""
        q = np.asarray(q, dtype=np.float64)
        share = q * (self.vol / (self.d + 1)).reshape((-1,) + (1,) * (q.ndim - 1))
        return self.B @ np.repeat(share, self.d + 1, axis=0)

    def rhs_quad(self, fq):
        """fq [M, Q]: the integrand at the quadrature points of every cell -> right-hand side [N]"""
        loc = self.vol[:, None] * np.einsum('q,qa,mq->ma', self.w, self.lam, fq)   # [M, d+1]
        return self.B @ loc.ravel()

    def at_points(self, nodal):
        """P1 field [N, ...] -> its values at the quadrature points [M, Q, ...]"""
        return np.einsum('qa,ma...->mq...', self.lam, np.asarray(nodal)[self.cells])

    def project_cell(self, q):
        return self.solve(self.rhs_cell(q))

    def project_quad(self, fq):
        return self.solve(self.rhs_quad(fq))

    # -- pieces ---------------------------------------------------------------------------------------------------------
    def grad_u(self, u):
        """[M, b, a] = d u_b / d x_a"""
        return np.einsum('mvb,mva->mba', np.asarray(u).reshape(self.N, self.d)[self.cells], self.grad)

    def lame(self):
        E, nu = self.cell["E"], self.cell["nu"]
        return E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))

    def _tensor(self, q):
        d = self.d
        return self.project_cell(q.reshape(self.M, d * d)).reshape(self.N, d, d)

    def stress_p1(self, u):
        g = self.grad_u(u)
        eps = 0.5 * (g + np.swapaxes(g, 1, 2))
        mu, lam = self.lame()
        tr = np.trace(eps, axis1=1, axis2=2)
        return self._tensor(2.0 * mu[:, None, None] * eps + (lam * tr)[:, None, None] * np.eye(self.d))

    def growth_scalar(self, c):
        gam = self.cell["gamma"]
        if np.all(gam == gam[0]):
            return np.asarray(c, dtype=np.float64) * gam[0]
        return self.project_quad(gam[:, None] * self.at_points(c))

    # -- the kinds ------------------------------------------------------------------------------------------------------
    def field(self, kind, c=None, u=None):
        d = self.d
        if kind == "strain_tensor":
            g = self.grad_u(u)
            return self._tensor(0.5 * (g + np.swapaxes(g, 1, 2)))
        if kind == "stress_tensor":
            return self.stress_p1(u)
        if kind == "pressure":
            return np.trace(self.stress_p1(u), axis1=1, axis2=2) / 3.0
        if kind == "van_mises_stress":
            sq = self.at_points(self.stress_p1(u))                               # [M, Q, d, d]
            dev = sq - (np.trace(sq, axis1=2, axis2=3) / 3.0)[..., None, None] * np.eye(d)
            return self.project_quad(np.sqrt(1.5 * (dev * dev).sum(axis=(2, 3))))
        if kind == "displacement_norm":
            uq = self.at_points(np.asarray(u).reshape(self.N, d))
            return self.project_quad(np.sqrt((uq * uq).sum(axis=2)))
        if kind == "log_growth":
            cq = self.at_points(c)
            return self.project_quad(self.cell["rho"][:, None] * cq * (1.0 - cq))
        if kind == "mech_expansion":
            return self.growth_scalar(c)
        if kind == "total_jacobian":
            return self.project_cell(np.linalg.det(np.eye(d) + self.grad_u(u)))
        if kind == "growth_induced_jacobian":
            return self.project_quad((1.0 + self.at_points(self.growth_scalar(c))) ** d)
        if kind == "concentration_deformed_config":
            cq = self.at_points(c)
            jt = np.linalg.det(np.eye(d) + self.grad_u(u))
            return self.project_quad(cq * (1.0 + self.cell["gamma"][:, None] * cq) ** d / jt[:, None])
        raise KeyError(kind)


# ---- test problems shared by the CPU and GPU tests -------------------------------------------------------------------------
# two labels that differ in all five materials (label 0 is not used by any cell)
TABLES = dict(D=[0.0, 0.1, 0.03], rho=[0.0, 0.1, 0.25], gamma=[0.0, 0.2, 0.12], E=[1.0, 3e-3, 9e-3], nu=[0.3, 0.40, 0.30])


def two_labels(mesh):
    """Label 2 inside a disc / ball around a point off the lattice, label 1 outside: interface rows on every mesh."""
    mid = mesh.cell_midpoints()
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    ctr = lo + 0.45 * (hi - lo)
    r = 0.3 * (hi - lo).min()
    return np.where(((mid - ctr) ** 2).sum(axis=1) < r * r, 2, 1).astype(np.int32)


def sample_fields(points, seed=0):
    """c = 0.2 + 0.6 rand, u = A x + 0.05 sin terms (lengths scaled to the mesh), A with a deviatoric part of order 0.05: the
    von Mises integrand stays away from the kink of the square root at zero."""
    rng = np.random.default_rng(seed)
    X = np.asarray(points, dtype=np.float64)
    n, d = X.shape
    L = (X.max(axis=0) - X.min(axis=0)).max()
    xs = (X - X.min(axis=0)) / L
    A = 0.02 * rng.standard_normal((d, d))
    A[0, 0] += 0.05
    A[1, 1] -= 0.05
    u = L * (xs @ A.T + 0.05 * np.sin(3.0 * xs + np.arange(d)) * np.cos(2.0 * xs[:, ::-1]))
    c = 0.2 + 0.6 * rng.random(n)
    return c, u
