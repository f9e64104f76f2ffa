"""Fit (E_WM, coupling) of TumorGrowthBrain on a 2-D four-tissue mesh to a displacement field with trust-constr and the exact
second-order elastic adjoint (ReducedFunctional(..., elastic_hessian=True): hessp through glims_adjoint_hessian_full), then
the 2 x 2 Laplace covariance of the fit and its correlation coefficient.  The stiffness of the white matter and the coupling
are nearly confounded -- a softer tissue and a weaker growth-induced strain move the displacement almost alike -- and only
the mixed second derivative d2J / dE_WM dcoupling shows by how much.  The target is the displacement of a run with
E_WM = 1.5, coupling = 0.1 plus noise; the fit starts from (1.0, 0.15)."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import fenics_local as fenics  # noqa: E402
from glimslib_amd.optimization import ReducedFunctional, minimize  # noqa: E402
from glimslib_amd.simulation import TumorGrowthBrain  # noqa: E402


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def make_sim(E_WM, coupling):
    mesh = fenics.RectangleMesh(fenics.Point(0, 0), fenics.Point(20, 18), 30, 27)
    mid = mesh.cell_midpoints()
    r = np.linalg.norm((mid - np.array([10, 9])) / np.array([10, 9]), axis=1)
    lab = np.where(r < 0.25, 4, np.where(r < 0.6, 3, np.where(r < 0.85, 2, 1)))
    sim = TumorGrowthBrain(mesh)
    sim.setup_global_parameters(subdomains=lab, domain_names={1: 'CSF', 3: 'WM', 2: 'GM', 4: 'Ventricles'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped_0': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                             'named_boundary': 'boundary_all', 'subspace_id': 0}})
    iv = fenics.Expression('exp(-a*pow(x[0]-x0, 2) - a*pow(x[1]-y0, 2))', degree=1, a=0.05, x0=12, y0=9)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0., 0.)), 1: iv}, sim_time=6, sim_time_step=1,
                               E_GM=1.0, E_WM=E_WM, E_CSF=0.5, E_VENT=0.5, nu_GM=0.45, nu_WM=0.4, nu_CSF=0.45,
                               nu_VENT=0.3, D_GM=0.01, D_WM=0.05, rho_GM=0.05, rho_WM=0.05, coupling=coupling)
    return sim


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_hess_el_")
run = dict(keep_nth=10 ** 9, save_method=None, clear_all=False, plot=False, output_dir=out)
truth = make_sim(1.5, 0.1)
truth.run(record_adjoint=True, **run)
assert truth._backend.solve_mechanics() == 0
u_end = truth._backend.get_state()[1].copy()
truth.close()
sigma = 0.02 * np.abs(u_end).max()
noisy = u_end + sigma * np.random.default_rng(0).standard_normal(u_end.shape)

terms = lambda sim, n_steps: [dict(step=n_steps, kind="u_l2", weight=1.0, target=noisy)]
sim = make_sim(1.0, 0.15)
rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out), names=("E_WM", "coupling"), elastic_hessian=True)
res = minimize(rf, [1.0, 0.15], bounds=([0.3, 0.02], [4.0, 0.5]), method="trust-constr",
               options={"maxiter": 80, "gtol": 1e-12, "xtol": 1e-14})
print("fitted E_WM = %.6f, coupling = %.6f: %d forward + backward runs, %d Hessian calls (J = %.3e)"
      % (res.x[0], res.x[1], rf.evaluations, rf.hessian_calls, res.fun))
H = rf.hessian_matrix(res.x)
cov = sigma ** 2 * np.linalg.inv(H)          # Laplace covariance of (E_WM, coupling)
sd = np.sqrt(np.diag(cov))
print("Hessian at the optimum:\n%s" % H)
print("Laplace covariance:\n%s" % cov)
print("standard deviations: E_WM %.3e, coupling %.3e;  E_WM-coupling correlation %.4f"
      % (sd[0], sd[1], cov[0, 1] / (sd[0] * sd[1])))
sim.close()
