"""Fit (D, rho) of TumorGrowth on a 2-D two-tissue mesh with trust-constr and the second-order device adjoint (hessp =
ReducedFunctional.hessian, the H that the reference's minimize_custom hands its optimizer), then the Laplace covariance of
the fit: the inverse Hessian at the optimum, scaled by the misfit variance sigma^2 of the images.  Targets are made by a run
with D = rho = 0.1 plus image noise; the fit starts from (0.05, 0.2)."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import fenics_local as fenics  # noqa: E402
from glimslib_amd.optimization import ReducedFunctional, minimize  # noqa: E402
from glimslib_amd.simulation import TumorGrowth  # noqa: E402


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def make_sim(D, rho):
    mesh = fenics.RectangleMesh(fenics.Point(-5, -5), fenics.Point(5, 5), 24, 24)
    labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1), fenics.FunctionSpace(mesh, "DG", 1))
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                               proliferation=rho, E=0.001, poisson=0.4, sim_time=10, sim_time_step=1)
    return sim


def thresh(c, level, smooth=0.1):
    return 0.5 * (np.tanh((c - level) / smooth) + 1.0)   # image_based_optimization.py:1404-1407, applied nodewise


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_hess_")
truth = make_sim(0.1, 0.1)
truth.run(save_method=None, plot=False, output_dir=out)
c_end = truth.solution.components[1].copy()
truth.close()
sigma = 0.02
noisy = c_end + sigma * np.random.default_rng(0).standard_normal(len(c_end))

terms = lambda sim, n_steps: [dict(step=n_steps, kind="c_thresh", level=0.16, target=thresh(c_end, 0.16), smooth=0.1),
                              dict(step=n_steps, kind="c_thresh", level=0.8, target=thresh(c_end, 0.8), smooth=0.1),
                              dict(step=n_steps, kind="c_l2", target=noisy)]
sim = make_sim(0.05, 0.2)
rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out))
res = minimize(rf, [0.05, 0.2], method="trust-constr", options={"maxiter": 60, "gtol": 1e-12, "xtol": 1e-14})
print("fitted D = %.6f, rho = %.6f: %d forward + backward runs, %d Hessian calls (J = %.3e)"
      % (res.x[0], res.x[1], rf.evaluations, rf.hessian_calls, res.fun))
H = rf.hessian_matrix(res.x)
cov = sigma ** 2 * np.linalg.inv(H)          # Laplace / Gauss-Newton covariance of (D, rho)
sd = np.sqrt(np.diag(cov))
print("Hessian at the optimum:\n%s" % H)
print("Laplace covariance:\n%s" % cov)
print("standard deviations: D %.3e, rho %.3e;  D-rho correlation %.4f" % (sd[0], sd[1], cov[0, 1] / (sd[0] * sd[1])))
sim.close()
