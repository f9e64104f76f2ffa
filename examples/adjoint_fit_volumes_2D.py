"""Fit (D, rho) of TumorGrowth to tumour VOLUMES alone -- the numbers a clinical series gives when no voxel image does: the
T2-like and T1-like tumour volume (concentration above a threshold; the reference's compute_from_conc_for_each_time_step /
compute_volume_thresholded, optimization_workflow/image_based_optimization.py:1333-1397, :1262-1301) at a few scan dates.  Each
datum is one volume misfit term 1/2 w (V - V_obs)^2 (sim.volume_term -> glims_adjoint_observable_terms): V is integrated and
differentiated on the device inside the backward sweep, so a fit costs one forward and one backward run per evaluation however
many parameters there are -- no finite differences of sim.observe.

The volumes are made by a two-tissue run with D = rho = 0.1 plus 1 % noise; the fit starts from (0.05, 0.2) and ends with the
Laplace covariance of the fitted parameters (smooth terms: the sharp volume is piecewise smooth and first order only).  One GPU:
volume terms are not available on partitioned runs."""
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


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_fit_volumes_")
levels = (0.2, 0.4)          # T2-like (oedema) and T1-like (tumour core) thresholds
scans = (2, 4, 6, 8, 10)     # time steps with a scan
smooth = 0.1
keys = [(lv, k) for lv in levels for k in scans]


def terms(sim, n_steps, data=None):
    """one smooth volume term per (threshold, scan); without data: targets 0, to read the volumes off the stored terms"""
    return [sim.volume_term(k, 0.0 if data is None else data[(lv, k)][0], threshold=lv, kind='smooth', smooth=smooth,
                            weight=1.0 if data is None else 1.0 / data[(lv, k)][1] ** 2) for lv, k in keys]


# the synthetic series: the volumes of the true run (as the device integrates them) with 1 % noise
truth = make_sim(0.1, 0.1)
truth.run(record_adjoint=True, save_method=None, plot=False, output_dir=out)
truth.adjoint_gradient(terms(truth, 10))
exact = {key: truth._backend.observable_term_info(i)["V"] for i, key in enumerate(keys)}
truth.close()
rng = np.random.default_rng(0)
data = {key: (v * (1.0 + 0.01 * rng.standard_normal()), 0.01 * v) for key, v in exact.items()}   # (V_obs, sigma)
for lv in levels:
    print("threshold %.2f: " % lv + "  ".join("t=%d V=%.3f" % (k, data[(lv, k)][0]) for k in scans))

# weights 1 / sigma^2: J is the negative log-likelihood, its Hessian at the optimum the inverse Laplace covariance
sim = make_sim(0.05, 0.2)
rf = ReducedFunctional(sim, 2, lambda s, n: terms(s, n, data), run_kwargs=dict(output_dir=out))
res = minimize(rf, [0.05, 0.2], options={"maxiter": 30, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16)
print("fitted D = %.6f, rho = %.6f after %d L-BFGS-B iterations, %d forward + backward runs (J = %.3e)"
      % (res.x[0], res.x[1], res.nit, rf.evaluations, res.fun))
info = sim._backend.observable_term_info(len(keys) - 1)
print("last term: %d cells counted, V = %.4f (observed %.4f)" % (info["counted"], info["V"], data[keys[-1]][0]))
H = rf.hessian_matrix(res.x)
cov = np.linalg.inv(H)
sd = np.sqrt(np.diag(cov))
print("Hessian at the optimum:\n%s" % H)
print("Laplace covariance:\n%s" % cov)
print("standard deviations: D %.3e, rho %.3e;  D-rho correlation %.4f" % (sd[0], sd[1], cov[0, 1] / (sd[0] * sd[1])))
sim.close()
