"""Fitting the anisotropy ratio together with D and rho: the set-up of examples/anisotropic_growth_2D.py -- a 16 x 16 rectangle,
horizontal fibres in tissue A (x >= 0), tissue B isotropic, T2- / T1-like threshold images of the last step -- with the ratio
of the fibre tensors T = s (I + (ratio - 1) e e^T), s = 2 / (1 + ratio), as a third control.

A DTI atlas gives the fibre directions, not the tumour's anisotropy: the factor is fitted.  `sim.set_diffusion_tensor_family`
takes a family (theta, centroids) -> (T, [dT/dtheta_k]); every run builds the field and its tangent from the present
`sim.tensor_params`, the backward sweep adds up dJ/dratio next to dJ/dD (one more bilinear form per cell, DESIGN.md section 17,
"Tangent fields"), and `ReducedFunctional(tensor_controls=('ratio',))` appends the ratio to the control vector.  First order:
L-BFGS-B, with bounds of its own for the ratio."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import fenics_local as fenics  # noqa: E402
from glimslib_amd.optimization import ReducedFunctional, minimize  # noqa: E402
from glimslib_amd.simulation import TumorGrowth  # noqa: E402
from glimslib_amd.utils.data_io import tensor_from_fibres  # noqa: E402

TRUTH = (0.1, 0.1, 6.0)     # D, rho, ratio
START = (0.05, 0.2, 2.0)


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def fibre_family(sim):
    """(theta, centroids) -> (T, [dT/dratio]): horizontal fibres in tissue 1, the identity (tangent 0) elsewhere."""
    def family(theta, centroids):
        e = np.zeros((len(centroids), 2))
        e[sim._labels() == 1, 0] = 1.0                 # a zero direction gives (I, 0)
        T, dT = tensor_from_fibres(e, theta["ratio"], derivative=True)
        return T, [dT]
    return family


def make_sim(D, rho, ratio):
    mesh = fenics.RectangleMesh(fenics.Point(-5, -5), fenics.Point(5, 5), 16, 16)
    labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1), fenics.FunctionSpace(mesh, "DG", 1))
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                               proliferation=rho, E=0.001, poisson=0.4, sim_time=5, sim_time_step=1)
    sim.set_diffusion_tensor_family(fibre_family(sim), dict(ratio=ratio), ("ratio",))
    return sim


def thresh(c, level, smooth=0.1):
    return 0.5 * (np.tanh((c - level) / smooth) + 1.0)


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_aniso_fit_")
truth = make_sim(*TRUTH)
truth.run(save_method=None, plot=False, output_dir=out)
c_end = truth.solution.components[1].copy()
truth.close()

terms = lambda sim, n_steps: [dict(step=n_steps, kind="c_thresh", level=lv, target=thresh(c_end, lv), smooth=0.1)
                              for lv in (0.16, 0.8)]
sim = make_sim(*START)
rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out), tensor_controls=("ratio",))
res = minimize(rf, list(START), bounds=([0.005, 0.005, 1.0], [0.5, 0.5, 20.0]),
               options={"maxiter": 200, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16)
print("  eval        D          rho        ratio          J        |dJ/dm|")
for k, (m, J, gn) in enumerate(rf.history):
    print("  %4d   %.8f  %.8f  %.8f   %.3e   %.2e" % (k, m[0], m[1], m[2], J, gn))
print("fitted D = %.8f, rho = %.8f, ratio = %.6f (truth %g, %g, %g) after %d L-BFGS-B iterations, %d forward + backward runs "
      "(J = %.3e)" % (res.x[0], res.x[1], res.x[2], *TRUTH, res.nit, rf.evaluations, res.fun))
sim.close()
