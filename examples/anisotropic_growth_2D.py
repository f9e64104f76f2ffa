"""Anisotropic diffusion on a 2-D two-tissue mesh: a fibre field in tissue A (x >= 0) makes the flux D * T grad c with
T = I + (ratio - 1) e e^T, scaled to trace 2 (data_io.tensor_from_fibres); tissue B stays isotropic.

  1. a forward run with and without the field, and the ratio of the tumour's principal second moments in both;
  2. a fit of (D, rho) to T2- / T1-like threshold images of the anisotropic run, the tensor field given -- the tensor is no
     control, it is data (a DTI atlas), and the per-tissue scalar D remains the control of the adjoint gradient.

P1 elements with a strongly anisotropic tensor lose the discrete maximum principle: small negative concentrations are possible
away from the tumour ("Anisotropic diffusion")."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import fenics_local as fenics  # noqa: E402
from glimslib_amd.optimization import ReducedFunctional, minimize  # noqa: E402
from glimslib_amd.simulation import TumorGrowth  # noqa: E402
from glimslib_amd.utils.data_io import tensor_from_fibres  # noqa: E402

RATIO = 6.0   # diffusion along the fibres relative to across them


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def fibre_tensors(sim):
    """A callable of the cell centroids: horizontal fibres in tissue 1, the identity elsewhere."""
    def field(centroids):
        labels = sim._labels()
        e = np.zeros((len(centroids), 2))
        e[labels == 1, 0] = 1.0                      # a zero direction gives the identity
        return tensor_from_fibres(e, RATIO)
    return field


def make_sim(D, rho, anisotropic=True):
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
                               proliferation=rho, E=0.001, poisson=0.4, sim_time=5, sim_time_step=1,
                               diffusion_tensor=fibre_tensors(sim) if anisotropic else None)
    return sim


def thresh(c, level, smooth=0.1):
    return 0.5 * (np.tanh((c - level) / smooth) + 1.0)


def principal_moments(sim, c):
    """Principal second moments of the concentration about its centre of mass (nodal quadrature), largest first."""
    w = sim._lumped() * c
    x = sim.mesh.points - (w[:, None] * sim.mesh.points).sum(axis=0) / w.sum()
    return np.linalg.eigvalsh(np.einsum('n,na,nb->ab', w, x, x) / w.sum())[::-1]


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_aniso_")
fields = {}
for name, aniso in (("anisotropic", True), ("isotropic", False)):
    sim = make_sim(0.1, 0.1, aniso)
    sim.run(save_method=None, plot=False, output_dir=out)
    fields[name] = sim.solution.components[1].copy()
    m = principal_moments(sim, fields[name])
    print("%-11s run: principal second moments %.4f, %.4f, ratio %.4f, min c = %.2e"
          % (name, m[0], m[1], m[0] / m[1], fields[name].min()))
    sim.close()

c_end = fields["anisotropic"]
terms = lambda sim, n_steps: [dict(step=n_steps, kind="c_thresh", level=lv, target=thresh(c_end, lv), smooth=0.1)
                              for lv in (0.16, 0.8)]
sim = make_sim(0.05, 0.2)
rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out))
res = minimize(rf, [0.05, 0.2], options={"maxiter": 60, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16)
print("fitted D = %.8f, rho = %.8f (truth 0.1, 0.1) after %d L-BFGS-B iterations, %d forward + backward runs (J = %.3e)"
      % (res.x[0], res.x[1], res.nit, rf.evaluations, res.fun))
sim.close()
