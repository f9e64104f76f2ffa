"""Fit (coupling, D) of TumorGrowth to the two kinds of image the reference's inverse problem uses
(optimization_workflow/image_based_optimization.py:660-708): a T2-like threshold image of the concentration and the DISPLACEMENT
image of an image registration (there an ANTs warp field, turned into a nodal function by _reconstruct_deformation_field,
:943-978).  Here the warp field stays an image: sim.displacement_image_term compares it with the simulated displacement at the
voxels where it was measured (glims_adjoint_displacement_image_terms), on a grid that does not align with the mesh, with a disc
around the seed masked out -- inside the tumour a registration is not to be trusted.

The truth is coupling = 0.3, D = 0.1 on two tissues; the fit starts 30 % off in both, by L-BFGS-B.  The term is quadratic in
the displacement, so the Hessian is exact: its inverse at the optimum is the Laplace covariance of the two parameters."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from glimslib_amd import fenics_local as fenics  # noqa: E402
from glimslib_amd.optimization import ReducedFunctional, minimize  # noqa: E402
from glimslib_amd.simulation import TumorGrowth  # noqa: E402
from glimslib_amd.utils.data_io import Image  # noqa: E402


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


def make_sim(coupling, D, n=48):
    mesh = fenics.RectangleMesh(fenics.Point(-5, -5), fenics.Point(5, 5), n, n)
    labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1), fenics.FunctionSpace(mesh, "DG", 1))
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=coupling,
                               proliferation=0.1, E=0.001, poisson=0.4, sim_time=10, sim_time_step=1)
    return sim


def thresh(c, level, smooth=0.1):
    return 0.5 * (np.tanh((c - level) / smooth) + 1.0)   # image_based_optimization.py:1404-1407, voxelwise


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_fit_displacement_image_")
# voxels of about the mesh width on a grid that overhangs the mesh and does not follow its lines
grid = dict(origin=(-5.07, -5.04), spacing=(0.211, 0.213), size=(49, 48))
level, seed, radius = 0.2, (1.0, 0.5), 1.5
truth = make_sim(0.3, 0.1)
truth.run(save_method=None, plot=False, output_dir=out)
last = max(truth.results.get_recording_steps())
conc = truth.sample_image('concentration', last, **grid)          # NaN outside the mesh
warp = truth.sample_image('displacement', last, **grid)           # a vector Image [y, x, component]: the "registration"
truth.close()
t2 = Image(thresh(conc.array, level), grid['origin'], grid['spacing'])
ax = [grid['origin'][a] + grid['spacing'][a] * np.arange(grid['size'][a]) for a in range(2)]
X, Y = np.meshgrid(ax[0], ax[1])                                  # [y, x], as the image arrays
mask = np.where((X - seed[0]) ** 2 + (Y - seed[1]) ** 2 < radius ** 2, 0.0, 1.0)
print("displacement image: up to %.3f in magnitude, %d of %d voxels masked out around the seed"
      % (np.nanmax(np.abs(warp.array)), int((mask == 0).sum()), mask.size))


def terms(sim, n_steps):
    # both are uploaded once and compared on the device at every evaluation; the weight puts the displacement image (|u| about
    # 0.1) on the scale of the threshold image
    return [sim.image_term(n_steps, t2, kind='img_thresh', level=level, smooth=0.1),
            sim.displacement_image_term(n_steps, warp, weight=100.0, mask=mask)]


start = [0.39, 0.07]
sim = make_sim(*start)
rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out), names=('coupling', 'diffusion'))
res = minimize(rf, start, options={"maxiter": 60, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16)
print("fitted coupling = %.6f, D = %.6f (truth 0.3, 0.1; start %.2f, %.2f) after %d L-BFGS-B iterations, %d forward + backward "
      "runs (J %.3e -> %.3e)" % (res.x[0], res.x[1], start[0], start[1], res.nit, rf.evaluations, rf.history[0][1], res.fun))
sid, n_points, n_obs = sim._backend.displacement_image_term_info(0)
print("the displacement image: %d voxels, %d observed (inside the mesh, outside the mask)" % (n_points, n_obs))
H = rf.hessian_matrix(res.x)
cov = np.linalg.inv(0.5 * (H + H.T))
print("Hessian at the optimum:\n%s\nLaplace covariance (for unit noise on the weighted residuals):\n%s\n"
      "standard deviations: coupling %.3e, D %.3e, correlation %.3f"
      % (H, cov, np.sqrt(cov[0, 0]), np.sqrt(cov[1, 1]), cov[0, 1] / np.sqrt(cov[0, 0] * cov[1, 1])))
sim.close()
