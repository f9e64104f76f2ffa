"""Fit (D, rho) of TumorGrowth to voxel IMAGES -- the reference's comparison of the simulated concentration with thresholded
T1 / T2 segmentations (optimization_workflow/image_based_optimization.py:660-708, thresh() at :1404) -- where the images
were measured: the misfit is a sum over the voxels of a grid that does not align with the mesh, evaluated and differentiated on
the device (sim.image_term -> glims_adjoint_image_terms).  The images are made by a run with D = rho = 0.1 plus image noise;
the fit starts from (0.05, 0.2) and ends with the Laplace covariance of the fitted parameters.

The same script runs partitioned under

    python -m torch.distributed.run --nproc-per-node 2 examples/adjoint_fit_images_2D.py

(one rank per GPU; GLIMS_TRANSPORT=gloo GLIMS_FORCE_DEVICE=0 rehearses it with all ranks on one GPU): every rank holds the
images, the grid's sampler is resolved over the ranks and rank 0 prints the same fit.  The Hessian, and with it the Laplace
covariance, is a single-GPU call and is skipped there."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
world = int(os.environ.get("WORLD_SIZE", "1"))
if world > 1:
    import torch
    import torch.distributed as dist
    forced = os.environ.get("GLIMS_FORCE_DEVICE")
    torch.cuda.set_device(int(forced if forced is not None else os.environ["LOCAL_RANK"]))
    dist.init_process_group(backend="gloo" if forced is not None else "cpu:gloo,cuda:nccl")
rank = dist.get_rank() if world > 1 else 0
say = print if rank == 0 else (lambda *a, **k: None)

from glimslib_amd import fenics_local as fenics  # noqa: E402
from glimslib_amd.optimization import ReducedFunctional, minimize  # noqa: E402
from glimslib_amd.simulation import TumorGrowth  # noqa: E402
from glimslib_amd.utils.data_io import Image  # noqa: E402


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
    return 0.5 * (np.tanh((c - level) / smooth) + 1.0)   # image_based_optimization.py:1404-1407, voxelwise


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_fit_images_")
# voxels of about half the mesh width (10 / 24) on a grid that overhangs the mesh and does not follow its lines
grid = dict(origin=(-5.07, -5.04), spacing=(0.211, 0.213), size=(49, 48))
sigma = 0.01   # image noise
truth = make_sim(0.1, 0.1)
truth.run(save_method=None, plot=False, output_dir=out)
c_img = truth.sample_image('concentration', max(truth.results.get_recording_steps()), **grid)   # NaN outside the mesh
truth.close()
rng = np.random.default_rng(0)
levels = (0.2, 0.4)   # T2-like (oedema) and T1-like (tumour core) outlines
images = [Image(thresh(c_img.array, lv) + sigma * rng.standard_normal(c_img.array.shape), grid['origin'], grid['spacing'])
          for lv in levels]

# one image term per image: uploaded once, compared on the device at every evaluation; NaN voxels are not observed
terms = lambda sim, n_steps: [sim.image_term(n_steps, im, kind='img_thresh', level=lv, smooth=0.1)
                              for im, lv in zip(images, levels)]
sim = make_sim(0.05, 0.2)
rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out))
res = minimize(rf, [0.05, 0.2], options={"maxiter": 30, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16)
say("fitted D = %.6f, rho = %.6f after %d L-BFGS-B iterations, %d forward + backward runs (J = %.3e)"
      % (res.x[0], res.x[1], res.nit, rf.evaluations, res.fun))
_, n_vox, n_obs = sim._backend.image_term_info(0)   # (partitioned: the observed count summed over the ranks)
say("each image: %d voxels, %d observed (inside the mesh)" % (n_vox, n_obs))
if world == 1:
    # Laplace covariance: J is 1/2 |voxel| sum (h - t)^2, so the noise variance per unit of J's weight is sigma^2 / |voxel|
    H = rf.hessian_matrix(res.x)
    cov = sigma ** 2 * float(np.prod(grid['spacing'])) * np.linalg.inv(H)
    sd = np.sqrt(np.diag(cov))
    print("Hessian at the optimum:\n%s" % H)
    print("Laplace covariance:\n%s" % cov)
    print("standard deviations: D %.3e, rho %.3e;  D-rho correlation %.4f" % (sd[0], sd[1], cov[0, 1] / (sd[0] * sd[1])))
sim.close()
if world > 1:
    dist.destroy_process_group()
