"""
Images in the DEFORMED configuration: a brain-like coupled run whose recorded steps stay on the device, then what the
reference's optimisation workflow builds with vtk and ANTs (ImageBasedOptimizationBase._create_deformed_image,
glimslib/optimization_workflow/image_based_optimization.py:876-941): the label map on the undeformed and on the displaced
mesh, the displacement image and its inverse, and an atlas-like image as the deformed anatomy would show it -- plus the tumour
concentration where an MR image would see it, at x = X + u(X).

The voxel grid is located once in the mesh displaced by the step's displacement (a deformed sampler); every image of that
step is then a gather on the device.

  python examples/deformed_images_3D.py [output_dir] [n_points of the unstructured mesh, default 100000] [voxel in mm, default 2]
"""
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import fenics_local as fenics
from glimslib_amd import workloads
from glimslib_amd.simulation import TumorGrowthBrain
from glimslib_amd.utils.data_io import Image

logging.basicConfig(format='%(levelname)s:%(message)s', level=logging.WARNING)
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "output_deformed_3D")
n_points = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
voxel = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0
os.makedirs(out_dir, exist_ok=True)


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


wl = workloads.config_brain_like(n_points)
mesh = wl.mesh
sim = TumorGrowthBrain(mesh)
sim.setup_global_parameters(subdomains=wl.cell_label, domain_names={1: 'CSF', 3: 'WM', 2: 'GM', 4: 'Ventricles'},
                            boundaries={'boundary_all': Boundary()},
                            dirichlet_bcs={'clamped_0': {'bc_value': fenics.Constant((0.0, 0.0, 0.0)),
                                                         'named_boundary': 'boundary_all', 'subspace_id': 0}})
iv = fenics.Expression('exp(-a*pow(x[0]-x0, 2) - a*pow(x[1]-y0, 2) - a*pow(x[2]-z0,2))', degree=1, a=0.005, x0=118,
                       y0=-109, z0=72)
sim.setup_model_parameters(iv_expression={0: fenics.Constant((0., 0., 0.)), 1: iv}, sim_time=20, sim_time_step=1,
                           E_GM=3000E-6, E_WM=3000E-6, E_CSF=1000E-6, E_VENT=1000E-6, nu_GM=0.45, nu_WM=0.45, nu_CSF=0.45,
                           nu_VENT=0.3, D_GM=0.01, D_WM=0.05, rho_GM=0.05, rho_WM=0.05, coupling=0.15)
sim.run(keep_nth=10, save_method=None, plot=False, output_dir=out_dir, results_on_device=True)

# an atlas-like reference image on the voxel grid: here the tissue labels themselves, smoothed into grey values
lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
size = np.floor((hi - lo) / voxel).astype(int)
origin, spacing = lo + 0.5 * voxel, (voxel, voxel, voxel)
labels = sim.label_image(origin=origin, spacing=spacing, size=size)
atlas = Image(np.take(np.array([0.0, 0.2, 0.6, 1.0, 0.1]), labels.array), origin, spacing)

last = sim.results.get_recording_steps()[-1]
t0 = time.perf_counter()
images = sim.create_deformed_images(last, atlas, output_dir=out_dir)          # label_img_orig, labels_warped, displacement_img,
c_def = sim.sample_image('concentration', last, like=atlas, deformed=True)    # displacement_img_inv, image_warped as .mha
c_ref = sim.sample_image('concentration', last, like=atlas)
c_def.write(os.path.join(out_dir, "concentration_deformed_%05d.mha" % last), compressed=True)
print("deformed images of recording step %d: %.2f s" % (last, time.perf_counter() - t0))

moved = (images['labels_warped'].array != images['label_img_orig'].array).sum()
inv = images['displacement_img_inv'].array
print("voxels whose label changes under the deformation: %d of %d" % (moved, labels.array.size))
print("largest |X(x) - x|: %.3f mm; largest |u|: %.3f mm" % (np.nanmax(np.linalg.norm(inv, axis=-1)),
                                                           np.nanmax(np.linalg.norm(images['displacement_img'].array, axis=-1))))
both = ~np.isnan(c_def.array) & ~np.isnan(c_ref.array)
print("largest change of the concentration image: %.3e" % np.abs(c_def.array - c_ref.array)[both].max())
print("written:", sorted(os.listdir(out_dir)))
sim.close()
