"""
Fields off their mesh: a brain-like coupled run whose recorded steps stay on the device, written out as a .mha series of
concentration and displacement images on a 1 mm voxel grid, and one field carried onto a second, coarser mesh.

The reference makes such images voxel by voxel (glimslib/utils/data_io.py, create_image_from_fenics_function) and moves
fields between meshes with fenics.LagrangeInterpolator (image_based_optimization.py, interpolate_non_matching); here both are
one sampler: the voxel grid is located in the mesh once and serves every recorded step.

  python examples/export_images_3D.py [output_dir] [n_points of the unstructured mesh, default 100000] [voxel in mm, default 1]
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
from glimslib_amd.utils import data_io

logging.basicConfig(format='%(levelname)s:%(message)s', level=logging.WARNING)
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "output_images_3D")
n_points = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
voxel = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
os.makedirs(out_dir, exist_ok=True)


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


# the unstructured brain-extent mesh of the benchmark (jittered-lattice Delaunay tetrahedra, white matter inside grey matter)
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
                           nu_VENT=0.3, D_GM=0.01, D_WM=0.05, rho_GM=0.05, rho_WM=0.05, coupling=0.1)
sim.run(keep_nth=5, save_method=None, plot=False, output_dir=out_dir, results_on_device=True)

# voxels (1 mm by default) over the mesh's bounding box, voxel centres half a voxel inside
lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
size = np.floor((hi - lo) / voxel).astype(int)
grid = dict(origin=lo + 0.5 * voxel, spacing=(voxel, voxel, voxel), size=size)
t0 = time.perf_counter()
for step in sim.results.get_recording_steps():
    c = sim.sample_image('concentration', step, **grid)            # device snapshot -> image, no nodal copy on the host
    u = sim.sample_image('displacement', step, **grid)             # the step's elastic solve runs when first asked for
    c.write(os.path.join(out_dir, "concentration_%05d.mha" % step), compressed=True)
    u.write(os.path.join(out_dir, "displacement_%05d.mha" % step), compressed=True)
    print("recording step %2d: %s voxels, %d inside the mesh, max c %.4f, max |u| %.4f mm" % (
        step, "x".join(str(v) for v in c.GetSize()), int((~np.isnan(c.array)).sum()), np.nanmax(c.array),
        np.nanmax(np.linalg.norm(u.array, axis=-1))))
print("images: %.2f s" % (time.perf_counter() - t0))

# the last concentration field on a second, coarser mesh of the same domain
last = sim.results.get_solution_function(subspace_id=1, recording_step=max(sim.results.get_recording_steps()))
coarse = workloads.config_brain_like(max(2000, n_points // 8), seed=1).mesh
on_coarse = data_io.interpolate_non_matching(last, coarse)
vals = on_coarse.values()
print("coarse mesh: %d nodes, %d outside the fine mesh, max c %.4f (fine mesh: %.4f)" % (
    coarse.num_vertices(), int(np.isnan(vals).sum()), np.nanmax(vals), np.asarray(last.values()).max()))
data_io.write_vtu(os.path.join(out_dir, "concentration_on_coarse_mesh.vtu"), coarse.points, coarse.cells,
                  point_fields={'concentration': np.nan_to_num(vals)})
sim.close()
