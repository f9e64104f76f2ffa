"""
Derived fields where the results live: a brain-like coupled run whose recorded steps stay on the device, then the pressure and
the von Mises stress of every recorded step as .mha images on a voxel grid, and the whole derived field set of the last step
as a .vtu file.

The reference projects these fields with fenics.project per field (PostProcess*, glimslib/simulation_helpers/helper_classes.py)
and makes images voxel by voxel (create_image_from_fenics_function); here a step is derived on the device (Handle.derive) and
sampled from the result's device buffer: nothing nodal crosses to the host on the way to an image.

  python examples/postprocess_images_3D.py [output_dir] [n_points of the unstructured mesh, default 100000] [voxel in mm, default 2]
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

logging.basicConfig(format='%(levelname)s:%(message)s', level=logging.WARNING)
out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "output_postprocess_3D")
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
                           nu_VENT=0.3, D_GM=0.01, D_WM=0.05, rho_GM=0.05, rho_WM=0.05, coupling=0.1)
sim.run(keep_nth=5, save_method=None, plot=False, output_dir=out_dir, results_on_device=True)

lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
size = np.floor((hi - lo) / voxel).astype(int)
grid = dict(origin=lo + 0.5 * voxel, spacing=(voxel, voxel, voxel), size=size)
t0 = time.perf_counter()
for step in sim.results.get_recording_steps():
    p = sim.sample_image('pressure', step, **grid)                 # derived and sampled on the device
    vm = sim.sample_image('van_mises_stress', step, **grid)        # the same step: no second elastic solve, the stress is cached
    p.write(os.path.join(out_dir, "pressure_%05d.mha" % step), compressed=True)
    vm.write(os.path.join(out_dir, "van_mises_stress_%05d.mha" % step), compressed=True)
    print("recording step %2d: pressure %.3e .. %.3e, max von Mises stress %.3e" % (
        step, np.nanmin(p.array), np.nanmax(p.array), np.nanmax(vm.array)))
print("images: %.2f s, %s" % (time.perf_counter() - t0, sim._backend.derive_info()))

pp = sim.init_postprocess(out_dir)                                 # steps recorded on the device take the device path
print("written:", pp.save_all(selection=slice(-1, None)))
sim.close()
