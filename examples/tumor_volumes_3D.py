"""
Tumour volumes and centres of mass per tissue where the results live: a coupled two-tissue box run whose recorded steps stay on
the device, then -- per recording step -- the volume of the tumour above the reference's two thresholds (T2 = 0.12, T1 = 0.80)
and its centre of mass, over the whole domain and per tissue, in the reference configuration and in the deformed one
x = X + u (what a segmentation of an image delivers).

The reference computes these with conditional(c >= threshold, 1, 0), assemble(q * dx(subdomain_id)) per step and tissue
(ImageBasedOptimizationBase.compute_from_conc_for_each_time_step, glimslib/optimization_workflow/image_based_optimization.py:
1333-1397); here ONE backend call makes one pass over the cells per recorded step (Handle.observe, csrc/observe.hip): every
cell is clipped at the level set, so the volumes are exact for the P1 field, and nothing nodal crosses to the host.

  python examples/tumor_volumes_3D.py [cells per axis, default 24] [steps, default 12]
"""
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glimslib_amd import fenics_local as fenics
from glimslib_amd.simulation import TumorGrowth

logging.basicConfig(format='%(levelname)s:%(message)s', level=logging.WARNING)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 12


class Boundary(fenics.SubDomain):
    def inside(self, x, on_boundary):
        return on_boundary


mesh = fenics.BoxMesh((0, 0, 0), (40.0, 30.0, 30.0), n, (3 * n) // 4, (3 * n) // 4)
tissue = np.where(mesh.cell_midpoints()[:, 0] < 22.0, 1, 2).astype(np.int32)        # white matter left, grey matter right
sim = TumorGrowth(mesh)
zero = fenics.Constant((0.0, 0.0, 0.0))
sim.setup_global_parameters(subdomains=tissue, domain_names={1: 'WM', 2: 'GM'}, boundaries={'boundary_all': Boundary()},
                            dirichlet_bcs={'clamp': {'bc_value': zero, 'named_boundary': 'boundary_all', 'subspace_id': 0}})
iv = fenics.Expression('exp(-0.05*(pow(x[0]-18, 2) + pow(x[1]-15, 2) + pow(x[2]-15, 2)))', degree=1)
sim.setup_model_parameters(iv_expression={0: zero, 1: iv}, sim_time=n_steps, sim_time_step=1,
                           diffusion={'WM': 0.5, 'GM': 0.1}, proliferation={'WM': 0.2, 'GM': 0.2}, coupling={'WM': 0.15, 'GM': 0.15},
                           E={'WM': 3000e-6, 'GM': 3000e-6}, poisson={'WM': 0.45, 'GM': 0.45})
sim.run(save_method=None, plot=False, results_on_device=True)

for name, threshold in (('T2', 0.12), ('T1', 0.80)):
    for deformed in (False, True):
        vol = sim.compute_from_conc_for_each_time_step(threshold=threshold, computation='volume', deformed=deformed)
        com = sim.compute_from_conc_for_each_time_step(threshold=threshold, computation='com', deformed=deformed)
        print("\n%s (c >= %.2f), %s configuration" % (name, threshold, "deformed" if deformed else "reference"))
        print(vol.merge(com, on='sim_time_step').to_string(index=False, float_format=lambda v: "%.4f" % v))

mass, steps = sim.observe([('mass',)])                                               # int c dx per tissue
print("\ntumour mass per step:", np.round(mass[:, 0, :, 0].sum(axis=1), 3))
print("observe_info:", sim._backend.observe_info())
sim.close()
