"""Fit WHERE a tumour started together with how fast it grows: (x0, y0, D, rho) of TumorGrowth from tumour volumes and centres of
mass alone.  The reference guesses the seed once from the target's centre of mass (get_seed_from_com,
optimization_workflow/image_based_optimization.py:1165) and never fits it; here the seed position is a control.

Data: the T2-like and T1-like tumour volume and centre of mass (concentration above a threshold; the reference's
compute_from_conc_for_each_time_step(computation='volume' | 'com')) at a few scan dates of a two-tissue run with a known seed.
A volume series fixes how fast the tumour grows, a centre-of-mass series where it started and which way it drifts: each volume
is one term 1/2 w (V - V_obs)^2 (sim.volume_term), each centre of mass one term 1/2 w |X - X_obs|^2 (sim.com_term ->
glims_adjoint_observable_terms3).  V, M and their derivatives are formed on the device inside the backward sweep.

Controls: ReducedFunctional(..., iv_controls=('x0', 'y0')) appends the user parameters x0, y0 of the initial-value Expression
exp(-a |x - x_seed|^2) to the model parameters; dJ/dx0 = dJ/dc0 . dc0/dx0 with dJ/dc0 from the adjoint and dc0/dx0 a central
difference of the nodal interpolant (two evaluations of the Expression on the host).  The seed controls get bounds of their own.
One GPU: volume and centre-of-mass terms are not available on partitioned runs."""
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


def make_sim(x0, y0, D, rho):
    mesh = fenics.RectangleMesh(fenics.Point(-5, -5), fenics.Point(5, 5), 24, 24)
    labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1), fenics.FunctionSpace(mesh, "DG", 1))
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    u0 = fenics.Expression('exp(-a*(pow(x[0]-x0,2)+pow(x[1]-y0,2)))', degree=1, a=0.5, x0=x0, y0=y0)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                               proliferation=rho, E=0.001, poisson=0.4, sim_time=10, sim_time_step=1)
    return sim


out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="glims_fit_seed_")
levels = (0.2, 0.4)          # T2-like (oedema) and T1-like (tumour core) thresholds
scans = (2, 4, 6, 8, 10)     # time steps with a scan
smooth = 0.1
com_weight = 100.0           # the centre of mass moves by tenths while the volumes change by tens
keys = [(lv, k) for lv in levels for k in scans]


def terms(sim, n_steps, data=None):
    """per (threshold, scan) a smooth volume term and a smooth centre-of-mass term; without data: targets 0, to read the
    volumes and centres of mass off the stored terms"""
    res = []
    for lv, k in keys:
        V, X = (0.0, [0.0, 0.0]) if data is None else data[(lv, k)]
        res.append(sim.volume_term(k, V, threshold=lv, kind='smooth', smooth=smooth))
        res.append(sim.com_term(k, X, threshold=lv, kind='smooth', smooth=smooth, weight=com_weight))
    return res


# the synthetic series: the volumes and centres of mass of the true run, as the device integrates them
seed_true, D_true, rho_true = (0.8, 0.4), 0.1, 0.1
truth = make_sim(seed_true[0], seed_true[1], D_true, rho_true)
truth.run(record_adjoint=True, save_method=None, plot=False, output_dir=out)
truth.adjoint_gradient(terms(truth, 10))
data = {}
for i, key in enumerate(keys):
    data[key] = (truth._backend.observable_term_info(2 * i)["V"], truth._backend.observable_term_info(2 * i + 1)["com"].copy())
truth.close()
for lv in levels:
    print("threshold %.2f: " % lv + "  ".join("t=%d V=%.3f X=(%.3f, %.3f)" % ((k, data[(lv, k)][0]) + tuple(data[(lv, k)][1]))
                                              for k in scans))

# the first guess the reference would make: the centre of mass of the first scan as the seed -- here displaced further, to show
# that the fit finds its way back
start = dict(x0=0.2, y0=-0.3, D=0.05, rho=0.2)
sim = make_sim(start["x0"], start["y0"], start["D"], start["rho"])
rf = ReducedFunctional(sim, 2, lambda s, n: terms(s, n, data), run_kwargs=dict(output_dir=out),
                       names=("diffusion", "proliferation"), iv_controls=("x0", "y0"))
# controls: (D, rho, x0, y0); the rates keep the reference's bounds, the seed may lie anywhere in the central box
res = minimize(rf, [start["D"], start["rho"], start["x0"], start["y0"]],
               bounds=([0.005, 0.005, -2.0, -2.0], [0.5, 0.5, 2.0, 2.0]),
               options={"maxiter": 60, "gtol": 1e-14, "ftol": 1e-18}, tol=1e-18)
print("the path of the seed (one line per forward + backward run):")
for m, J, gnorm in rf.history:
    print("  seed (%.6f, %.6f)  D %.6f  rho %.6f  J %.3e  |dJ/dm| %.3e" % (m[2], m[3], m[0], m[1], J, gnorm))
print("fitted seed (%.6f, %.6f) [true (%.1f, %.1f)], D = %.6f, rho = %.6f [true %.1f, %.1f] after %d L-BFGS-B iterations, "
      "%d forward + backward runs (J = %.3e)" % (res.x[2], res.x[3], seed_true[0], seed_true[1], res.x[0], res.x[1], D_true,
                                                 rho_true, res.nit, rf.evaluations, res.fun))
info = sim._backend.observable_term_info(len(keys) * 2 - 1)
print("last centre-of-mass term: %d cells counted, V = %.4f, X = (%.4f, %.4f), empty = %s"
      % (info["counted"], info["V"], info["com"][0], info["com"][1], info["empty"]))
sim.close()
