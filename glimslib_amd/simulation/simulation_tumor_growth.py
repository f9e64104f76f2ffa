"""
Mechanically-coupled reaction-diffusion model of tumour growth -- counterpart of
glimslib/simulation/simulation_tumor_growth.py:13-173 on the HIP backend.

Equations (reference :110-120), P1 elements, backward Euler, cell-wise constant coefficients:

    F_m  = int sigma(u):eps(v) dx - int sigma(v):(c gamma I) dx - int f.v dx - oint g_u.v ds          (:110-113)
    F_rd = int (c - c_prev) w dx + dt int D grad c.grad w dx - dt int rho c (1 - c) w dx
           - dt int s w dx - dt oint g_c D w ds                                                         (:115-120)

The reference solves F = F_m + F_rd monolithically with SNES + LU each step (:124-130).  F_rd does not contain u,
and F_m is linear in u, so the backend advances c with Newton-PCG on the device and solves the (constant) elastic
system for u only at recorded steps; same fixed point, checked against the monolithic oracle in tests/.
"""
from __future__ import annotations

import logging
import os

import numpy as np

from .. import fenics_local as fenics
from ..fenics_local import Constant, Expression, Function, interpolate_nodal
from ..simulation_helpers import math_linear_elasticity as mle, math_reaction_diffusion as mrd  # noqa: F401
from ..simulation_helpers.helper_classes import DiscontinuousScalar
from .simulation_base import FenicsSimulation
from . import config
from .. import _backend


class SolverDidNotConverge(RuntimeError):
    pass


class HipTimeStepSolver:
    """
    What ``self.solver`` is on this backend: ``solve()`` advances the concentration by one implicit step
    (``solve(k)`` by k steps without returning to Python), raising on non-convergence like DOLFIN's solver does.
    """

    def __init__(self, sim, handle, mechanics):
        self.sim = sim
        self.handle = handle
        self.mechanics = mechanics
        self.steps_done_in_last_call = 0
        self.time_dependent_inputs = sim._has_time_dependent_inputs()
        self._mech_current = False

    def solve(self, n_steps=1):
        before = self.handle.stats()['steps']
        status = self.handle.step(int(n_steps))
        self.steps_done_in_last_call = int(self.handle.stats()['steps'] - before)
        self._mech_current = False
        if status != _backend.GLIMS_OK:
            raise SolverDidNotConverge("libglimship status %d (%s)" % (
                status, {1: "iteration cap reached", 2: "non-finite residual"}.get(status, "?")))

    def update_time_dependent_inputs(self):
        self.sim._upload_loads_and_bcs(self.handle)

    def supports_snapshots(self):
        return hasattr(self.handle, 'snapshot_save')

    def snapshot(self):
        """Record the current step on the device; returns a lazily materialised Function."""
        sid = self.handle.snapshot_save()
        return DeviceSnapshotFunction(self.sim.mesh, self.sim.functionspace.subspaces.names, self, sid)

    def sync_solution(self, with_mechanics=True):
        if self.mechanics and with_mechanics and not self._mech_current:
            st = self.handle.solve_mechanics()
            if st != _backend.GLIMS_OK:
                self.sim.logger.warning("    - displacement solve did not converge (status %d)" % st)
            self._mech_current = True
        c, u = self.handle.get_state(want_u=self.mechanics)
        sol = self.sim.solution
        sol.components[1] = c
        if u is not None:
            sol.components[0] = u.reshape(-1, self.sim.geometric_dimension)


class _LazyComponents(dict):
    """{0: displacement, 1: concentration} of one recorded step, fetched / solved on first access."""

    def __init__(self, solver, sid, dim, n):
        super().__init__()
        self._solver, self._sid, self._dim, self._n = solver, sid, dim, n

    def _materialise(self, k):
        if dict.__contains__(self, k):
            return
        if k == 1:
            dict.__setitem__(self, 1, self._solver.handle.snapshot_load(self._sid))
        elif k == 0:
            if self._solver.mechanics:
                u, st = self._solver.handle.snapshot_mechanics(self._sid)
                self._solver._mech_current = False          # the device's displacement buffer now belongs to this step
                if st != _backend.GLIMS_OK:
                    self._solver.sim.logger.warning("    - displacement solve did not converge (status %d)" % st)
                dict.__setitem__(self, 0, u.reshape(self._n, self._dim))
            else:
                dict.__setitem__(self, 0, np.zeros((self._n, self._dim)))
        else:
            raise KeyError(k)

    def __getitem__(self, k):
        self._materialise(k)
        return dict.__getitem__(self, k)

    def __contains__(self, k):
        return k in (0, 1)

    def keys(self):
        return [0, 1]

    def __iter__(self):
        return iter([0, 1])

    def __len__(self):
        return 2

    def items(self):
        return [(k, self[k]) for k in (0, 1)]

    def values(self):
        return [self[k] for k in (0, 1)]


class DeviceSnapshotFunction(Function):
    """
    A recorded solution that lives on the device (``glims_snapshot_save``): the concentration is downloaded and the
    displacement is SOLVED only when first accessed -- legitimate because the displacement of a step depends on that
    step's concentration alone (one-way coupling, simulation_tumor_growth.py:110-120).  Immutable: ``copy()`` returns
    self, which is what ``Results.add_to_results`` (a deep copy per recorded step in the reference) stores.
    """

    def __init__(self, mesh, names, solver, sid):
        self.mesh = mesh
        self.names = names
        self._name = 'solution_function'
        self.label = 'solution_function'
        self.components = _LazyComponents(solver, sid, mesh.dim, mesh.num_vertices())
        self.snapshot_id = sid

    def copy(self, deepcopy=True):
        return self

    def assign(self, other):
        raise TypeError("device snapshots are immutable")


class TumorGrowth(FenicsSimulation):
    """See module docstring; constructor and parameter names as in the reference (:63, :74-76)."""

    def __init__(self, mesh, time_dependent=True, **kwargs):
        super().__init__(mesh, time_dependent=time_dependent, **kwargs)
        self.units = {'motility': 'm^2/s', 'Emodulus': 'N/m^2', 'none': '', 'growth_rate': '1/s'}

    def _setup_functionspace(self):
        """Mixed space [P1^dim, P1], names {0: 'displacement', 1: 'concentration'} (:67-72)."""
        element = {0: self.geometric_dimension, 1: 1}
        subspace_names = {0: 'displacement', 1: 'concentration'}
        self.functionspace.init_function_space(element, subspace_names)

    def _define_model_params(self):
        self.required_params = ['diffusion', 'coupling', 'proliferation', 'E', 'poisson']
        self.optional_params = []

    # -- anisotropic diffusion ----------------------------------------------------------------------------------
    def setup_model_parameters(self, iv_expression, diffusion_tensor=None, **kwargs):
        """As the base class; ``diffusion_tensor`` (extension): see ``set_diffusion_tensor``."""
        super().setup_model_parameters(iv_expression, **kwargs)
        self.set_diffusion_tensor(diffusion_tensor)

    def set_diffusion_tensor(self, T):
        """A per-cell diffusion tensor (extension; the reference's flux is D grad c): the flux of a cell of tissue t becomes
        D_t * T_cell grad c with the tissue's scalar `diffusion` D_t -- still the control of every gradient and Hessian -- and a
        dimensionless symmetric positive-definite tensor per cell, fixed during a fit.  Takes effect with the next run.

        T: an array [n_cells, d, d]; the packed [n_cells, d (d + 1) / 2] upper triangles row by row (the ITK order); ONE
        [d, d] matrix for every cell; a callable of the cell centroids [n_cells, d] returning one of these; a tensor ``Image``
        with d (d + 1) / 2 components, sampled nearest-voxel at the centroids (cells outside the image or on a NaN voxel get
        the identity, their number is warned about once); None = isotropic.  ``data_io.tensor_from_fibres`` builds the tensors
        of a fibre field.  A non-symmetric or wrongly shaped T raises ValueError here; a tensor that is not positive definite
        is refused by the library when the run sets the problem up.  Clears a family of ``set_diffusion_tensor_family``."""
        from ..utils import data_io
        d = self.geometric_dimension
        nc = len(self.mesh.cells)
        self._tensor_family, self._tensor_names, self.tensor_params, self._diffusion_tangents = None, (), {}, None
        if T is None:
            self._diffusion_tensor = None
            return
        if isinstance(T, data_io.Image):
            T, n_out = data_io.tensor_image_at_points(T, self.mesh.cell_midpoints())
            if n_out:
                self.logger.warning("diffusion tensor image: %d of %d cells lie outside the image or on a NaN voxel and get "
                                    "the identity" % (n_out, nc))
        elif callable(T):
            T = T(self.mesh.cell_midpoints())
        self._diffusion_tensor = _backend.pack_diffusion_tensor(T, nc, d)

    def set_diffusion_tensor_family(self, family, theta, names):
        """A tensor field that depends on up to 4 scalar parameters theta -- an anisotropy ratio, say -- which the adjoint
        differentiates by: ``family(theta_dict, centroids) -> (T, [dT_k])`` returns the field and one tangent field
        dT/dtheta_k per name in ``names``, in that order, each in any form ``set_diffusion_tensor`` takes for an array
        (``data_io.tensor_from_fibres(..., derivative=True)`` builds both for a fibre field).  ``theta``: the start values,
        a dict name -> value or a sequence in the order of ``names``; ``sim.tensor_params`` holds the current values and
        may be changed between runs.  Every ``run()`` builds T and the tangents from them and hands both to the handle;
        ``adjoint_gradient`` then returns dJ/dtheta_k per label under the key 'tensor', and
        ``ReducedFunctional(tensor_controls=...)`` makes them controls.  First order only."""
        names = tuple(names)
        if not 1 <= len(names) <= _backend.DT_MAX_TANGENTS or len(set(names)) != len(names):
            raise ValueError("set_diffusion_tensor_family: 1 .. %d distinct parameter names expected, got %s"
                             % (_backend.DT_MAX_TANGENTS, names))
        if isinstance(theta, dict):
            if set(theta) != set(names):
                raise ValueError("set_diffusion_tensor_family: theta has %s, names are %s" % (tuple(theta), names))
            values = [theta[n] for n in names]
        else:
            values = list(np.atleast_1d(theta))
            if len(values) != len(names):
                raise ValueError("set_diffusion_tensor_family: %d values for %d names" % (len(values), len(names)))
        if not callable(family):
            raise ValueError("set_diffusion_tensor_family: family(theta_dict, centroids) -> (T, [dT_k]) expected")
        before = (getattr(self, '_tensor_family', None), getattr(self, '_tensor_names', ()), getattr(self, 'tensor_params', {}))
        self._tensor_family, self._tensor_names = family, names
        self.tensor_params = {n: float(v) for n, v in zip(names, values)}
        try:
            self._build_tensor_family()
        except Exception:   # a family that does not fit leaves the simulation as it was
            self._tensor_family, self._tensor_names, self.tensor_params = before
            raise

    def _build_tensor_family(self):
        """T and the tangents of the family at sim.tensor_params, packed (the ValueErrors of set_diffusion_tensor)."""
        d, nc = self.geometric_dimension, len(self.mesh.cells)
        names = self._tensor_names
        if set(self.tensor_params) != set(names):
            raise ValueError("sim.tensor_params has %s, the family's names are %s" % (tuple(self.tensor_params), names))
        T, dTs = self._tensor_family({n: float(self.tensor_params[n]) for n in names}, self.mesh.cell_midpoints())
        dTs = list(dTs)
        if len(dTs) != len(names):
            raise ValueError("the tensor family returned %d tangent fields for %d names" % (len(dTs), len(names)))
        self._diffusion_tensor = _backend.pack_diffusion_tensor(T, nc, d)
        self._diffusion_tangents = _backend.pack_diffusion_tensor_tangents(dTs, nc, d)

    def _tensor_gradient(self):
        """{name: dJ/dtheta per label} of the last backward sweep, or None without a family."""
        if getattr(self, '_tensor_family', None) is None:
            return None
        g = self._backend.adjoint_tensor_gradient()
        return {n: g[k] for k, n in enumerate(self._tensor_names)}

    # -- coefficient tables -----------------------------------------------------------------------------------
    def _labels(self):
        return np.asarray(self.subdomains.subdomains.array(), dtype=np.int32)

    @staticmethod
    def _table(param, n_labels):
        if isinstance(param, DiscontinuousScalar):
            return param.table(n_labels)
        if isinstance(param, Constant):
            param = float(param)
        return np.full(n_labels, float(param))

    def _material_tables(self, n_labels):
        p = self.params
        return dict(D=self._table(p.diffusion, n_labels), rho=self._table(p.proliferation, n_labels),
                    gamma=self._table(p.coupling, n_labels), E=self._table(p.E, n_labels),
                    nu=self._table(p.poisson, n_labels))

    # -- loads / BCs --------------------------------------------------------------------------------------------
    def _rd_source(self):
        """The source term s of F_rd ('source_term', :95-96, :119)."""
        return getattr(self, 'source_term', None)

    def _time_objects(self):
        objs = [self._rd_source(), getattr(self, 'source_term', None), getattr(self, 'body_force', None)]
        for attr in ('dirichlet_bcs_dict', 'von_neumann_bcs_dict'):
            objs += [bc.get('bc_value') for bc in getattr(self.bcs, attr, {}).values()]
        return objs

    def _has_time_dependent_inputs(self):
        return any(hasattr(o, 't') for o in self._time_objects() if o is not None)

    def _lumped(self):
        vol = self.mesh.cell_volumes()
        d = self.geometric_dimension
        out = np.zeros(self.mesh.num_vertices())
        np.add.at(out, self.mesh.cells.reshape(-1), np.repeat(vol / (d + 1), d + 1))
        return out

    def _mass_apply(self, s):
        vol = self.mesh.cell_volumes()
        d = self.geometric_dimension
        sl = s[self.mesh.cells]
        loc = (vol / ((d + 1) * (d + 2)))[:, None] * (sl + sl.sum(axis=1, keepdims=True))
        out = np.zeros(self.mesh.num_vertices())
        np.add.at(out, self.mesh.cells.reshape(-1), loc.reshape(-1))
        return out

    def _upload_loads_and_bcs(self, h):
        d = self.geometric_dimension
        dt = float(self.params.sim_time_step)
        n = self.mesh.num_vertices()
        labels = self._labels()
        # reaction-diffusion load: dt * ( int s w dx + oint g D w ds )                       (:119-120)
        rd = np.zeros(n)
        src = self._rd_source()
        if src is not None:
            if isinstance(src, (int, float)) or (isinstance(src, Constant)):
                if float(src) != 0.0:
                    rd += float(src) * self._lumped()
            else:
                rd += self._mass_apply(interpolate_nodal(src, self.mesh, 1))
        if getattr(self.bcs, 'von_neumann_bcs', None):
            Dcell = self._table(self.params.diffusion, int(labels.max()) + 1)[labels]
            rd += self.bcs.implement_von_neumann_bc(Dcell, subspace_id=1)
        h.set_rd_load(dt * rd if np.any(rd != 0.0) else None)
        # mechanical load: int f.v dx + oint g.v ds                                           (:112-113)
        ml = np.zeros(n * d)
        bf = getattr(self, 'body_force', None)
        if bf is not None:
            f = interpolate_nodal(bf, self.mesh, d)
            if np.any(f != 0.0):
                if isinstance(bf, Constant) or not callable(bf):
                    ml += (self._lumped()[:, None] * f).reshape(-1)
                else:
                    ml += np.stack([self._mass_apply(f[:, a]) for a in range(d)], axis=1).reshape(-1)
        if getattr(self.bcs, 'von_neumann_bcs', None):
            ml += self.bcs.implement_von_neumann_bc(None, subspace_id=0)
        h.set_mech_load(ml if np.any(ml != 0.0) else None)
        dofs, vals = self.bcs.dirichlet_dofs(0)
        h.set_dirichlet_u(dofs, vals)
        nodes, cvals = self.bcs.dirichlet_dofs(1)
        h.set_dirichlet_c(nodes, cvals)
        return nodes, cvals

    # -- problem --------------------------------------------------------------------------------------------------
    def _setup_problem(self, u_previous):
        labels = self._labels()
        if labels.min() < 0 or labels.max() > 255:
            raise ValueError("tissue ids must lie in [0, 255]")
        n_labels = int(labels.max()) + 1
        if not hasattr(self, 'body_force'):
            self.body_force = Constant(np.zeros(self.geometric_dimension))
        if not hasattr(self, 'source_term'):
            self.source_term = Constant(0.0)
        mechanics = bool(self.solver_options.get('mechanics', True))
        if self._backend is None:
            from ..parallel import dist_info, DistributedHandle
            dist, rank, world = dist_info()
            if world > 1:
                # SPMD like the reference under mpirun: this rank owns a Morton range of the nodes on its own GPU
                device = int(os.environ.get("GLIMS_FORCE_DEVICE", os.environ.get("LOCAL_RANK", self.device)))
                self._backend = DistributedHandle(self.mesh.points, self.mesh.cells, labels, dist, rank, world, device)
            else:
                self._backend = _backend.Handle(self.mesh.points, self.mesh.cells, labels, device=self.device)
        h = self._backend
        t = self._material_tables(n_labels)
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        if getattr(self, '_tensor_family', None) is not None:
            self._build_tensor_family()   # T and its tangents at the present sim.tensor_params
        h.set_diffusion_tensor(getattr(self, '_diffusion_tensor', None))
        if getattr(self, '_diffusion_tangents', None) is not None or getattr(h, 'n_tangents', 0):
            h.set_diffusion_tensor_tangents(getattr(self, '_diffusion_tangents', None))
        opts = {k: v for k, v in self.solver_options.items() if k != 'mechanics'}
        h.set_options(dt=float(self.params.sim_time_step), **opts)
        self._upload_loads_and_bcs(h)
        h.setup(with_mechanics=mechanics)
        # the initial state is the initial-value function itself (simulation_base.py:253): Dirichlet data constrain the
        # unknown of each step, not u_previous
        h.set_state(u_previous.components[1], u_previous.components[0].reshape(-1) if mechanics else None)
        h.reset_stats()
        if getattr(self, '_record_adjoint', False):
            h.adjoint_record(True)
        elif hasattr(h, 'adjoint_record'):
            h.adjoint_record(False)
        if hasattr(h, 'snapshot_clear'):
            h.snapshot_clear()
        self.solution = self.functionspace.new_function(name='solution_function')
        self.solution.label = 'solution_function'
        self.solution.assign(u_previous)
        self.solver = HipTimeStepSolver(self, h, mechanics)

    # -- images of the results ------------------------------------------------------------------------------------
    def _grid_sampler(self, origin, spacing, size):
        """(key, sampler) of a voxel grid: located in the mesh once per simulation (handle) and grid."""
        h = self._backend
        key = (tuple(float(v) for v in origin), tuple(float(v) for v in spacing), tuple(int(v) for v in size))
        cache = getattr(self, '_image_samplers', None)
        if cache is None or cache[0] is not h:
            cache = self._image_samplers = (h, {})
        if key not in cache[1]:
            cache[1][key] = h.sampler_grid(*key)
        return key, cache[1][key]

    def _deformed_grid_sampler(self, recording_step, origin, spacing, size):
        """(key, sampler) of a voxel grid located in the mesh DISPLACED by the displacement of `recording_step`.  One deformed
        sampler is kept per grid: asking for another step closes it (a 128^3 sampler is about 110 MB of device memory).  A step
        recorded on the device is the snapshot source (one elastic solve, shared with the derived fields of that step); host-
        resident results hand over the step's displacement array."""
        h = self._backend
        if h is None:
            raise RuntimeError("a deformed image needs a run() first (the grid is located in the run's displaced device mesh)")
        if not isinstance(h, _backend.Handle):
            raise NotImplementedError("deformed-configuration images are not available on partitioned runs (the grid would "
                                      "have to be located in every rank's displaced cells); run on one GPU")
        obs = self.results.get_result(recording_step)
        if obs is None:
            raise KeyError("no result for recording step %r" % (recording_step,))
        key = (tuple(float(v) for v in origin), tuple(float(v) for v in spacing), tuple(int(v) for v in size))
        cache = getattr(self, '_deformed_samplers', None)
        if cache is None or cache[0] is not h or cache[1] is not self.results:
            if cache is not None and cache[0] is h:
                for _, old in cache[2].values():
                    old.close()
            cache = self._deformed_samplers = (h, self.results, {})
        ent = cache[2].get(key)
        if ent is not None and ent[0] == recording_step:
            return key, ent[1]
        if ent is not None:
            ent[1].close()
            del cache[2][key]
        field = obs.get_field()
        if isinstance(field, DeviceSnapshotFunction) and self.solver.mechanics:
            sampler = h.sampler_grid(*key, deformed_by=int(field.snapshot_id))
            self.solver._mech_current = False           # the device's displacement buffer now belongs to this step
        else:
            sampler = h.sampler_grid(*key, deformed_by=np.asarray(field.components[0], dtype=np.float64))
        if sampler.n_inverted > 0:
            self.logger.warning("    - recording step %r: the displaced mesh has %d inverted cell(s) (smallest det(I + grad u) = "
                                "%.3e); where it overlaps itself the smallest cell index wins"
                                % (recording_step, sampler.n_inverted, sampler.min_jacobian))
        cache[2][key] = (recording_step, sampler)
        return key, sampler

    def image_term(self, step, image, kind='img_thresh', level=0.0, smooth=1.0, weight=1.0, mask=None,
                   volume_weighted=True, deformed=False, scale=1.0):
        """
        A misfit term that compares the concentration of recorded step `step` with the voxel image `image`
        (utils.data_io.Image) WHERE THE IMAGE WAS MEASURED:  1/2 w sum_voxels q (h(c(x_voxel)) - image)^2  with h the
        identity (kind='img_l2') or the tanh threshold of level / smooth ('img_thresh': a T1- / T2-like segmentation,
        image_based_optimization.py:660-708).  Pass it to adjoint_gradient / adjoint_hessian / ReducedFunctional in the same
        list as the nodal terms.  The grid sampler is the cached one of sample_image; NaN voxels and voxels outside the mesh
        are not observed; `mask` (array like the image, >= 0) weighs the voxels.  With volume_weighted the weight is
        multiplied by the voxel volume, so that J approximates 1/2 w int (h(c) - image)^2 dx and is on the scale of the nodal
        mass-matrix terms.  The same arguments give the same term object, whose arrays the backend uploads once.

        deformed=True: the image shows the DEFORMED configuration x = X + scale u(X) (what sample_image(..., deformed=True)
        produces: a segmentation of a tumour with mass effect).  The term then carries the grid of `image` and no sampler;
        every gradient call locates the voxels in the mesh displaced by the step's own displacement and differentiates
        through that location, so the coupling, E and the Poisson ratio get a gradient from image data alone.  J has a kink
        where a voxel centre crosses a cell face; second order (adjoint_hessian) is not available with such a term, and
        neither are partitioned runs.
        """
        if self._backend is None:
            raise RuntimeError("image_term needs a run() first (the grid is located in the run's device mesh)")
        if getattr(image, 'is_vector', False):
            raise ValueError("image_term takes a scalar image")
        if deformed and not isinstance(self._backend, _backend.Handle):
            raise NotImplementedError("image_term(deformed=True) is not available on partitioned runs (the voxels would have "
                                      "to be located in every rank's displaced cells); run on one GPU")
        if deformed and not self.solver.mechanics:
            raise ValueError("image_term(deformed=True) needs a run with mechanics (the voxels move with the displacement)")
        key = (int(step), id(image), kind, float(level), float(smooth), float(weight), id(mask), bool(volume_weighted),
               bool(deformed), float(scale))
        cache = getattr(self, '_image_terms', None)
        if cache is None or cache[0] is not self._backend:
            cache = self._image_terms = (self._backend, {})
        if key not in cache[1]:
            sampler = None if deformed else self._grid_sampler(image.GetOrigin(), image.GetSpacing(), image.GetSize())[1]
            target = np.ascontiguousarray(image.array, dtype=np.float64).reshape(-1)     # [z, y, x]: the sampler's order
            q = None
            if mask is not None:
                q = np.ascontiguousarray(mask, dtype=np.float64).reshape(-1)
                if q.shape != target.shape:
                    raise ValueError("image_term: the mask has %d voxels, the image %d" % (q.size, target.size))
            w = float(weight) * (float(np.prod(image.GetSpacing())) if volume_weighted else 1.0)
            term = dict(step=int(step), kind=kind, level=float(level), smooth=float(smooth), weight=w, target=target,
                        pweight=q)
            if deformed:
                term.update(deformed=True, scale=float(scale),
                            grid=(tuple(float(v) for v in image.GetOrigin()), tuple(float(v) for v in image.GetSpacing()),
                                  tuple(int(v) for v in image.GetSize())))
            else:
                term['sampler'] = sampler
            cache[1][key] = (term, image, mask)   # (image and mask stay alive: their identity is the key)
        return cache[1][key][0]

    def _displacement_term_checks(self, who):
        if self._backend is None:
            raise RuntimeError("%s needs a run() first (the points are located in the run's device mesh)" % who)
        if not self.solver.mechanics:
            raise ValueError("%s needs a run with mechanics (it observes the displacement)" % who)
        if not isinstance(self._backend, _backend.Handle):
            raise NotImplementedError("%s is not available on partitioned runs; run on one GPU" % who)

    @staticmethod
    def _component_weights(components, dim, who):
        if components is None:
            return None
        cw = tuple(float(v) for v in np.ravel(components))
        if len(cw) != dim:
            raise ValueError("%s: components has %d entries, the mesh %d dimensions" % (who, len(cw), dim))
        return cw

    def displacement_image_term(self, step, image, weight=1.0, mask=None, volume_weighted=True, scale=1.0, components=None):
        """
        A misfit term that compares the displacement of recorded step `step` with a WARP-FIELD image (utils.data_io.Image
        with `dim` channels, e.g. the deformation field of an image registration, image_based_optimization.py:943-978) where
        the image was measured:  1/2 w sum_voxels q sum_a kappa_a (scale u_a(X_voxel) - image_a)^2.  The voxels are points of
        the REFERENCE configuration (the cached grid sampler of sample_image; sample_image('displacement', step) produces
        such an image).  Voxels outside the mesh and voxels with a NaN in an observed component are not observed; `mask`
        (array like one channel of the image, >= 0) weighs the voxels -- mask out where the registration is unreliable;
        `components` are the per-component weights kappa (default 1; (1, 0, 0) observes a midline shift alone); `scale`
        converts the simulated displacement to the image's sign convention and unit.  With volume_weighted the weight is
        multiplied by the voxel volume.  Pass the term to adjoint_gradient / adjoint_hessian / ReducedFunctional with the
        other terms: it is quadratic in u, so second order is exact, also in E and nu (elastic_hessian=True).  The same
        arguments give the same term object, whose arrays the backend uploads once.  Needs a run with mechanics (ValueError);
        partitioned runs raise NotImplementedError.
        """
        who = "displacement_image_term"
        if self._backend is None:
            raise RuntimeError("%s needs a run() first (the grid is located in the run's device mesh)" % who)
        dim = self._backend.dim
        if not getattr(image, 'is_vector', False):
            raise ValueError("%s takes a vector image with %d channels (image_term takes the scalar ones)" % (who, dim))
        if image.GetNumberOfComponentsPerPixel() != dim or image.dim != dim:
            raise ValueError("%s: the image has %d channels on %d axes, the mesh %d dimensions"
                             % (who, image.GetNumberOfComponentsPerPixel(), image.dim, dim))
        self._displacement_term_checks(who)
        cw = self._component_weights(components, dim, who)
        key = ('grid', int(step), id(image), float(weight), id(mask), bool(volume_weighted), float(scale), cw)
        cache = getattr(self, '_displacement_terms', None)
        if cache is None or cache[0] is not self._backend:
            cache = self._displacement_terms = (self._backend, {})
        if key not in cache[1]:
            sampler = self._grid_sampler(image.GetOrigin(), image.GetSpacing(), image.GetSize())[1]
            target = np.ascontiguousarray(image.array, dtype=np.float64).reshape(-1, dim)   # [z, y, x][a]: the sampler's order
            q = None
            if mask is not None:
                q = np.ascontiguousarray(mask, dtype=np.float64).reshape(-1)
                if q.shape[0] != target.shape[0]:
                    raise ValueError("%s: the mask has %d voxels, the image %d" % (who, q.size, target.shape[0]))
            w = float(weight) * (float(np.prod(image.GetSpacing())) if volume_weighted else 1.0)
            term = dict(step=int(step), kind='img_u_l2', sampler=sampler, target=target, pweight=q, weight=w,
                        scale=float(scale), cweight=cw)
            cache[1][key] = (term, image, mask)   # (image and mask stay alive: their identity is the key)
        return cache[1][key][0]

    def landmark_term(self, step, points, displacements, weight=1.0, pweight=None, scale=1.0, components=None):
        """
        displacement_image_term for a POINT SET: `points` [n, dim] are landmarks of the reference configuration,
        `displacements` [n, dim] what was measured there (NaN = not observed), `pweight` [n] optional weights >= 0.
        1/2 w sum_p q_p sum_a kappa_a (scale u_a(X_p) - displacements_pa)^2.  The point sampler is located once per point
        array and simulation; the same arguments give the same term object.
        """
        who = "landmark_term"
        self._displacement_term_checks(who)
        h = self._backend
        dim = h.dim
        cw = self._component_weights(components, dim, who)
        key = ('points', int(step), id(points), id(displacements), float(weight), id(pweight), float(scale), cw)
        cache = getattr(self, '_displacement_terms', None)
        if cache is None or cache[0] is not h:
            cache = self._displacement_terms = (h, {})
        if key not in cache[1]:
            xyz = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, dim)
            target = np.ascontiguousarray(displacements, dtype=np.float64).reshape(-1, dim)
            if target.shape != xyz.shape:
                raise ValueError("%s: %d points, %d displacements" % (who, xyz.shape[0], target.shape[0]))
            q = None
            if pweight is not None:
                q = np.ascontiguousarray(pweight, dtype=np.float64).reshape(-1)
                if q.shape[0] != xyz.shape[0]:
                    raise ValueError("%s: %d points, %d weights" % (who, xyz.shape[0], q.size))
            pcache = getattr(self, '_landmark_samplers', None)
            if pcache is None or pcache[0] is not h:
                pcache = self._landmark_samplers = (h, {})
            if id(points) not in pcache[1]:
                pcache[1][id(points)] = (h.sampler_points(xyz), points)
            term = dict(step=int(step), kind='img_u_l2', sampler=pcache[1][id(points)][0], target=target, pweight=q,
                        weight=float(weight), scale=float(scale), cweight=cw)
            cache[1][key] = (term, points, displacements, pweight)
        return cache[1][key][0]

    def volume_term(self, step, target, threshold=0.12, kind='smooth', smooth=0.01, tissues=None, weight=1.0, deformed=False,
                    scale=1.0):
        """
        A misfit term that compares a tumour VOLUME of recorded step `step` with the number `target`:
        1/2 weight (V - target)^2, V the volume compute_from_conc_for_each_time_step(threshold, 'volume', kind, smooth) reports
        (reference configuration) -- kind 'sharp' (c >= threshold, exact clipping), 'smooth' (the thresh() field of width
        `smooth`) or 'mass' (int c dx, `threshold` unused).  `tissues`: names of that table's columns (the tissue names of
        subdomains.tissue_id_name_map, any case) whose cells are counted; None = the whole domain ('all').  Pass it to
        adjoint_gradient / ReducedFunctional in the same list as nodal and image terms: the backend stores it on the device and
        adds weight (V - target) dV/dc to the backward sweep.  'sharp' is first order only (V is piecewise smooth: its
        second derivative jumps where the level set crosses a mesh node); 'smooth' and 'mass' also serve adjoint_hessian.
        Partitioned runs raise NotImplementedError when the term is used.

        deformed=True: V is the volume of the DEFORMED configuration x = X + scale u(X) of that step, the number
        compute_from_conc_for_each_time_step(deformed=True) reports and the one a scan shows.  Its gradient goes through the
        displacement as well, so such terms carry the coupling, E and nu (parameters a reference-configuration volume gives an
        exactly zero gradient).  A 'sharp' term whose threshold lies below every concentration (threshold=-1) has the
        indicator 1 everywhere: it is the deformed volume of the counted `tissues` themselves -- the volume of a compressed
        neighbouring tissue, such as the ventricles under mass effect.  Needs a run with mechanics (ValueError otherwise) and
        one GPU (NotImplementedError on a partitioned run); first order only (adjoint_hessian raises NotImplementedError).
        With deformed=False the returned dict is the one described above, without further keys.
        """
        return self._measure_term('volume_term', step, float(target), threshold, kind, smooth, tissues, weight, deformed, scale)

    def com_term(self, step, target, threshold=0.12, kind='smooth', smooth=0.01, tissues=None, weight=1.0, deformed=False,
                 scale=1.0):
        """
        A misfit term that compares the CENTRE OF MASS of recorded step `step` with the point `target` = [x, y(, z)]:
        1/2 weight |X - target|^2, X = M / V the centre of mass compute_from_conc_for_each_time_step(threshold, 'com', kind,
        smooth) and compute_com_all report, of the same measure as volume_term (same kind, threshold, smooth, `tissues`,
        deformed and scale, with the same errors).  A volume series fixes how fast a tumour grows, a centre-of-mass series
        where it started and which way it drifts; with deformed=True the centre of mass of x = X + scale u(X) also carries
        the coupling, E and nu.  Pass it to adjoint_gradient / ReducedFunctional in the same list as the other terms.  Where
        the measure is empty at an evaluation (V not > 0: nothing above the threshold yet) the term contributes J = 0 and no
        gradient there, with one RuntimeWarning per term list.  First order only (adjoint_hessian raises
        NotImplementedError); partitioned runs raise NotImplementedError when the term is used.
        """
        x = np.asarray(target, dtype=np.float64).reshape(-1)
        if x.shape != (int(self.mesh.points.shape[1]),):
            raise ValueError("com_term: target has %d entries, the mesh has dimension %d" % (x.size, self.mesh.points.shape[1]))
        term = self._measure_term('com_term', step, 0.0, threshold, kind, smooth, tissues, weight, deformed, scale)
        term.update(kind='obs_com', target=x.copy())
        return term

    def _measure_term(self, who, step, target, threshold, kind, smooth, tissues, weight, deformed, scale):
        """The dict of volume_term / com_term: the query, the counted labels and the configuration."""
        if kind not in _backend.OBSERVE_KINDS:
            raise ValueError("%s: kind must be one of %s" % (who, tuple(_backend.OBSERVE_KINDS)))
        if deformed and self._backend is not None and not isinstance(self._backend, _backend.Handle):
            raise NotImplementedError("%s(deformed=True) is not available on partitioned runs" % who)
        if deformed and not self.solver.mechanics:
            raise ValueError("%s(deformed=True) needs a run with mechanics (the cells move with the displacement)" % who)
        mask = None
        if tissues is not None:
            if isinstance(tissues, str):
                tissues = [tissues]
            n_labels = int(self._labels().max()) + 1
            ids = {str(name).lower(): int(tid) for tid, name in getattr(self.subdomains, 'tissue_id_name_map', {}).items()}
            mask = np.zeros(n_labels, dtype=np.uint8)
            for name in tissues:
                tid = ids.get(str(name).lower())
                if tid is None:
                    raise ValueError("%s: unknown tissue %r (known: %s)" % (who, name, sorted(ids)))
                if tid < n_labels:          # (a tissue that no cell carries counts nothing)
                    mask[tid] = 1
        term = dict(step=int(step), kind='obs_volume', observable=kind, level=float(threshold), smooth=float(smooth),
                    target=float(target), weight=float(weight), labels=mask)
        if deformed:
            term.update(deformed=True, scale=float(scale))
        return term

    DERIVED_IMAGES = ('pressure', 'van_mises_stress', 'total_jacobian', 'growth_induced_jacobian',
                      'concentration_deformed_config', 'log_growth', 'displacement_norm', 'strain_tensor', 'stress_tensor')

    def sample_image(self, subspace_name, recording_step, like=None, origin=None, spacing=None, size=None, fill=np.nan,
                     deformed=False):
        """
        The recorded field `subspace_name` ('concentration' | 'displacement') of `recording_step`, or one of its derived
        fields (DERIVED_IMAGES: the PostProcess fields; tensors as their symmetric components xx, yy, (zz,) xy, (xz, yz) in
        the last axis; a step recorded on the device is derived and sampled there, nothing nodal crosses to the host),
        evaluated on a voxel grid
        -> utils.data_io.Image (array [z,] y, x [, component]; voxels outside the mesh hold `fill`).  The grid is that of
        the Image `like`, or origin / spacing / size (points per axis).  What the reference does voxel by voxel with
        create_image_from_fenics_function (data_io.py:176-225), here one gather on the device: the grid is located in the
        mesh once per simulation and grid, and serves every recording step.  With run(results_on_device=True) the
        concentration goes from its device snapshot to the image without a nodal copy on the host; the displacement through
        the lazy elastic solve of the results.  Partitioned runs: collective, every rank returns the same image.

        deformed=True: the image in the DEFORMED configuration x = X + u(X), what an MR image of the grown tumour shows -- the
        grid is located in the mesh displaced by that step's displacement, so a voxel at x holds the field at the material
        point X(x) that sits there.  One deformed sampler is cached per grid and replaced when another step is asked for;
        a warning is logged when the displaced mesh has inverted cells.  Not available on partitioned runs.
        """
        from ..utils.data_io import _grid_image
        if like is not None:
            origin, spacing, size = like.GetOrigin(), like.GetSpacing(), like.GetSize()
        if origin is None or spacing is None or size is None:
            raise ValueError("sample_image needs `like` or origin, spacing and size")
        h = self._backend
        if h is None:
            raise RuntimeError("sample_image needs a run() first")
        if deformed:
            key, sampler = self._deformed_grid_sampler(recording_step, origin, spacing, size)
        else:
            key, sampler = self._grid_sampler(origin, spacing, size)
        if subspace_name in self.DERIVED_IMAGES:
            if self.results.get_result(recording_step) is None:
                raise KeyError("no result for recording step %r" % (recording_step,))
            pp = getattr(self, '_image_postprocess', None)
            if pp is None or pp._backend is not h or pp._results is not self.results:
                pp = self._image_postprocess = self._make_postprocess(None, None)
            return _grid_image(pp.sample(subspace_name, recording_step, sampler, fill), key[2], key[0], key[1])
        sid = self.functionspace.get_subspace_id(subspace_name)
        obs = self.results.get_result(recording_step)
        if obs is None:
            raise KeyError("no result for recording step %r" % (recording_step,))
        field = obs.get_field()
        if sid == 1 and isinstance(field, DeviceSnapshotFunction) and isinstance(h, _backend.Handle):
            out = sampler.apply('c', snapshot=field.snapshot_id, fill=fill)
        else:
            out = sampler.apply(np.asarray(field.components[sid]), fill=fill)
        return _grid_image(out, key[2], key[0], key[1])

    @staticmethod
    def _grid_of(like, origin, spacing, size, who):
        if like is not None:
            origin, spacing, size = like.GetOrigin(), like.GetSpacing(), like.GetSize()
        if origin is None or spacing is None or size is None:
            raise ValueError("%s needs `like` or origin, spacing and size" % who)
        return origin, spacing, size

    def label_image(self, recording_step=None, like=None, origin=None, spacing=None, size=None, deformed=False, fill=0):
        """
        The cell labels (tissue ids) at the voxels of a grid -> Image: the reference's `label_map` image
        (vtk_utils.resample_to_image of the result mesh, image_based_optimization.py:895-911).  A voxel holds the label of
        the cell the sampler found it in, `fill` outside the mesh.  With deformed=True and a recording step the grid is
        located in the mesh displaced by that step's displacement (the deformed label map); without a step it is the
        undeformed one.  The array is int32 for an integer `fill`, float64 otherwise.
        """
        from ..utils.data_io import _grid_image
        origin, spacing, size = self._grid_of(like, origin, spacing, size, "label_image")
        if self._backend is None:
            raise RuntimeError("label_image needs a run() first")
        if deformed and recording_step is not None:
            key, sampler = self._deformed_grid_sampler(recording_step, origin, spacing, size)
        else:
            key, sampler = self._grid_sampler(origin, spacing, size)
        cells = np.asarray(sampler.cells)
        labels = np.asarray(self._labels())
        integral = float(fill) == int(fill) if np.isfinite(fill) else False
        out = np.full(len(cells), fill, dtype=np.int32 if integral else np.float64)
        found = cells >= 0
        out[found] = labels[cells[found]]
        return _grid_image(out, key[2], key[0], key[1])

    def warp_image(self, image, recording_step, like=None, order='linear', fill=np.nan):
        """
        `image` (utils.data_io.Image, scalar or vector) as the deformed anatomy of `recording_step` would show it, on the grid
        of `like` (default: the image's own):  out(x) = image(X(x)),  X(x) the reference position of the material point that
        the step's displacement carries to x -- the exact inverse of the P1 map X -> X + u_h(X), evaluated on the device
        without building a displacement image.  What the reference does with ANTs and the negated displacement image
        (image_based_optimization.py:927-929).  order: 'linear' | 'nearest'; voxels outside the displaced mesh, and voxels
        whose X falls outside `image`, hold `fill`.
        """
        from ..utils.data_io import _grid_image
        grid = like if like is not None else image
        key, sampler = self._deformed_grid_sampler(recording_step, grid.GetOrigin(), grid.GetSpacing(), grid.GetSize())
        out = sampler.warp(np.asarray(image.array, dtype=np.float64), image.GetOrigin(), image.GetSpacing(), order=order,
                           fill=fill)
        return _grid_image(out, key[2], key[0], key[1])

    def create_deformed_images(self, recording_step, ref_image, output_dir=None):
        """
        The images of the reference's `_create_deformed_image` (image_based_optimization.py:876-941) on the grid of
        `ref_image`, as a dict of Images; written as <name>.mha into `output_dir` when one is given:
          label_img_orig        the cell labels on the undeformed mesh
          labels_warped         the cell labels on the mesh displaced by the step's displacement
          displacement_img      u(X) on the reference frame (NaN outside the mesh)
          displacement_img_inv  X(x) - x on the deformed frame (NaN outside the displaced mesh): the exact inverse of the P1
                                map.  (Deviation: the reference writes -u(X) on the REFERENCE frame, the first-order
                                approximation of this field that ANTs then applies.)
          image_warped          ref_image(X(x)), d-linear: the reference image as the deformed anatomy would show it
        """
        from ..utils.data_io import Image
        o, sp, sz = ref_image.GetOrigin(), ref_image.GetSpacing(), ref_image.GetSize()
        self._deformed_grid_sampler(recording_step, o, sp, sz)      # (the refusals first: no run yet, a partitioned run)
        out = {'label_img_orig': self.label_image(like=ref_image),
               'labels_warped': self.label_image(recording_step, like=ref_image, deformed=True),
               'displacement_img': self.sample_image('displacement', recording_step, like=ref_image)}
        key, sampler = self._deformed_grid_sampler(recording_step, o, sp, sz)
        d = len(sz)
        ax = [float(o[a]) + np.arange(int(sz[a]), dtype=np.float64) * float(sp[a]) for a in range(d)]
        grid = np.stack(np.meshgrid(*ax[::-1], indexing='ij')[::-1], axis=-1)          # [z,] y, x, component
        X = sampler.back_map().reshape(grid.shape)
        out['displacement_img_inv'] = Image(X - grid, o, sp, is_vector=True)
        out['image_warped'] = self.warp_image(ref_image, recording_step)
        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
            for name, img in out.items():
                img.write(os.path.join(output_dir, name + '.mha'))
        return out

    # -- discrete adjoint (the backward half of the reference's adjoint entry points) -----------------------------
    def _adjoint_raw(self, terms, need_dD=True, elastic=False):
        """(J, dD, drho, dgamma, dc0) per tissue label of the run recorded by ``run(record_adjoint=True)``; with elastic=True
        followed by (dE, dnu)."""
        h = self._backend
        if h is None or not hasattr(h, 'adjoint_gradient'):
            raise RuntimeError("adjoint_gradient needs a run(record_adjoint=True) first")
        if need_dD and getattr(self.bcs, 'von_neumann_bcs', None):
            labels = self._labels()
            flux = self.bcs.implement_von_neumann_bc(np.ones(len(labels)), subspace_id=1)
            if np.any(np.asarray(flux) != 0.0):
                raise NotImplementedError("adjoint_gradient: von Neumann data on the concentration scale with D; "
                                          "dJ/dD is not available for such a run")
        return h.adjoint_gradient(terms, elastic=elastic)   # one entry per label of the handle's set_materials

    def adjoint_gradient(self, terms):
        """
        J and dJ/dm of the recorded run for the misfit ``terms`` (see ``Handle.adjoint_gradient``; the counterpart of
        fenics.ReducedFunctional(J, controls).derivative, image_based_optimization.py:700-708).  Returns
        {'J', 'diffusion', 'proliferation', 'coupling', 'E', 'poisson' (per-label arrays: the tables of DiscontinuousScalar),
        'c0'}.  'E' and 'poisson' are 0 unless a term observes the displacement.  With a tensor family
        (``set_diffusion_tensor_family``) the dict gains 'tensor': {name: dJ/dtheta per label}.
        """
        J, dD, drho, dgamma, dc0, dE, dnu = self._adjoint_raw(terms, elastic=True)
        g = {'J': J, 'diffusion': dD, 'proliferation': drho, 'coupling': dgamma, 'E': dE, 'poisson': dnu, 'c0': dc0}
        tensor = self._tensor_gradient()
        if tensor is not None:
            g['tensor'] = tensor
        return g

    def _adjoint_hessian_raw(self, terms, directions, elastic=False):
        """Handle.adjoint_hessian of the recorded run; directions keyed 'D' / 'rho' / 'gamma' / 'c0' (elastic=True: also
        'E' / 'nu')."""
        h = self._backend
        if h is None or not hasattr(h, 'adjoint_hessian'):
            raise RuntimeError("adjoint_hessian needs a run(record_adjoint=True) first")
        if getattr(self.bcs, 'von_neumann_bcs', None):
            flux = self.bcs.implement_von_neumann_bc(np.ones(len(self._labels())), subspace_id=1)
            if np.any(np.asarray(flux) != 0.0):
                raise NotImplementedError("adjoint_hessian: von Neumann data on the concentration scale with D; "
                                          "second derivatives in D are not available for such a run")
        if any(t.get('kind') == 'obs_com' for t in terms):
            raise NotImplementedError("adjoint_hessian: second order of a centre-of-mass term (com_term) is not built; use "
                                      "a first-order method")
        if any(t.get('deformed') and t.get('kind') == 'obs_volume' for t in terms):
            raise NotImplementedError("adjoint_hessian: second order through the displacement of a deformed volume term "
                                      "(volume_term(deformed=True)) is not built; use a first-order method")
        if any(t.get('deformed') for t in terms):
            raise NotImplementedError("adjoint_hessian: second order through the location of a deformed image term "
                                      "(image_term(deformed=True)) is not built; use a first-order method")
        if any(t.get('kind') == 'obs_volume' and t.get('observable') == 'sharp' for t in terms):
            raise NotImplementedError("adjoint_hessian: a sharp volume term (volume_term(kind='sharp')) is piecewise smooth, "
                                      "with jumps in its second derivative; use kind='smooth' or a first-order method")
        if elastic:   # (a partitioned run's DistributedHandle raises NotImplementedError)
            return h.adjoint_hessian_full(terms, directions)
        return h.adjoint_hessian(terms, directions)

    def adjoint_hessian(self, terms, directions, elastic=False):
        """
        Hessian-vector products of J for the recorded run (the counterpart of fenics.ReducedFunctional.hessian), with J and
        the gradient that come with them.  ``directions``: 1 .. 8 dicts keyed like adjoint_gradient's output --
        'diffusion', 'proliferation', 'coupling' (per-label arrays, or a scalar for every label) and 'c0' ([n_nodes]);
        missing keys are 0.  E and poisson are first order only.  Returns (g, hv): g = {'J', 'diffusion', 'proliferation',
        'coupling', 'c0'}, hv = one dict {'diffusion', 'proliferation', 'coupling', 'c0'} per direction.
        elastic=True (one GPU): directions take 'E' and 'poisson' as well (the exact second-order elastic adjoint), and g
        and every hv gain those two keys.
        """
        key = {'diffusion': 'D', 'proliferation': 'rho', 'coupling': 'gamma', 'c0': 'c0'}
        if elastic:
            key.update(E='E', poisson='nu')
        bad = [k for d in directions for k in d if k not in key]
        if bad:
            raise ValueError("adjoint_hessian: directions take %s, got %s" % (tuple(key), bad))
        r = self._adjoint_hessian_raw(terms, [{key[k]: v for k, v in d.items()} for d in directions], elastic=elastic)
        g = {'J': r['J'], 'diffusion': r['D'], 'proliferation': r['rho'], 'coupling': r['gamma'], 'c0': r['c0']}
        hv = [{'diffusion': r['hv_D'][p], 'proliferation': r['hv_rho'][p], 'coupling': r['hv_gamma'][p],
               'c0': r['hv_c0'][p]} for p in range(len(directions))]
        if elastic:
            g.update(E=r['E'], poisson=r['nu'])
            for p, h in enumerate(hv):
                h.update(E=r['hv_E'][p], poisson=r['hv_nu'][p])
        return g, hv

    # -- parameter sweeps (the forward half of the reference's adjoint entry points) -------------------------------
    def run_for_adjoint(self, parameters, output_dir=config.output_dir_simulation_tmp):
        """:142-155 -- update (diffusion, proliferation, coupling) and re-run on the same mesh / space."""
        self.params.diffusion, self.params.proliferation, self.params.coupling = parameters
        self.run(keep_nth=1, save_method=None, clear_all=False, plot=False, output_dir=output_dir)
        return self.solution

    def run_for_adjoint2(self, parameters, output_dir=config.output_dir_simulation_tmp):
        """:157-170"""
        self.params.diffusion, self.params.proliferation = parameters
        self.run(keep_nth=1, save_method=None, clear_all=False, plot=False, output_dir=output_dir)
        return self.solution

    def _make_postprocess(self, output_dir, device):
        from ..simulation_helpers.postprocess import PostProcessTumorGrowth
        if self._backend is None:
            raise RuntimeError("init_postprocess needs a finished run() (the L2 projections run on its device backend)")
        labels = self._labels()
        t = self._material_tables(int(labels.max()) + 1)
        return PostProcessTumorGrowth(self.results, self.params, output_dir=output_dir, backend=self._backend, tables=t,
                                      labels=labels, device=device)

    def init_postprocess(self, output_dir=config.output_dir_simulation_tmp, device=None):
        """:172-173 -- derived fields (stress, pressure, Jacobians ...) of the recorded solutions.  ``device`` (extension):
        None computes the steps that were recorded on the device (run(results_on_device=True), one GPU) there and the others
        in numpy; True sends host-resident results to the device as well; False keeps numpy throughout."""
        self.postprocess = self._make_postprocess(output_dir, device)
        return self.postprocess

    # -- volumes and centres of mass per tissue ------------------------------------------------------------------------------
    def observe(self, queries, steps=None, deformed=False, device=None):
        """
        Measure and first moments of `queries` per tissue label for the recording steps `steps` (default: all) ->
        (array [n_steps, n_q, n_labels, 1 + dim] = (V, M_0 ..), list of steps).  `queries`: (kind[, level[, smooth]]) tuples
        with kind 'mass' (q = c), 'sharp' (q = 1 where c >= level, exact) or 'smooth' (the reference's thresh(): q =
        1/2 (tanh((c - level) / smooth) + 1), degree-7 quadrature); simulation_helpers/observables.py states them in numpy.
        deformed=True integrates over the configuration x = X + u of each step: the volume an image shows.
        Steps recorded on the device (run(results_on_device=True), one GPU) are observed there in ONE backend call -- one cell
        pass per step, the displacement solved lazily on the device where `deformed` asks for it; host-resident steps go
        through numpy unless device=True; device=False and partitioned runs keep numpy throughout.
        """
        from ..simulation_helpers import observables
        h = self._backend
        if h is None:
            raise RuntimeError("observe needs a finished run()")
        qs = observables.normalise_queries(queries)
        steps = list(self.results.get_recording_steps()) if steps is None else [int(s) for s in steps]
        labels = self._labels()
        n_labels = int(labels.max()) + 1
        dim = self.geometric_dimension
        deformed = bool(deformed) and bool(self.solver.mechanics)          # (no mechanics: u = 0)
        on_dev = device is not False and isinstance(h, _backend.Handle)
        out = np.zeros((len(steps), len(qs), n_labels, 1 + dim))
        fields = []
        for s in steps:
            obs = self.results.get_result(s)
            if obs is None:
                raise KeyError("no result for recording step %r" % (s,))
            fields.append(obs.get_field())
        snap = [k for k, f in enumerate(fields) if on_dev and getattr(f, 'snapshot_id', None) is not None]
        if snap:
            res = h.observe(qs, snapshots=[int(fields[k].snapshot_id) for k in snap], deformed=deformed)
            if deformed:
                self.solver._mech_current = False          # the device's displacement buffer now belongs to a recorded step
            if h.last_observe_status != _backend.GLIMS_OK:
                self.logger.warning("    - observe: a displacement solve did not converge (status %d)" % h.last_observe_status)
            out[snap] = res[:, :, :n_labels]
        for k, f in enumerate(fields):
            if k in snap:
                continue
            c = np.asarray(f.components[1], dtype=np.float64)
            u = np.asarray(f.components[0], dtype=np.float64) if deformed else None
            if on_dev and device:
                out[k] = h.observe(qs, c=c, u=u, deformed=deformed)[0][:, :n_labels]
            else:
                out[k] = observables.observe(self.mesh.points, self.mesh.cells, labels, c, qs, n_labels, u=u)
        return out, steps

    def compute_from_conc_for_each_time_step(self, threshold=0.12, computation='volume', kind='sharp', smooth=0.01,
                                             deformed=False, device=None):
        """
        ImageBasedOptimizationBase.compute_from_conc_for_each_time_step (image_based_optimization.py:1333-1397) for this
        simulation: per recording step the tumour volume above `threshold` ('volume') or its centre of mass ('com'), over the
        whole domain and per tissue -> pandas DataFrame with the reference's columns: 'sim_time_step', then 'all' and one
        column per tissue name of subdomains.tissue_id_name_map (lower-cased) for 'volume', 'all_0..', '<name>_0..' for
        'com'.  The centre of mass is NaN where the volume is not > 0 (compute_com).  kind='sharp' integrates
        conditional(c >= threshold, 1, 0) exactly, 'smooth' the thresh() field of width `smooth`, 'mass' gives int c dx
        (`threshold` unused).  `deformed`, `device`: see observe().  The reference's L2 projection of q before the
        per-tissue integrals is left out.
        """
        import pandas as pd
        from ..simulation_helpers import observables
        if computation not in ('volume', 'com'):
            raise ValueError("computation must be 'volume' or 'com'")
        table, steps = self.observe([(kind, threshold, smooth)], deformed=deformed, device=device)
        V, com = observables.totals_and_com(table[:, 0])                   # [n_steps, 1 + n_labels], [.., dim]
        names = [('all', 0)] + [(str(name).lower(), 1 + int(tid)) for tid, name in
                                getattr(self.subdomains, 'tissue_id_name_map', {}).items() if int(tid) + 1 < V.shape[1]]
        cols = {'sim_time_step': steps}
        for name, k in names:
            if computation == 'volume':
                cols[name] = V[:, k]
            else:
                for a in range(com.shape[-1]):
                    cols["%s_%d" % (name, a)] = com[:, k, a]
        return pd.DataFrame(cols)

    def solver_statistics(self):
        return self._backend.stats() if self._backend is not None else {}
