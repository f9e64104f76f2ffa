"""
Parameter fitting on the device adjoint -- the counterpart of the reference's optimisation loop
(optimization_workflow/image_based_optimization.py:660-767): a misfit J of the simulated fields, wrapped in
``fenics.ReducedFunctional`` with the tissue parameters as controls (:700-708), handed with dJ/dm to scipy's L-BFGS-B
(:710-722).

Here J and dJ/dm come from one forward run with ``record_adjoint=True`` and one backward sweep on the GPU
(``sim.adjoint_gradient``); there is no CPU gradient.  The controls follow the reference's forward entry
points: ``TumorGrowthBrain.run_for_adjoint*`` (simulation_tumor_growth_brain_quad.py:127-210) with 2 / 3 / 4 / 5 parameters,
``TumorGrowth.run_for_adjoint2`` / ``run_for_adjoint`` (simulation_tumor_growth.py:142-170) with 2 / 3.
"""
from __future__ import annotations

import numpy as np

__all__ = ["ReducedFunctional", "minimize", "parameter_map"]

BRAIN_NAMES = ("D_WM", "D_GM", "rho_WM", "rho_GM", "coupling")
TUMOR_NAMES = ("diffusion", "proliferation", "coupling")
# every parameter of TumorGrowthBrain.adjoint_gradient, for ReducedFunctional(names=...)
BRAIN_CONTROLS = BRAIN_NAMES + ("E_GM", "E_WM", "E_CSF", "E_VENT", "nu_GM", "nu_WM", "nu_CSF", "nu_VENT")


def parameter_map(n_params, brain=True):
    """
    (names, P): the model parameters ``names`` are ``P @ m`` for the control vector m (linear maps of the reference:
    2 parameters (D_WM, rho) with D_GM = 0.2 D_WM, rho_GM = rho_WM; 3: + coupling; 4: (D_WM, D_GM, rho, coupling);
    5: all five).  Parameters not in ``names`` keep their values.
    """
    if brain:
        P = {2: [[1, 0], [0.2, 0], [0, 1], [0, 1], [0, 0]],
             3: [[1, 0, 0], [0.2, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1]],
             4: [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1]],
             5: np.eye(5)}.get(int(n_params))
        if P is None:
            raise ValueError("TumorGrowthBrain controls: 2, 3, 4 or 5 parameters")
        P = np.asarray(P, dtype=np.float64)
        if n_params == 2:
            return BRAIN_NAMES[:4], P[:4]   # the 2-parameter variant leaves the coupling alone
        return BRAIN_NAMES, P
    if int(n_params) not in (2, 3):
        raise ValueError("TumorGrowth controls: 2 (diffusion, proliferation) or 3 (+ coupling) parameters")
    return TUMOR_NAMES[:n_params], np.eye(int(n_params))


class ReducedFunctional:
    """
    J(m) and dJ/dm(m) for a simulation ``sim`` (TumorGrowth / TumorGrowthBrain) and the controls of ``parameter_map``, or,
    with ``names`` (a tuple of TumorGrowthBrain parameter names, BRAIN_CONTROLS), exactly those parameters (P = identity):
    ``names=('E_WM', 'coupling')`` makes m = (E_WM, coupling).  On a TumorGrowth simulation ``names`` picks among
    ('diffusion', 'proliferation', 'coupling'), e.g. ``names=('coupling', 'diffusion')`` for a fit to a deformed image.

    ``elastic_hessian=True`` (one GPU) lets ``hessian`` / ``hessian_matrix`` -- and so ``minimize(method='trust-constr')`` --
    cover E_* / nu_* controls through ``sim.adjoint_hessian(..., elastic=True)``, the exact second-order elastic adjoint; by
    default such controls are first order only and the Hessian raises.

    A term list with a deformed image term (``sim.image_term(..., deformed=True)``) is first order only: ``hessian`` and
    ``hessian_matrix`` raise NotImplementedError.  So is a list with a sharp volume term (``sim.volume_term(kind='sharp')``);
    smooth and mass volume terms have their second order.

    ``iv_controls=('x0', 'y0')`` appends SEED controls: user parameters of the concentration's initial-value ``Expression``
    (attributes, see ``fenics_local.Expression``), e.g. the seed position of ``exp(-a |x - x_seed|^2)``.  The control vector
    is the model parameters followed by the initial-value parameters; dJ/dp = dJ/dc0 . dc0/dp with dJ/dc0 from the adjoint and
    dc0/dp the central difference of the NODAL INTERPOLANT alone (two evaluations of the Expression on the host, never of the
    simulation; step 1e-6 max(1, |p|)).  Seed controls are first order only (``hessian`` / ``hessian_matrix`` raise
    NotImplementedError) and need bounds of their own in ``minimize`` (``bounds=(lo_list, hi_list)``: a position is not a
    rate).  A seed is only identifiable with a centre-of-mass term (``sim.com_term``) or an image as data.  A list with a
    centre-of-mass term is first order only as well.

    ``tensor_controls=('ratio',)`` appends TENSOR controls: parameters of the simulation's tensor family
    (``sim.set_diffusion_tensor_family``; ValueError for a name the family does not have).  The control vector is the model
    parameters, then ``iv_controls``, then the tensor controls -- vectors without them are prefixes.  dJ/dtheta_k is the sum
    over the labels of ``sim.adjoint_gradient(...)['tensor'][name]``, from the same backward sweep as the rest.  Tensor
    controls are first order only (``hessian`` / ``hessian_matrix`` raise NotImplementedError before any device work; use
    L-BFGS-B) and need bounds of their own in ``minimize`` (``bounds=(lo_list, hi_list)``: a ratio is not a rate).

    ``terms_builder(sim, n_steps)`` returns the misfit terms (see ``Handle.adjoint_gradient``) once the forward run of m has
    taken ``n_steps`` steps.  The last m is cached: scipy's ``fun`` / ``jac`` pair for one m costs one forward and one
    backward run.
    """

    def __init__(self, sim, n_params, terms_builder, run_kwargs=None, names=None, elastic_hessian=False, iv_controls=(),
                 tensor_controls=()):
        self.sim = sim
        self.tensor_controls = tuple(tensor_controls)
        if self.tensor_controls:
            have = tuple(getattr(sim, "tensor_params", None) or ())
            bad = [n for n in self.tensor_controls if n not in have]
            if bad or len(set(self.tensor_controls)) != len(self.tensor_controls):
                raise ValueError("tensor_controls: distinct parameter names of the simulation's tensor family %s expected "
                                 "(sim.set_diffusion_tensor_family), got %s" % (have, self.tensor_controls))
        self.iv_controls = tuple(iv_controls)
        if len(set(self.iv_controls)) != len(self.iv_controls):
            raise ValueError("iv_controls: distinct parameter names expected, got %s" % (self.iv_controls,))
        if self.iv_controls:
            iv = self._iv_expression()
            bad = [n for n in self.iv_controls if n not in iv._param_names]
            if bad:
                raise ValueError("iv_controls: %s are no user parameters of the concentration's initial-value Expression "
                                 "(it has %s)" % (bad, tuple(iv._param_names)))
        self.elastic_hessian = bool(elastic_hessian)
        self.n_params = int(n_params)
        self.brain = hasattr(sim.params, "D_WM")
        if names is None:
            self.names, self.P = parameter_map(self.n_params, self.brain)
        else:
            names = tuple(names)
            allowed = BRAIN_CONTROLS if self.brain else TUMOR_NAMES   # (TumorGrowth: e.g. names=('coupling', 'diffusion'))
            bad = [n for n in names if n not in allowed]
            if bad or len(set(names)) != len(names) or len(names) != self.n_params:
                raise ValueError("names: %d distinct parameters of %s expected, got %s" % (self.n_params, allowed, names))
            self.names, self.P = names, np.eye(len(names))
        self.terms_builder = terms_builder
        self.run_kwargs = dict(keep_nth=10 ** 9, save_method=None, clear_all=False, plot=False)
        self.run_kwargs.update(run_kwargs or {})
        self._m = None
        self._J = None
        self._dJ = None
        self._H = None
        self._n_steps = None
        self.evaluations = 0
        self.hessian_calls = 0
        self.history = []   # (m, J, |dJ/dm|) per evaluation (the reference's eval_cb_post / derivative_cb_post)

    def _iv_expression(self):
        """The initial-value Expression of the concentration (subspace 1 of the coupled space)."""
        params = self.sim.params
        iv = params.get_iv(1) if params._functionspace.has_subspaces else params.get_iv(None)
        if iv is None or not hasattr(iv, "_param_names"):
            raise ValueError("iv_controls need an initial-value Expression with user parameters for the concentration")
        return iv

    def iv_derivative(self, name):
        """dc0/dp [n_nodes] for the initial-value parameter `name` at its present value: the central difference of the nodal
        interpolant with step h = 1e-6 max(1, |p|) (truncation h^2 / 6 times the third derivative of c0 by p and rounding
        eps / h, both about 1e-10 for a Gaussian of unit width).  The parameter is left as it was."""
        iv = self._iv_expression()
        X = np.asarray(self.sim.mesh.points, dtype=np.float64)
        p = float(getattr(iv, name))
        h = 1e-6 * max(1.0, abs(p))
        try:
            setattr(iv, name, p + h)
            up = np.asarray(iv(X), dtype=np.float64).reshape(-1)
            setattr(iv, name, p - h)
            dn = np.asarray(iv(X), dtype=np.float64).reshape(-1)
        finally:
            setattr(iv, name, p)
        return (up - dn) / (2.0 * h)

    def _set_params(self, m):
        n_iv = self.n_params + len(self.iv_controls)
        for name, v in zip(self.tensor_controls, m[n_iv:]):
            self.sim.tensor_params[name] = float(v)
        m, seed = m[:self.n_params], m[self.n_params:n_iv]
        if self.iv_controls:
            iv = self._iv_expression()
            for name, v in zip(self.iv_controls, seed):
                setattr(iv, name, float(v))
        q = self.P @ m
        for name, v in zip(self.names, q):
            setattr(self.sim.params, name, float(v))

    def _model_gradient(self, g):
        """dJ/d(names) from sim.adjoint_gradient's dict: per-label arrays sum over the labels (one scalar per name)."""
        return np.array([float(np.sum(g[name])) for name in self.names])

    def _evaluate(self, m):
        m = np.array(m, dtype=np.float64).reshape(-1)
        n_controls = self.n_params + len(self.iv_controls) + len(self.tensor_controls)
        if m.shape != (n_controls,):
            raise ValueError("expected %d controls, got %s" % (n_controls, m.shape))
        if self._m is not None and np.array_equal(m, self._m):
            return
        self._set_params(m)
        self.sim.run(record_adjoint=True, **self.run_kwargs)
        n_steps = int(self.sim._backend.stats()["steps"])
        g = self.sim.adjoint_gradient(self.terms_builder(self.sim, n_steps))
        self._m, self._J = m, float(g["J"])
        self._dJ = self.P.T @ self._model_gradient(g)
        if self.iv_controls:
            dc0 = np.asarray(g["c0"], dtype=np.float64).reshape(-1)
            self._dJ = np.concatenate([self._dJ, [float(dc0 @ self.iv_derivative(name)) for name in self.iv_controls]])
        if self.tensor_controls:
            self._dJ = np.concatenate([self._dJ, [float(np.sum(g["tensor"][name])) for name in self.tensor_controls]])
        self._H, self._n_steps = None, n_steps
        self.evaluations += 1
        self.history.append((m.copy(), self._J, float(np.linalg.norm(self._dJ))))

    def __call__(self, m):
        self._evaluate(m)
        return self._J

    def derivative(self, m):
        self._evaluate(m)
        return self._dJ.copy()

    def _model_directions(self):
        """The n_params directions P e_j in the simulation's adjoint_hessian keys."""
        if not self.elastic_hessian and any(n.startswith(("E_", "nu_")) for n in self.names):
            raise ValueError("ReducedFunctional.hessian: E / nu controls %s are first order only (the Hessian covers D, rho "
                             "and the coupling)" % [n for n in self.names if n.startswith(("E_", "nu_"))])
        key = (lambda n: n) if self.brain else {"diffusion": "diffusion", "proliferation": "proliferation",
                                                 "coupling": "coupling"}.get
        return [{key(name): float(v) for name, v in zip(self.names, self.P[:, j]) if v != 0.0}
                for j in range(self.n_params)]

    def hessian_matrix(self, m):
        """P^T H P at m: all n_params directions in one Hessian call (after the forward run of m, shared with ``__call__``
        and ``derivative``); cached with m."""
        if self.tensor_controls:
            raise NotImplementedError("ReducedFunctional.hessian: tensor controls %s are first order only; use a "
                                      "first-order method (L-BFGS-B)" % (self.tensor_controls,))
        if self.iv_controls:
            raise NotImplementedError("ReducedFunctional.hessian: initial-value controls %s are first order only; use a "
                                      "first-order method (L-BFGS-B)" % (self.iv_controls,))
        dirs = self._model_directions()
        self._evaluate(m)
        if self._H is None:
            terms = self.terms_builder(self.sim, self._n_steps)
            if any(t.get("kind") == "obs_com" for t in terms):
                raise NotImplementedError("ReducedFunctional.hessian: second order of a centre-of-mass term is not built; "
                                          "use a first-order method (L-BFGS-B)")
            if any(t.get("deformed") and t.get("kind") == "obs_volume" for t in terms):
                raise NotImplementedError("ReducedFunctional.hessian: second order through the displacement of a deformed "
                                          "volume term is not built; use a first-order method (L-BFGS-B)")
            if any(t.get("deformed") for t in terms):
                raise NotImplementedError("ReducedFunctional.hessian: second order through the location of a deformed image "
                                          "term is not built; use a first-order method (L-BFGS-B)")
            if any(t.get("kind") == "obs_volume" and t.get("observable") == "sharp" for t in terms):
                raise NotImplementedError("ReducedFunctional.hessian: a sharp volume term is piecewise smooth, with jumps in "
                                          "its second derivative; use volume_term(kind='smooth') or a first-order method")
            if self.elastic_hessian:
                _, hv = self.sim.adjoint_hessian(terms, dirs, elastic=True)
            else:
                _, hv = self.sim.adjoint_hessian(terms, dirs)
            H = np.array([[float(np.sum(h[name])) for name in self.names] for h in hv]).T   # column j = H P e_j
            self._H = self.P.T @ H
            self.hessian_calls += 1
        return self._H.copy()

    def hessian(self, m, dm):
        """The Hessian action P^T H P dm at m (fenics.ReducedFunctional.hessian; scipy's ``hessp``)."""
        return self.hessian_matrix(m) @ np.asarray(dm, dtype=np.float64).reshape(-1)


def minimize(rf, m0, bounds=(0.005, 0.5), method="L-BFGS-B", tol=1e-6, options=None):
    """scipy.optimize.minimize on ``rf`` with ``jac=rf.derivative`` and the reference's defaults (bounds 0.005 .. 0.5 on
    every control, L-BFGS-B, tol 1e-6, gtol 1e-6; image_based_optimization.py:710-722).  method='trust-constr' also gets
    ``hessp=rf.hessian``, the second-order adjoint.  ``bounds`` is one (lo, hi) pair for every control or per-control
    ``(lo_list, hi_list)``; with ``iv_controls`` give the latter: the seed controls need bounds of their own (the box the
    seed may lie in) -- the default rate bounds would pin a position to 0.005 .. 0.5.  The same holds with
    ``tensor_controls`` (ValueError otherwise): a ratio is not a rate."""
    from scipy.optimize import minimize as _minimize
    m0 = np.asarray(m0, dtype=np.float64)
    if getattr(rf, "tensor_controls", ()) and np.ndim(bounds[0]) == 0:
        raise ValueError("minimize: tensor controls %s need bounds of their own, bounds=(lo_list, hi_list)"
                         % (rf.tensor_controls,))
    opts = {"disp": False, "gtol": 1e-6}
    opts.update(options or {})
    bnds = [tuple(bounds)] * len(m0) if np.ndim(bounds[0]) == 0 else list(zip(*bounds))
    if method.lower() == "trust-constr":
        return _minimize(rf, m0, jac=rf.derivative, hessp=rf.hessian, bounds=bnds, method=method, tol=tol, options=opts)
    return _minimize(rf, m0, jac=rf.derivative, bounds=bnds, method=method, tol=tol, options=opts)
