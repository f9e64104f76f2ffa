"""
Brain-specific variant -- counterpart of glimslib/simulation/simulation_tumor_growth_brain.py:8-152: the same
equations as TumorGrowth with per-tissue constants for the subdomains named 'CSF', 'WM', 'GM', 'Ventricles'
(and optionally 'outside'), no diffusion / proliferation in CSF and ventricles (:93-104).

Reference quirk q1: with an 'outside' subdomain the reference calls the non-existent
``mrd.compute_expansion`` (:75) and raises AttributeError.  The intended term -- the growth-induced strain with the
global coupling, as in simulation_tumor_growth_brain_quad.py:76 -- is what is implemented here, with the hard-wired
'outside' material E = 10e3, nu = 0.45 (:37-38).

The reference's brain form names its source term ``rd_source_term`` (:46, :104) and carries neither a body force nor
von Neumann terms (':105 No Von Neumann BC implemented here').  Here ``rd_source_term`` is read first (``source_term`` is
accepted as a synonym); body force and Neumann data are honoured when given -- an extension over the reference's brain
form, identical to it when they are absent, as in every bundled script.
"""
from __future__ import annotations

import numpy as np

from ..fenics_local import Constant
from .simulation_tumor_growth import TumorGrowth
from . import config


class TumorGrowthBrain(TumorGrowth):

    def _define_model_params(self):
        self.required_params = ['E_GM', 'E_WM', 'E_CSF', 'E_VENT',
                                'nu_GM', 'nu_WM', 'nu_CSF', 'nu_VENT',
                                'D_GM', 'D_WM',
                                'rho_GM', 'rho_WM',
                                'coupling']
        self.optional_params = []

    def _rd_source(self):
        src = getattr(self, 'rd_source_term', None)
        return src if src is not None else getattr(self, 'source_term', None)

    def _material_tables(self, n_labels):
        p = self.params
        f = lambda v: float(v) if isinstance(v, Constant) or not hasattr(v, '__len__') else float(np.asarray(v))
        tissues = {
            'CSF': dict(D=0.0, rho=0.0, E=f(p.E_CSF), nu=f(p.nu_CSF)),
            'WM': dict(D=f(p.D_WM), rho=f(p.rho_WM), E=f(p.E_WM), nu=f(p.nu_WM)),
            'GM': dict(D=f(p.D_GM), rho=f(p.rho_GM), E=f(p.E_GM), nu=f(p.nu_GM)),
            'Ventricles': dict(D=0.0, rho=0.0, E=f(p.E_VENT), nu=f(p.nu_VENT)),
            'outside': dict(D=0.0, rho=0.0, E=10E3, nu=0.45),
        }
        t = dict(D=np.zeros(n_labels), rho=np.zeros(n_labels), gamma=np.zeros(n_labels),
                 E=np.ones(n_labels), nu=np.full(n_labels, 0.3))
        present = np.unique(self._labels())
        known = {}
        for name, vals in tissues.items():
            tid = self.subdomains.tissue_name_id_map.get(name) if hasattr(self.subdomains, 'tissue_name_id_map') \
                else {v: k for k, v in getattr(self.subdomains, 'tissue_id_name_map', {}).items()}.get(name)
            if tid is None:
                if name != 'outside':
                    self.logger.error("Subdomain '%s' does not exist" % name)
                continue
            known[tid] = name
            if tid < n_labels:
                for k in ('D', 'rho', 'E', 'nu'):
                    t[k][tid] = vals[k]
                t['gamma'][tid] = f(p.coupling)
        missing = [int(l) for l in present if int(l) not in known]
        if missing:
            raise ValueError("cells carry tissue ids %s that TumorGrowthBrain has no material for "
                             "(expected names CSF/WM/GM/Ventricles[/outside] in domain_names)" % missing)
        return t

    def _tissue_id(self, name):
        sd = self.subdomains
        if hasattr(sd, 'tissue_name_id_map'):
            return sd.tissue_name_id_map.get(name)
        return {v: k for k, v in getattr(sd, 'tissue_id_name_map', {}).items()}.get(name)

    def adjoint_gradient(self, terms):
        """J and dJ/d(D_WM, D_GM, rho_WM, rho_GM, coupling, E_GM, E_WM, E_CSF, E_VENT, nu_GM, nu_WM, nu_CSF, nu_VENT) of the
        recorded run (see TumorGrowth.adjoint_gradient).  The fixed 'outside' material is no parameter and has no key."""
        J, dD, drho, dgamma, dc0, dE, dnu = self._adjoint_raw(terms, elastic=True)
        wm, gm = self._tissue_id('WM'), self._tissue_id('GM')
        pick = lambda a, t: float(a[t]) if t is not None and t < len(a) else 0.0
        g = {'J': J, 'D_WM': pick(dD, wm), 'D_GM': pick(dD, gm), 'rho_WM': pick(drho, wm), 'rho_GM': pick(drho, gm),
             # one global coupling constant on every tissue (_material_tables)
             'coupling': float(np.sum(dgamma)), 'c0': dc0}
        for suffix, tissue in (('GM', 'GM'), ('WM', 'WM'), ('CSF', 'CSF'), ('VENT', 'Ventricles')):
            t = self._tissue_id(tissue)
            g['E_' + suffix] = pick(dE, t)
            g['nu_' + suffix] = pick(dnu, t)
        tensor = self._tensor_gradient()   # (a family of set_diffusion_tensor_family: per-label arrays by name)
        if tensor is not None:
            g['tensor'] = tensor
        return g

    _ELASTIC_TISSUES = (('GM', 'GM'), ('WM', 'WM'), ('CSF', 'CSF'), ('VENT', 'Ventricles'))

    def adjoint_hessian(self, terms, directions, elastic=False):
        """Hessian-vector products (see TumorGrowth.adjoint_hessian) with directions keyed by the scalar names D_WM, D_GM,
        rho_WM, rho_GM, coupling (one constant on every tissue) and c0; missing keys are 0.  Returns (g, hv) with g =
        {'J', 'D_WM', 'D_GM', 'rho_WM', 'rho_GM', 'coupling', 'c0'} and one dict of the same keys (no 'J') per direction.
        elastic=True (one GPU): directions also take E_GM, E_WM, E_CSF, E_VENT, nu_GM, nu_WM, nu_CSF, nu_VENT, and g and
        every hv gain those keys; without it such a key is a ValueError (E / nu are first order only by default)."""
        names = ('D_WM', 'D_GM', 'rho_WM', 'rho_GM', 'coupling', 'c0')
        enames = tuple(p + s for p in ('E_', 'nu_') for s, _ in self._ELASTIC_TISSUES) if elastic else ()
        bad = [k for d in directions for k in d if k not in names + enames]
        if bad and elastic:
            raise ValueError("adjoint_hessian: directions take %s, got %s" % (names + enames, bad))
        if bad:
            raise ValueError("adjoint_hessian: directions take %s (E / nu are first order only), got %s" % (names, bad))
        L = self._backend.n_labels if self._backend is not None else 0
        wm, gm = self._tissue_id('WM'), self._tissue_id('GM')
        dirs = []
        for d in directions:
            dD, drho = np.zeros(L), np.zeros(L)
            for t, sfx in ((wm, 'WM'), (gm, 'GM')):
                if t is not None and t < L:
                    dD[t] += float(d.get('D_' + sfx, 0.0))
                    drho[t] += float(d.get('rho_' + sfx, 0.0))
            dirs.append({'D': dD, 'rho': drho, 'gamma': np.full(L, float(d.get('coupling', 0.0))), 'c0': d.get('c0')})
            if elastic:
                dE, dnu = np.zeros(L), np.zeros(L)
                for sfx, tissue in self._ELASTIC_TISSUES:
                    t = self._tissue_id(tissue)
                    if t is not None and t < L:
                        dE[t] += float(d.get('E_' + sfx, 0.0))
                        dnu[t] += float(d.get('nu_' + sfx, 0.0))
                dirs[-1].update(E=dE, nu=dnu)
        r = self._adjoint_hessian_raw(terms, dirs, elastic=elastic)
        pick = lambda a, t: float(a[t]) if t is not None and t < len(a) else 0.0

        def named(D, rho, gamma, c0, E=None, nu=None):
            out = {'D_WM': pick(D, wm), 'D_GM': pick(D, gm), 'rho_WM': pick(rho, wm), 'rho_GM': pick(rho, gm),
                   'coupling': float(np.sum(gamma)), 'c0': c0}
            if elastic:
                for sfx, tissue in self._ELASTIC_TISSUES:
                    t = self._tissue_id(tissue)
                    out['E_' + sfx] = pick(E, t)
                    out['nu_' + sfx] = pick(nu, t)
            return out

        eg = (r['E'], r['nu']) if elastic else ()
        g = dict(named(r['D'], r['rho'], r['gamma'], r['c0'], *eg), J=r['J'])
        hv = [named(r['hv_D'][p], r['hv_rho'][p], r['hv_gamma'][p], r['hv_c0'][p],
                    *((r['hv_E'][p], r['hv_nu'][p]) if elastic else ())) for p in range(len(directions))]
        return g, hv

    def run_for_adjoint(self, parameters, output_dir=config.output_dir_simulation_tmp):
        """:127-145 -- (D_WM, D_GM, rho_WM, rho_GM, coupling)"""
        self.params.D_WM, self.params.D_GM = parameters[0], parameters[1]
        self.params.rho_WM, self.params.rho_GM = parameters[2], parameters[3]
        self.params.coupling = parameters[4]
        self.run(keep_nth=1, save_method=None, clear_all=False, plot=False, output_dir=output_dir)
        return self.solution

    def _make_postprocess(self, output_dir, device):
        from ..simulation_helpers.postprocess import PostProcessTumorGrowthBrain
        if self._backend is None:
            raise RuntimeError("init_postprocess needs a finished run()")
        labels = self._labels()
        t = self._material_tables(int(labels.max()) + 1)
        pp = PostProcessTumorGrowthBrain(self.results, self.params, output_dir=output_dir, backend=self._backend, tables=t,
                                         labels=labels, device=device)
        pp.map_params()
        return pp

    def init_postprocess(self, output_dir=config.output_dir_simulation_tmp, device=None):
        """:148-152; ``device`` as in TumorGrowth.init_postprocess"""
        self.postprocess = self._make_postprocess(output_dir, device)
        return self.postprocess
