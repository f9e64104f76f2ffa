"""
Centre-of-mass misfit terms on the GPU (glims_adjoint_observable_terms3 / _info3; k_observe_mom_cells, k_observe_mom_sum, the
COM = 1 instances of k_observe_grad_cells and k_observe_def_load_cells): J and the gradient in D, rho, gamma, E, nu and c0 against
the numpy statement of tests/com_terms_common.py (itself checked by central differences in tests/test_com_terms_cpu.py) in both
configurations, scale = 0, known answers, more terms on a step than one cell pass serves, the bits of a volume-only list,
an empty measure, the count of elastic solves, repeatability and neutrality, a permuted node order, every refusal, and a
(x0, y0, D, rho) fit through the public API with seed controls.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as in test_gpu_adjoint_image.py)
import torch  # noqa: F401

import adjoint_deformed_common as adc
import com_terms_common as cc
import deformed_volume_common as dvc
import observable_terms_common as otc
from adjoint_common import Problem, renumber
from test_gpu_adjoint import _SKIP, _handle, _record, _rel

pytestmark = pytest.mark.gpu

OUT = ("J", "D", "rho", "gamma", "c0", "E", "nu")
TOL = 1e-8       # GPU against numpy: tests/test_gpu_deformed_volume.py, tests/test_gpu_observable_terms.py


def _mrel(a, b):
    """relative difference in the max norm"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _nostat(st):
    return {k: v for k, v in st.items() if k not in _SKIP}


def _problem(dim):
    """clamped_problem(2, 9): 162 cells, clamped_problem(3, 5): 750 cells -- no multiples of 64, more than one block in 3-D and
    more than one wave in 2-D, two labels.  (The meshes of the volume-term tests at Problem(2, 9) / Problem(3, 5) size.)"""
    return (dvc.clamped_problem(2, 9), 4) if dim == 2 else (dvc.clamped_problem(3, 5), 4)


def _gradient(h, terms, L):
    return dict(zip(OUT, h.adjoint_gradient(terms, L, elastic=True)))


def _u_of(prob):
    return dvc.oracle_of(prob).mech_solve


_reference = {}


def _numpy(key, prob, traj, terms):
    """the numpy statement of a list, computed once per key (the trajectories of two handles on one problem share their bits)"""
    if key not in _reference:
        _reference[key] = cc.evaluate(prob, dvc.oracle_of(prob), traj, terms)
    return _reference[key]


def _against_numpy(h, prob, traj, terms, key, keys=OUT, tol=TOL, what=""):
    g = _gradient(h, terms, prob.n_labels)
    ref = _numpy(key, prob, traj, terms)
    for k in keys:
        print("%s %s: rel. difference to numpy (max norm) %.3e" % (what, k, _mrel(g[k], ref[k])))
    for k in keys:
        assert _mrel(g[k], ref[k]) <= tol, (what, k, g[k], ref[k])
    obs = [t for t in terms if t["kind"] in (cc.KIND, cc.VOLUME)]
    for k, (t, info) in enumerate(zip(obs, ref["info"])):
        dev = h.observable_term_info(k)
        assert abs(dev["V"] - info["V"]) <= tol * abs(info["V"]), (k, dev, info)
        if t["kind"] == cc.KIND:
            assert dev["empty"] is False and not info["empty"]
            assert np.abs(dev["com"] - info["com"]).max() <= tol * cc.diameter(prob), (k, dev, info)
        else:
            assert "com" not in dev
    return g, ref


# ---- 1. against numpy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_reference_configuration_terms_match_the_numpy_statement(backend, dim):
    """The mixed list of com_terms_common.standard_terms: SMOOTH, SHARP (a middle step) and MASS centre-of-mass terms over the
    whole domain and on one tissue, with a volume term and a nodal term on the same step; then every centre-of-mass term alone."""
    prob, N = _problem(dim)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = cc.standard_terms(prob, traj, seed=dim)
    assert [t["kind"] for t in terms] == [cc.KIND] * 3 + [cc.VOLUME, cc.KIND, "c_thresh"]
    assert np.abs(traj[terms[1]["step"]] - terms[1]["level"]).min() >= 1e-2          # the gap rule
    h.set_observable_terms([t for t in terms if t["kind"] != "c_thresh"])
    first = h.observable_term_info(0)
    assert np.isnan(first["V"]) and np.all(np.isnan(first["com"])) and first["empty"] is False   # before the first evaluation
    g, ref = _against_numpy(h, prob, traj, terms, ("ref", dim), keys=("J", "D", "rho", "c0"), what="%d-D" % dim)
    for k in ("gamma", "E", "nu"):
        assert np.all(g[k] == 0.0)                                         # no displacement anywhere
    assert h.observable_term_info(1)["cut"] >= 1
    for k in (0, 1, 2, 4):
        _against_numpy(h, prob, traj, [terms[k]], ("ref", dim, k), keys=("J", "D", "rho", "c0"), what="%d-D term %d alone" % (dim, k))
    st = h.adjoint_stats()
    assert st["backward_steps"] == st["gradients"] * N and st["mech_solves"] == 0
    h.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_deformed_terms_match_the_numpy_statement(backend, dim):
    prob, N = _problem(dim)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = cc.standard_terms(prob, traj, _u_of(prob), seed=dim, deformed=True)
    g, ref = _against_numpy(h, prob, traj, terms, ("def", dim), what="%d-D deformed" % dim)
    coms = [t for t in terms if t["kind"] == cc.KIND]
    ga, _ = _against_numpy(h, prob, traj, coms, ("def", dim, "com"), what="%d-D deformed, centre-of-mass terms alone" % dim)
    for k in ("gamma", "E", "nu"):
        assert np.all(ga[k] != 0.0), (k, ga[k])
    _against_numpy(h, prob, traj, [terms[1]], ("def", dim, 1), what="%d-D deformed SHARP alone" % dim)
    h.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_scale_zero_is_the_reference_configuration(backend, dim):
    prob, N = _problem(dim)
    h = _handle(backend, prob)
    traj = _record(h, N)
    flat = [t for t in cc.standard_terms(prob, traj, seed=dim + 10) if t["kind"] == cc.KIND]
    zero = [dict(t, deformed=True, scale=0.0) for t in flat]
    g, gf = _gradient(h, zero, prob.n_labels), _gradient(h, flat, prob.n_labels)
    for key in ("gamma", "E", "nu"):
        assert np.all(g[key] == 0.0) and np.all(gf[key] == 0.0), (key, g[key])
    for key in ("J", "D", "rho", "c0"):
        print("%d-D scale 0, %s: rel. difference to the reference-configuration terms %.3e" % (dim, key, _mrel(g[key], gf[key])))
        assert np.any(g[key]) and _mrel(g[key], gf[key]) <= 1e-12, (key, g[key], gf[key])
    h.close()


# ---- 2. known answers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_known_answers(backend, dim):
    """Uniform c on the unit box: a MASS term has X = the box centre to 1e-12, J = 1/2 w |centre - target|^2 and, the centre of
    mass being homogeneous of degree 0 in c, sum_i c_i dJ/dc0_i = 0 (step 0: dJ/dc0 is the term's own c-gradient).  On a grown
    state com of the info call equals M / V of Handle.observe."""
    prob, N = _problem(dim)
    base = dvc.clamped_problem(dim, 9 if dim == 2 else 5)
    flat = Problem.from_mesh(base.points, base.cells, base.labels, base.D, base.rho, base.gamma, base.E, base.nu,
                             np.full(len(base.points), 0.4), dt=base.dt, dir_c=None, dir_u=base.dir_u)
    h = _handle(backend, flat)
    _record(h, 1)
    target = np.full(dim, 0.5) + 0.1
    t = cc.com_term(0, "mass", target, weight=1.7)
    g = _gradient(h, [t], flat.n_labels)
    info = h.observable_term_info(0)
    lo, hi = base.points.min(axis=0), base.points.max(axis=0)
    centre = 0.5 * (lo + hi)
    print("%d-D uniform c: com - centre %s, c . dJ/dc0 = %.3e, |dJ/dc0| = %.3e" % (dim, info["com"] - centre, flat.c0 @ g["c0"],
                                                                                np.abs(g["c0"]).max()))
    assert np.abs(info["com"] - centre).max() <= 1e-12
    assert g["J"] == pytest.approx(0.5 * 1.7 * float((centre - target) @ (centre - target)), rel=1e-11)
    assert np.abs(g["c0"]).max() > 1e-6 and abs(flat.c0 @ g["c0"]) <= 1e-12 * np.abs(g["c0"]).sum() * 0.4
    h.close()
    h = _handle(backend, prob)
    traj = _record(h, N)
    sid = h.snapshot_save()
    only1 = np.array([0, 1], dtype=np.uint8)
    for q, mask, deformed, scale in ((("smooth", 0.3, 0.08), only1, False, 1.0), (("sharp", otc.gap_level(traj[N])[0], 1.0), None, True, 0.5),
                                     (("mass", 0.0, 1.0), None, True, 1.0)):
        t = cc.com_term(N, q[0], np.zeros(dim), level=q[1], smooth=q[2], labels=mask, deformed=deformed, scale=scale)
        _gradient(h, [t], prob.n_labels)
        info = h.observable_term_info(0)
        table = h.observe([q], snapshots=[sid], deformed=deformed, scale=scale)[0, 0]
        tot = table[1] if mask is not None else table.sum(axis=0)
        print("%d-D %s: com %s, observe M / V %s" % (dim, q[0], info["com"], tot[1:] / tot[0]))
        assert info["V"] > 0 and np.abs(info["com"] - tot[1:] / tot[0]).max() <= 1e-6
        if not deformed:
            assert np.abs(info["com"] - tot[1:] / tot[0]).max() <= 1e-12
    h.close()


# ---- 3. batching and list behaviour -----------------------------------------------------------------------------------------
def test_nine_mixed_terms_on_one_step_take_two_batches(backend):
    prob, N = _problem(2)
    assert backend.OBSERVE_MAX_QUERIES == 8
    h = _handle(backend, prob)
    traj = _record(h, N)
    step = N // 2
    c, u = traj[step], _u_of(prob)(traj[step])
    rng = np.random.default_rng(31)
    only1 = np.array([0, 1], dtype=np.uint8)
    level, dist = otc.gap_level(c)
    assert dist >= 1e-2
    #        com    kind      level  smooth labels deformed scale
    specs = [(True, "smooth", 0.2, 0.1, None, False, 1.0), (False, "mass", 0.0, 1.0, None, True, 1.0),
             (True, "sharp", level, 1.0, None, True, 0.5), (True, "smooth", 0.4, 0.05, only1, True, 1.0),
             (False, "mass", 0.0, 1.0, only1, False, 1.0), (True, "sharp", level, 1.0, only1, False, 1.0),
             (False, "sharp", -1.0, 1.0, only1, True, 1.0), (True, "mass", 0.0, 1.0, None, True, 0.7),
             (True, "smooth", 0.25, 0.07, only1, True, 1.0)]          # the ninth: a second batch, a deformed centre of mass
    terms = []
    for com, kind, lv, sm, lab, deformed, scale in specs:
        w = float(rng.uniform(0.5, 2.0))
        if com:
            t = cc.com_term(step, kind, np.zeros(2), level=lv, smooth=sm, weight=w, labels=lab, deformed=deformed, scale=scale)
            t["target"] = cc.com_of(prob, t, c, u)[1] + 0.05 * cc.diameter(prob) * np.array([np.cos(w), np.sin(w)])
        else:
            t = dvc.volume_term(step, kind, 0.0, level=lv, smooth=sm, weight=w, labels=lab, deformed=deformed, scale=scale)
            t["target"] = float(rng.uniform(0.5, 0.9) * dvc.measure(prob, t, c, u))
        terms.append(t)
    _against_numpy(h, prob, traj, terms, "nine", what="nine terms")
    terms[8] = cc.com_term(step, "smooth", terms[8]["target"], level=0.25, smooth=0.07, weight=terms[8]["weight"], labels=only1)
    _against_numpy(h, prob, traj, terms, "nine_b", what="nine terms, the ninth undeformed")
    h.close()


def test_a_volume_only_list_through_terms3_has_the_bits_of_terms2(backend):
    prob, N = _problem(2)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = [t for t in dvc.standard_terms(prob, traj, _u_of(prob), seed=2) if t["kind"] == dvc.KIND]
    h.set_observable_terms(terms)                                      # glims_adjoint_observable_terms2
    old = _gradient(h, [], prob.n_labels)
    info_old = [h.observable_term_info2(k) for k in range(len(terms))]
    arr = (backend.ObservableMisfit3 * len(terms))()
    keep = []
    for k, t in enumerate(terms):
        lab = None if t["labels"] is None else np.ascontiguousarray(np.asarray(t["labels"]) != 0, dtype=np.uint8)
        keep.append(lab)
        arr[k] = backend.ObservableMisfit3(int(t["step"]), backend.OBSERVE_KINDS[t["observable"]], t["level"], t["smooth"],
                                           t["weight"], t["target"], None if lab is None else lab.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           1 if t.get("deformed") else 0, float(t.get("scale", 1.0)), 0,
                                           (C.c_double * 3)(np.nan, np.nan, np.nan))   # (target_x of a volume term means nothing)
    h._check(h.lib.glims_adjoint_observable_terms3(h._h, len(terms), arr))
    new = _gradient(h, [], prob.n_labels)
    assert new["J"] > 0 and new["J"] == old["J"]
    for key in OUT[1:]:
        assert np.array_equal(new[key], old[key]), key
    assert info_old == [h.observable_term_info2(k) for k in range(len(terms))] or all(
        (a["V"], a["cut"], a["folded"]) == (b["V"], b["cut"], b["folded"])
        for a, b in zip(info_old, [h.observable_term_info2(k) for k in range(len(terms))]))
    i3 = h.observable_term_info3(0)
    assert i3["empty"] is False and np.all(np.isnan(i3["com"]))
    h.close()


def test_repeatable_bits_and_neutral_towards_everything_else(backend):
    prob, N = _problem(2)
    a, b = _handle(backend, prob), _handle(backend, prob)
    traj = _record(a, N)
    assert b.step(N) == 0
    nodal = [dict(step=N, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5,
                  target=np.random.default_rng(3).uniform(0, 1, len(prob.points)))]
    g0 = _gradient(a, nodal, prob.n_labels)               # before any term was set
    sa, ca = a.stats(), a.get_state(want_u=False)[0]
    terms = [t for t in cc.standard_terms(prob, traj, _u_of(prob), seed=9, deformed=True) if t["kind"] != "c_thresh"]
    aa = a.adjoint_stats()
    a.set_observable_terms(terms)
    assert a.adjoint_stats() == aa and _nostat(a.stats()) == _nostat(sa)      # the new entry points count nowhere
    calls = [_gradient(a, nodal, prob.n_labels) for _ in range(3)]            # (the stored terms stay)
    for other in calls[1:]:
        assert other["J"] == calls[0]["J"] and all(np.array_equal(other[k], calls[0][k]) for k in OUT[1:])
    assert calls[0]["J"] != g0["J"] and np.any(calls[0]["gamma"])
    assert _nostat(a.stats()) == _nostat(sa) and np.array_equal(a.get_state(want_u=False)[0], ca)
    a.set_observable_terms([])                            # the list cleared: the call is what it was
    g1 = _gradient(a, nodal, prob.n_labels)
    assert g1["J"] == g0["J"] and all(np.array_equal(g1[k], g0[k]) for k in OUT[1:])
    assert a.step(3) == 0 and b.step(3) == 0              # the forward run goes on as on a handle that never set a term
    assert np.array_equal(a.get_state(want_u=False)[0], b.get_state(want_u=False)[0])
    assert _nostat(a.stats()) == _nostat(b.stats())
    a.close()
    b.close()


# ---- 4. an empty measure ---------------------------------------------------------------------------------------------------
def test_an_empty_term_contributes_nothing_and_leaves_the_batch_alone(backend):
    prob, N = _problem(2)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = [t for t in cc.standard_terms(prob, traj, seed=5) if t["kind"] != "c_thresh"]
    g = _gradient(h, terms, prob.n_labels)
    empty = cc.com_term(N, "sharp", np.array([0.3, 0.3]), level=2.0 * max(c.max() for c in traj), weight=3.0)
    with pytest.warns(RuntimeWarning, match="empty") as rec:
        ge = _gradient(h, terms[:2] + [empty] + terms[2:], prob.n_labels)
        _gradient(h, terms[:2] + [empty] + terms[2:], prob.n_labels)         # the same stored list: no second warning
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert ge["J"] == g["J"] and all(np.array_equal(ge[k], g[k]) for k in OUT[1:])
    info = h.observable_term_info(2)
    assert info["empty"] is True and info["V"] == 0.0 and np.all(np.isnan(info["com"])) and info["cut"] == 0
    assert h.observable_term_info(0)["empty"] is False
    with pytest.warns(RuntimeWarning, match="empty"):
        alone = _gradient(h, [empty], prob.n_labels)
    assert alone["J"] == 0.0 and all(not np.any(alone[k]) for k in OUT[1:])
    h.close()


# ---- 5. elastic solves ------------------------------------------------------------------------------------------------------
def test_one_elastic_solve_pair_per_observed_step(backend):
    prob = dvc.clamped_problem(2, 9)
    N = 4
    h = _handle(backend, prob)
    _record(h, N)
    rng = np.random.default_rng(5)
    n, d = len(prob.points), prob.dim

    def solves(terms):
        before = h.adjoint_stats()["mech_solves"]
        h.adjoint_gradient(terms, prob.n_labels, elastic=True)
        return h.adjoint_stats()["mech_solves"] - before

    com = lambda step, deformed: cc.com_term(step, "smooth", [0.4, 0.6], level=0.3, smooth=0.1, deformed=deformed)
    vol = lambda step, deformed: dvc.volume_term(step, "smooth", 0.1, level=0.3, smooth=0.1, deformed=deformed)
    u_l2 = dict(step=N, kind="u_l2", weight=10.0, target=0.01 * rng.standard_normal(n * d))
    x = 0.5 + 0.45 * rng.uniform(-1.0, 1.0, (60, d))
    img = adc.deformed_term(x, N, "img_l2", rng.uniform(0, 0.6, len(x)), None, weight=2.0)
    assert solves([com(N, False), com(2, False), vol(N, False)]) == 0
    assert solves([com(N, False), u_l2]) == 2
    assert solves([com(N, True)]) == 2
    assert solves([com(N, True), vol(N, True), com(N, False), com(2, True)]) == 4
    assert solves([com(N, True), img, u_l2, vol(N, True), com(1, True), com(1, False)]) == 4
    h.close()


def test_permuted_node_order_gives_the_same_gradient(backend):
    base = dvc.clamped_problem(2, 9)
    N, d = 4, 2
    out = []
    terms = None
    for seed in (None, 11):
        if seed is None:
            prob, perm = base, np.arange(len(base.points))
        else:
            pts, cells, perm = renumber(base.points, base.cells, seed)
            inv = np.argsort(perm)
            dofs = inv[base.dir_u[0] // d] * d + base.dir_u[0] % d
            prob = Problem.from_mesh(pts, cells, base.labels, base.D, base.rho, base.gamma, base.E, base.nu, base.c0[perm],
                                     dt=base.dt, dir_c=(inv[base.dir_c[0]], base.dir_c[1]), dir_u=(dofs, base.dir_u[1]))
        h = _handle(backend, prob)
        traj = _record(h, N)
        if terms is None:
            terms = [t for t in cc.standard_terms(base, traj, _u_of(base), seed=7, deformed=True) if t["kind"] != "c_thresh"]
        g = _gradient(h, terms, prob.n_labels)
        h.close()
        back = np.empty_like(g["c0"])
        back[perm] = g["c0"]   # to the base numbering
        out.append(dict(g, c0=back))
    for key in OUT:
        print("%s: rel. difference between the numberings %.3e" % (key, _mrel(out[1][key], out[0][key])))
        assert _mrel(out[1][key], out[0][key]) <= TOL, (key, out[1][key], out[0][key])


# ---- 6. misuse -------------------------------------------------------------------------------------------------------------
def test_every_new_refusal_leaves_the_old_list_in_place(backend):
    prob = dvc.clamped_problem(2, 9)
    N = 3
    good = cc.com_term(N, "smooth", [0.4, 0.6], level=0.3, smooth=0.1, labels=[0, 1], deformed=True)
    flat = {k: v for k, v in good.items() if k not in ("deformed", "scale")}
    plain = _handle(backend, prob, mechanics=False)
    _record(plain, N)
    plain.set_observable_terms([flat])
    J0 = plain.adjoint_gradient([], 2)[0]
    with pytest.raises(backend.BackendError) as e:
        plain.set_observable_terms([flat, good])
    assert e.value.code == backend.GLIMS_E_USAGE and "with_mechanics" in str(e.value), e.value
    assert plain.observable_term_info(0)["counted"] == int((prob.labels == 1).sum()) and plain.adjoint_gradient([], 2)[0] == J0
    plain.close()
    h = _handle(backend, prob)
    _record(h, N)
    h.set_observable_terms([good, dvc.volume_term(0, "mass", 0.5)])
    J0 = h.adjoint_gradient([], 2)[0]
    assert J0 > 0

    def usage(fn, match):
        with pytest.raises(backend.BackendError) as e:
            fn()
        assert e.value.code == backend.GLIMS_E_USAGE, e.value
        assert match in str(e.value), e.value
        assert h.observable_term_info3(0)["counted"] == int((prob.labels == 1).sum())
        assert h.observable_term_info3(1)["counted"] == len(prob.cells) and h.adjoint_gradient([], 2)[0] == J0

    usage(lambda: h.set_observable_terms([dict(good, moment=2)]), "moment")
    usage(lambda: h.set_observable_terms([good, dict(good, moment=-1)]), "moment")
    usage(lambda: h.set_observable_terms([dict(good, target=[0.1, np.nan])]), "target_x")
    usage(lambda: h.set_observable_terms([dict(good, target=[np.inf, 0.1])]), "target_x")
    usage(lambda: h.set_observable_terms([dict(good, scale=np.inf)]), "scale")
    usage(lambda: h.set_observable_terms([dict(good, smooth=0.0)]), "smooth")
    usage(lambda: h.set_observable_terms([dict(good, step=-1)]), "step")
    usage(lambda: h.observable_term_info3(2), "no stored term")
    usage(lambda: h._check(h.lib.glims_adjoint_observable_terms3(h._h, 1, None)), "bad term list")
    with pytest.raises(ValueError):
        h.set_observable_terms([dict(good, target=[0.1, 0.2, 0.3])])
    # second order: every Hessian entry point refuses while a centre-of-mass term is stored; the gradient works
    h.set_observable_terms([flat])
    dirs = [dict(D=[1.0, 0.0])]
    for call in (lambda: h.adjoint_hessian([], dirs), lambda: h.adjoint_hessian([], dirs, collective=True),
                 lambda: h.adjoint_hessian_full([], dirs)):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == backend.GLIMS_E_USAGE and "centre-of-mass" in str(e.value) and "second order" in str(e.value), e.value
    for call in (lambda: h.adjoint_hessian([flat], dirs), lambda: h.adjoint_hessian_full([flat], dirs)):
        with pytest.raises(NotImplementedError):
            call()
    assert h.adjoint_gradient([flat], 2)[0] > 0
    h.set_observable_terms([dvc.volume_term(N, "smooth", 0.1, level=0.3, smooth=0.1)])
    assert h.adjoint_hessian([], dirs)["J"] > 0               # a volume term has its second order
    h.close()


def test_partitioned_handle_refuses_on_every_rank(backend):
    from glimslib_amd import _backend as B
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    prob = Problem(2, 12)
    world = 2

    def body(rank, tr):
        part = partition_mesh(prob.points, prob.cells, world, rank)
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=part.n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt)
        h.setup(with_mechanics=False)
        h.set_state(prob.c0[part.global_ids])
        try:
            h.set_observable_terms([cc.com_term(0, "mass", [0.5, 0.5])])
            code, why = 0, ""
        except B.BackendError as e:
            code, why = e.code, str(e)
        h.set_observable_terms([])                # clearing is fine there
        h.adjoint_record(True)
        assert h.step(2) == 0
        nodal = [dict(step=2, kind="c_l2", target=np.zeros(len(part.global_ids)))]
        h.adjoint_gradient(nodal)                 # the handle still works (a collective call every rank makes)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return code, "partitioned" in why

    assert run_threaded_ranks(world, body) == [(B.GLIMS_E_USAGE, True)] * world


# ---- 7. the public API -----------------------------------------------------------------------------------------------------
def test_fit_of_seed_D_and_rho_through_the_public_api(tmp_path):
    """examples/adjoint_fit_seed_2D.py at test size (com_terms_common.FIT): the data are the T2- / T1-like SMOOTH volumes and
    centres of mass of the whole domain at five steps of a truth run.  The numpy / scipy twin of this fit
    (tests/test_com_terms_cpu.py) recovers (x0, y0, D, rho) to 3.9e-12 (x0, y0: absolute, in units of the length 1; D, rho:
    relative), which sets the bar B = 1e-11 (com_terms_common.FIT["bar"]); the bar here is the same B."""
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.optimization import ReducedFunctional, minimize
    from glimslib_amd.simulation import TumorGrowth
    F = cc.FIT

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    def make_sim(x0, y0, D, rho):
        mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
        labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1),
                                fenics.FunctionSpace(mesh, "DG", 1))
        sim = TumorGrowth(mesh)
        sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                    boundaries={'boundary_all': Boundary()},
                                    dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                               'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                    von_neumann_bcs={})
        u0 = fenics.Expression('exp(-a*(pow(x[0]-x0,2)+pow(x[1]-y0,2)))', degree=1, a=F["a"], x0=x0, y0=y0)
        sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                                   proliferation=rho, E=0.001, poisson=0.4, sim_time=F["steps"] * F["dt"],
                                   sim_time_step=F["dt"])
        return sim

    def terms(s, n_steps, targets=None):
        out = cc.fit_terms(lambda k, lv: s.volume_term(k, 0.0, threshold=lv, kind='smooth', smooth=F["smooth"]),
                           lambda k, lv: s.com_term(k, [0.0, 0.0], threshold=lv, kind='smooth', smooth=F["smooth"],
                                                    weight=F["com_weight"]))
        if targets is not None:
            for t, v in zip(out, targets):
                t["target"] = v
        return out

    truth = make_sim(*F["truth"])
    truth.run(record_adjoint=True, save_method=None, plot=False, output_dir=str(tmp_path))
    truth.adjoint_gradient(terms(truth, F["steps"]))
    infos = [truth._backend.observable_term_info(i) for i in range(4 * len(F["obs_steps"]))]
    targets = [i["com"].copy() if "com" in i else float(i["V"]) for i in infos]
    truth.close()
    assert all(not i.get("empty", False) and i["V"] > 0 for i in infos)

    sim = make_sim(*F["start"])
    rf = ReducedFunctional(sim, 2, lambda s, n: terms(s, n, targets), run_kwargs=dict(output_dir=str(tmp_path)),
                           names=("diffusion", "proliferation"), iv_controls=("x0", "y0"))
    x0, y0, D, rho = F["start"]
    lo, hi = F["lo_bounds"], F["hi_bounds"]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)          # (no empty measure on the way)
        res = minimize(rf, [D, rho, x0, y0], bounds=([lo[2], lo[3], lo[0], lo[1]], [hi[2], hi[3], hi[0], hi[1]]),
                       options=dict(F["options"]), tol=F["tol"])
    t = np.array(F["truth"])
    got = np.array([res.x[2], res.x[3], res.x[0], res.x[1]])
    err = np.abs(got - t) / np.array([1.0, 1.0, t[2], t[3]])
    print("fit of the seed, D and rho: %d iterations, %d evaluations, (x0, y0, D, rho) = %s, error %s"
          % (res.nit, rf.evaluations, got, err))
    assert res.nit <= F["options"]["maxiter"]
    assert np.all(err <= F["bar"]), res
    with pytest.raises(NotImplementedError):
        rf.hessian_matrix(res.x)
    with pytest.raises(NotImplementedError):
        rf.hessian(res.x, np.ones(4))
    with pytest.raises(NotImplementedError):
        sim.adjoint_hessian(terms(sim, F["steps"], targets), [dict(diffusion=1.0)])
    sim.close()
