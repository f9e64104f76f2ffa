"""
Volume misfit terms in the deformed configuration on the GPU (glims_adjoint_observable_terms2 / _info2; k_observe_grad_cells<D, 1>,
k_observe_def_load_cells, k_observe_def_sum and the D-component gather k_observe_grad_rows<NV, D>): J and the gradient in D,
rho, gamma, E, nu and c0 against the numpy statement of tests/deformed_volume_common.py (itself checked by central differences
in tests/test_deformed_volume_cpu.py), the deformed terms alone (the case that fails without the feature), scale = 0, known
answers, more terms on a step than one cell pass serves, the bits of reference terms, a folded mesh, the count of elastic
solves, repeatability and neutrality, a permuted node order, every refusal, and a (coupling, D) fit to deformed volume series
through the public API.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as in test_gpu_adjoint_image.py)
import torch  # noqa: F401

import adjoint_deformed_common as adc
import deformed_volume_common as dvc
import observable_terms_common as otc
from adjoint_common import Problem, renumber
from test_gpu_adjoint import _SKIP, _handle, _record, _rel

pytestmark = pytest.mark.gpu

OUT = ("J", "D", "rho", "gamma", "c0", "E", "nu")
TOL = 1e-8       # GPU against numpy: tests/test_gpu_adjoint_deformed.py, tests/test_gpu_observable_terms.py


def _nostat(st):
    return {k: v for k, v in st.items() if k not in _SKIP}


def _three_labels(base):
    """The problem with a third tissue (label 2) that no cell carries."""
    ext = lambda a, v: np.append(a, v)
    return Problem.from_mesh(base.points, base.cells, base.labels, ext(base.D, 0.03), ext(base.rho, 0.5), ext(base.gamma, 0.1),
                             ext(base.E, 1.5), ext(base.nu, 0.3), base.c0, dt=base.dt, dir_c=base.dir_c, dir_u=base.dir_u)


def _problem(dim):
    """clamped_problem(2, 17): 578 cells, three 256-lane blocks of the cell passes with the last one partial; clamped_problem(3,
    6): 1296 cells.  (N: the 2-D run stops at step 4, where the gap rule still holds -- tests/test_gpu_observable_terms.py.)"""
    return (_three_labels(dvc.clamped_problem(2, 17)), 4) if dim == 2 else (_three_labels(dvc.clamped_problem(3, 6)), 6)


def _gradient(h, terms, L):
    return dict(zip(OUT, h.adjoint_gradient(terms, L, elastic=True)))


def _against_numpy(h, prob, traj, terms, tol=TOL, what=""):
    """The device gradient of `terms` on its own trajectory against numpy's, and the info2 figures against numpy's counts."""
    g = _gradient(h, terms, prob.n_labels)
    ref = dvc.evaluate(prob, dvc.oracle_of(prob), traj, terms)
    for key in OUT:
        print("%s %s: rel. difference to numpy %.3e" % (what, key, _rel(g[key], ref[key])))
    for key in OUT:
        assert _rel(g[key], ref[key]) <= tol, (what, key, g[key], ref[key])
    for k, info in enumerate(ref["info"]):
        dev = h.observable_term_info2(k)
        assert (dev["counted"], dev["cut"], dev["folded"]) == (info["counted"], info["cut"], info["folded"]), (k, dev, info)
        assert abs(dev["V"] - info["V"]) <= tol * max(abs(info["V"]), 1e-300) or info["V"] == dev["V"] == 0.0, (k, dev, info)
        if np.isnan(info["min_ratio"]):
            assert np.isnan(dev["min_ratio"]), (k, dev, info)
        else:
            assert dev["min_ratio"] == pytest.approx(info["min_ratio"], rel=tol), (k, dev, info)
        old = h.observable_term_info(k)
        assert old == dict(counted=dev["counted"], cut=dev["cut"], V=dev["V"])
    return g, ref


def _u_of(prob):
    o = dvc.oracle_of(prob)
    return o.mech_solve


# ---- 1. against numpy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_gradient_and_J_match_the_numpy_statement(backend, dim):
    """The mixed list of deformed_volume_common.standard_terms -- deformed SMOOTH, SHARP (scale 0.5, a middle step) and MASS,
    the level -1 tissue volume, a reference-configuration term and a nodal c_thresh term -- with the masks "all", "label 1"
    and a label that no cell carries."""
    prob, N = _problem(dim)
    assert (dim, len(prob.cells)) in ((2, 578), (3, 1296)) and 2 not in prob.labels
    h = _handle(backend, prob)
    traj = _record(h, N)
    for labels in ("all", "one", [0, 0, 1]):
        terms = dvc.standard_terms(prob, traj, _u_of(prob), seed=dim, labels=labels)
        assert [bool(t.get("deformed")) for t in terms] == [True, True, True, True, False, False]
        assert np.abs(traj[terms[1]["step"]] - terms[1]["level"]).min() >= 1e-2          # the gap rule
        h.set_observable_terms([t for t in terms if t["kind"] == dvc.KIND])
        first = h.observable_term_info2(0)
        assert first["folded"] == -1 and np.isnan(first["V"]) and np.isnan(first["min_ratio"])   # before the first evaluation
        g, ref = _against_numpy(h, prob, traj, terms, what="%d-D mask %s" % (dim, labels))
        assert ref["info"][4]["folded"] == -1 and h.observable_term_info2(4)["folded"] == -1      # the reference term
        if labels == "all":
            assert all(i["folded"] == 0 and i["min_ratio"] < 0.95 for i in ref["info"][:4])
            assert ref["info"][1]["cut"] >= 1 and ref["info"][3]["cut"] == 0
        if labels == [0, 0, 1]:
            for k in range(3):
                dev = h.observable_term_info2(k)
                assert dev["counted"] == 0 and dev["V"] == 0.0 and dev["folded"] == 0 and np.isnan(dev["min_ratio"])
        # each deformed term alone, so that no term's error hides behind a larger one
        if labels == "all":
            for k in range(4):
                _against_numpy(h, prob, traj, [terms[k]], what="%d-D term %d alone" % (dim, k))
    st = h.adjoint_stats()
    assert st["backward_steps"] == st["gradients"] * N
    h.close()


# ---- 2. fails without the feature -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_deformed_volume_terms_alone_give_gamma_E_and_nu(backend, dim):
    """No displacement term and no deformed image term: dJ/dgamma, dJ/dE and dJ/dnu come from the cofactor load alone; the same
    terms with deformed=False give exact zeros there."""
    prob, N = _problem(dim)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = [t for t in dvc.standard_terms(prob, traj, _u_of(prob), seed=2) if dvc.is_deformed_volume(t)]
    assert len(terms) == 4
    g, ref = _against_numpy(h, prob, traj, terms, what="%d-D deformed alone" % dim)
    for key in ("gamma", "E", "nu"):
        assert np.all(g[key][:2] != 0.0) and np.abs(g[key]).max() > 1e-4, (key, g[key])
    flat = [{k: v for k, v in t.items() if k not in ("deformed", "scale")} for t in terms]
    before = h.adjoint_stats()["mech_solves"]
    gf = _gradient(h, flat, prob.n_labels)
    assert gf["J"] > 0 and gf["J"] != g["J"] and h.adjoint_stats()["mech_solves"] == before
    for key in ("gamma", "E", "nu"):
        assert np.all(gf[key] == 0.0), (key, gf[key])
    h.close()


# ---- 3. scale = 0 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_scale_zero_is_the_reference_configuration(backend, dim):
    """The load is multiplied by the scale and the elastic solve returns exact zeros for a zero right-hand side: dJ/dgamma, dJ/dE
    and dJ/dnu are exactly 0.  J, dD, drho and dc0 agree with the reference-configuration terms to 1e-12 (the stored cell volume
    and the one formed in the lane need not share bits)."""
    prob, N = _problem(dim)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = [dict(t, scale=0.0) for t in dvc.standard_terms(prob, traj, _u_of(prob), seed=4) if dvc.is_deformed_volume(t)]
    g = _gradient(h, terms, prob.n_labels)
    for k in range(len(terms)):
        info = h.observable_term_info2(k)
        assert info["folded"] == 0 and info["min_ratio"] == 1.0
    gf = _gradient(h, [{k: v for k, v in t.items() if k not in ("deformed", "scale")} for t in terms], prob.n_labels)
    for key in ("gamma", "E", "nu"):
        assert np.all(g[key] == 0.0) and np.all(gf[key] == 0.0), (key, g[key])
    for key in ("J", "D", "rho", "c0"):
        print("%d-D scale 0, %s: rel. difference to the reference-configuration terms %.3e" % (dim, key, _rel(g[key], gf[key])))
        assert np.any(g[key]) and _rel(g[key], gf[key]) <= 1e-12, (key, g[key], gf[key])
    h.close()


# ---- 4. known answers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_known_answers(backend, dim):
    """The level -1 term over all labels on the clamped mesh measures the whole domain: V = |Omega| = 1 to 1e-12 whatever the
    displacement, and its dJ/dgamma, dJ/dE, dJ/dnu are at most 1e-8 of those of the label-1-only term (the whole domain's volume
    cannot change).  V of a term is the figure Handle.observe(deformed=True, scale) gives for the same state, to the 1e-6 of
    sum |T| of tests/test_gpu_observe.py where two elastic solves of the same system meet."""
    prob, N = _problem(dim)
    h = _handle(backend, prob)
    traj = _record(h, N)
    sid = h.snapshot_save()                                            # c_N, for observe()
    only1 = np.array([0, 1, 0], dtype=np.uint8)
    whole = dvc.volume_term(N, "sharp", 0.5, level=-1.0, deformed=True)
    part = dvc.volume_term(N, "sharp", 0.5 * 0.5, level=-1.0, labels=only1, deformed=True)
    gw = _gradient(h, [whole], prob.n_labels)
    iw = h.observable_term_info2(0)
    gp = _gradient(h, [part], prob.n_labels)
    ip = h.observable_term_info2(0)
    print("%d-D whole domain: V - 1 = %.3e; label 1: V = %.12f" % (dim, iw["V"] - 1.0, ip["V"]))
    assert abs(iw["V"] - 1.0) <= 1e-12 and iw["counted"] == len(prob.cells) and iw["cut"] == 0 and iw["folded"] == 0
    assert gw["J"] == 0.5 * (iw["V"] - 0.5) ** 2
    for key in ("gamma", "E", "nu"):
        print("%s: whole domain %.3e, label 1 %.3e" % (key, np.abs(gw[key]).max(), np.abs(gp[key]).max()))
        assert np.abs(gp[key]).max() > 0 and np.abs(gw[key]).max() <= 1e-8 * np.abs(gp[key]).max(), (key, gw[key], gp[key])
    assert not np.any(gw["D"]) or np.abs(gw["D"]).max() <= 1e-8 * np.abs(gp["D"]).max()
    # glims_observe on the same recorded state
    sum_abs = 1.0
    # (the level set of the SHARP query need not reach tissue 1: that term counts every label)
    for scale, q, mask in ((1.0, ("smooth", 0.3, 0.08), only1), (0.5, ("sharp", otc.gap_level(traj[N])[0], 1.0), None),
                           (1.0, ("sharp", -1.0, 1.0), only1)):
        t = dvc.volume_term(N, q[0], 0.0, level=q[1], smooth=q[2], labels=mask, deformed=True, scale=scale)
        _gradient(h, [t], prob.n_labels)
        V = h.observable_term_info2(0)["V"]
        table = h.observe([q], snapshots=[sid], deformed=True, scale=scale)[0, 0, :, 0]
        Vo = table[1] if mask is not None else table.sum()
        print("%d-D %s scale %.1f: V %.12e, observe %.12e" % (dim, q[0], scale, V, Vo))
        assert V > 0 and abs(V - Vo) <= 1e-6 * sum_abs
    h.close()


# ---- 5. more terms than one pass serves -----------------------------------------------------------------------------------
def test_nine_mixed_terms_on_one_step_take_two_cell_passes(backend):
    prob, N = _problem(2)
    assert backend.OBSERVE_MAX_QUERIES == 8
    h = _handle(backend, prob)
    traj = _record(h, N)
    step = N // 2
    c, u = traj[step], _u_of(prob)(traj[step])
    rng = np.random.default_rng(31)
    only1 = np.array([0, 1, 0], dtype=np.uint8)
    level, dist = otc.gap_level(c)
    assert dist >= 1e-2
    #        kind      level  smooth labels deformed scale
    specs = [("smooth", 0.2, 0.1, None, False, 1.0), ("mass", 0.0, 1.0, None, True, 1.0), ("sharp", level, 1.0, None, True, 0.5),
             ("smooth", 0.4, 0.05, only1, True, 1.0), ("mass", 0.0, 1.0, only1, False, 1.0), ("sharp", level, 1.0, only1, False, 1.0),
             ("sharp", -1.0, 1.0, only1, True, 1.0), ("smooth", 0.5, 0.1, None, True, 0.7),
             ("smooth", 0.25, 0.07, only1, True, 1.0)]           # the ninth: a second pass, deformed
    terms = []
    for kind, lv, sm, lab, deformed, scale in specs:
        t = dvc.volume_term(step, kind, 0.0, level=lv, smooth=sm, weight=float(rng.uniform(0.5, 2.0)), labels=lab,
                            deformed=deformed, scale=scale)
        t["target"] = float(rng.uniform(0.5, 0.9) * dvc.measure(prob, t, c, u))
        terms.append(t)
    _against_numpy(h, prob, traj, terms, what="nine terms")
    # the second pass alone is a reference-configuration batch when the ninth term is one
    terms[8] = {k: v for k, v in terms[8].items() if k not in ("deformed", "scale")}
    _against_numpy(h, prob, traj, terms, what="nine terms, the ninth undeformed")
    h.close()


# ---- 6. reference terms keep their bits ------------------------------------------------------------------------------------
def test_reference_terms_through_the_new_entry_point_have_the_bits_of_the_old_one(backend):
    prob, N = _problem(2)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = [t for t in otc.standard_terms(prob, traj, seed=2, empty_label=2) if t["kind"] == otc.KIND]
    before = h.adjoint_stats()["mech_solves"]
    h.set_observable_terms(terms)                                      # glims_adjoint_observable_terms2, deformed = 0
    new = _gradient(h, [], prob.n_labels)                              # (an empty list: the stored terms stay)
    info_new = [h.observable_term_info2(k) for k in range(len(terms))]
    arr = (backend.ObservableMisfit * len(terms))()
    keep = []
    for k, t in enumerate(terms):
        lab = None if t["labels"] is None else np.ascontiguousarray(np.asarray(t["labels"]) != 0, dtype=np.uint8)
        keep.append(lab)
        arr[k] = backend.ObservableMisfit(int(t["step"]), backend.OBSERVE_KINDS[t["observable"]], t["level"], t["smooth"],
                                          t["weight"], t["target"],
                                          None if lab is None else lab.ctypes.data_as(C.POINTER(C.c_uint8)))
    h._check(h.lib.glims_adjoint_observable_terms(h._h, len(terms), arr))
    old = _gradient(h, [], prob.n_labels)
    assert new["J"] > 0 and new["J"] == old["J"]
    for key in OUT[1:]:
        assert np.array_equal(new[key], old[key]), key
    for a, b in zip(info_new, [h.observable_term_info2(k) for k in range(len(terms))]):
        assert (a["V"], a["cut"], a["counted"]) == (b["V"], b["cut"], b["counted"])
    assert all(i["folded"] == -1 and np.isnan(i["min_ratio"]) for i in info_new)
    assert h.adjoint_stats()["mech_solves"] == before                  # no elastic solve for a list without a deformed term
    h.close()


# ---- 7. a folded mesh ------------------------------------------------------------------------------------------------------
def test_folded_cells_count_negatively_and_are_warned_about_once(backend):
    """scale = 4 folds cells of clamped_problem(2, 16): the folded count equals numpy's, the gradient still matches (V is a
    polynomial in u: nothing special happens at a fold), and the Python layer warns once per stored list, citing min_ratio."""
    prob = dvc.clamped_problem(2, 16)
    N = 3
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = [dict(t, scale=4.0) for t in dvc.standard_terms(prob, traj, _u_of(prob), seed=31) if dvc.is_deformed_volume(t)]
    for t in terms:                                                   # (targets of the folded configuration itself)
        t["target"] = 0.7 * dvc.measure(prob, t, traj[t["step"]], _u_of(prob)(traj[t["step"]]))
    with pytest.warns(RuntimeWarning, match="min_ratio") as rec:
        g, ref = _against_numpy(h, prob, traj, terms, what="folded")
        h.adjoint_gradient(terms, prob.n_labels)            # the same stored list: no second warning
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert ref["info"][0]["folded"] > 0 and ref["info"][0]["min_ratio"] < 0
    assert h.observable_term_info2(0)["folded"] == ref["info"][0]["folded"]
    with pytest.warns(RuntimeWarning, match="min_ratio"):   # a new stored list warns again
        h.adjoint_gradient(terms[:1], prob.n_labels)
    h.close()


# ---- 8. one elastic solve pair per observed step -------------------------------------------------------------------------
def test_one_elastic_solve_pair_per_observed_step(backend):
    prob = dvc.clamped_problem(2, 16)
    N = 4
    h = _handle(backend, prob)
    traj = _record(h, N)
    rng = np.random.default_rng(5)
    n, d = len(prob.points), prob.dim

    def solves(terms):
        before = h.adjoint_stats()["mech_solves"]
        h.adjoint_gradient(terms, prob.n_labels, elastic=True)
        return h.adjoint_stats()["mech_solves"] - before

    vol = lambda step, deformed: dvc.volume_term(step, "smooth", 0.1, level=0.3, smooth=0.1, deformed=deformed)
    u_l2 = dict(step=N, kind="u_l2", weight=10.0, target=0.01 * rng.standard_normal(n * d))
    x = 0.5 + 0.45 * rng.uniform(-1.0, 1.0, (60, d))
    img = adc.deformed_term(x, N, "img_l2", rng.uniform(0, 0.6, len(x)), None, weight=2.0)
    # without a deformed volume term: exactly the old counts
    assert solves([vol(N, False), vol(2, False)]) == 0
    assert solves([vol(N, False), u_l2]) == 2
    assert solves([vol(N, False), img]) == 2
    # u_k and mu_k once per observed step, however many terms of whatever kind observe it
    assert solves([vol(N, True)]) == 2
    assert solves([vol(N, True), vol(N, True), vol(2, True)]) == 4
    assert solves([vol(N, True), u_l2]) == 2
    assert solves([vol(N, True), img]) == 2
    assert solves([vol(N, True), img, u_l2, vol(1, True), vol(1, False)]) == 4
    h.close()


# ---- 9. bits and neutrality -----------------------------------------------------------------------------------------------
def test_repeatable_bits_and_neutral_towards_everything_else(backend):
    prob, N = _problem(2)
    a, b = _handle(backend, prob), _handle(backend, prob)
    traj = _record(a, N)
    assert b.step(N) == 0
    nodal = [dict(step=N, kind="c_thresh", level=0.6, smooth=0.1, weight=0.5,
                  target=np.random.default_rng(3).uniform(0, 1, len(prob.points)))]
    g0 = _gradient(a, nodal, prob.n_labels)               # before any volume term was set
    sa, ca = a.stats(), a.get_state(want_u=False)[0]
    terms = [t for t in dvc.standard_terms(prob, traj, _u_of(prob), seed=9) if t["kind"] == dvc.KIND]
    aa = a.adjoint_stats()
    a.set_observable_terms(terms)
    assert a.adjoint_stats() == aa and _nostat(a.stats()) == _nostat(sa)      # the new entry points count nowhere
    calls = [_gradient(a, nodal, prob.n_labels) for _ in range(3)]            # (the stored volume terms stay)
    for other in calls[1:]:
        assert other["J"] == calls[0]["J"] and all(np.array_equal(other[k], calls[0][k]) for k in OUT[1:])
    assert calls[0]["J"] != g0["J"] and np.any(calls[0]["gamma"])
    assert _nostat(a.stats()) == _nostat(sa) and np.array_equal(a.get_state(want_u=False)[0], ca)
    a.set_observable_terms([])                            # the list cleared: the call is what it was
    g1 = _gradient(a, nodal, prob.n_labels)
    assert g1["J"] == g0["J"] and all(np.array_equal(g1[k], g0[k]) for k in OUT[1:])
    with pytest.raises(backend.BackendError):
        a.observable_term_info2(0)
    assert a.step(3) == 0 and b.step(3) == 0              # the forward run goes on as on a handle that never set a term
    assert np.array_equal(a.get_state(want_u=False)[0], b.get_state(want_u=False)[0])
    assert _nostat(a.stats()) == _nostat(b.stats())
    a.close()
    b.close()


def test_permuted_node_order_gives_the_same_gradient(backend):
    base = dvc.clamped_problem(2, 17)
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
            terms = [t for t in dvc.standard_terms(base, traj, _u_of(base), seed=7) if t["kind"] == dvc.KIND]
        g = _gradient(h, terms, prob.n_labels)
        h.close()
        back = np.empty_like(g["c0"])
        back[perm] = g["c0"]   # to the base numbering
        out.append(dict(g, c0=back))
    for key in OUT:
        print("%s: rel. difference between the numberings %.3e" % (key, _rel(out[1][key], out[0][key])))
        assert _rel(out[1][key], out[0][key]) <= TOL, (key, out[1][key], out[0][key])


# ---- 10. misuse -------------------------------------------------------------------------------------------------------------
def test_every_new_refusal_leaves_the_old_list_in_place(backend):
    prob = dvc.clamped_problem(2, 9)
    N = 3
    good = dvc.volume_term(N, "smooth", 0.2, level=0.3, smooth=0.1, labels=[0, 1], deformed=True)
    # a handle set up without mechanics
    plain = _handle(backend, prob, mechanics=False)
    _record(plain, N)
    flat = {k: v for k, v in good.items() if k not in ("deformed", "scale")}
    plain.set_observable_terms([flat])
    J0 = plain.adjoint_gradient([], 2)[0]
    with pytest.raises(backend.BackendError) as e:
        plain.set_observable_terms([flat, good])
    assert e.value.code == backend.GLIMS_E_USAGE and "with_mechanics" in str(e.value), e.value
    assert plain.observable_term_info2(0)["counted"] == int((prob.labels == 1).sum()) and plain.adjoint_gradient([], 2)[0] == J0
    with pytest.raises(backend.BackendError):
        plain.observable_term_info2(1)
    plain.close()
    h = _handle(backend, prob)
    _record(h, N)
    h.set_observable_terms([good, dvc.volume_term(0, "mass", 0.5)])
    J0 = h.adjoint_gradient([], 2)[0]

    def usage(fn, match):
        with pytest.raises(backend.BackendError) as e:
            fn()
        assert e.value.code == backend.GLIMS_E_USAGE, e.value
        assert match in str(e.value), e.value
        assert h.observable_term_info2(0)["counted"] == int((prob.labels == 1).sum())
        assert h.observable_term_info2(1)["counted"] == len(prob.cells) and h.adjoint_gradient([], 2)[0] == J0

    usage(lambda: h.set_observable_terms([dict(good, scale=np.inf)]), "scale")
    usage(lambda: h.set_observable_terms([good, dict(good, scale=np.nan)]), "scale")
    usage(lambda: h.set_observable_terms([dict(good, smooth=0.0)]), "smooth")
    usage(lambda: h.set_observable_terms([dict(good, step=-1)]), "step")
    usage(lambda: h.observable_term_info2(2), "no stored term")
    usage(lambda: h._check(h.lib.glims_adjoint_observable_terms2(h._h, 1, None)), "bad term list")
    h.set_observable_terms([dict(flat, scale=np.inf)])        # the scale of a reference term means nothing
    # second order: every Hessian entry point refuses while a deformed volume term is stored; the gradient works
    h.set_observable_terms([good])
    dirs = [dict(D=[1.0, 0.0])]
    for call in (lambda: h.adjoint_hessian([], dirs), lambda: h.adjoint_hessian([], dirs, collective=True),
                 lambda: h.adjoint_hessian_full([], dirs)):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == backend.GLIMS_E_USAGE and "deformed" in str(e.value) and "second order" in str(e.value), e.value
    for call in (lambda: h.adjoint_hessian([good], dirs), lambda: h.adjoint_hessian_full([good], dirs)):
        with pytest.raises(NotImplementedError):
            call()
    assert h.adjoint_gradient([good], 2)[0] > 0
    h.set_observable_terms([flat])
    assert h.adjoint_hessian([], dirs)["J"] > 0               # the reference-configuration term has its second order
    # a step beyond the recording is reported by the gradient call
    h.set_observable_terms([dict(good, step=N + 4)])
    with pytest.raises(backend.BackendError) as e:
        h.adjoint_gradient([], 2)
    assert e.value.code == backend.GLIMS_E_USAGE and "observes step %d" % (N + 4) in str(e.value)
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
            h.set_observable_terms([dvc.volume_term(0, "mass", 1.0, deformed=True)])
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


# ---- 11. the public API -----------------------------------------------------------------------------------------------------
def test_fit_of_coupling_and_D_to_deformed_volume_series_through_the_public_api(tmp_path):
    """examples/adjoint_fit_deformed_volumes_2D.py at test size (deformed_volume_common.FIT): the data are the deformed T2- /
    T1-like SMOOTH volumes of the whole domain and the deformed volume of the neighbouring tissue B at five steps of a truth run
    with mass effect, and nothing else.  The numpy / scipy twin of this fit (tests/test_deformed_volume_cpu.py) recovers
    (coupling, D) to 1e-3, so the bar is 1e-3."""
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.optimization import ReducedFunctional, minimize
    from glimslib_amd.simulation import TumorGrowth
    F = dvc.FIT

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    def make_sim(coupling, D):
        mesh = fenics.RectangleMesh(fenics.Point(F["lo"], F["lo"]), fenics.Point(F["hi"], F["hi"]), F["n"], F["n"])
        labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1),
                                fenics.FunctionSpace(mesh, "DG", 1))
        sim = TumorGrowth(mesh)
        sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                    boundaries={'boundary_all': Boundary()},
                                    dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                               'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                    von_neumann_bcs={})
        u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
        sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=coupling,
                                   proliferation=F["rho"], E=F["E"], poisson=F["nu"], sim_time=F["steps"] * F["dt"],
                                   sim_time_step=F["dt"])
        return sim

    def terms(s, n_steps, targets=None):
        out = dvc.fit_terms(lambda k, kind, lv, sm, tissue, w: s.volume_term(
            k, 0.0, threshold=lv, kind=kind, smooth=sm, tissues=['b'] if tissue else None, weight=w, deformed=True))
        if targets is not None:
            for t, v in zip(out, targets):
                t["target"] = float(v)
        return out

    # the data: the deformed volumes of the true run, read off the stored terms after one gradient call
    truth = make_sim(*F["truth"])
    truth.run(record_adjoint=True, save_method=None, plot=False, output_dir=str(tmp_path))
    truth.adjoint_gradient(terms(truth, F["steps"]))
    n_terms = 3 * len(F["obs_steps"])
    infos = [truth._backend.observable_term_info2(i) for i in range(n_terms)]
    targets = [i["V"] for i in infos]
    sim_labels = truth._labels()
    truth.close()
    VB = targets[2::3]
    print("tissue B under mass effect: %s" % VB)
    assert all(i["folded"] == 0 and 0.0 < i["min_ratio"] < 1.0 for i in infos)
    assert VB[0] > VB[-1] and VB[0] - VB[-1] > 0.1 and infos[2]["counted"] == int((sim_labels == 2).sum()) > 0

    sim = make_sim(*F["start"])
    rf = ReducedFunctional(sim, 2, lambda s, n: terms(s, n, targets), run_kwargs=dict(output_dir=str(tmp_path)),
                           names=("coupling", "diffusion"))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)          # (no folded cell on the way)
        res = minimize(rf, list(F["start"]), bounds=F["bounds"], options=dict(F["options"]), tol=F["tol"])
    t = np.array(F["truth"])
    print("fit to deformed volume series: %d iterations, %d evaluations, (coupling, D) = (%.12g, %.12g), rel. error %s"
          % (res.nit, rf.evaluations, res.x[0], res.x[1], np.abs(res.x - t) / t))
    assert res.nit <= F["options"]["maxiter"]
    assert np.all(np.abs(res.x - t) <= 1e-3 * t), res
    with pytest.raises(NotImplementedError):
        rf.hessian_matrix(res.x)
    with pytest.raises(NotImplementedError):
        rf.hessian(res.x, np.ones(2))
    with pytest.raises(NotImplementedError):
        sim.adjoint_hessian(terms(sim, F["steps"], targets), [dict(diffusion=1.0)])
    sim.close()
