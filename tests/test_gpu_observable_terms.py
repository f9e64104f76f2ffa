"""
Volume misfit terms on the GPU (glims_adjoint_observable_terms / glims_adjoint_observable_info; k_observe_grad_cells,
k_observe_second_cells, k_observe_grad_sum and the row-owned gather k_observe_grad_rows): J, the gradient and Hessian-vector
products against the numpy statement of tests/observable_terms_common.py (itself checked by central differences in
tests/test_observable_terms_cpu.py), more terms on a step than one cell pass serves, known answers, bitwise repeatability and
neutrality, every refusal, a permuted node order, and a (D, rho) fit to two volume series through the public API.
"""
import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as in test_gpu_adjoint_hessian.py)
import torch  # noqa: F401

import adjoint_image_common as aic
import observable_terms_common as otc
import observe_common as oc
from adjoint_common import Problem, renumber
from test_gpu_adjoint import _record, _rel
from test_gpu_adjoint_image import _attach, _handle, _nostat

pytestmark = pytest.mark.gpu


def _three_labels(base):
    """The problem with a third tissue (label 2) that no cell carries."""
    ext = lambda a, v: np.append(a, v)
    return Problem.from_mesh(base.points, base.cells, base.labels, ext(base.D, 0.03), ext(base.rho, 0.5), ext(base.gamma, 0.1),
                             ext(base.E, 1.5), ext(base.nu, 0.3), base.c0, dt=base.dt, dir_c=base.dir_c)


def _problem(dim):
    """Problem(2, 17): 578 cells, three blocks of the cell pass, the last one partial; Problem(3, 6): 1296 cells.  (N: the 2-D
    run stops at step 4, where the gap rule still holds -- tests/test_observable_terms_cpu.py.)"""
    return (_three_labels(Problem(2, 17)), 4) if dim == 2 else (_three_labels(Problem(3, 6)), 6)


def _check_info(h, prob, traj, terms):
    vol = [t for t in terms if t["kind"] == otc.KIND]
    sum_abs = float(np.abs(otc._Cells(prob).vol).sum())
    bound = oc.bound(len(prob.cells), sum_abs, 1.0)[0]
    for k, t in enumerate(vol):
        c = traj[t["step"]]
        info = h.observable_term_info(k)
        V = otc.measure(prob, t, c)
        print("term %d (%s): V %.12e, numpy %.12e, difference %.3e (bound %.3e), counted %d, cut %d"
              % (k, t["observable"], info["V"], V, abs(info["V"] - V), bound, info["counted"], info["cut"]))
        assert info["counted"] == int(otc.counted_cells(prob, t).sum())
        assert info["cut"] == (otc.cut_cells(prob, t, c) if t["observable"] == "sharp" else -1)
        assert abs(info["V"] - V) <= bound


@pytest.mark.parametrize("dim", [2, 3])
def test_gradient_and_J_match_the_numpy_statement(backend, dim):
    """All three kinds on the last step (masks: all, label 1 only, a label that no cell carries) with a nodal c_thresh term, a
    SHARP term at N/2 and a MASS term at step 0; SHARP levels by the gap rule; Dirichlet nodes on c."""
    prob, N = _problem(dim)
    assert (dim, len(prob.cells)) in ((2, 578), (3, 1296)) and 2 not in prob.labels
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = otc.standard_terms(prob, traj, seed=dim, empty_label=2)
    assert [t.get("observable") for t in terms] == ["sharp", "smooth", "mass", None, "sharp", "mass", "smooth"]
    assert [t["step"] for t in terms] == [N, N, N, N, N // 2, 0, N]
    for t in terms:
        if t.get("observable") == "sharp":
            assert np.abs(traj[t["step"]] - t["level"]).min() >= 1e-2
    if dim == 3:          # the corner, the prism and the cell minus a corner all occur
        n = otc.in_counts(prob, terms[4], traj[N // 2])
        print("3-D in-counts at N/2:", np.bincount(n, minlength=5))
        assert all((n == k).sum() > 0 for k in (1, 2, 3))
    J, dD, drho, _, dc0 = h.adjoint_gradient(terms, prob.n_labels)
    Jn, dDn, drhon, dc0n = otc.adjoint(prob, prob.oracle(), traj, terms)
    for a, b, what in ((J, Jn, "J"), (dD, dDn, "dD"), (drho, drhon, "drho"), (dc0, dc0n, "dc0")):
        print("%d-D %s: rel. difference to numpy %.3e" % (dim, what, _rel(a, b)))
        assert _rel(a, b) <= 1e-8, (what, a, b)
    _check_info(h, prob, traj, terms)
    # the term on the label that no cell carries: V = 0 exactly, J = 1/2 w target^2 exactly, nothing added to the gradient
    empty = terms[-1]
    assert h.observable_term_info(5) == dict(counted=0, cut=-1, V=0.0)
    g6 = h.adjoint_gradient(terms[:-1], prob.n_labels)
    assert all(np.array_equal(x, y) for x, y in zip((dD, drho, dc0), (g6[1], g6[2], g6[4])))
    ge = h.adjoint_gradient([empty], prob.n_labels)
    assert ge[0] == 0.5 * empty["weight"] * empty["target"] ** 2 and not any(np.any(x) for x in ge[1:])
    # each kind alone, so that no kind's error hides behind a larger one
    for kind in ("sharp", "smooth", "mass"):
        only = [t for t in terms[:-1] if t.get("observable") == kind]
        got = h.adjoint_gradient(only, prob.n_labels)
        ref = otc.adjoint(prob, prob.oracle(), traj, only)
        for a, b, what in ((got[0], ref[0], "J"), (got[1], ref[1], "dD"), (got[2], ref[2], "drho"), (got[4], ref[3], "dc0")):
            print("%d-D %s alone, %s: rel. difference to numpy %.3e" % (dim, kind, what, _rel(a, b)))
            assert _rel(a, b) <= 1e-8, (kind, what, a, b)
    h.close()


def _nine_terms(prob, c, step):
    rng = np.random.default_rng(31)
    only1 = np.zeros(prob.n_labels, dtype=np.uint8)
    only1[1] = 1
    level, dist = otc.gap_level(c)
    assert dist >= 1e-2
    specs = [("smooth", 0.2, 0.1, None), ("mass", 0.0, 1.0, None), ("sharp", level, 1.0, None), ("smooth", 0.4, 0.05, only1),
             ("mass", 0.0, 1.0, only1), ("sharp", level, 1.0, only1), ("smooth", 0.3, 0.2, None), ("smooth", 0.5, 0.1, None),
             ("smooth", 0.25, 0.07, only1)]
    terms = []
    for kind, lv, sm, lab in specs:
        t = otc.volume_term(step, kind, 0.0, level=lv, smooth=sm, weight=float(rng.uniform(0.5, 2.0)), labels=lab)
        t["target"] = float(rng.uniform(0.5, 0.9) * otc.measure(prob, t, c))
        terms.append(t)
    return terms


def test_nine_terms_on_one_step_take_two_cell_passes(backend):
    """More terms on a step than GLIMS_OBSERVE_MAX_QUERIES.  On a recording of no steps dJ/dc0 is the terms' own gradient: the
    nine terms in one list give the bits of the first eight and the ninth sent as two lists and added in that order (J
    likewise).  With steps after the observed one the sums pass through linear solves, where the order of the additions is
    no longer defined: there the list matches numpy to 1e-8."""
    prob, N = _problem(2)
    assert backend.OBSERVE_MAX_QUERIES == 8
    h = _handle(backend, prob)
    traj = _record(h, 0)
    terms = _nine_terms(prob, traj[0], 0)
    g9 = h.adjoint_gradient(terms, prob.n_labels)
    gA = h.adjoint_gradient(terms[:8], prob.n_labels)
    gB = h.adjoint_gradient(terms[8:], prob.n_labels)
    assert g9[0] == gA[0] + gB[0] and np.array_equal(g9[4], gA[4] + gB[4]) and np.any(gB[4])
    ref = otc.adjoint(prob, prob.oracle(), traj, terms)
    assert _rel(g9[0], ref[0]) <= 1e-8 and _rel(g9[4], ref[3]) <= 1e-8
    h.close()
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = _nine_terms(prob, traj[N // 2], N // 2)
    got = h.adjoint_gradient(terms, prob.n_labels)
    ref = otc.adjoint(prob, prob.oracle(), traj, terms)
    for a, b, what in ((got[0], ref[0], "J"), (got[1], ref[1], "dD"), (got[2], ref[2], "drho"), (got[4], ref[3], "dc0")):
        print("nine terms, %s: rel. difference to numpy %.3e" % (what, _rel(a, b)))
        assert _rel(a, b) <= 1e-8, (what, a, b)
    _check_info(h, prob, traj, terms)
    h.close()


def test_known_answers_on_the_box(backend):
    """observe_common.box() with c = x_0, a recording of no steps, target 0, weight 1: J = 1/2 V^2 and dJ/dc0 = V dV/dc.
    SHARP, level 0.7: V = (2 - 0.7) * 1 * 1.5 = 1.95 and sum_i dV/dc_i = -dV/dlevel = the cross-section 1.5.
    MASS on one label: dV/dc is that label's lumped mass vector."""
    mesh = oc.box()
    lab = oc.half_labels(mesh)
    n_labels = 3
    t = oc.tables(n_labels)
    h = backend.Handle(mesh.points, mesh.cells, lab)
    h.set_materials(*[t[k] for k in ("D", "rho", "gamma", "E", "nu")])
    h.set_options(dt=1.0)
    h.setup(False)
    h.set_state(np.ascontiguousarray(mesh.points[:, 0]))
    h.adjoint_record(True)
    J, _, _, _, dc0 = h.adjoint_gradient([otc.volume_term(0, "sharp", 0.0, level=0.7)], n_labels)
    V = h.observable_term_info(0)["V"]
    print("sharp: V %.15g, J %.15g, sum dJ/dc0 %.15g" % (V, J, dc0.sum()))
    assert abs(V - 1.95) <= 1e-10 * 1.95 and abs(J - 0.5 * 1.95 ** 2) <= 1e-10 * J
    assert abs(dc0.sum() - 1.95 * 1.5) <= 1e-10 * 1.95 * 1.5
    mask = np.array([0, 0, 1], dtype=np.uint8)
    J, _, _, _, dc0 = h.adjoint_gradient([otc.volume_term(0, "mass", 0.0, labels=mask)], n_labels)
    V = h.observable_term_info(0)["V"]
    cells = np.asarray(mesh.cells)
    vol = np.abs([oc._vol(mesh.points[c].tolist()) for c in cells])
    lumped = np.bincount(cells[lab == 2].ravel(), weights=np.repeat(vol[lab == 2] / 4.0, 4), minlength=len(mesh.points))
    assert V > 0 and _rel(dc0 / V, lumped) <= 1e-10, _rel(dc0 / V, lumped)
    assert h.observable_term_info(0)["counted"] == int((lab == 2).sum())
    h.close()


# ---- second order ---------------------------------------------------------------------------------------------------------
def _directions(prob, seed, count):
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    out = []
    for k in range(count):
        d = dict(D=prob.D * rng.uniform(-1, 1, L), rho=prob.rho * rng.uniform(-1, 1, L))
        if k % 2 == 0:
            d["c0"] = 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
        out.append(d)
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_hessian_products_match_the_numpy_second_order_recursion(backend, dim):
    prob, N = _problem(dim)
    h = _handle(backend, prob)
    traj = _record(h, N)
    terms = [t for t in otc.standard_terms(prob, traj, seed=10 + dim) if t.get("observable") != "sharp"]
    assert [t.get("observable") for t in terms] == ["smooth", "mass", None, "mass"]
    dirs = _directions(prob, 13, 3)
    J, dD, drho, dc0, hv = otc.hessian(prob, prob.oracle(), traj, terms, dirs)
    g = h.adjoint_gradient(terms, prob.n_labels)
    r = h.adjoint_hessian(terms, dirs)
    for a, b, what in ((r["J"], J, "J"), (r["D"], dD, "dD"), (r["rho"], drho, "drho"), (r["c0"], dc0, "dc0")):
        assert _rel(a, b) <= 1e-8, (what, a, b)
    for p in range(len(dirs)):
        for key in ("D", "rho", "c0"):
            e = _rel(r["hv_" + key][p], hv[p][key])
            print("%d-D column %d, hv_%s: rel. difference to numpy %.3e" % (dim, p, key, e))
            assert e <= 1e-8, (p, key, r["hv_" + key][p], hv[p][key])
    # the volume terms alone (the nodal term's second order is far larger)
    vol = [t for t in terms if t["kind"] == otc.KIND]
    hvv = otc.hessian(prob, prob.oracle(), traj, vol, dirs[:1])[4][0]
    rv = h.adjoint_hessian(vol, dirs[:1])
    for key in ("D", "rho", "c0"):
        e = _rel(rv["hv_" + key][0], hvv[key])
        print("%d-D volume terms alone, hv_%s: rel. difference to numpy %.3e" % (dim, key, e))
        assert e <= 1e-8, (key, rv["hv_" + key][0], hvv[key])
    r = h.adjoint_hessian(terms, dirs)
    # J and the gradient are bitwise the gradient call's; the collective entry point and the full one give the same bits
    assert r["J"] == g[0] and all(np.array_equal(x, y) for x, y in zip((r["D"], r["rho"], r["gamma"], r["c0"]), g[1:]))
    rs = h.adjoint_hessian(terms, dirs, collective=True)
    rf = h.adjoint_hessian_full(terms, dirs)
    for key in ("J", "D", "rho", "c0", "hv_D", "hv_rho", "hv_c0"):
        assert np.array_equal(r[key], rs[key]) and np.array_equal(r[key], rf[key]), key
    assert not np.any(rf["hv_E"]) and not np.any(rf["hv_nu"])
    # a stored SHARP term: every Hessian entry point refuses, the gradient still works
    sharp = otc.volume_term(N, "sharp", 1.0, level=otc.gap_level(traj[N])[0])
    h.set_observable_terms([sharp])
    for call in (lambda: h.adjoint_hessian([], dirs), lambda: h.adjoint_hessian([], dirs, collective=True),
                 lambda: h.adjoint_hessian_full([], dirs)):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == backend.GLIMS_E_USAGE and "SHARP" in str(e.value), e.value
    with pytest.raises(NotImplementedError):
        h.adjoint_hessian([sharp], dirs)
    assert h.adjoint_gradient([sharp], prob.n_labels)[0] > 0
    h.close()


# ---- repeatability, neutrality ----------------------------------------------------------------------------------------------
def test_repeatable_bits_and_neutral_towards_everything_else(backend):
    prob = Problem(2, 17)
    N = 4
    img_terms, grid, xp = aic.standard_terms(prob, N, seed=21)          # nodal + image terms
    dirs = _directions(prob, 23, 2)
    a, b = _handle(backend, prob), _handle(backend, prob)
    _attach(a, img_terms, grid, xp)
    traj = _record(a, N)
    assert b.step(N) == 0
    g0 = a.adjoint_gradient(img_terms, 2)        # before any volume term was set
    h0 = a.adjoint_hessian(img_terms, dirs)
    sa, ca, aa = a.stats(), a.get_state(want_u=False)[0], a.adjoint_stats()
    vol = [t for t in otc.standard_terms(prob, traj, seed=3) if t["kind"] == otc.KIND]
    smooth = [t for t in vol if t["observable"] != "sharp"]
    a.set_observable_terms(vol)
    assert a.adjoint_stats() == aa and _nostat(a.stats()) == _nostat(sa)   # the new entry points count nowhere
    assert np.isnan(a.observable_term_info(0)["V"]) and a.observable_term_info(0)["cut"] == -1
    g1 = a.adjoint_gradient(img_terms, 2)        # (the stored volume terms stay: the list carries none of its own)
    g2 = a.adjoint_gradient(img_terms, 2)
    assert g1[0] == g2[0] and all(np.array_equal(x, y) for x, y in zip(g1[1:], g2[1:]))
    assert g1[0] != g0[0] and a.observable_term_info(0)["V"] > 0
    a.set_observable_terms(smooth)
    r1, r2 = a.adjoint_hessian(img_terms, dirs), a.adjoint_hessian(img_terms, dirs)
    assert r1["J"] == r2["J"] and r1["J"] != h0["J"]
    assert all(np.array_equal(r1[k], r2[k]) for k in ("D", "rho", "c0", "hv_D", "hv_rho", "hv_c0"))
    assert _nostat(a.stats()) == _nostat(sa) and np.array_equal(a.get_state(want_u=False)[0], ca)
    a.set_observable_terms([])                   # the list cleared: the calls are what they were
    g3 = a.adjoint_gradient(img_terms, 2)
    h3 = a.adjoint_hessian(img_terms, dirs)
    assert g3[0] == g0[0] and all(np.array_equal(x, y) for x, y in zip(g3[1:], g0[1:]))
    assert h3["J"] == h0["J"] and all(np.array_equal(h3[k], h0[k]) for k in ("D", "rho", "gamma", "c0", "hv_D", "hv_rho",
                                                                              "hv_gamma", "hv_c0"))
    ab = a.adjoint_stats()
    assert {k: v for k, v in ab.items() if k not in ("gradients", "backward_steps", "pcg_its", "ms_backward")} == \
        {k: v for k, v in aa.items() if k not in ("gradients", "backward_steps", "pcg_its", "ms_backward")}
    with pytest.raises(backend.BackendError):
        a.observable_term_info(0)
    assert a.step(3) == 0 and b.step(3) == 0   # the forward run goes on as on a handle that never set a term
    assert np.array_equal(a.get_state(want_u=False)[0], b.get_state(want_u=False)[0])
    assert _nostat(a.stats()) == _nostat(b.stats())
    a.close()
    b.close()


def test_terms_survive_setup_materials_state_and_a_new_recording(backend):
    prob = Problem(2, 9)
    h = _handle(backend, prob)
    traj = _record(h, 2)
    t = otc.volume_term(2, "smooth", 0.1, level=0.3, smooth=0.1, labels=[0, 1])
    h.set_observable_terms([t])
    J0 = h.adjoint_gradient([], 2)[0]
    assert J0 > 0
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.setup(with_mechanics=False)
    h.set_state(prob.c0)
    _record(h, 2)
    assert h.adjoint_gradient([], 2)[0] == pytest.approx(J0, rel=1e-12)
    assert h.observable_term_info(0)["counted"] == int((prob.labels == 1).sum())
    h.close()


def test_mixed_lists_resend_the_stored_terms_only_on_a_change(backend):
    prob = Problem(2, 9)
    h = _handle(backend, prob)
    traj = _record(h, 3)
    terms = otc.standard_terms(prob, traj, seed=25)
    sent = []
    send = h.set_observable_terms
    h.set_observable_terms = lambda ts, **kw: (sent.append(len(ts)), send(ts, **kw))[1]
    g1 = h.adjoint_gradient(terms, 2)
    g2 = h.adjoint_gradient([dict(t) for t in terms], 2)        # equal terms, other objects
    assert sent == [5] and g1[0] == g2[0]
    other = [dict(t, weight=2.0 * t["weight"]) if t.get("observable") == "mass" else t for t in terms]
    g3 = h.adjoint_gradient(other, 2)
    assert sent == [5, 5] and g3[0] != g1[0]
    h.adjoint_gradient(terms[3:4], 2)          # a nodal-only list clears what a mixed list had stored
    assert sent == [5, 5, 0]
    h.close()


# ---- misuse ---------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_old_list_in_place(backend):
    prob = Problem(2, 9)
    N = 3
    fresh = backend.Handle(prob.points, prob.cells, prob.labels)
    fresh.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    with pytest.raises(backend.BackendError) as e:
        fresh.set_observable_terms([otc.volume_term(0, "mass", 1.0)])
    assert e.value.code == backend.GLIMS_E_USAGE and "before glims_setup" in str(e.value)
    fresh.close()
    h = _handle(backend, prob)
    traj = _record(h, N)
    good = otc.volume_term(N, "smooth", 0.2, level=0.3, smooth=0.1, labels=[0, 1])
    h.set_observable_terms([good, otc.volume_term(0, "mass", 0.5)])
    J0 = h.adjoint_gradient([], 2)[0]
    counted = int((prob.labels == 1).sum())

    def usage(fn, match):
        with pytest.raises(backend.BackendError) as e:
            fn()
        assert e.value.code == backend.GLIMS_E_USAGE, e.value
        assert match in str(e.value), e.value
        # the old list is in place
        assert h.observable_term_info(0)["counted"] == counted and h.observable_term_info(1)["counted"] == len(prob.cells)
        assert h.adjoint_gradient([], 2)[0] == J0

    usage(lambda: h.set_observable_terms([dict(good, observable=7)]), "unknown kind")
    usage(lambda: h.set_observable_terms([good, dict(good, smooth=0.0)]), "smooth")
    usage(lambda: h.set_observable_terms([dict(good, smooth=-1.0)]), "smooth")
    usage(lambda: h.set_observable_terms([dict(good, level=np.inf)]), "level")
    usage(lambda: h.set_observable_terms([dict(good, weight=np.nan)]), "weight")
    usage(lambda: h.set_observable_terms([dict(good, target=np.inf)]), "target")
    usage(lambda: h.set_observable_terms([dict(good, step=-1)]), "step")
    usage(lambda: h.observable_term_info(2), "no stored term")
    usage(lambda: h._check(h.lib.glims_adjoint_observable_terms(h._h, 1, None)), "bad term list")
    # smooth <= 0 matters for SMOOTH alone
    h.set_observable_terms([dict(good, observable="sharp", smooth=0.0), dict(good, observable="mass", smooth=-1.0)])
    # a step beyond the recording is reported by the gradient / Hessian call
    h.set_observable_terms([dict(good, step=N + 4)])
    for call in (lambda: h.adjoint_gradient([], 2), lambda: h.adjoint_hessian([], [dict(D=[1.0, 0.0])]),
                 lambda: h.adjoint_hessian_full([], [dict(D=[1.0, 0.0])])):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == backend.GLIMS_E_USAGE and "observes step %d" % (N + 4) in str(e.value)
    # a stored mask whose length is no longer n_labels
    h.set_observable_terms([good])
    ext = lambda a: np.append(a, a[-1])
    h.set_materials(ext(prob.D), ext(prob.rho), ext(prob.gamma), ext(prob.E), ext(prob.nu))
    h.setup(with_mechanics=False)
    h.set_state(prob.c0)
    _record(h, N)
    for call in (lambda: h.adjoint_gradient([], 3), lambda: h.adjoint_hessian([], [dict(D=[1.0, 0.0, 0.0])])):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == backend.GLIMS_E_USAGE and "label mask" in str(e.value), e.value
    h.set_observable_terms([])
    assert h.adjoint_gradient([], 3)[0] == 0.0
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
            h.set_observable_terms([otc.volume_term(0, "mass", 1.0)])
            code = 0
        except B.BackendError as e:
            code = e.code
        h.set_observable_terms([])                # clearing is fine there
        h.adjoint_record(True)
        assert h.step(2) == 0
        nodal = [dict(step=2, kind="c_l2", target=np.zeros(len(part.global_ids)))]
        h.adjoint_gradient(nodal)                 # the handle still works (a collective call every rank makes)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return code

    assert run_threaded_ranks(world, body) == [B.GLIMS_E_USAGE] * world


def test_permuted_node_order_gives_the_same_gradient(backend):
    base = Problem(2, 17)
    N = 4
    out = []
    terms0 = None
    for seed in (None, 11):
        if seed is None:
            prob, perm = base, np.arange(len(base.points))
        else:
            pts, cells, perm = renumber(base.points, base.cells, seed)
            inv = np.argsort(perm)
            prob = Problem.from_mesh(pts, cells, base.labels, base.D, base.rho, base.gamma, base.E, base.nu, base.c0[perm],
                                     dt=base.dt, dir_c=(inv[base.dir_c[0]], base.dir_c[1]))
        h = _handle(backend, prob)
        traj = _record(h, N)
        if terms0 is None:
            terms0 = otc.standard_terms(base, traj, seed=7)
        terms = [dict(t, target=t["target"][perm]) if t["kind"] != otc.KIND else dict(t) for t in terms0]
        J, dD, drho, _, dc0 = h.adjoint_gradient(terms, prob.n_labels)
        h.close()
        back = np.empty_like(dc0)
        back[perm] = dc0   # to the base numbering
        out.append((J, dD, drho, back))
    for a, b, what in zip(out[1], out[0], ("J", "dD", "drho", "dc0")):
        print("%s: rel. difference between the numberings %.3e" % (what, _rel(a, b)))
        assert _rel(a, b) <= 1e-8, (what, a, b)


# ---- the public API -------------------------------------------------------------------------------------------------------
def test_fit_of_D_and_rho_to_two_volume_series_through_the_public_api(tmp_path):
    """The mesh, model, start, bounds and optimiser options of adjoint_image_common.FIT; the data are the T2- and T1-like SMOOTH
    volumes of the whole domain at five steps of a true run (observable_terms_common.FIT_VOLUMES) and nothing else.  The numpy /
    scipy twin of this fit (tests/test_observable_terms_cpu.py) recovers (D, rho) to the 1e-3 of the image fit, so the bar
    stays 1e-3."""
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.optimization import ReducedFunctional, minimize
    from glimslib_amd.simulation import TumorGrowth
    F, FV = aic.FIT, otc.FIT_VOLUMES

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    def make_sim(D, rho):
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
        sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=D, coupling=0.1,
                                   proliferation=rho, E=0.001, poisson=0.4, sim_time=F["steps"] * F["dt"],
                                   sim_time_step=F["dt"])
        return sim

    keys = [(lv, k) for lv in FV["levels"] for k in FV["steps"]]

    def terms(s, n_steps, targets=None, kind='smooth'):
        return [s.volume_term(k, 0.0 if targets is None else targets[(lv, k)], threshold=lv, kind=kind, smooth=FV["smooth"])
                for lv, k in keys]

    # the data: the volumes of the true run, read off the stored terms after one gradient call
    truth = make_sim(*F["truth"])
    truth.run(record_adjoint=True, save_method=None, plot=False, output_dir=str(tmp_path))
    truth.adjoint_gradient(terms(truth, F["steps"]))
    targets = {key: truth._backend.observable_term_info(i)["V"] for i, key in enumerate(keys)}
    table, steps = truth.observe([("smooth", FV["levels"][0], FV["smooth"])])   # (sim.observe of the last step: the same number)
    assert steps[-1] == F["steps"], steps
    assert abs(table[-1, 0, :, 0].sum() - targets[(FV["levels"][0], F["steps"])]) <= 1e-12 * table[-1, 0, :, 0].sum()
    truth.close()
    assert all(v > 0 for v in targets.values()) and targets[(0.2, 10)] > targets[(0.4, 10)] > targets[(0.4, 2)]

    sim = make_sim(*F["start"])
    rf = ReducedFunctional(sim, 2, lambda s, n: terms(s, n, targets), run_kwargs=dict(output_dir=str(tmp_path)))
    res = minimize(rf, list(F["start"]), bounds=F["bounds"], options=dict(F["options"]), tol=F["tol"])
    print("fit to two volume series: %d iterations, %d evaluations, m = %s" % (res.nit, rf.evaluations, res.x))
    assert res.nit <= F["options"]["maxiter"]
    assert abs(res.x[0] - 0.1) <= 1e-3 * 0.1 and abs(res.x[1] - 0.1) <= 1e-3 * 0.1, res
    h = sim._backend
    assert h.observable_term_info(len(keys) - 1)["counted"] == 2 * F["n"] ** 2
    H = rf.hessian_matrix(res.x)                           # the Laplace covariance's ingredient
    assert np.allclose(H, H.T, rtol=1e-8, atol=0) and np.all(np.linalg.eigvalsh(0.5 * (H + H.T)) > 0), H
    # a tissue mask by name, and a sharp term: first order only
    tA = sim.volume_term(F["steps"], 1.0, tissues=['a'])
    assert list(tA["labels"]) == [0, 1, 0] and sim.volume_term(1, 1.0)["labels"] is None
    # ... and through the device: the volume of tissue 'A' alone is the per-label figure glims_observe gives for the final state
    gA = sim.adjoint_gradient([tA])
    info = h.observable_term_info(0)
    VA = h.observe([("smooth", 0.12, 0.01)])[0, 0, 1, 0]
    VB = h.observe([("smooth", 0.12, 0.01)])[0, 0, 2, 0]
    print("tissue A: V %.12e (observe %.12e, tissue B %.12e), counted %d" % (info["V"], VA, VB, info["counted"]))
    assert info["counted"] == int((sim._labels() == 1).sum()) and 0 < info["counted"] < 2 * F["n"] ** 2
    assert abs(info["V"] - VA) <= 1e-12 * VA and abs(VA - VB) > 1e-3 * VA
    assert gA["J"] == 0.5 * (info["V"] - 1.0) ** 2 and np.any(gA["diffusion"]) and np.any(gA["c0"])
    with pytest.raises(ValueError):
        sim.volume_term(1, 1.0, tissues=['nowhere'])
    rf2 = ReducedFunctional(sim, 2, lambda s, n: terms(s, n, targets, kind='sharp'), run_kwargs=dict(output_dir=str(tmp_path)))
    with pytest.raises(NotImplementedError):
        rf2.hessian_matrix(res.x)
    sim.close()
