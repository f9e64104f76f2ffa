"""
Image-space misfit terms on the GPU (glims_adjoint_image_terms / glims_adjoint_image_info; k_img_misfit, k_img_misfit_dir and the
device-pointer transpose): J, the gradient and Hessian-vector products against the numpy statement of
tests/adjoint_image_common.py (itself checked by central differences in tests/test_adjoint_image_cpu.py), chunk and reduction
boundaries of the transpose, a recording of no steps, a permuted node order, central differences of the device's own J on the
brain-like mesh, bitwise repeatability and neutrality, misuse statuses, and a (D, rho) fit to two threshold images through the
public API.
"""
import ctypes as C

import numpy as np
import pytest
# (imported at collection, before any test loads libglimship, as in test_gpu_adjoint_hessian.py: the threaded transport's
#  ctypes.CDLL("libamdhip64.so") must resolve to the runtime the library itself uses)
import torch  # noqa: F401

import adjoint_image_common as aic
import sampler_common as sc
from adjoint_common import Problem, renumber
from test_gpu_adjoint import _SKIP, _record, _rel

pytestmark = pytest.mark.gpu


def _handle(backend, prob, **opts):
    h = backend.Handle(prob.points, prob.cells, prob.labels)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, **opts)
    if prob.dir_c is not None:
        h.set_dirichlet_c(prob.dir_c[0], prob.dir_c[1])
    h.setup(with_mechanics=False)
    h.set_state(prob.c0)
    return h


def _attach(h, terms, grid, xp):
    """The library's samplers of the grid and the point set, put into the image terms."""
    sg, sp = h.sampler_grid(*grid), h.sampler_points(xp)
    for t in terms:
        if t.get("where"):
            t["sampler"] = sg if t["where"] == "grid" else sp
    return sg, sp


def _nostat(st):
    return {k: v for k, v in st.items() if k not in _SKIP}


def _check_info(h, terms, least=0.5):
    """glims_adjoint_image_info of every stored term: the sampler, its point count and numpy's observed count, exactly; no
    term passes on an empty set of points."""
    img = [t for t in terms if t["kind"] in aic.IMAGE_KINDS]
    for k, t in enumerate(img):
        ok, _ = aic.observed(t)
        assert h.image_term_info(k) == (t["sampler"].id, len(ok), int(ok.sum())), (k, h.image_term_info(k), ok.sum())
        assert ok.sum() >= max(3, least * len(ok)), "term %d observes %d of its %d points" % (k, ok.sum(), len(ok))


def _compare_gradient(backend, prob, n_steps, terms, grid, xp, tol=1e-8, least=0.5):
    h = _handle(backend, prob)
    _attach(h, terms, grid, xp)
    traj = _record(h, n_steps)
    J, dD, drho, _, dc0 = h.adjoint_gradient(terms, prob.n_labels)
    Jn, dDn, drhon, dc0n = aic.adjoint(prob, prob.oracle(), traj, terms)
    for a, b, what in ((J, Jn, "J"), (dD, dDn, "dD"), (drho, drhon, "drho"), (dc0, dc0n, "dc0")):
        if n_steps == 0 and what in ("dD", "drho"):
            assert not np.any(a) and not np.any(b), (what, a, b)
            continue
        print("%s: rel. difference to numpy %.3e" % (what, _rel(a, b)))
        assert _rel(a, b) <= tol, (what, a, b)
    _check_info(h, terms, least)
    return h, (J, dD, drho, dc0)


@pytest.mark.parametrize("dim", [2, 3])
def test_gradient_and_J_match_the_numpy_statement(backend, dim):
    """img_thresh (grid; NaN targets, a pweight with zeros and non-unit values, points outside the mesh) + img_l2 (point set)
    + a nodal c_thresh on the last step, an image term midway and one at step 0; Dirichlet nodes on c."""
    prob = Problem(2, 16) if dim == 2 else Problem(3, 6)
    N = 6
    terms, grid, xp = aic.standard_terms(prob, N)
    assert prob.dir_c is not None and len(prob.dir_c[0]) > 0
    assert [t["kind"] for t in terms] == ["img_thresh", "img_l2", "c_thresh", "img_l2", "img_thresh"]
    assert [t["step"] for t in terms] == [N, N, N, N // 2, 0]
    g = terms[0]
    assert (g["loc"][0] < 0).any() and 0.05 < np.isnan(g["target"]).mean() < 0.2
    assert (g["pweight"] == 0).any() and (g["pweight"] > 1).any()
    h, _ = _compare_gradient(backend, prob, N, terms, grid, xp)
    st = h.adjoint_stats()
    assert st["gradients"] == 1 and st["backward_steps"] == N and st["recorded_states"] == N + 1
    h.close()


@pytest.mark.parametrize("case", ["coarse_mesh_fine_grid", "fine_mesh_coarse_grid"])
def test_chunk_and_reduction_boundaries(backend, case):
    """3 x 3 cells under a 97 x 61 grid: a cell holds more than 256 points (several transpose chunks per cell, 24 reduction
    blocks, a last block of 29 points); 24 x 24 cells under a 5 x 4 grid: most cells hold no point."""
    if case == "coarse_mesh_fine_grid":
        prob, size = Problem(2, 3), [97, 61]
    else:
        prob, size = Problem(2, 24), [5, 4]
    N = 3
    terms, grid, xp = aic.standard_terms(prob, N, seed=3, grid_size=size, n_pts=77)
    cell = terms[0]["loc"][0]
    per_cell = np.bincount(cell[cell >= 0], minlength=len(prob.cells))
    assert len(cell) % 256 != 0
    if case == "coarse_mesh_fine_grid":
        assert per_cell.max() > 256 and len(cell) > 256 * 20
    else:
        assert (per_cell == 0).mean() > 0.9
    # (a 5 x 4 grid that overhangs the mesh has 6 of its 20 points inside)
    h, _ = _compare_gradient(backend, prob, N, terms, grid, xp, least=0.5 if case == "coarse_mesh_fine_grid" else 0.15)
    h.close()


def test_recording_of_no_steps(backend):
    """N = 0: only c_0 is recorded, every term observes it; dJ/dc0 is the terms' own gradient, the D and rho rows are 0."""
    prob = Problem(2, 12)
    terms, grid, xp = aic.standard_terms(prob, 0, seed=5)
    assert all(t["step"] == 0 for t in terms)
    h, (J, dD, drho, dc0) = _compare_gradient(backend, prob, 0, terms, grid, xp)
    assert J > 0 and np.any(dc0 != 0)
    r = h.adjoint_hessian(terms, [dict(c0=prob.c0)])
    hv = aic.hessian(prob, prob.oracle(), [prob.c0], terms, [dict(c0=prob.c0)])[4][0]
    assert _rel(r["hv_c0"][0], hv["c0"]) <= 1e-8 and r["J"] == J and np.array_equal(r["c0"], dc0)
    h.close()


def test_permuted_node_order_gives_the_same_gradient(backend):
    base = Problem(2, 16)
    N = 5
    terms0, grid, xp = aic.standard_terms(base, N, seed=7)
    out = []
    for seed in (None, 11):
        if seed is None:
            prob, perm = base, np.arange(len(base.points))
        else:
            pts, cells, perm = renumber(base.points, base.cells, seed)
            inv = np.argsort(perm)
            prob = Problem.from_mesh(pts, cells, base.labels, base.D, base.rho, base.gamma, base.E, base.nu, base.c0[perm],
                                     dt=base.dt, dir_c=(inv[base.dir_c[0]], base.dir_c[1]))
        terms = [dict(t) if t["kind"] in aic.IMAGE_KINDS else dict(t, target=t["target"][perm]) for t in terms0]
        h = _handle(backend, prob)
        _attach(h, terms, grid, xp)
        h.adjoint_record(True)
        assert h.step(N) == 0
        J, dD, drho, _, dc0 = h.adjoint_gradient(terms, prob.n_labels)
        h.close()
        back = np.empty_like(dc0)
        back[perm] = dc0   # to the base numbering
        out.append((J, dD, drho, back))
    for a, b, what in zip(out[1], out[0], ("J", "dD", "drho", "dc0")):
        print("%s: rel. difference between the numberings %.3e" % (what, _rel(a, b)))
        assert _rel(a, b) <= 1e-12, (what, a, b)


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


@pytest.fixture(scope="module")
def hessian_case(backend):
    """One recorded run, its 8-direction Hessian call and the numpy products, shared by the n_dir cases."""
    prob = Problem(2, 16)
    N = 5
    terms, grid, xp = aic.standard_terms(prob, N, seed=9)
    h = _handle(backend, prob)
    _attach(h, terms, grid, xp)
    traj = _record(h, N)
    dirs = _directions(prob, 13, 8)
    ref = aic.hessian(prob, prob.oracle(), traj, terms, dirs)
    g = h.adjoint_gradient(terms, prob.n_labels)
    r8 = h.adjoint_hessian(terms, dirs)
    yield dict(prob=prob, h=h, terms=terms, dirs=dirs, ref=ref, g=g, r8=r8)
    h.close()


@pytest.mark.parametrize("n_dir", [1, 3, 8])
def test_hessian_products_match_the_numpy_second_order_recursion(hessian_case, n_dir):
    s = hessian_case
    h, terms, dirs, g, r8 = s["h"], s["terms"], s["dirs"], s["g"], s["r8"]
    r = r8 if n_dir == 8 else h.adjoint_hessian(terms, dirs[:n_dir])
    J, dD, drho, dc0, hv = s["ref"]
    for a, b, what in ((r["J"], J, "J"), (r["D"], dD, "dD"), (r["rho"], drho, "drho"), (r["c0"], dc0, "dc0")):
        assert _rel(a, b) <= 1e-8, (what, a, b)
    for p in range(n_dir):
        for key in ("D", "rho", "c0"):
            e = _rel(r["hv_" + key][p], hv[p][key])
            print("n_dir %d, column %d, hv_%s: rel. difference to numpy %.3e" % (n_dir, p, key, e))
            assert e <= 1e-8, (p, key, r["hv_" + key][p], hv[p][key])
    # J and the gradient are bitwise the gradient call's
    assert r["J"] == g[0] and all(np.array_equal(x, y) for x, y in zip((r["D"], r["rho"], r["gamma"], r["c0"]), g[1:]))
    assert r["stats"]["tlm_pcg_its"] > 0 and r["stats"]["soa_pcg_its"] > 0


def test_hessian_columns_are_bitwise_independent_of_n_dir(hessian_case):
    s = hessian_case
    for j in (0, 3, 7):
        r1 = s["h"].adjoint_hessian(s["terms"], [s["dirs"][j]])
        for key in ("hv_D", "hv_rho", "hv_gamma", "hv_c0"):
            assert np.array_equal(s["r8"][key][j], r1[key][0]), (j, key)


def test_assembled_hessian_is_symmetric(hessian_case):
    s = hessian_case
    prob = s["prob"]
    L, n = prob.n_labels, len(prob.points)
    rng = np.random.default_rng(17)
    dirs = [{key: np.eye(L)[l]} for key in ("D", "rho") for l in range(L)] + [dict(c0=rng.uniform(-1, 1, n)) for _ in range(2)]
    r = s["h"].adjoint_hessian(s["terms"], dirs)
    V = np.array([aic.flat(prob, d) for d in dirs])
    HV = np.array([np.concatenate([r["hv_D"][j], r["hv_rho"][j], r["hv_c0"][j]]) for j in range(len(dirs))])
    H = V @ HV.T
    print("asymmetry %.3e of max |H| %.3e" % (np.abs(H - H.T).max(), np.abs(H).max()))
    assert np.abs(H - H.T).max() <= 1e-8 * np.abs(H).max(), H


def test_brain_like_mesh_central_differences_of_the_device_J(backend):
    """40 k-node brain-like mesh under a 48^3 grid (NV = 4, voxels outside the brain): the gradient against central
    differences of the device's own J, a Hessian column against central differences of the device's own gradient."""
    from glimslib_amd import workloads
    w = workloads.config_brain_like(40000, isolate=True)
    t = {k: np.asarray(v, dtype=np.float64) for k, v in w.tables.items()}
    pts, cells, lab = w.mesh.points, w.mesh.cells, np.asarray(w.cell_label, dtype=np.int32)
    L = len(t["D"])
    n_steps = 8
    size = np.array([48, 48, 48])
    origin, spacing = sc.overhanging_grid(pts, size)
    keep = {}

    def run(D, rho, fn):
        h = backend.Handle(pts, cells, lab)
        h.set_materials(D, rho, t["gamma"], t["E"], t["nu"])
        h.set_options(dt=w.dt, newton_rtol=1e-13, newton_atol=1e-18)
        h.setup(with_mechanics=False)
        h.set_state(w.c0)
        h.adjoint_record(True)
        assert h.step(n_steps) == 0
        s = h.sampler_grid(origin, spacing, size)
        if not keep:   # targets near the simulated image: J is made where the tumour is
            v = s.apply('c')
            th = lambda x, lv: 0.5 * (np.tanh((x - lv) / 0.1) + 1.0)
            keep["targets"] = [th(1.1 * v, 0.3), th(0.9 * v, 0.7), 0.95 * v]
            keep["mask"] = np.random.default_rng(2).uniform(0.5, 1.5, len(v))
            assert 0.05 < np.isnan(v).mean() < 0.5
        tg = keep["targets"]
        terms = [dict(step=n_steps, kind="img_thresh", level=0.3, smooth=0.1, sampler=s, target=tg[0], pweight=keep["mask"]),
                 dict(step=n_steps, kind="img_thresh", level=0.7, smooth=0.1, weight=0.5, sampler=s, target=tg[1]),
                 dict(step=n_steps // 2, kind="img_l2", sampler=s, target=tg[2])]
        out = fn(h, terms)
        assert h.image_term_info(0)[2] == int((~np.isnan(tg[0])).sum())
        h.close()
        return out

    D0, rho0 = t["D"], t["rho"]
    rng = np.random.default_rng(4)
    pD, pr = D0 * rng.uniform(-1, 1, L), rho0 * rng.uniform(-1, 1, L)
    grad = lambda h, terms: h.adjoint_gradient(terms, L, want_dc0=False)[:3]
    both = lambda h, terms: (grad(h, terms), h.adjoint_hessian(terms, [dict(D=pD, rho=pr)]))
    (J, dD, drho), hv = run(D0, rho0, both)
    eps = 1e-4
    Jp, dDp, drhop = run(D0 + eps * pD, rho0 + eps * pr, grad)
    Jm, dDm, drhom = run(D0 - eps * pD, rho0 - eps * pr, grad)
    num, ana = (Jp - Jm) / (2 * eps), dD @ pD + drho @ pr
    print("J %.6e, directional derivative: adjoint %.9e, central differences %.9e" % (J, ana, num))
    assert J > 0 and abs(ana - num) <= 1e-5 * abs(num), (J, ana, num)
    hnum = np.concatenate([dDp - dDm, drhop - drhom]) / (2 * eps)
    hana = np.concatenate([hv["hv_D"][0], hv["hv_rho"][0]])
    print("Hessian column: rel. difference to central differences of the gradient %.3e" % _rel(hana, hnum))
    assert _rel(hana, hnum) <= 1e-5, (hana, hnum)


# ---- repeatability, neutrality ----------------------------------------------------------------------------------------------
def test_repeatable_bits_and_neutral_towards_everything_else(backend):
    prob = Problem(2, 24)
    N = 6
    terms, grid, xp = aic.standard_terms(prob, N, seed=21)
    nodal = prob.terms(N, with_u=False)
    dirs = _directions(prob, 23, 2)
    a, b = _handle(backend, prob), _handle(backend, prob)
    _attach(a, terms, grid, xp)
    a.adjoint_record(True)
    assert a.step(N) == 0 and b.step(N) == 0
    g0 = a.adjoint_gradient(nodal, 2)       # before any image term was set
    h0 = a.adjoint_hessian(nodal, dirs)
    sa, ca, aa = a.stats(), a.get_state(want_u=False)[0], a.adjoint_stats()
    a.set_image_terms([t for t in terms if t["kind"] in aic.IMAGE_KINDS])
    assert a.image_term_info(0)[0] == terms[0]["sampler"].id
    assert a.adjoint_stats() == aa and _nostat(a.stats()) == _nostat(sa)   # the new entry points count nowhere
    g1 = a.adjoint_gradient(terms, 2)
    g2 = a.adjoint_gradient(terms, 2)
    assert g1[0] == g2[0] and all(np.array_equal(x, y) for x, y in zip(g1[1:], g2[1:]))
    assert g1[0] != g0[0]
    r1, r2 = a.adjoint_hessian(terms, dirs), a.adjoint_hessian(terms, dirs)
    assert r1["J"] == r2["J"] == g1[0]
    assert all(np.array_equal(r1[k], r2[k]) for k in ("D", "rho", "c0", "hv_D", "hv_rho", "hv_c0"))
    assert _nostat(a.stats()) == _nostat(sa) and np.array_equal(a.get_state(want_u=False)[0], ca)
    a.set_image_terms([])                    # the list cleared: nodal-only calls are what they were
    g3 = a.adjoint_gradient(nodal, 2)
    h3 = a.adjoint_hessian(nodal, dirs)
    assert g3[0] == g0[0] and all(np.array_equal(x, y) for x, y in zip(g3[1:], g0[1:]))
    assert h3["J"] == h0["J"] and all(np.array_equal(h3[k], h0[k]) for k in ("D", "rho", "gamma", "c0", "hv_D", "hv_rho",
                                                                              "hv_gamma", "hv_c0"))
    with pytest.raises(backend.BackendError):
        a.image_term_info(0)
    assert a.step(4) == 0 and b.step(4) == 0   # the forward run goes on as on a handle that never saw an adjoint call
    assert np.array_equal(a.get_state(want_u=False)[0], b.get_state(want_u=False)[0])
    assert _nostat(a.stats()) == _nostat(b.stats())
    a.close()
    b.close()


def test_mixed_lists_resend_the_stored_terms_only_on_a_change(backend):
    prob = Problem(2, 12)
    N = 3
    terms, grid, xp = aic.standard_terms(prob, N, seed=25)
    h = _handle(backend, prob)
    _attach(h, terms, grid, xp)
    _record(h, N)
    sent = []
    send = h.set_image_terms
    h.set_image_terms = lambda ts, **kw: (sent.append(len(ts)), send(ts, **kw))[1]
    g1 = h.adjoint_gradient(terms, 2)
    g2 = h.adjoint_gradient(terms, 2)
    assert sent == [4] and g1[0] == g2[0]
    other = [dict(t, weight=2.0 * t["weight"]) if t["kind"] == "img_l2" else t for t in terms]
    g3 = h.adjoint_gradient(other, 2)
    assert sent == [4, 4] and g3[0] != g1[0]
    h.adjoint_gradient(other[2:3], 2)         # a nodal-only list clears what a mixed list had stored
    assert sent == [4, 4, 0]
    h.close()


# ---- misuse ---------------------------------------------------------------------------------------------------------------
def test_misuse_gives_usage_status_not_a_fault(backend):
    prob = Problem(2, 8)
    N = 3
    terms, grid, xp = aic.standard_terms(prob, N, seed=27)
    h = _handle(backend, prob)
    sg, sp = _attach(h, terms, grid, xp)
    _record(h, N)
    img = [t for t in terms if t["kind"] in aic.IMAGE_KINDS]
    h.set_image_terms(img)
    J0 = h.adjoint_gradient([], 2)[0]
    good = img[0]

    def usage(fn, match):
        with pytest.raises(backend.BackendError) as e:
            fn()
        assert e.value.code == backend.GLIMS_E_USAGE, e.value
        assert match in str(e.value), e.value
        # the old list is in place
        assert h.image_term_info(3)[0] == sp.id and h.adjoint_gradient([], 2)[0] == J0

    usage(lambda: h.set_image_terms([dict(good, sampler=12345)]), "unknown sampler")
    usage(lambda: h.set_image_terms([dict(good, kind=7)]), "unknown kind")
    usage(lambda: h.set_image_terms([good, dict(good, smooth=0.0)]), "smooth")
    usage(lambda: h.set_image_terms([dict(good, weight=np.nan)]), "weight")
    bad_q = np.ones(sg.n_points)
    bad_q[5] = -1.0
    usage(lambda: h.set_image_terms([dict(good, pweight=bad_q)]), "pweight[5]")
    bad_q[5] = np.inf
    usage(lambda: h.set_image_terms([dict(good, pweight=bad_q)]), "pweight[5]")
    raw = (backend.ImageMisfit * 1)(backend.ImageMisfit(N, sg.id, 0, 0.0, 1.0, 1.0, None, None))
    usage(lambda: h._check(h.lib.glims_adjoint_image_terms(h._h, 1, raw)), "null target")
    usage(lambda: h._check(h.lib.glims_adjoint_image_info(h._h, 9, (C.c_int64 * 3)())), "no stored term")
    # a sampler in use is not destroyed, and still works
    usage(sg.close, "is used by stored image term")
    assert np.isfinite(sg.apply(prob.c0, fill=0.0)).all()
    # a step beyond the recording is reported by the gradient / Hessian call
    h.set_image_terms([dict(good, step=N + 4)])
    for call in (lambda: h.adjoint_gradient([], 2), lambda: h.adjoint_hessian([], [dict(D=[1.0, 0.0])])):
        with pytest.raises(backend.BackendError) as e:
            call()
        assert e.value.code == backend.GLIMS_E_USAGE and "observes step %d" % (N + 4) in str(e.value)
    h.set_image_terms([])
    sg.close()                                 # no term uses it any more
    assert h.adjoint_gradient(terms[2:3], 2)[0] > 0
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
        s = h.sampler_points(part.points[:part.n_own] * 0.999 + 0.0005)
        try:
            h.set_image_terms([dict(step=0, kind="img_l2", sampler=s, target=np.zeros(s.n_points))])
            code = 0
        except B.BackendError as e:
            code = e.code
        h.set_image_terms([])                  # clearing is fine there
        h.adjoint_record(True)
        assert h.step(2) == 0
        nodal = [dict(step=2, kind="c_l2", target=np.zeros(len(part.global_ids)))]
        h.adjoint_gradient(nodal)              # the handle still works (a collective call every rank makes)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return code

    assert run_threaded_ranks(world, body) == [B.GLIMS_E_USAGE] * world


# ---- the public API -------------------------------------------------------------------------------------------------------
def test_fit_of_D_and_rho_to_two_threshold_images_through_the_public_api(tmp_path):
    """The setting of adjoint_image_common.FIT (its numpy / scipy twin converges in tests/test_adjoint_image_cpu.py): T2- and
    T1-like threshold images of a true run on a grid of about half the mesh width that does not align with the mesh."""
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.optimization import ReducedFunctional, minimize
    from glimslib_amd.simulation import TumorGrowth
    from glimslib_amd.utils.data_io import Image
    F = aic.FIT

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

    truth = make_sim(*F["truth"])
    truth.run(save_method=None, plot=False, output_dir=str(tmp_path))
    c_img = truth.sample_image('concentration', max(truth.results.get_recording_steps()), origin=F["origin"],
                               spacing=F["spacing"], size=F["size"])
    truth.close()
    th = lambda x, lv: 0.5 * (np.tanh((x - lv) / F["smooth"]) + 1.0)
    images = [Image(th(c_img.array, lv), F["origin"], F["spacing"]) for lv in F["levels"]]
    assert 0.0 < np.isnan(images[0].array).mean() < 0.5 and c_img.array.shape == tuple(reversed(F["size"]))

    def terms(s, n_steps):
        return [s.image_term(n_steps, im, kind='img_thresh', level=lv, smooth=F["smooth"])
                for im, lv in zip(images, F["levels"])]

    sim = make_sim(*F["start"])
    rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=str(tmp_path)))
    res = minimize(rf, list(F["start"]), bounds=F["bounds"], options=dict(F["options"]), tol=F["tol"])
    print("fit to two threshold images: %d iterations, %d evaluations, m = %s" % (res.nit, rf.evaluations, res.x))
    assert res.nit <= F["options"]["maxiter"]
    assert abs(res.x[0] - 0.1) <= 1e-3 * 0.1 and abs(res.x[1] - 0.1) <= 1e-3 * 0.1, res
    h = sim._backend
    assert len(sim._image_terms[1]) == 2                  # the same two term objects served every evaluation
    n_vox = int(np.prod(F["size"]))
    assert h.image_term_info(1)[1:] == (n_vox, int((~np.isnan(images[1].array)).sum()))
    H = rf.hessian_matrix(res.x)                           # the Laplace covariance's ingredient
    assert np.allclose(H, H.T, rtol=1e-8, atol=0) and np.all(np.linalg.eigvalsh(0.5 * (H + H.T)) > 0), H
    sim.close()
