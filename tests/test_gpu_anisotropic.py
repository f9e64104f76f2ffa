"""
Anisotropic diffusion on the device (glims_set_diffusion_tensor; DESIGN.md, "Anisotropic diffusion"): trajectory, gradient and
Hessian-vector products against the numpy statement of tests/anisotropic_common.py (itself checked by finite differences in
tests/test_anisotropic_cpu.py), the stretch identity, the identity field, bitwise neutrality of a cleared field, the cell order,
the fast paths of the stepper, the stiff multigrid regime, two threaded ranks, the refusals, and the public API.

Bars.  Gradients and Hessian-vector products: 1e-8 on the GPU's own trajectory, the bar of tests/test_gpu_adjoint*.py for the
same quantities.  Trajectory: no isotropic test compares the device trajectory of these Problems with the oracle's, so TOL_FWD
is 10 x the ISOTROPIC device-to-oracle distance, measured without a field (the parent commit's kernels, instruction for
instruction) with the options of _handle (newton_rtol 1e-13):
    Problem(2, 17), 5 steps: 4.7e-15   Problem(3, 6), 5 steps: 1.2e-14   many_tissues(2, 9, n=12), 3 steps: 5.0e-15
    Problem(3, 10, dt=1) with the RD multigrid, 3 steps: 5.3e-14
(the largest relative l2 distance over the steps; both sides stop Newton at a relative residual of 1e-13 / 1e-14, so the
distance is a small multiple of that tolerance times the condition of the step's Jacobian).
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before libglimship: see tests/test_gpu_adjoint_hessian_partitioned.py)

import anisotropic_common as ac
from adjoint_common import Problem, many_tissues
from test_anisotropic_cpu import FIT_BAR
from test_gpu_adjoint import _SKIP

pytestmark = pytest.mark.gpu

TOL = 1e-8
TOL_FWD = {"2d": 10 * 4.7e-15, "3d": 10 * 1.2e-14, "tissues": 10 * 5.0e-15, "stiff": 10 * 5.3e-14}
# two threaded ranks against the single rank: 10 x the largest distance measured (printed by the test)
TOL_SINGLE = 10 * 1.8e-15
HV = ("hv_D", "hv_rho", "hv_gamma", "hv_c0")


def _handle(backend, prob, T=None, mechanics=True, flags_or=0, **opts):
    h = backend.Handle(prob.points, prob.cells, prob.labels)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12, flags=h.options.flags | flags_or, **opts)
    if prob.dir_c is not None:
        h.set_dirichlet_c(prob.dir_c[0], prob.dir_c[1])
    if mechanics:
        h.set_dirichlet_u(prob.dir_u[0], prob.dir_u[1])
    if T is not None:
        h.set_diffusion_tensor(T)
    h.setup(with_mechanics=mechanics)
    h.set_state(prob.c0)
    return h


def _record(h, n_steps):
    h.adjoint_record(True)
    traj = [h.get_state(want_u=False)[0]]
    for _ in range(n_steps):
        assert h.step(1) == 0
        traj.append(h.get_state(want_u=False)[0])
    return traj


def _rel(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dist(a, b):
    return _rel(a, b) if np.any(b) else float(np.abs(np.asarray(a)).max())


def _traj_dist(ta, tb):
    return max(_rel(x, y) for x, y in zip(ta[1:], tb[1:]))


def _directions(prob, seed, count, gamma=True):
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    out = []
    for k in range(count):
        d = dict(D=prob.D * rng.uniform(-1, 1, L), rho=prob.rho * rng.uniform(-1, 1, L))
        if gamma:
            d["gamma"] = prob.gamma * rng.uniform(-1, 1, L)
        if k % 2 == 0:
            d["c0"] = 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
        out.append(d)
    return out


def _case(name):
    """(prob, T, steps, terms, forward bar) of the three shapes; the random field has eigenvalue ratios up to 10."""
    if name == "2d":
        prob, N = Problem(2, 17), 5            # 578 cells: three blocks of the cell passes, the last one partial
    elif name == "3d":
        prob, N = Problem(3, 6), 5             # 1296 cells
    else:
        prob, N = many_tissues(2, 9, n=12, zero=(4,)), 3   # nine labels (the second GL_ADJ_LT chunk), label 4 with D = rho = 0
        assert prob.D[4] == 0.0 and len(np.unique(prob.labels)) == 9
    T = ac.random_spd(len(prob.cells), prob.dim, seed=3)
    return prob, T, N, prob.terms(N, smooth=0.1), TOL_FWD[name]


def _check_gradient(prob, T, traj, terms, g, tol=TOL):
    ref = ac.adjoint(prob, ac.aniso_oracle(prob, T), traj, terms, T)
    for a, b, what in zip(g, ref, ("J", "dD", "drho", "dgamma", "dc0")):
        e = _dist(a, b)
        print("  %s: %.2e" % (what, e))
        assert e <= tol, (what, e, a, b)
    return ref


# ---- 1. trajectory and gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d", "3d", "tissues"])
def test_trajectory_and_gradient_match_the_numpy_statement(backend, name):
    prob, T, N, terms, tol_fwd = _case(name)
    h = _handle(backend, prob, T)
    info = h.diffusion_tensor_info()
    assert info["present"] and info["n_cells"] == len(prob.cells)
    traj = _record(h, N)
    o = ac.aniso_oracle(prob, T)
    e = _traj_dist(traj, prob.trajectory(o, N))
    print("%s: device trajectory against the numpy statement %.2e (bar %.1e)" % (name, e, tol_fwd))
    assert e <= tol_fwd
    # ... and far from the isotropic trajectory: the tensor is in the operator
    assert _traj_dist(traj, prob.trajectory(prob.oracle(), N)) > 1e-3
    g = h.adjoint_gradient(terms, prob.n_labels)
    _check_gradient(prob, T, traj, terms, g)
    assert np.abs(g[1]).max() > 0 and np.abs(g[3]).max() > 0
    h.close()


# ---- 2. Hessian-vector products ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d", "3d", "tissues"])
def test_hessian_vector_products_match_the_numpy_statement(backend, name):
    prob, T, N, terms, _ = _case(name)
    N = 3
    terms = prob.terms(N, smooth=0.1)
    dirs = _directions(prob, 7, 3)
    h = _handle(backend, prob, T)
    traj = _record(h, N)
    p3 = h.adjoint_hessian(terms, dirs, prob.n_labels)
    p1 = [h.adjoint_hessian(terms, [d], prob.n_labels) for d in dirs]
    J, dD, drho, dgam, dc0, hv = ac.hessian(prob, ac.aniso_oracle(prob, T), traj, terms, dirs, T)
    for a, b, what in ((p3["J"], J, "J"), (p3["D"], dD, "D"), (p3["rho"], drho, "rho"), (p3["gamma"], dgam, "gamma"),
                       (p3["c0"], dc0, "c0")):
        assert _dist(a, b) <= TOL, (what, a, b)
    for p in range(3):
        for key in ("D", "rho", "gamma", "c0"):
            e3, e1 = _dist(p3["hv_" + key][p], hv[p][key]), _dist(p1[p]["hv_" + key][0], hv[p][key])
            print("  %s direction %d hv_%s: %.2e (P = 3), %.2e (P = 1)" % (name, p, key, e3, e1))
            assert e3 <= TOL and e1 <= TOL, (p, key, e3, e1)
        for key in HV:   # column p of the 3-direction call: the bits of the one-direction call
            assert np.array_equal(p3[key][p], p1[p][key][0]), (p, key)
    assert np.abs(p3["hv_D"]).max() > 0
    h.close()


# ---- 3. the stretch identity on the device -------------------------------------------------------------------------------------
def test_stretch_identity_on_the_device(backend):
    """TT = diag(a^2, 1) on the mesh against the isotropic problem on the mesh with x / a (tests/test_anisotropic_cpu.py):
    two device runs, each within TOL_FWD of its numpy statement, and the two statements agree to 1e-12."""
    a, N = 2.0, 4
    prob = Problem(2, 17)
    sq = Problem(2, 17)
    sq.points = prob.points / np.array([a, 1.0])
    ha = _handle(backend, prob, ac.uniform_stretch(len(prob.cells), 2, a), mechanics=False)
    hi = _handle(backend, sq, None, mechanics=False)
    ta, ti = _record(ha, N), _record(hi, N)
    e = _traj_dist(ta, ti)
    print("stretch identity on the device: %.2e (bar %.1e)" % (e, 2 * TOL_FWD["2d"]))
    assert e <= 2 * TOL_FWD["2d"]
    assert abs(ha.diffusion_tensor_info()["max_ratio"] - a * a) <= 1e-12
    ha.close()
    hi.close()


# ---- 4. the identity field ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d", "3d"])
def test_identity_field_agrees_with_no_field(backend, name):
    prob, _, N, terms, tol_fwd = _case(name)
    hI = _handle(backend, prob, ac.identity_field(len(prob.cells), prob.dim))
    h0 = _handle(backend, prob, None)
    tI, t0 = _record(hI, N), _record(h0, N)
    e = _traj_dist(tI, t0)
    print("%s: identity field against no field, trajectory %.2e" % (name, e))
    assert e <= tol_fwd
    gI, g0 = hI.adjoint_gradient(terms, prob.n_labels), h0.adjoint_gradient(terms, prob.n_labels)
    for a, b, what in zip(gI, g0, ("J", "dD", "drho", "dgamma", "dc0")):
        assert _dist(a, b) <= TOL, (what, a, b)
    assert hI.diffusion_tensor_info() == dict(present=True, n_cells=len(prob.cells), max_ratio=1.0)
    assert h0.diffusion_tensor_info() == dict(present=False, n_cells=len(prob.cells), max_ratio=1.0)
    hI.close()
    h0.close()


# ---- 5. neutrality --------------------------------------------------------------------------------------------------------------
def test_a_cleared_field_leaves_the_bits_of_a_handle_that_never_had_one(backend):
    prob, T, N, terms, _ = _case("2d")
    a = _handle(backend, prob, T)
    assert a.step(2) == 0
    a.set_diffusion_tensor(None)
    with pytest.raises(backend.BackendError):   # the operators are gone with the field: glims_setup first
        a.step(1)
    a.setup(with_mechanics=True)
    a.set_state(prob.c0)
    a.reset_stats()
    b = _handle(backend, prob, None)
    b.reset_stats()
    ta, tb = _record(a, N), _record(b, N)
    assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
    ga, gb = a.adjoint_gradient(terms, prob.n_labels), b.adjoint_gradient(terms, prob.n_labels)
    assert ga[0] == gb[0] and all(np.array_equal(x, y) for x, y in zip(ga[1:], gb[1:]))
    assert a.solve_mechanics() == 0 and b.solve_mechanics() == 0
    assert np.array_equal(a.get_state()[1], b.get_state()[1])
    sa, sb = a.stats(), b.stats()
    assert {k: v for k, v in sa.items() if k not in _SKIP} == {k: v for k, v in sb.items() if k not in _SKIP}
    a.close()
    b.close()


# ---- 6. the cell order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d", "3d"])
def test_cells_permuted_with_their_tensors_give_the_same_gradient(backend, name):
    prob, T, N, terms, _ = _case(name)
    h = _handle(backend, prob, T)
    _record(h, N)
    g = h.adjoint_gradient(terms, prob.n_labels)
    h.close()
    perm = np.random.default_rng(8).permutation(len(prob.cells))
    pp = Problem.from_mesh(prob.points, prob.cells[perm], prob.labels[perm], prob.D, prob.rho, prob.gamma, prob.E, prob.nu,
                           prob.c0, dt=prob.dt, dir_c=prob.dir_c, dir_u=prob.dir_u)
    h = _handle(backend, pp, T[perm])
    _record(h, N)
    gp = h.adjoint_gradient(terms, prob.n_labels)
    h.close()
    for a, b, what in zip(gp, g, ("J", "dD", "drho", "dgamma", "dc0")):
        e = _dist(a, b)
        print("  %s permuted cells, %s: %.2e" % (name, what, e))
        assert e <= TOL, (what, e)
    # (the unpermuted field on the permuted cells is another problem: a wrong cell order would show)
    h = _handle(backend, pp, T)
    _record(h, N)
    gw = h.adjoint_gradient(terms, prob.n_labels)
    h.close()
    assert _dist(gw[1], g[1]) > 1e-4


# ---- 7. the fast paths of the stepper --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["random", "uniform"])
def test_fast_paths_decide_from_the_values_of_S(backend, field):
    """The thin box of tests/test_gpu_value_codes.py (linear and non-linear slices in every step) with a tensor field: the
    default flags against each fast path switched off, the same bits.  A uniform tensor keeps the slices of S coded (congruent
    cells); the random field leaves slices whose entries need more than 32 dictionary bases, which are simply uncoded."""
    from test_gpu_value_codes import COUNTS, _thin_box
    w = _thin_box(120, False)
    nc = len(w.mesh.cells)
    T = ac.random_spd(nc, 3, seed=4) if field == "random" else np.broadcast_to(np.diag([3.0, 1.0, 0.5]), (nc, 3, 3))
    t = w.tables

    def run(flags_or):
        h = backend.Handle(w.mesh.points, w.mesh.cells, w.cell_label)
        h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
        h.set_options(dt=w.dt, flags=h.options.flags | flags_or)
        h.set_diffusion_tensor(T)
        h.setup(False)
        h.set_state(w.c0)
        st = 0
        for _ in range(6):
            st |= h.step(1)
        c, s = h.get_state(want_u=False)[0], h.stats()
        h.close()
        assert st == 0 and np.all(np.isfinite(c))
        return c, s

    c0, s0 = run(0)
    print("%s field: slices of S coded %d, uncoded %d, coded passes %d, dot-free solves %d" %
          (field, s0['rd_scode_slices'], s0['rd_scode_uncoded_slices'], s0['cheb_coded_passes'], s0['cheb_solves']))
    assert s0['cheb_solves'] > 0
    if field == "uniform":
        assert s0['rd_scode_uncoded_slices'] == 0 and s0['cheb_coded_passes'] > 0
    else:
        assert s0['rd_scode_uncoded_slices'] > 0
    for flag in ("NO_VALUE_CODES", "RECORD_WORDS_FULL", "SLOT_WORDS32", "NO_FUSED_GUESS", "STORE_LINEAR_SLICES"):
        c1, s1 = run(getattr(backend, "FLAG_" + flag))
        assert np.array_equal(c0, c1), flag
        for k in ('newton_its', 'rd_assemblies', 'cg_its', 'cheb_its', 'cheb_solves'):
            assert k in COUNTS and s0[k] == s1[k], (flag, k, s0[k], s1[k])


# ---- 8. the stiff regime ----------------------------------------------------------------------------------------------------------
def test_stiff_regime_with_the_rd_multigrid(backend):
    N = 3
    prob = Problem(3, 10, dt=1.0, D=(0.1, 0.2), rho=(0.05, 0.1))
    xb = np.nonzero(((prob.points <= 1e-12) | (prob.points >= 1.0 - 1e-12)).any(axis=1))[0]
    prob.dir_c = (xb, np.full(len(xb), 0.05))
    T = ac.random_spd(len(prob.cells), 3, seed=5)
    terms = prob.terms(N, with_u=False)
    h = _handle(backend, prob, T, mechanics=False, rd_precond=backend.RD_PRECOND_MULTIGRID)
    traj = _record(h, N)
    assert h.stats()["rd_precond_used"] == backend.RD_PRECOND_MULTIGRID
    e = _traj_dist(traj, prob.trajectory(ac.aniso_oracle(prob, T), N))
    print("stiff regime: device trajectory against the numpy statement %.2e (bar %.1e)" % (e, TOL_FWD["stiff"]))
    assert e <= TOL_FWD["stiff"]
    g = h.adjoint_gradient(terms, prob.n_labels)
    _check_gradient(prob, T, traj, terms, g)
    h.close()


# ---- 9. two threaded ranks --------------------------------------------------------------------------------------------------------
def _rank(prob, T, world, rank, tr, owner, N, terms, dirs):
    from glimslib_amd import _backend as B
    from glimslib_amd.partition import build_local_part
    n = len(prob.points)
    if world > 1:
        part = build_local_part(prob.points, prob.cells, owner, rank, world)
        gid, n_own = part.global_ids, part.n_own
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(prob.points.min(axis=0), prob.points.max(axis=0))
        h.set_diffusion_tensor(T[part.cell_ids])       # rank-local: the rank's cells
    else:
        gid, n_own = np.arange(n), n
        h = B.Handle(prob.points, prob.cells, prob.labels)
        h.set_diffusion_tensor(T)
    g2l = np.full(n, -1, dtype=np.int64)
    g2l[gid[:n_own]] = np.arange(n_own)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16)
    loc = g2l[np.asarray(prob.dir_c[0])]
    h.set_dirichlet_c(loc[loc >= 0], np.asarray(prob.dir_c[1], float)[loc >= 0])
    h.setup(with_mechanics=False)
    h.set_state(prob.c0[gid])
    h.adjoint_record(True)
    traj = [h.get_state(want_u=False)[0][:n_own]]
    for _ in range(N):
        assert h.step(1) == 0
        traj.append(h.get_state(want_u=False)[0][:n_own])
    lt = [dict(t, target=np.asarray(t["target"], float)[gid]) for t in terms]
    ld = [dict(d, c0=np.asarray(d["c0"])[gid]) if d.get("c0") is not None else dict(d) for d in dirs]
    g = h.adjoint_gradient(lt)
    r = h.adjoint_hessian(lt, ld, collective=world > 1)
    assert not np.any(r["hv_c0"][:, n_own:])
    out = dict(gid=gid[:n_own], traj=traj, grad=(g[0], g[1], g[2], g[3], g[4][:n_own]),
               res=dict(r, c0=r["c0"][:n_own], hv_c0=r["hv_c0"][:, :n_own]))
    h.close()
    if tr is not None and getattr(tr, "failed", None) is not None:
        raise tr.failed
    return out


def _gather(res, n, pick):
    out = np.full(n, np.nan)
    for r in res:
        out[r["gid"]] = pick(r)
    assert not np.isnan(out).any()
    return out


def test_two_threaded_ranks_with_stripes_that_cut_cells(backend):
    """The stripe owners of test_stripes_cut_cells_of_many_labels_and_a_label_missing_on_a_rank, the field localised by the
    part's cell_ids.  Every rank: the same bits of J and the per-label arrays; against numpy 1e-8; the distance to the single
    rank is printed and held to TOL_SINGLE."""
    from glimslib_amd.parallel import run_threaded_ranks
    world, N = 2, 3
    prob = many_tissues(2, 9, n=12, seed=5)
    owner = (np.floor(prob.points[:, 1] * 4 - 1e-9).astype(np.int64).clip(0, 3) % 2).astype(np.int32)
    T = ac.random_spd(len(prob.cells), 2, seed=6)
    terms = prob.terms(N, with_u=False)
    dirs = _directions(prob, 9, 3, gamma=False)
    n = len(prob.points)
    ref = _rank(prob, T, 1, 0, None, None, N, terms, dirs)
    res = run_threaded_ranks(world, lambda r, tr: _rank(prob, T, world, r, tr, owner, N, terms, dirs))
    keys = ("D", "rho", "gamma", "hv_D", "hv_rho", "hv_gamma")
    for r in res:
        assert r["res"]["J"] == res[0]["res"]["J"] == r["grad"][0]
        for k in keys:
            assert np.array_equal(r["res"][k], res[0]["res"][k]), k
        assert all(np.array_equal(p, q) for p, q in zip((r["res"]["D"], r["res"]["rho"], r["res"]["gamma"]), r["grad"][1:4]))
    traj = [_gather(res, n, lambda r, k=k: r["traj"][k]) for k in range(N + 1)]
    J, dD, drho, dgam, dc0, hv = ac.hessian(prob, ac.aniso_oracle(prob, T), traj, terms, dirs, T)
    x = res[0]["res"]
    c0 = _gather(res, n, lambda r: r["res"]["c0"])
    hc0 = [_gather(res, n, lambda r, p=p: r["res"]["hv_c0"][p]) for p in range(3)]
    for a, b, what in ((x["J"], J, "J"), (x["D"], dD, "D"), (x["rho"], drho, "rho"), (c0, dc0, "c0")):
        assert _dist(a, b) <= TOL, (what, a, b)
    for p in range(3):
        for key in ("D", "rho"):
            assert _dist(x["hv_" + key][p], hv[p][key]) <= TOL, (p, key)
        assert _dist(hc0[p], hv[p]["c0"]) <= TOL, (p, "c0")
    y = ref["res"]
    worst = max([_dist(x[k], y[k]) for k in ("J",) + keys] + [_dist(c0, y["c0"])] +
                [_dist(hc0[p], y["hv_c0"][p]) for p in range(3)])
    print("two threaded ranks with a tensor field: largest rel. distance to the single rank %.3e (bar %.1e)" % (worst, TOL_SINGLE))
    assert worst <= TOL_SINGLE


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------
def test_bad_tensors_are_refused_and_the_old_field_stays(backend):
    prob, T, N, terms, _ = _case("2d")
    h = _handle(backend, prob, T, mechanics=False)
    want = ac.max_ratio(T)
    assert abs(h.diffusion_tensor_info()["max_ratio"] - want) <= 1e-12
    assert h.step(1) == 0
    c1 = h.get_state(want_u=False)[0]
    P = ac.pack(T)
    semi = np.array([1.0, 2.0, 4.0])          # (1, 2)(1, 2)^T: determinant exactly 0
    for value, cellsbad in (((np.nan, 0.0, 1.0), [431, 17, 300]), ((1.0, 2.0, 1.0), [5]), (semi, [577, 64])):
        Q = P.copy()
        Q[cellsbad] = value
        with pytest.raises(backend.BackendError) as e:
            h.set_diffusion_tensor(Q)
        assert e.value.code == backend.GLIMS_E_USAGE
        msg = str(e.value)
        assert ("%d diffusion tensor(s)" % len(cellsbad)) in msg, msg
        assert "the first one is cell %d " % min(cellsbad) in msg, msg
        # the old field is in place and the handle still steps, without a new setup
        assert abs(h.diffusion_tensor_info()["max_ratio"] - want) <= 1e-12
    assert h.step(1) == 0
    c2 = h.get_state(want_u=False)[0]
    h.close()
    # ... to the state a handle reaches that saw no refused call
    h = _handle(backend, prob, T, mechanics=False)
    assert h.step(2) == 0
    assert np.array_equal(h.get_state(want_u=False)[0], c2) and not np.array_equal(c1, c2)
    h.close()
    # 3-D: the ratio of a field with coinciding eigenvalues (fibre tensors) and of the random field
    p3 = Problem(3, 6)
    from glimslib_amd.utils.data_io import tensor_from_fibres
    e3 = np.random.default_rng(2).standard_normal((len(p3.cells), 3))
    for T3 in (ac.random_spd(len(p3.cells), 3, seed=9), tensor_from_fibres(e3, 7.0)):
        h = backend.Handle(p3.points, p3.cells, p3.labels)
        h.set_diffusion_tensor(T3)
        got, want3 = h.diffusion_tensor_info()["max_ratio"], ac.max_ratio(T3)
        assert abs(got - want3) <= 1e-12, (got, want3)
        bad = ac.pack(T3)
        bad[[700, 123], 5] = -0.1             # zz < 0: indefinite
        with pytest.raises(backend.BackendError, match="2 diffusion tensor.*first one is cell 123 "):
            h.set_diffusion_tensor(bad)
        h.close()


# ---- 11. the public API -----------------------------------------------------------------------------------------------------------
def test_public_api_fit_and_second_moments(backend, tmp_path):
    from glimslib_amd.optimization import ReducedFunctional, minimize
    F = ac.FIT
    _make_sim = ac.make_fit_sim
    prob, T = ac.fit_problem()
    out = str(tmp_path)
    truth = _make_sim(F["D"], F["rho"])
    assert np.array_equal(truth._labels(), prob.labels) and np.array_equal(truth._diffusion_tensor, ac.pack(T))
    truth.run(save_method=None, plot=False, output_dir=out)
    c_end = truth.solution.components[1].copy()
    lumped = truth._lumped()
    truth.close()
    # the same discrete problem as the twin's
    ref = prob.trajectory(ac.aniso_oracle(prob, T), F["steps"])[-1]
    assert _rel(c_end, ref) <= 1e-8
    iso = _make_sim(F["D"], F["rho"], with_tensor=False)
    iso.run(save_method=None, plot=False, output_dir=out)
    c_iso = iso.solution.components[1].copy()
    iso.close()
    # second moment along the fibres (x) relative to across them, with and without the field
    Ca, Ci = ac.second_moment_ratio(prob.points, lumped, c_end)[1], ac.second_moment_ratio(prob.points, lumped, c_iso)[1]
    ra, ri = Ca[0, 0] / Ca[1, 1], Ci[0, 0] / Ci[1, 1]
    print("second moment along / across the fibres: %.4f with the field, %.4f without" % (ra, ri))
    assert ra > ri
    terms = lambda sim, n_steps: ac.fit_terms(c_end, n_steps)
    sim = _make_sim(*F["start"])
    rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out))
    res = minimize(rf, list(F["start"]), options={"maxiter": 60, "gtol": 1e-12, "ftol": 1e-16}, tol=1e-16)
    err = float(np.abs(res.x / np.array([F["D"], F["rho"]]) - 1.0).max())
    print("device fit: D = %.10f, rho = %.10f, recovery error %.2e (bar %.1e), J = %.2e, %d evaluations" %
          (res.x[0], res.x[1], err, FIT_BAR, res.fun, rf.evaluations))
    sim.close()
    assert err <= FIT_BAR
