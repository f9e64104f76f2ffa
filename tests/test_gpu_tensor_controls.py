"""
Tensor-field controls on the device (glims_set_diffusion_tensor_tangents / glims_adjoint_tensor_gradient; DESIGN.md,
"Anisotropic diffusion", section "Tangent fields"): the per-label sums of k_sens_tangent against the numpy statement
tests/tensor_controls_common.tangent_gradient (itself checked by central differences in tests/test_tensor_controls_cpu.py) where
the kernel branches -- K = 1 .. 4, 2-D and 3-D, a partial last block, two label windows with a label that has no cells, terms
on several steps, no base field, indefinite and zero tangents --, the identity tangent = TT, bitwise neutrality for every
other output of the gradient and Hessian calls, no invalidation of a recording, the cell order, the refusals, two threaded
ranks, and the fit of (D, rho, ratio) through the public API.

Bars.  TOL = 1e-8 on the GPU's own trajectory, the bar of tests/test_gpu_anisotropic.py for dJ/dD: the tangent sums are that
sum with another matrix in the middle.  TOL_SINGLE (two ranks against one) is that file's, measured there for the dD sums of
the same reduction.  FIT_RATIO_BAR comes from the scipy twin in tests/test_tensor_controls_cpu.py.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before libglimship: see tests/test_gpu_adjoint_hessian_partitioned.py)

import anisotropic_common as ac
import tensor_controls_common as tc
from adjoint_common import Problem, many_tissues
from test_gpu_anisotropic import TOL, TOL_SINGLE, _directions, _dist, _gather, _handle, _record
from test_tensor_controls_cpu import FIT_RATIO_BAR

pytestmark = pytest.mark.gpu


def _tangents(prob, T, K, seed=31):
    """K fields: the fibre tangent of a random-direction family first, then an indefinite Gaussian field, the base tensor
    itself (the identity case) and the zero field."""
    nc, d = len(prob.cells), prob.dim
    fibre = tc.fibre_family(tc.random_directions(nc, d, seed))(4.0)[1]
    base = T if T is not None else ac.identity_field(nc, d)
    return np.stack([fibre, tc.random_tangents(nc, d, 1, seed + 1)[0], base, np.zeros((nc, d, d))][:K])


def _case(name):
    """(prob, T, steps, terms, tangents) of the gradient cases."""
    if name.startswith("2d"):
        prob, N = Problem(2, 17), 4                # 578 cells: three blocks of the cell pass, the last one partial, and far
    elif name.startswith("3d"):                    # fewer than one stride of the fixed grid
        prob, N = Problem(3, 6), 3                 # 1296 cells
    else:
        # nine label ids in two windows of GL_ADJ_LT = 8, id 6 without cells
        prob, N = many_tissues(2, 9, n=12, empty=(6,), seed=5), 3
        assert len(np.unique(prob.labels)) == 8 and prob.n_labels == 9 and not np.any(prob.labels == 6)
    nc = len(prob.cells)
    assert nc % 256 != 0
    T = None if name == "2d-no-base-K2" else ac.random_spd(nc, prob.dim, seed=3)
    terms = prob.terms(N, smooth=0.1)
    if name == "2d-steps-K2":                      # a concentration term on every step: the sums accumulate over the sweep
        rng = np.random.default_rng(2)
        terms = [dict(step=k, kind="c_l2" if k % 2 else "c_thresh", level=0.3, smooth=0.1, weight=1.0 + k,
                      target=rng.uniform(0, 0.6, len(prob.points))) for k in range(1, N + 1)]
    if name == "2d-indefinite-K1":
        dTs = tc.random_tangents(nc, prob.dim, 1, seed=8)
        w = np.linalg.eigvalsh(dTs[0])
        assert np.mean((w[:, 0] < 0) & (w[:, -1] > 0)) > 0.5    # most cells: one negative and one positive eigenvalue
    else:
        dTs = _tangents(prob, T, int(name[-1]))
    return prob, T, N, terms, dTs


def _reference(prob, T, traj, terms, dTs):
    o = ac.aniso_oracle(prob, T) if T is not None else prob.oracle()
    return tc.tangent_gradient(prob, o, traj, terms, T, dTs)


def _check(name, got, ref, tol=TOL):
    assert got.shape == ref.shape
    for k in range(len(ref)):
        e = _dist(got[k], ref[k])
        print("  %s tangent %d: dJ/dtheta per label against numpy %.2e" % (name, k, e))
        assert e <= tol, (name, k, e, got[k], ref[k])


def _usage_error(backend, call):
    with pytest.raises(backend.BackendError) as e:
        call()
    assert e.value.code == backend.GLIMS_E_USAGE
    return str(e.value)


# ---- 1. the gradient cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d-K1", "2d-K4", "3d-K2", "3d-K4", "tissues-K3", "2d-steps-K2", "2d-no-base-K2",
                                  "2d-indefinite-K1"])
def test_tensor_gradient_matches_the_numpy_statement(backend, name):
    prob, T, N, terms, dTs = _case(name)
    h = _handle(backend, prob, T)
    h.set_diffusion_tensor_tangents(dTs)
    traj = _record(h, N)
    g = h.adjoint_gradient(terms, prob.n_labels)
    got = h.adjoint_tensor_gradient()
    ref = _reference(prob, T, traj, terms, dTs)
    _check(name, got, ref)
    assert np.abs(got[0]).max() > 0
    if name == "tissues-K3":
        assert not np.any(got[:, 6])               # the label without cells: exactly 0
        assert np.abs(got[0, 8]).max() > 0         # the second label window
    if name.endswith("K4"):
        assert not np.any(got[3])                  # the zero tangent: exactly 0
    if len(dTs) >= 3 and T is not None:
        # 2. the identity on the device: tangent = the stored TT gives D_t dJ/dD_t of the same call
        e = _dist(got[2], prob.D * g[1])
        print("  %s: tangent = TT against D dJ/dD of the same call %.2e" % (name, e))
        assert e <= TOL
    h.close()


# ---- 3. nothing else moves; 4. no invalidation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d-K4", "3d-K2"])
def test_tangents_change_no_other_output_and_invalidate_nothing(backend, name):
    prob, T, N, terms, dTs = _case(name)
    dirs = _directions(prob, 7, 2)
    h = _handle(backend, prob, T)
    traj = _record(h, N)
    msg = _usage_error(backend, h.adjoint_tensor_gradient)            # nothing stored
    assert "no tangent fields" in msg, msg
    g0 = h.adjoint_gradient(terms, prob.n_labels)
    r0 = h.adjoint_hessian(terms, dirs, prob.n_labels)
    # tangents after the recorded run: no new run, no new setup
    h.set_diffusion_tensor_tangents(dTs)
    msg = _usage_error(backend, h.adjoint_tensor_gradient)            # no sweep since they were set
    assert "no backward sweep has completed" in msg, msg
    g1 = h.adjoint_gradient(terms, prob.n_labels)
    tg = h.adjoint_tensor_gradient()
    _check(name, tg, _reference(prob, T, traj, terms, dTs))
    r1 = h.adjoint_hessian(terms, dirs, prob.n_labels)
    th = h.adjoint_tensor_gradient()
    assert g0[0] == g1[0] and all(np.array_equal(a, b) for a, b in zip(g0[1:], g1[1:]))
    assert set(r0) == set(r1)
    for key in r0:
        if key != "stats":
            assert np.array_equal(r0[key], r1[key]), key
    assert np.array_equal(th, tg)                                      # the same sweep in both calls: the same bits
    assert np.array_equal(h.adjoint_tensor_gradient(), tg)             # the getter does not consume
    # new tangents close the getter until the next sweep, which then serves them
    h.set_diffusion_tensor_tangents(dTs * 2.0)
    _usage_error(backend, h.adjoint_tensor_gradient)
    g2 = h.adjoint_gradient(terms, prob.n_labels)
    assert np.array_equal(h.adjoint_tensor_gradient(), 2.0 * tg)       # (a power of two: exact)
    assert all(np.array_equal(a, b) for a, b in zip(g0[1:], g2[1:]))
    # a new tensor field leaves the stored tangents alone (they belong to the mesh's cells)
    h.set_diffusion_tensor(ac.identity_field(len(prob.cells), prob.dim))
    assert h.n_tangents == len(dTs)
    h.close()


# ---- 5. the cell order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2d-K4", "3d-K2"])
def test_cells_permuted_with_their_tensors_and_tangents_give_the_same_tensor_gradient(backend, name):
    prob, T, N, terms, dTs = _case(name)

    def run(p, Tp, dTp):
        h = _handle(backend, p, Tp)
        h.set_diffusion_tensor_tangents(dTp)
        _record(h, N)
        h.adjoint_gradient(terms, prob.n_labels)
        out = h.adjoint_tensor_gradient()
        h.close()
        return out

    g = run(prob, T, dTs)
    perm = np.random.default_rng(8).permutation(len(prob.cells))
    pp = Problem.from_mesh(prob.points, prob.cells[perm], prob.labels[perm], prob.D, prob.rho, prob.gamma, prob.E, prob.nu,
                           prob.c0, dt=prob.dt, dir_c=prob.dir_c, dir_u=prob.dir_u)
    gp = run(pp, T[perm], dTs[:, perm])
    for k in range(len(dTs)):
        e = _dist(gp[k], g[k])
        print("  %s permuted cells, tangent %d: %.2e" % (name, k, e))
        assert e <= TOL
    # (the unpermuted tangents on the permuted cells are another problem: a wrong cell order would show)
    gw = run(pp, T[perm], dTs)
    assert _dist(gw[0], g[0]) > 1e-4


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_bad_tangents_are_refused_and_the_stored_ones_stay(backend):
    prob, T, N, terms, _ = _case("2d-K1")
    dTs = _tangents(prob, T, 3)
    h = _handle(backend, prob, T)
    h.set_diffusion_tensor_tangents(dTs)
    _record(h, N)
    g = h.adjoint_gradient(terms, prob.n_labels)
    tg = h.adjoint_tensor_gradient()
    nan2, inf0, both = dTs.copy(), dTs.copy(), dTs.copy()
    nan2[2, [300, 7], 0, 0] = np.nan
    inf0[0, 3, 0, 1] = inf0[0, 3, 1, 0] = np.inf
    both[2, [300, 7], 0, 0] = np.nan
    both[0, 3, 1, 1] = -np.inf
    for bad, parts in ((nan2, ["tangent 2: 2 cell(s)", "the first one is cell 7"]),
                       (inf0, ["tangent 0: 1 cell(s)", "the first one is cell 3"]),
                       (both, ["tangent 0: 1 cell(s)", "the first one is cell 3", "tangent 2: 2 cell(s)", "the first one is cell 7"])):
        with np.errstate(invalid="ignore"):       # (inf - inf in the Python-side symmetry check: goes on to the library)
            msg = _usage_error(backend, lambda: h.set_diffusion_tensor_tangents(bad))
        assert all(p in msg for p in parts), msg
        assert "tangent 1" not in msg, msg
        # the stored tangents stay, and so does the last sweep's result
        assert h.n_tangents == 3 and np.array_equal(h.adjoint_tensor_gradient(), tg)
    msg = _usage_error(backend, lambda: h.set_diffusion_tensor_tangents(np.concatenate([dTs, dTs[:2]])))   # K = 5
    assert "at most 4" in msg, msg
    assert h.n_tangents == 3
    g1 = h.adjoint_gradient(terms, prob.n_labels)
    assert np.array_equal(h.adjoint_tensor_gradient(), tg)            # the next gradient: the previous bits
    assert all(np.array_equal(a, b) for a, b in zip(g[1:], g1[1:]))
    with pytest.raises(ValueError, match="not symmetric"):            # the messages of the tensor
        skew = dTs.copy()
        skew[1, 5, 0, 1] += 1e-3
        h.set_diffusion_tensor_tangents(skew)
    h.set_diffusion_tensor_tangents(None)                              # None clears
    assert h.n_tangents == 0
    _usage_error(backend, h.adjoint_tensor_gradient)
    g2 = h.adjoint_gradient(terms, prob.n_labels)
    assert all(np.array_equal(a, b) for a, b in zip(g[1:], g2[1:]))
    _usage_error(backend, h.adjoint_tensor_gradient)
    h.close()


# ---- 7. two threaded ranks --------------------------------------------------------------------------------------------------------
def _rank(prob, T, dTs, world, rank, tr, owner, N, terms, dirs):
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
        h.set_diffusion_tensor(T[part.cell_ids])                       # rank-local: the rank's cells
        h.set_diffusion_tensor_tangents(dTs[:, part.cell_ids])
    else:
        gid, n_own = np.arange(n), n
        h = B.Handle(prob.points, prob.cells, prob.labels)
        h.set_diffusion_tensor(T)
        h.set_diffusion_tensor_tangents(dTs)
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
    tg = h.adjoint_tensor_gradient()
    h.adjoint_hessian(lt, ld, collective=world > 1)
    th = h.adjoint_tensor_gradient()
    out = dict(gid=gid[:n_own], traj=traj, dD=g[1], tg=tg, th=th)
    h.close()
    if tr is not None and getattr(tr, "failed", None) is not None:
        raise tr.failed
    return out


def test_two_threaded_ranks_with_stripes_that_cut_cells(backend):
    """The stripe owners of tests/test_gpu_anisotropic.py's test of the same name, tensors and tangents localised by the part's
    cell_ids.  Every rank: the same bits, after the gradient call and after the collective Hessian call; against numpy TOL;
    the distance to the single rank is printed and held to TOL_SINGLE."""
    from glimslib_amd.parallel import run_threaded_ranks
    world, N = 2, 3
    prob = many_tissues(2, 9, n=12, seed=5)
    owner = (np.floor(prob.points[:, 1] * 4 - 1e-9).astype(np.int64).clip(0, 3) % 2).astype(np.int32)
    T = ac.random_spd(len(prob.cells), 2, seed=6)
    dTs = _tangents(prob, T, 2)
    terms = prob.terms(N, with_u=False)
    dirs = _directions(prob, 9, 1, gamma=False)
    n = len(prob.points)
    ref = _rank(prob, T, dTs, 1, 0, None, None, N, terms, dirs)
    res = run_threaded_ranks(world, lambda r, tr: _rank(prob, T, dTs, world, r, tr, owner, N, terms, dirs))
    for r in res:
        assert r["tg"].shape == (2, prob.n_labels)
        assert np.array_equal(r["tg"], res[0]["tg"]) and np.array_equal(r["th"], res[0]["tg"])
    assert np.array_equal(ref["th"], ref["tg"])
    traj = [_gather(res, n, lambda r, k=k: r["traj"][k]) for k in range(N + 1)]
    _check("two ranks", res[0]["tg"], _reference(prob, T, traj, terms, dTs))
    worst = max(_dist(res[0]["tg"][k], ref["tg"][k]) for k in range(2))
    print("two threaded ranks, tensor gradient: largest rel. distance to the single rank %.3e (bar %.1e; dD: %.3e)"
          % (worst, TOL_SINGLE, _dist(res[0]["dD"], ref["dD"])))
    assert worst <= TOL_SINGLE


# ---- 8. the public API ------------------------------------------------------------------------------------------------------------
def test_public_api_fits_diffusion_proliferation_and_the_anisotropy_ratio(backend, tmp_path):
    from glimslib_amd.optimization import ReducedFunctional, minimize
    F = ac.FIT
    out = str(tmp_path)
    truth = ac.make_fit_sim(F["D"], F["rho"])
    truth.run(save_method=None, plot=False, output_dir=out)
    c_end = truth.solution.components[1].copy()
    truth.close()
    terms = lambda sim, n_steps: ac.fit_terms(c_end, n_steps)
    sim = ac.make_fit_sim(tc.FIT_START[0], tc.FIT_START[1], with_tensor=False)
    sim.set_diffusion_tensor_family(tc.fit_family(sim._labels()), dict(ratio=tc.FIT_START[2]), ("ratio",))
    with pytest.raises(ValueError, match="tensor_controls"):
        ReducedFunctional(sim, 2, terms, tensor_controls=("aspect",))
    rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out), tensor_controls=("ratio",))
    with pytest.raises(NotImplementedError):
        rf.hessian_matrix(list(tc.FIT_START))
    assert rf.evaluations == 0
    res = minimize(rf, list(tc.FIT_START), bounds=tc.FIT_BOUNDS, options=dict(tc.FIT_OPTIONS), tol=1e-16)
    true = np.array([F["D"], F["rho"], F["ratio"]])
    err = float(np.abs(res.x / true - 1.0).max())
    print("device fit: D = %.10f, rho = %.10f, ratio = %.8f, recovery error %.2e (bar %.1e), J = %.2e, %d evaluations"
          % (res.x[0], res.x[1], res.x[2], err, FIT_RATIO_BAR, res.fun, rf.evaluations))
    for m, J, gn in rf.history[:3] + rf.history[-2:]:
        print("    m = (%.6f, %.6f, %.5f)  J = %.3e  |dJ/dm| = %.2e" % (m[0], m[1], m[2], J, gn))
    # the gradient dict of the simulation: 'tensor' only with a family
    g = sim.adjoint_gradient(terms(sim, F["steps"]))
    assert set(g["tensor"]) == {"ratio"} and g["tensor"]["ratio"].shape == (3,)
    sim.set_diffusion_tensor(sim._diffusion_tensor)                    # a plain field: the family is gone
    sim.run(record_adjoint=True, save_method=None, plot=False, output_dir=out, keep_nth=10 ** 9, clear_all=False)
    assert "tensor" not in sim.adjoint_gradient(terms(sim, F["steps"]))
    sim.close()
    assert err <= FIT_RATIO_BAR
