"""
Second-order discrete adjoint on the GPU (glims_adjoint_hessian) where its kernels branch: every direction count of the
P-column solver (k_spmm<P>, k_mp_vec / k_mp_dir / k_mp_scalar<P>, P = 1 .. 8) under both column encodings, columns that are
done before the first iteration, the label chunks of k_hsens and of the coupling passes (GL_ADJ_LT = 8 labels per launch), a
mesh beyond the fixed grids of k_hsens (2048 x 256 cells) and k_mp_vec (1024 x 256 rows), a Delaunay mesh under shuffled
numberings, displacement terms at several steps with clamp values and a load, the forward variants ForwardGuard swaps around,
the stiff multigrid regime with Dirichlet c, degenerate term sets and recordings, and the public parameter maps end to end.
The reference is the numpy tangent-linear + second-order adjoint of tests/adjoint_hessian_common.py on the GPU's own trajectory
(itself checked by central differences in tests/test_adjoint_hessian_cpu.py).  Every scenario also checks the bits DESIGN.md
section 13 claims (_check).
"""
import numpy as np
import pytest

from adjoint_common import Problem, many_tissues, renumber, u_terms
from adjoint_hessian_common import hessian
from test_gpu_adjoint import _record, _rel
from test_gpu_adjoint_coverage import _VARIANTS, _brain_sim, _handle, _nostat

pytestmark = pytest.mark.gpu

_GRAD = ("D", "rho", "gamma", "c0")
_HV = ("hv_D", "hv_rho", "hv_gamma", "hv_c0")


def _check(h, prob, traj, terms, dirs, tol=1e-8):
    """One Hessian call of the recorded run along ``dirs``, against the numpy second-order adjoint on the GPU's trajectory
    ``traj`` (<= tol relative per output; not when traj is None), and the bits DESIGN.md section 13 claims: J and the gradient
    are glims_adjoint_gradient's, and column j is the one-direction call of dirs[j].  Returns (result, numpy products)."""
    r = h.adjoint_hessian(terms, dirs)
    hv = None
    if traj is not None:
        J, dD, drho, dgam, dc0, hv = hessian(prob, prob.oracle(), traj, terms, dirs)
        rel = {"J": _rel(r["J"], J)}
        rel.update({k: _rel(r[k], v) for k, v in zip(_GRAD, (dD, drho, dgam, dc0))})
        for p in range(len(dirs)):
            rel.update({"%s[%d]" % (k, p): _rel(r[k][p], hv[p][k[3:]]) for k in _HV})
        print("relative error vs numpy: at most %.2e (%s)" % (max(rel.values()), max(rel, key=rel.get)))
        bad = {k: v for k, v in rel.items() if not v <= tol}
        assert not bad, bad
    g = h.adjoint_gradient(terms)
    assert r["J"] == g[0] and all(np.array_equal(r[k], x) for k, x in zip(_GRAD, g[1:]))
    for j, d in enumerate(dirs):
        r1 = h.adjoint_hessian(terms, [d])
        for k in _HV:
            assert np.array_equal(r[k][j], r1[k][0]), (j, k)
    return r, hv


def _mixed(prob, seed, count=3):
    """Directions with dD, drho and dgamma on every label (a passive tissue's too), and a dc0 on every other one."""
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    out = []
    for k in range(count):
        d = dict(D=0.03 * rng.uniform(-1, 1, L), rho=0.4 * rng.uniform(-1, 1, L), gamma=0.15 * rng.uniform(-1, 1, L))
        if k % 2 == 0:
            d["c0"] = 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
        out.append(d)
    return out


def _all_zero(r, keys=_HV):
    return all(not r[k].any() for k in keys)


# ---- 1. every direction count, both column encodings ----------------------------------------------------------------------
def _eight(prob, seed):
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    c0 = lambda: 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
    uni = lambda: rng.uniform(-1, 1, L)
    return [dict(D=prob.D * uni(), rho=prob.rho * uni(), c0=c0()),                           # D + rho + c0
            dict(rho=prob.rho * uni()),                                                      # rho only
            {},                                                                              # zero
            dict(gamma=prob.gamma * uni()),                                                  # gamma only
            dict(c0=c0()),                                                                   # c0 only
            dict(D=np.eye(L)[1]),                                                            # a unit vector on one label
            dict(D=0.01, rho=-0.1),                                                          # one value for every label
            dict(D=prob.D * uni(), rho=prob.rho * uni(), gamma=prob.gamma * uni(), c0=c0())]   # everything


@pytest.mark.parametrize("int32", [False, True], ids=["codes16", "int32_columns"])
def test_every_direction_count(backend, int32):
    """P = 1 .. 8 (k_spmm<P>, k_mp_*<P>; P = 8 runs all 16 waves of k_mp_scalar) with directions of different character, the
    column codes of k_spmm on every slice (default) or on none (GLIMS_FLAG_INT32_COLUMNS): every column = numpy and bitwise
    the one-direction call of its direction, so its PCG iterations add up; the zero direction is done at the start."""
    prob = Problem(2, 16)
    N = 6
    terms = prob.terms(N)
    assert {t["kind"] for t in terms} == {"c_l2", "c_thresh", "u_l2"} and prob.dir_c is not None
    n_u = len({t["step"] for t in terms if t["kind"] == "u_l2"})
    h = _handle(backend, prob, flags=backend.FLAG_INT32_COLUMNS if int32 else 0)
    st = h.stats()
    assert st["nnz_idx16"] == (0 if int32 else st["nnz_padded"])
    traj = _record(h, N)
    assert h.stats()["rd_precond_used"] == backend.RD_PRECOND_JACOBI   # the P-column solver (no column-by-column V-cycle)
    dirs = _eight(prob, 1)
    r8, hv = _check(h, prob, traj, terms, dirs)
    ones = [h.adjoint_hessian(terms, [d]) for d in dirs]
    for P in range(1, 9):
        r = r8 if P == 8 else h.adjoint_hessian(terms, dirs[:P])
        for j in range(P):
            for k in _HV:
                assert np.array_equal(r[k][j], ones[j][k][0]), (P, j, k)
                assert _rel(r[k][j], hv[j][k[3:]]) <= 1e-8, (P, j, k)
        s = r["stats"]
        assert s["mech_solves"] == 2 * P * n_u
        assert s["tlm_pcg_its"] == sum(o["stats"]["tlm_pcg_its"] for o in ones[:P])
        assert s["soa_pcg_its"] == sum(o["stats"]["soa_pcg_its"] for o in ones[:P])
        if P >= 3:
            assert all(not r[k][2].any() for k in _HV)   # the zero direction: exactly 0
    assert ones[0]["stats"]["tlm_pcg_its"] > 0 and ones[0]["stats"]["soa_pcg_its"] > 0
    assert ones[2]["stats"]["tlm_pcg_its"] == 0 and ones[2]["stats"]["soa_pcg_its"] == 0
    # one value for every label: the bits of the broadcast vectors
    L = prob.n_labels
    a = h.adjoint_hessian(terms, [dict(D=0.01, rho=-0.1)])
    b = h.adjoint_hessian(terms, [dict(D=np.full(L, 0.01), rho=np.full(L, -0.1))])
    assert all(np.array_equal(a[k], b[k]) for k in _HV)
    # every column done at the start: zero directions; gamma-only directions and no displacement term
    c_terms = [t for t in terms if t["kind"] != "u_l2"]
    for tt, dd in ((terms, [{}, {}]), (c_terms, [dict(gamma=prob.gamma), dict(gamma=-2.0 * prob.gamma)])):
        r, _ = _check(h, prob, traj, tt, dd)
        assert _all_zero(r), r
        assert r["stats"]["tlm_pcg_its"] == 0 and r["stats"]["soa_pcg_its"] == 0
    h.close()


# ---- 2. label chunks ------------------------------------------------------------------------------------------------------
def _neighbour(prob, b, allowed):
    """The label in ``allowed`` with the most cells on the nodes of label b's cells."""
    touch = np.isin(prob.cells, np.unique(prob.cells[prob.labels == b])).any(axis=1)
    count = np.bincount(prob.labels[touch], minlength=prob.n_labels)
    return int(max(allowed, key=lambda l: count[l]))


@pytest.mark.parametrize("dim,L,n,empty,zero", [(2, 9, 16, 3, 5), (3, 17, 6, 12, 9)])
def test_label_chunks(backend, dim, L, n, empty, zero):
    """9 labels: one past the first chunk of 8; 17: a third chunk holding one label.  One id no cell carries, one tissue with
    D = rho = gamma = 0, a displacement term (the coupling sums of gt_pass run over the chunks as well).  Unit directions on
    a label a of the first chunk and on the last label b: (H e_a)_b = (H e_b)_a across the chunks."""
    prob = many_tissues(dim, L, n=n, empty=(empty,), zero=(zero,), zero_gamma=(zero,), seed=L)
    count = np.bincount(prob.labels, minlength=L)
    assert count[empty] == 0 and np.all(np.delete(count, empty) > 0)
    N = 5
    terms = prob.terms(N)
    h = _handle(backend, prob)
    traj = _record(h, N)
    b = L - 1
    a = _neighbour(prob, b, [l for l in range(8) if l != empty])
    units = [(key, l) for key in ("D", "rho", "gamma") for l in (a, b)]
    dirs = _mixed(prob, L, 1) + [{key: np.eye(L)[l]} for key, l in units]
    r, _ = _check(h, prob, traj, terms, dirs)
    for k in ("hv_D", "hv_rho", "hv_gamma"):
        assert not r[k][:, empty].any(), k               # no cell carries it
        assert r[k][0, b] != 0 and r[k][0, zero] != 0, k   # the last (partial) chunk; the passive tissue
    for i, (ki, li) in enumerate(units):
        for j, (kj, lj) in enumerate(units):
            if li == a and lj == b:
                x, y = r["hv_" + kj][1 + i][lj], r["hv_" + ki][1 + j][li]   # (H e_i)_j, (H e_j)_i
                assert x != 0 and abs(x - y) <= 1e-8 * max(abs(x), abs(y)), (ki, kj, a, b, x, y)
    h.close()


# ---- 3. beyond the fixed grids --------------------------------------------------------------------------------------------
def test_mesh_beyond_the_fixed_grids(backend):
    """530 x 530 rectangle: 561 800 cells > 2048 x 256 threads of k_hsens, 281 961 rows > 1024 x 256 threads of k_mp_vec (the
    grid-stride tails), 4 406 slices (k_spmm's partials from 1 102 blocks).  The steps are stiff at this size (dt D / h^2 up to
    ~800), so the RD preconditioner is pinned to Jacobi: with the multigrid the solves would run column by column and never
    reach the P-column solver.  P = 3 (an odd width) against numpy once; P = 8 with the same first three directions bitwise
    P = 3; two fresh handles recorded the same way give the same bits."""
    prob = many_tissues(2, 10, n=530, seed=11)
    n = len(prob.points)
    assert prob.cells.shape[0] == 561800 > 2048 * 256 and n == 281961 > 1024 * 256 and -(-n // 64) == 4406
    N = 2
    rng = np.random.default_rng(12)
    terms = [dict(step=N, kind="c_thresh", level=0.3, smooth=0.1, weight=1.0, target=rng.uniform(0, 1, n)),
             dict(step=1, kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, n))]
    dirs = _mixed(prob, 13, 3)
    jacobi = dict(mechanics=False, rd_precond=backend.RD_PRECOND_JACOBI)
    h = _handle(backend, prob, **jacobi)
    traj = _record(h, N)
    assert h.stats()["rd_precond_used"] == backend.RD_PRECOND_JACOBI
    r3, _ = _check(h, prob, traj, terms, dirs)
    assert r3["stats"]["tlm_pcg_its"] > 0 and r3["stats"]["soa_pcg_its"] > 0
    r8 = h.adjoint_hessian(terms, dirs + _mixed(prob, 14, 5))
    h.close()
    for k in _HV:
        assert np.array_equal(r8[k][:3], r3[k]), k
    for _ in range(2):
        h = _handle(backend, prob, **jacobi)
        h.adjoint_record(True)
        for _ in range(N):
            assert h.step(1) == 0
        r = h.adjoint_hessian(terms, dirs)
        h.close()
        assert r["J"] == r3["J"] and all(np.array_equal(r[k], r3[k]) for k in _GRAD + _HV)


# ---- 4. unstructured mesh, shuffled numberings ----------------------------------------------------------------------------
def test_unstructured_mesh_in_shuffled_numberings(backend):
    """Delaunay mesh of random points under two random node numberings: dc0 goes in and hv_c0 comes out through k_perm in
    the caller's numbering; k_hess_rows / k_gdir_rows see rows of ~6 to ~45 incidences; the column codes of a general mesh.
    The terms and directions are drawn once, in the mesh's own numbering."""
    from glimslib_amd import workloads
    w = workloads.config_unstructured(n_points=6000, seed=1)
    base = many_tissues(3, 6, mesh=(w.mesh.points, w.mesh.cells), u_clamp=0.01, seed=13)
    n = len(base.points)
    N = 4
    terms0 = base.terms(N) + u_terms(base, [2], seed=14)
    assert len({t["step"] for t in terms0 if t["kind"] == "u_l2"}) == 2
    dirs0 = _mixed(base, 15, 3)
    out = []
    for seed in (5, 6):
        pts, cells, perm = renumber(w.mesh.points, w.mesh.cells, seed)
        prob = many_tissues(3, 6, mesh=(pts, cells), u_clamp=0.01, seed=13)
        assert np.array_equal(prob.labels, base.labels) and np.array_equal(prob.c0, base.c0[perm])
        terms = [dict(t, target=np.asarray(t["target"]).reshape(n, -1)[perm].ravel()) for t in terms0]
        dirs = [dict(d, c0=d["c0"][perm]) if "c0" in d else d for d in dirs0]
        h = _handle(backend, prob)
        st = h.stats()
        print("numbering %d: %d of %d stored entries in slices with 16-bit column codes" %
              (seed, st["nnz_idx16"], st["nnz_padded"]))
        # the library's own numbering gives every slice codes whatever the caller's is: the shuffle does not reach the
        # int32 half of k_spmm (test_every_direction_count runs it)
        assert st["nnz_idx16"] == st["nnz_padded"] > 0
        traj = _record(h, N)
        r, _ = _check(h, prob, traj if not out else None, terms, dirs)
        h.close()
        hv_c0 = np.empty_like(r["hv_c0"])
        hv_c0[:, perm] = r["hv_c0"]   # back to the mesh's own numbering
        out.append(dict(r, hv_c0=hv_c0))
    for k in _HV:
        for p in range(len(dirs0)):
            assert _rel(out[1][k][p], out[0][k][p]) <= 1e-10, (k, p)


# ---- 5. displacement terms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["BLOCK_JACOBI", "MULTIGRID"])
@pytest.mark.parametrize("dim", [2, 3])
def test_displacement_terms_with_clamp_values_and_load(backend, dim, precond):
    """u_l2 at step 0, midway and twice at the last step, non-zero Dirichlet displacement and a mechanical load: du and dmu of
    every direction at each observed step (the two terms at N share them), the dgamma G_t^T mu pass."""
    prob = many_tissues(dim, 3, n=16 if dim == 2 else 6, u_clamp=0.02, mech_load=1.0, seed=20 + dim)
    N = 4
    terms = u_terms(prob, [0, 2, N, N], seed=21) + [dict(step=N, kind="c_l2", weight=1.0,
                                                         target=np.full(len(prob.points), 0.2))]
    dirs = _mixed(prob, 22, 3)
    assert all("gamma" in d for d in dirs) and "c0" in dirs[0]
    h = _handle(backend, prob, mech_precond=getattr(backend, "PRECOND_" + precond))
    r, _ = _check(h, prob, _record(h, N), terms, dirs)
    assert r["stats"]["mech_solves"] == 2 * len(dirs) * 3   # du and dmu per direction at steps 0, 2 and N
    assert r["hv_gamma"].any()
    h.close()


# ---- 6. forward variants --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_forward_variants(backend, variant):
    """(a) the Hessian of a run under each variant matches numpy on its trajectory; (b) a handle that made a Hessian call steps
    on and solves mechanics to the bits and stats of a twin that never did."""
    moving = variant == "rd_load_and_moving_dirichlet_c"
    prob = many_tissues(2, 3, n=20, u_clamp=0.01, mech_load=0.5, rd_load=0.3 if moving else 0.0, seed=30)
    opts = _VARIANTS[variant](backend)
    N = 5
    terms = prob.terms(N)
    a, b = _handle(backend, prob, **opts), _handle(backend, prob, **opts)
    a.adjoint_record(True)
    traj = [a.get_state(want_u=False)[0]]
    for k in range(N):
        if moving:   # the same Dirichlet nodes, other values after every step
            for h in (a, b):
                h.set_dirichlet_c(prob.dir_c[0], 0.05 + 0.02 * (k + 1))
        assert a.step(1) == 0 and b.step(1) == 0
        traj.append(a.get_state(want_u=False)[0])
    assert np.array_equal(traj[-1], b.get_state(want_u=False)[0]) and _nostat(a) == _nostat(b)
    _check(a, prob, traj, terms, _mixed(prob, 31, 3))
    if variant == "rd_multigrid_fp32_smoother":
        assert a.stats()["rd_precond_used"] == backend.RD_PRECOND_MULTIGRID
    assert _nostat(a) == _nostat(b)
    assert a.step(3) == 0 and b.step(3) == 0
    assert np.array_equal(a.get_state()[0], b.get_state()[0])
    assert a.solve_mechanics() == 0 and b.solve_mechanics() == 0
    assert np.array_equal(a.get_state()[1], b.get_state()[1])
    assert _nostat(a) == _nostat(b)
    a.close()
    b.close()


def test_stiff_multigrid_regime_with_dirichlet_c(backend):
    """dt D / h^2 ~ 100 with the RD multigrid: the solves of both sweeps run column by column through the V-cycle PCG, here
    with Dirichlet c (the constrained rows of rd_solve)."""
    prob = Problem(3, 10, dt=1.0, D=(0.1, 0.2), rho=(0.05, 0.1))
    assert prob.dir_c is not None
    N = 4
    terms = prob.terms(N, with_u=False)
    h = _handle(backend, prob, mechanics=False, rd_precond=backend.RD_PRECOND_MULTIGRID)
    traj = _record(h, N)
    assert h.stats()["rd_precond_used"] == backend.RD_PRECOND_MULTIGRID
    r, _ = _check(h, prob, traj, terms, _mixed(prob, 32, 3))
    assert r["stats"]["tlm_pcg_its"] > 0 and r["stats"]["soa_pcg_its"] > 0
    assert h.stats()["rd_precond_used"] == backend.RD_PRECOND_MULTIGRID
    h.close()


# ---- 7. degenerate term sets and recordings -------------------------------------------------------------------------------
def test_degenerate_term_sets(backend):
    prob = many_tissues(2, 3, n=12, u_clamp=0.01, seed=40)
    n = len(prob.points)
    rng = np.random.default_rng(41)
    at0 = [dict(step=0, kind="c_thresh", level=0.3, smooth=0.1, weight=1.5, target=rng.uniform(0, 1, n)),
           dict(step=0, kind="c_l2", weight=0.5, target=rng.uniform(0, 0.5, n))] + u_terms(prob, [0], seed=42)
    dirs = _mixed(prob, 43, 3)
    N = 3
    h = _handle(backend, prob)
    traj = _record(h, N)
    # no terms: J = 0 and every output exactly 0
    r, _ = _check(h, prob, traj, [], dirs)
    assert r["J"] == 0.0 and _all_zero(r, _GRAD + _HV)
    # terms at step 0 only: no backward step has a right-hand side
    r, _ = _check(h, prob, traj, at0, dirs)
    assert not r["hv_D"].any() and not r["hv_rho"].any() and r["stats"]["soa_pcg_its"] == 0
    assert r["hv_gamma"].any() and r["hv_c0"].any()
    # a zero weight is the term omitted
    terms = prob.terms(N)
    ref, _ = _check(h, prob, traj, terms, dirs)
    for extra in (dict(terms[2], weight=0.0), dict(u_terms(prob, [1], seed=44)[0], weight=0.0)):
        got = h.adjoint_hessian(terms + [extra], dirs)
        assert got["J"] == ref["J"] and all(np.array_equal(got[k], ref[k]) for k in _GRAD + _HV), extra["kind"]
    h.close()
    # N = 0: hv_c0 from the copy branch
    h = _handle(backend, prob)
    traj = _record(h, 0)
    r, _ = _check(h, prob, traj, at0, dirs)
    assert not r["hv_D"].any() and not r["hv_rho"].any() and r["hv_c0"].any()
    assert r["stats"]["tlm_pcg_its"] == 0 and r["stats"]["soa_pcg_its"] == 0
    h.close()


# ---- 8. public parameter maps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,m0", [("TumorGrowthBrain", [0.1, 0.02, 0.1, 0.05, 0.1]), ("TumorGrowth", [0.05, 0.1, 0.1])])
def test_hessian_matrix_matches_central_differences(tmp_path, cls, m0):
    """Every column of ReducedFunctional.hessian_matrix against central differences of rf.derivative: the 5 TumorGrowthBrain
    controls (WM = 3 before GM = 2) and TumorGrowth's (diffusion, proliferation, coupling), each a sum over the labels of the
    handle's products; unknown direction keys are refused."""
    from glimslib_amd import simulation
    sim, rf = _brain_sim(tmp_path, getattr(simulation, cls), len(m0))
    m0 = np.array(m0)
    H = rf.hessian_matrix(m0)
    h = sim._backend
    L = h.n_labels
    if cls == "TumorGrowthBrain":
        wm, gm = sim._tissue_id("WM"), sim._tissue_id("GM")
        e = lambda l: np.eye(L)[l]
        dirs = [dict(D=e(wm)), dict(D=e(gm)), dict(rho=e(wm)), dict(rho=e(gm)), dict(gamma=np.ones(L))]
        col = lambda r, j: [r["hv_D"][j][wm], r["hv_D"][j][gm], r["hv_rho"][j][wm], r["hv_rho"][j][gm],
                            r["hv_gamma"][j].sum()]
    else:
        dirs = [dict(D=1.0), dict(rho=1.0), dict(gamma=1.0)]
        col = lambda r, j: [r["hv_D"][j].sum(), r["hv_rho"][j].sum(), r["hv_gamma"][j].sum()]
    r, _ = _check(h, None, None, rf.terms_builder(sim, rf._n_steps), dirs)
    assert np.allclose(H, np.array([col(r, j) for j in range(len(m0))]).T, rtol=1e-12, atol=0)
    for bad in (dict(bogus=1.0), dict(D=1.0)):
        with pytest.raises(ValueError):
            sim.adjoint_hessian([], [bad])
    for i in range(len(m0)):
        eps = 1e-4 * m0[i]
        e = np.eye(len(m0))[i] * eps
        num = (rf.derivative(m0 + e) - rf.derivative(m0 - e)) / (2 * eps)
        assert _rel(H[:, i], num) <= 1e-5, (i, H[:, i], num)
    sim.close()
