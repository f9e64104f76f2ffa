"""
Exact Hessian-vector products in the per-label E and nu on the GPU (glims_adjoint_hessian_full, DESIGN.md section 13, "Second
order in E and nu"): against the numpy reference of tests/adjoint_hessian_elastic_common.py on the GPU's own trajectory
(<= 1e-8; itself checked by central differences in tests/test_adjoint_hessian_elastic_cpu.py), where the kernels branch
(1 .. 8 columns, the label chunks, clamp values with a load, several observed steps, shuffled numberings, both column
encodings), the bits the section claims, central differences of the GPU's own full gradient and the symmetry of the per-tissue
matrix on the brain-like mesh (<= 1e-5, <= 1e-8), the differentiated scale identity (<= 1e-9), the refusals, and the public
API up to a trust-constr fit of E_WM.
"""
import numpy as np
import pytest
# (imported at collection, before any test loads libglimship: see test_gpu_adjoint_elastic.py)
import torch  # noqa: F401

from adjoint_common import many_tissues, renumber, u_terms
from adjoint_hessian_elastic_common import KEYS, hessian_full, unit_directions
from test_gpu_adjoint import _record, _rel
from test_gpu_adjoint_coverage import _handle, _nostat
from test_gpu_adjoint_elastic import _brain_like_problem, _brain_sim, _brain_terms, _problem, _terms

pytestmark = pytest.mark.gpu

_GRAD = ("D", "rho", "gamma", "E", "nu", "c0")
_HV = tuple("hv_" + k for k in _GRAD)
_OLD_HV = ("hv_D", "hv_rho", "hv_gamma", "hv_c0")


def _check(h, prob, traj, terms, dirs, tol=1e-8, columns=True):
    """One full Hessian call of the recorded run along ``dirs``: against numpy on the GPU's trajectory ``traj`` (<= tol
    relative per output; not when traj is None), J and the six gradient arrays bitwise those of glims_adjoint_gradient_full,
    and column j bitwise the one-direction call of dirs[j].  Returns (result, numpy products)."""
    r = h.adjoint_hessian_full(terms, dirs)
    hv = None
    if traj is not None:
        J, g, hv = hessian_full(prob, prob.oracle(), traj, terms, dirs)
        rel = {"J": _rel(r["J"], J)}
        rel.update({k: _rel(r[k], g[k]) for k in _GRAD})
        for p in range(len(dirs)):
            rel.update({"%s[%d]" % (k, p): _rel(r[k][p], hv[p][k[3:]]) for k in _HV})
        print("relative error vs numpy: at most %.2e (%s)" % (max(rel.values()), max(rel, key=rel.get)))
        bad = {k: v for k, v in rel.items() if not v <= tol}
        assert not bad, bad
    g = h.adjoint_gradient(terms, elastic=True)
    assert r["J"] == g[0]
    for k, x in zip(("D", "rho", "gamma", "c0", "E", "nu"), g[1:]):
        assert np.array_equal(r[k], x), k
    for j, d in enumerate(dirs if columns else []):
        r1 = h.adjoint_hessian_full(terms, [d])
        for k in _HV:
            assert np.array_equal(r[k][j], r1[k][0]), (j, k)
    return r, hv


def _elastic_dirs(prob, seed):
    """Pure dE, pure dnu, and everything at once (dD, drho, dgamma, dE, dnu on every label, dc0)."""
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    uni = lambda: rng.uniform(-1, 1, L)
    return [dict(E=prob.E * uni()), dict(nu=0.1 * uni()),
            dict(D=0.03 * uni(), rho=0.4 * uni(), gamma=0.15 * uni(), E=prob.E * uni(), nu=0.1 * uni(),
                 c0=0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1))]


# ---- 1. against the numpy reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["MULTIGRID", "BLOCK_JACOBI"])
@pytest.mark.parametrize("dim", [2, 3])
def test_matches_numpy_reference(backend, dim, precond):
    """Four tissues (id 3 on no cell, gamma_1 = 0), clamp values and a load (the lifting term dK u_D), displacement terms at
    steps 1, N, N: pure dE, pure dnu and a direction in every block."""
    prob = _problem(dim)
    assert np.any(prob.dir_u[1] != 0.0) and prob.mech_load is not None
    N = 3
    terms = _terms(prob, N)
    h = _handle(backend, prob, mech_precond=getattr(backend, "PRECOND_" + precond))
    traj = _record(h, N)
    dirs = _elastic_dirs(prob, 1)
    r, _ = _check(h, prob, traj, terms, dirs)
    assert r["stats"]["mech_solves"] == 2 * len(dirs) * 2                  # du and dmu per direction at steps 1 and N: none added
    old_dirs = [{k: v for k, v in dirs[2].items() if k not in ("E", "nu")}] * 3
    assert r["stats"]["mech_solves"] == h.adjoint_hessian(terms, old_dirs)["stats"]["mech_solves"]
    assert not r["hv_E"][:, 3].any() and not r["hv_nu"][:, 3].any()        # the empty label
    assert abs(r["hv_E"][0][1]) > 1e-3 * np.abs(r["hv_E"][0]).max()        # gamma = 0: dK still acts
    assert r["stats"]["tlm_pcg_its"] > 0 and h.adjoint_hessian_full(terms, dirs[:2])["stats"]["tlm_pcg_its"] == 0
    h.close()


# ---- 2. where the kernels branch ---------------------------------------------------------------------------------------------
def _eight(prob, seed):
    rng = np.random.default_rng(seed)
    n, L = len(prob.points), prob.n_labels
    uni = lambda: rng.uniform(-1, 1, L)
    c0 = lambda: 0.2 * rng.uniform(-1, 1, n) * (prob.c0 + 0.1)
    return [dict(E=prob.E * uni()), dict(nu=0.1 * uni()), {}, dict(gamma=0.15 * uni()), dict(E=np.eye(L)[2]),
            dict(D=0.03 * uni(), nu=0.05), dict(E=0.5, c0=c0()),
            dict(D=0.03 * uni(), rho=0.4 * uni(), gamma=0.15 * uni(), E=prob.E * uni(), nu=0.1 * uni(), c0=c0())]


@pytest.mark.parametrize("int32", [False, True], ids=["codes16", "int32_columns"])
def test_every_direction_count(backend, int32):
    """P = 1 .. 8 columns of k_dkel_rows (and of the P-column solver) with directions of different character, under both
    column encodings: every column = numpy and bitwise the one-direction call of its direction."""
    prob = _problem(2)
    N = 3
    terms = _terms(prob, N)
    h = _handle(backend, prob, flags=backend.FLAG_INT32_COLUMNS if int32 else 0)
    st = h.stats()
    assert st["nnz_idx16"] == (0 if int32 else st["nnz_padded"])
    traj = _record(h, N)
    dirs = _eight(prob, 2)
    r8, hv = _check(h, prob, traj, terms, dirs, columns=False)
    ones = [h.adjoint_hessian_full(terms, [d]) for d in dirs]
    for P in range(1, 9):
        r = r8 if P == 8 else h.adjoint_hessian_full(terms, dirs[:P])
        for j in range(P):
            for k in _HV:
                assert np.array_equal(r[k][j], ones[j][k][0]), (P, j, k)
        assert r["stats"]["mech_solves"] == 2 * P * 2
        if P >= 3:
            assert all(not r[k][2].any() for k in _HV)   # the zero direction: exactly 0
    h.close()


@pytest.mark.parametrize("dim,L,n,empty,zero", [(2, 9, 12, 3, 5), (3, 17, 5, 12, 9)])
def test_label_chunks(backend, dim, L, n, empty, zero):
    """9 labels: one past the first chunk of 8 of k_hesens and the coupling passes; 17: a third chunk holding one label.  One
    id no cell carries, one tissue with D = rho = gamma = 0 (its E and nu still act through dK).  Unit directions in E and nu
    on a label of the first chunk and on the last label: (H e_i)_j = (H e_j)_i across the chunks."""
    prob = many_tissues(dim, L, n=n, empty=(empty,), zero=(zero,), zero_gamma=(zero,), u_clamp=0.02, mech_load=0.5, seed=L)
    count = np.bincount(prob.labels, minlength=L)
    assert count[empty] == 0 and np.all(np.delete(count, empty) > 0)
    N = 3
    terms = prob.terms(N)
    h = _handle(backend, prob)
    traj = _record(h, N)
    a, b = (0 if empty != 0 else 1), L - 1
    units = [(key, l) for key in ("E", "nu") for l in (a, b)]
    rng = np.random.default_rng(L)
    mixed = dict(D=0.03 * rng.uniform(-1, 1, L), gamma=0.15 * rng.uniform(-1, 1, L), E=prob.E * rng.uniform(-1, 1, L),
                 nu=0.1 * rng.uniform(-1, 1, L))
    dirs = [mixed] + [{key: np.eye(L)[l]} for key, l in units]
    r, _ = _check(h, prob, traj, terms, dirs, columns=False)
    for k in ("hv_E", "hv_nu"):
        assert not r[k][:, empty].any(), k                   # no cell carries it
        assert r[k][0, b] != 0 and r[k][0, zero] != 0, k     # the last (partial) chunk; the passive tissue
    for i, (ki, li) in enumerate(units):
        for j, (kj, lj) in enumerate(units):
            if i < j:
                x, y = r["hv_" + kj][1 + i][lj], r["hv_" + ki][1 + j][li]   # (H e_i)_j, (H e_j)_i
                assert abs(x - y) <= 1e-8 * max(np.abs(r["hv_" + kj][1 + i]).max(), np.abs(r["hv_" + ki][1 + j]).max()), \
                    (ki, li, kj, lj, x, y)
    h.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_displacement_terms_at_steps_0_2_N_N(backend, dim):
    """u_l2 at step 0, midway and twice at the last step, non-zero Dirichlet displacement and a mechanical load: dK u_k, dK mu_k,
    du, dmu and the E / nu sums at each observed step (the two terms at N share them)."""
    prob = many_tissues(dim, 3, n=12 if dim == 2 else 5, u_clamp=0.02, mech_load=1.0, seed=20 + dim)
    N = 4
    terms = u_terms(prob, [0, 2, N, N], seed=21) + [dict(step=N, kind="c_l2", weight=1.0, target=np.full(len(prob.points), 0.2))]
    dirs = _elastic_dirs(prob, 22)
    h = _handle(backend, prob)
    r, _ = _check(h, prob, _record(h, N), terms, dirs)
    assert r["stats"]["mech_solves"] == 2 * len(dirs) * 3
    h.close()


def test_unstructured_mesh_in_shuffled_numberings(backend):
    """A Delaunay mesh of random points under two random node numberings: k_dkel_rows sees rows of ~6 to ~45 incidences; the
    per-label outputs agree to 1e-10, hv_c0 after mapping back."""
    from glimslib_amd import workloads
    w = workloads.config_unstructured(n_points=6000, seed=1)       # (the mesh of the first-order and Hessian coverage tests)
    base = many_tissues(3, 6, mesh=(w.mesh.points, w.mesh.cells), u_clamp=0.01, seed=13)
    n = len(base.points)
    N = 4
    terms0 = base.terms(N) + u_terms(base, [2], seed=14)
    dirs0 = _elastic_dirs(base, 15)
    out = []
    for seed in (5, 6):
        pts, cells, perm = renumber(w.mesh.points, w.mesh.cells, seed)
        prob = many_tissues(3, 6, mesh=(pts, cells), u_clamp=0.01, seed=13)
        assert np.array_equal(prob.labels, base.labels) and np.array_equal(prob.c0, base.c0[perm])
        terms = [dict(t, target=np.asarray(t["target"]).reshape(n, -1)[perm].ravel()) for t in terms0]
        dirs = [dict(d, c0=d["c0"][perm]) if "c0" in d else d for d in dirs0]
        h = _handle(backend, prob)
        _record(h, N)
        r, _ = _check(h, prob, None, terms, dirs, columns=False)
        h.close()
        hv_c0 = np.empty_like(r["hv_c0"])
        hv_c0[:, perm] = r["hv_c0"]
        out.append(dict(r, hv_c0=hv_c0))
    for k in _HV:
        for p in range(len(dirs0)):
            assert _rel(out[1][k][p], out[0][k][p]) <= 1e-10, (k, p)
    assert out[0]["hv_E"].any() and out[0]["hv_nu"].any()


# ---- 3. the bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_bit_claims(backend, dim):
    prob = _problem(dim)
    N = 3
    terms = _terms(prob, N)
    rng = np.random.default_rng(7)
    L, n = prob.n_labels, len(prob.points)
    old_dirs = [dict(D=0.03 * rng.uniform(-1, 1, L), rho=0.4 * rng.uniform(-1, 1, L), c0=0.2 * rng.uniform(-1, 1, n) * prob.c0),
                dict(gamma=0.15 * rng.uniform(-1, 1, L))]
    dirs = _elastic_dirs(prob, 8)
    res = []
    for _ in range(2):   # two fresh handles
        h = _handle(backend, prob)
        _record(h, N)
        old = h.adjoint_hessian(terms, old_dirs)
        full = h.adjoint_hessian_full(terms, old_dirs)     # dir_E = dir_nu = NULL
        for k in ("J", "D", "rho", "gamma", "c0") + _OLD_HV:
            assert np.array_equal(old[k], full[k]), k
        assert full["hv_E"].any() and full["hv_nu"].any()          # the mixed rows of directions in D, rho, gamma, c0
        assert full["stats"]["mech_solves"] == old["stats"]["mech_solves"]
        r, _ = _check(h, prob, None, terms, dirs)                   # the gradient's bits, column j = one direction
        again = h.adjoint_hessian_full(terms, dirs)        # two calls
        assert all(np.array_equal(r[k], again[k]) for k in ("J",) + _GRAD + _HV)
        res.append((full, r))
        h.close()
    for x, y in zip(res[0], res[1]):
        assert all(np.array_equal(x[k], y[k]) for k in ("J",) + _GRAD + _HV)


def test_concentration_terms_only_give_exact_zeros_and_no_elastic_solve(backend):
    prob = _problem(3)
    N = 3
    terms = [t for t in _terms(prob, N) if t["kind"] != "u_l2"] + prob.terms(N, with_u=False)
    h = _handle(backend, prob)
    _record(h, N)
    dirs = _elastic_dirs(prob, 9)
    before = h.adjoint_stats()
    r = h.adjoint_hessian_full(terms, dirs)
    old = h.adjoint_hessian(terms, [{k: v for k, v in dirs[2].items() if k not in ("E", "nu")}])
    assert not r["E"].any() and not r["nu"].any() and not r["hv_E"].any() and not r["hv_nu"].any()
    assert r["hv_D"][2].any() and not r["hv_D"][0].any() and not r["hv_c0"][1].any()
    assert r["stats"]["mech_solves"] == old["stats"]["mech_solves"] == 0 and h.adjoint_stats() == before
    for k in _OLD_HV:
        assert np.array_equal(r[k][2], old[k][0]), k
    h.close()


def test_forward_state_and_stats_untouched(backend):
    """Twin handles record the same run; one makes the full Hessian call, the other none: the next steps, the displacement and
    glims_stats agree bit for bit."""
    prob = _problem(3)
    N = 3
    terms = _terms(prob, N)
    a, b = _handle(backend, prob), _handle(backend, prob)
    for h in (a, b):
        h.adjoint_record(True)
        assert h.step(N) == 0 and h.solve_mechanics() == 0
    assert _nostat(a) == _nostat(b)
    a.adjoint_hessian_full(terms, _elastic_dirs(prob, 10))
    assert _nostat(a) == _nostat(b)
    for h in (a, b):
        assert h.step(2) == 0 and h.solve_mechanics() == 0
    (ca, ua), (cb, ub) = a.get_state(), b.get_state()
    assert np.array_equal(ca, cb) and np.array_equal(ua, ub) and _nostat(a) == _nostat(b)
    a.close()
    b.close()


# ---- 4. central differences of the GPU's own gradient, symmetry, on the brain-like mesh -----------------------------------
def _full_gradient(backend, prob, N, terms, **tables):
    """[dD, drho, dgamma, dE, dnu] of a fresh handle with some per-label tables replaced."""
    saved = {k: getattr(prob, k) for k in tables}
    for k, v in tables.items():
        setattr(prob, k, v)
    try:
        h = _handle(backend, prob)
        h.adjoint_record(True)
        assert h.step(N) == 0
        g = h.adjoint_gradient(terms, elastic=True, want_dc0=False)
        h.close()
    finally:
        for k, v in saved.items():
            setattr(prob, k, v)
    return np.concatenate([g[1], g[2], g[3], g[5], g[6]])


def test_brain_like_central_differences_and_symmetry(backend):
    """The per-tissue matrix over (D, rho, gamma, E, nu) on the brain-like mesh, one of its two tissues made nearly
    incompressible (nu = 0.49; the workload's own are 0.45): symmetric to 1e-8, and three of its columns -- E and nu of one
    tissue each, and the coupling -- against central differences of glims_adjoint_gradient_full, each block (D, rho, gamma, E,
    nu rows) relative to its largest entry."""
    prob = _brain_like_problem(12000)
    N = 2
    terms = _brain_terms(prob, N)
    L = prob.n_labels
    present = [int(t) for t in np.unique(prob.labels)]
    assert len(present) >= 2
    prob.nu = prob.nu.copy()
    prob.nu[present[0]] = 0.49
    dirs = unit_directions(prob, labels=present)
    h = _handle(backend, prob)
    h.adjoint_record(True)
    assert h.step(N) == 0
    cols = []
    for i in range(0, len(dirs), 8):
        r = h.adjoint_hessian_full(terms, dirs[i:i + 8])
        cols += [np.concatenate([r["hv_" + k][p][present] for k in KEYS]) for p in range(len(dirs[i:i + 8]))]
    h.close()
    H = np.array(cols).T
    nb = len(present)
    for i in range(5):
        for j in range(5):
            A, B = H[i * nb:(i + 1) * nb, j * nb:(j + 1) * nb], H[j * nb:(j + 1) * nb, i * nb:(i + 1) * nb]
            assert np.abs(A - B.T).max() <= 1e-8 * max(np.abs(A).max(), 1e-300), (KEYS[i], KEYS[j], A, B)
    stiff = max(present, key=lambda t: prob.nu[t])              # a nu = 0.49 tissue
    soft = max((t for t in present if prob.gamma[t] != 0), key=lambda t: abs(H[3 * nb + present.index(t), 3 * nb + present.index(t)]))
    # steps: 1e-4 relative in E and gamma (as the first-order test); in nu the derivatives grow like 1 / (1 - 2 nu)^k, the
    # truncation h^2 f''' / (6 f') ~ 4 h^2 / (1 - 2 nu)^2 stays below 1e-6 at nu = 0.49 with h = 1e-5
    for key, t, hstep in (("E", soft, 1e-4 * prob.E[soft]), ("nu", stiff, 1e-5), ("gamma", soft, 1e-4 * prob.gamma[soft])):
        base = getattr(prob, key)
        e = np.zeros(L)
        e[t] = hstep
        num = (_full_gradient(backend, prob, N, terms, **{key: base + e}) -
               _full_gradient(backend, prob, N, terms, **{key: base - e})) / (2 * hstep)
        ana = H[:, KEYS.index(key) * nb + present.index(t)]
        for i, blk in enumerate(KEYS):
            want = num[i * L:(i + 1) * L][present]
            got = ana[i * nb:(i + 1) * nb]
            assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), (key, t, blk, got, want)


# ---- 5. the scale identity, differentiated once --------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_scale_identity_differentiated_once(backend, dim):
    """No load, zero clamp values: sum_s E_s H[q, E_s] = 0 for q in D, rho, gamma, nu and sum_s E_s H[E_t, E_s] = -dJ/dE_t."""
    prob = _problem(dim, mech_load=0.0, u_clamp=0.0)
    assert prob.mech_load is None and not np.any(prob.dir_u[1])
    N = 2
    L = prob.n_labels
    h = _handle(backend, prob)
    h.adjoint_record(True)
    assert h.step(N) == 0
    r = h.adjoint_hessian_full(_terms(prob, N), unit_directions(prob, keys=("E",)))
    h.close()
    for q in ("D", "rho", "gamma", "nu"):
        for t in range(L):
            s = prob.E * r["hv_" + q][:, t]
            assert abs(s.sum()) <= 1e-9 * np.abs(s).sum(), (q, t, s)
    seen = 0.0
    for t in range(L):
        s = np.append(prob.E * r["hv_E"][:, t], r["E"][t])
        assert abs(s.sum()) <= 1e-9 * np.abs(s).sum(), (t, s)
        seen += np.abs(s).sum()
    assert seen > 0.0


# ---- 6. misuse ---------------------------------------------------------------------------------------------------------------
def test_misuse_statuses(backend):
    prob = _problem(2)
    N = 2
    L = prob.n_labels
    terms = _terms(prob, N)
    c_terms = [t for t in terms if t["kind"] != "u_l2"]

    def usage(h, tt, dirs, match):
        with pytest.raises(backend.BackendError) as e:
            h.adjoint_hessian_full(tt, dirs)
        assert e.value.code == backend.GLIMS_E_USAGE and match in str(e.value), str(e.value)

    h = _handle(backend, prob)
    usage(h, terms, [dict(E=1.0)], "no valid trajectory")
    _record(h, N)
    ref = h.adjoint_hessian_full(terms, [dict(E=1.0)])
    usage(h, terms, [], "n_dir")
    usage(h, terms, [dict(E=1.0)] * 9, "n_dir")
    x = prob.points * 0.98 + 0.01
    h.set_deformed_image_terms([dict(step=N, kind="img_l2", points=x, target=np.zeros(len(x)))])
    usage(h, terms, [dict(E=1.0)], "deformed image")
    h.set_deformed_image_terms([])
    again = h.adjoint_hessian_full(terms, [dict(E=1.0)])      # the handle is as it was
    assert all(np.array_equal(ref[k], again[k]) for k in ("J",) + _GRAD + _HV)
    with pytest.raises(ValueError, match="adjoint_hessian_full"):
        h.adjoint_hessian(terms, [dict(E=1.0)])
    h.close()
    # a handle set up without mechanics: each of dir_E / dir_nu / hv_E / hv_nu alone is refused, a call with all four NULL is
    # accepted and is glims_adjoint_hessian (the gradient's dJ_dE / dJ_dnu may be asked for: they are 0)
    import ctypes as C
    h = _handle(backend, prob, mechanics=False)
    _record(h, N)
    old = h.adjoint_hessian(c_terms, [dict(D=0.01)])
    assert old["hv_D"].any()
    arr, keep = h._misfit_array(h._split_terms(c_terms))
    n = len(prob.points)
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None

    def raw(**el):
        """One direction dD = 0.01 through the C entry with the given E / nu arrays ([L] each, else NULL)"""
        J = C.c_double(0.0)
        g = [np.zeros(L) for _ in range(3)] + [np.zeros(n)] + [np.ones(L), np.ones(L)]
        hv = [np.zeros((1, L)) for _ in range(3)] + [np.zeros((1, n))]
        st = h.lib.glims_adjoint_hessian_full(
            h._h, len(c_terms), arr, 1, ptr(np.full((1, L), 0.01)), None, None, None, ptr(el.get("dir_E")), ptr(el.get("dir_nu")),
            C.byref(J), *[ptr(a) for a in g], *[ptr(a) for a in hv], ptr(el.get("hv_E")), ptr(el.get("hv_nu")), None)
        return st, J.value, g, hv

    for key in ("dir_E", "dir_nu", "hv_E", "hv_nu"):
        st = raw(**{key: np.zeros((1, L))})[0]
        assert st == backend.GLIMS_E_USAGE, key
        assert b"with_mechanics" in h.lib.glims_last_error(h._h), key
    st, J, g, hv = raw()
    assert st == 0 and J == old["J"] and not g[4].any() and not g[5].any()
    assert all(np.array_equal(x, old[k]) for x, k in zip(g[:4], ("D", "rho", "gamma", "c0")))
    assert all(np.array_equal(x, old[k]) for x, k in zip(hv, _OLD_HV))
    # the binding: refused with a direction in E / nu, otherwise the call above (hv_E / hv_nu NULL, returned as zeros)
    usage(h, c_terms, [dict(D=0.01, E=1.0)], "with_mechanics")
    r = h.adjoint_hessian_full(c_terms, [dict(D=0.01)])
    assert all(np.array_equal(r[k], old[k]) for k in ("J",) + _OLD_HV) and not r["hv_E"].any() and not r["hv_nu"].any()
    del keep
    h.close()


def test_partitioned_handle_refuses_on_every_rank(backend):
    from glimslib_amd import _backend as B
    from glimslib_amd.parallel import run_threaded_ranks
    from glimslib_amd.partition import partition_mesh
    from adjoint_common import Problem
    from test_gpu_adjoint_elastic import _clamp_all_exterior
    # (u clamped on every exterior node: every rank owns constrained dofs, which the partitioned elastic solves need --
    #  a rank without any skips the exchange of the clamp values that the others make)
    prob = _clamp_all_exterior(Problem(2, 12), 0.02)
    world = 2
    n, d = len(prob.points), prob.dim
    terms = prob.terms(2)
    assert any(t["kind"] == "u_l2" for t in terms)

    def body(rank, tr):
        """Ranks set up WITH mechanics and a displacement term: nothing but the partitioned handle itself stands against the
        call."""
        part = partition_mesh(prob.points, prob.cells, world, rank)
        gid, n_own = part.global_ids, part.n_own
        g2l = np.full(n, -1, dtype=np.int64)
        g2l[gid[:n_own]] = np.arange(n_own)
        h = B.Handle(part.points, part.cells, prob.labels[part.cell_ids], n_own=n_own, device=0)
        h.set_transport(rank, world, tr.halo_cb, tr.allreduce_cb)
        h.set_halo(part.peer_rank, part.send_ptr, part.send_idx, part.recv_count)
        h.set_mg_frame(prob.points.min(axis=0), prob.points.max(axis=0))
        h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
        h.set_options(dt=prob.dt, mech_precond=B.PRECOND_BLOCK_JACOBI)
        dofs, vals = prob.dir_u
        loc = g2l[np.asarray(dofs) // d]
        keep = loc >= 0
        assert keep.any()
        h.set_dirichlet_u(loc[keep] * d + (np.asarray(dofs) % d)[keep], np.asarray(vals, float)[keep])
        h.setup(with_mechanics=True)
        h.set_state(prob.c0[gid])
        h.adjoint_record(True)
        assert h.step(2) == 0
        loc = [dict(t, target=np.asarray(t["target"], float).reshape(n, -1)[gid].reshape(-1)) for t in terms]
        try:
            h.adjoint_hessian_full(loc, [dict(D=[1.0, 0.0], E=[0.5, 0.0])])
            code, msg = 0, ""
        except B.BackendError as e:
            code, msg = e.code, str(e)
        h.adjoint_gradient(loc, elastic=True)   # the handle still works (a collective call every rank makes)
        h.close()
        if tr.failed is not None:
            raise tr.failed
        return code, msg

    res = run_threaded_ranks(world, body)
    assert [c for c, _ in res] == [B.GLIMS_E_USAGE] * world
    assert all("partitioned" in m and "with_mechanics" not in m for _, m in res), res
    from glimslib_amd.parallel import DistributedHandle
    with pytest.raises(NotImplementedError, match="elastic"):
        DistributedHandle.adjoint_hessian_full(None, [], [])


# ---- 7. public API -----------------------------------------------------------------------------------------------------------
def _tumor_growth_sim(tmp_path, poisson):
    from glimslib_amd import fenics_local as fenics
    from glimslib_amd.simulation import TumorGrowth

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    mesh = fenics.RectangleMesh(fenics.Point(-5, -5), fenics.Point(5, 5), 16, 16)
    labels = fenics.project(fenics.Expression('(x[0]>=0.0) ? (1.0) : (2.0)', degree=1), fenics.FunctionSpace(mesh, "DG", 1))
    sim = TumorGrowth(mesh)
    sim.setup_global_parameters(label_function=labels, domain_names={0: 'outside', 1: 'A', 2: 'B'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    u0 = fenics.Expression('exp(-(pow(x[0]-1.0,2)+pow(x[1]-0.5,2))/2.0)', degree=1)
    sim.setup_model_parameters(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: u0}, diffusion=0.1, coupling=0.1,
                               proliferation=0.1, E=0.001, poisson=poisson, sim_time=4, sim_time_step=1)
    sim.run(save_method=None, plot=False, output_dir=str(tmp_path), record_adjoint=True)
    return sim


def test_tumor_growth_takes_E_and_poisson(backend, tmp_path):
    """TumorGrowth.adjoint_hessian(..., elastic=True): the keys 'E' / 'poisson' in and out, equal to the handle's products, and
    the poisson column (one value on every label) against central differences of adjoint_gradient in the parameter poisson.
    (Not the E column: without a load, scaling the one E of every tissue moves nothing.)"""
    nu0 = 0.4
    sim = _tumor_growth_sim(tmp_path, nu0)
    n_steps = int(sim._backend.stats()["steps"])
    assert sim._backend.solve_mechanics() == 0
    ut = [dict(step=n_steps, kind="u_l2", weight=1.0, target=0.5 * sim._backend.get_state()[1])]
    g, hv = sim.adjoint_hessian(ut, [dict(poisson=1.0), dict(E=1.0, coupling=1.0)], elastic=True)
    keys = {'diffusion', 'proliferation', 'coupling', 'E', 'poisson', 'c0'}
    assert set(g) == keys | {'J'} and all(set(h) == keys for h in hv)
    L = sim._backend.n_labels
    raw = sim._backend.adjoint_hessian_full(ut, [dict(nu=np.ones(L)), dict(E=np.ones(L), gamma=np.ones(L))])
    for p in range(2):
        assert np.array_equal(hv[p]['E'], raw['hv_E'][p]) and np.array_equal(hv[p]['poisson'], raw['hv_nu'][p])
        assert np.array_equal(hv[p]['coupling'], raw['hv_gamma'][p])
    g1 = sim.adjoint_gradient(ut)
    assert g['J'] == g1['J'] and np.array_equal(g['E'], g1['E']) and np.array_equal(g['poisson'], g1['poisson'])
    assert hv[0]['poisson'].any() and hv[1]['E'].any()
    with pytest.raises(ValueError, match="directions take"):
        sim.adjoint_hessian(ut, [dict(E=1.0)])
    sim.close()
    num = {}
    eps = 1e-4 * nu0
    for sgn in (1, -1):
        s2 = _tumor_growth_sim(tmp_path, nu0 + sgn * eps)
        num[sgn] = s2.adjoint_gradient(ut)
        s2.close()
    for key in ('E', 'poisson', 'coupling'):
        fd = (num[1][key] - num[-1][key]) / (2 * eps)
        assert np.abs(hv[0][key] - fd).max() <= 1e-5 * np.abs(fd).max(), (key, hv[0][key], fd)


@pytest.mark.timeout(900)
def test_public_api_hessian_matrix_and_trust_constr_fit_of_E_WM(backend, tmp_path):
    from glimslib_amd.optimization import ReducedFunctional, minimize
    out = str(tmp_path)
    run = dict(keep_nth=10 ** 9, save_method=None, clear_all=False, plot=False, output_dir=out)
    sim = _brain_sim(1.5)
    sim.run(record_adjoint=True, **run)
    n_steps = int(sim._backend.stats()["steps"])
    assert sim._backend.solve_mechanics() == 0
    target = sim._backend.get_state()[1].copy()
    ut = [dict(step=n_steps, kind="u_l2", weight=1.0, target=0.5 * target)]
    g, hv = sim.adjoint_hessian(ut, [dict(E_WM=1.0), dict(coupling=1.0, nu_GM=0.1)], elastic=True)
    names = ("E_GM", "E_WM", "E_CSF", "E_VENT", "nu_GM", "nu_WM", "nu_CSF", "nu_VENT")
    for d in [g] + hv:
        assert all(k in d and np.isfinite(d[k]) for k in names + ("D_WM", "D_GM", "rho_WM", "rho_GM", "coupling")), d.keys()
    assert "J" in g and "J" not in hv[0] and hv[0]["E_WM"] != 0.0 and hv[0]["coupling"] != 0.0
    g1 = sim.adjoint_gradient(ut)
    assert all(g[k] == g1[k] for k in names + ("J", "coupling"))
    raw = sim._backend.adjoint_hessian_full(ut, [dict(E=np.eye(sim._backend.n_labels)[sim._tissue_id("WM")])])
    assert set(raw) >= {"E", "nu", "hv_E", "hv_nu"} and hv[0]["E_WM"] == raw["hv_E"][0][sim._tissue_id("WM")]
    with pytest.raises(ValueError, match="first order"):
        sim.adjoint_hessian([], [dict(E_WM=1.0)])
    sim.close()

    def terms(s, k):
        return [dict(step=k, kind="u_l2", weight=1.0, target=target)]

    # (E_WM, coupling): the matrix is symmetric and its columns are central differences of the gradient
    sim = _brain_sim(1.0)
    rf = ReducedFunctional(sim, 2, terms, run_kwargs=dict(output_dir=out), names=("E_WM", "coupling"), elastic_hessian=True)
    m0 = np.array([1.0, 0.12])
    H = rf.hessian_matrix(m0)
    assert abs(H[0, 1] - H[1, 0]) <= 1e-8 * np.abs(H).max(), H
    for i in range(2):
        eps = 1e-4 * m0[i]
        e = np.eye(2)[i] * eps
        num = (rf.derivative(m0 + e) - rf.derivative(m0 - e)) / (2 * eps)
        assert _rel(H[:, i], num) <= 1e-5, (i, H[:, i], num)
    sim.close()
    # the E_WM fit of test_gpu_adjoint_elastic.py, by trust-constr with the exact Hessian
    sim = _brain_sim(1.0)
    rf = ReducedFunctional(sim, 1, terms, run_kwargs=dict(output_dir=out), names=("E_WM",), elastic_hessian=True)
    # (the bounds make trust-constr an interior-point method: its barrier starts small enough not to move the minimum)
    res = minimize(rf, [1.0], bounds=(0.5, 3.0), method="trust-constr", tol=1e-15,
                   options={"maxiter": 60, "gtol": 1e-14, "xtol": 1e-14, "initial_barrier_parameter": 1e-12,
                            "barrier_tol": 1e-11})
    sim.close()
    assert abs(res.x[0] - 1.5) <= 1e-4 * 1.5, (res.x, rf.history[-3:])
    assert rf.hessian_calls > 0
