"""
Discrete adjoint on the GPU where its kernels branch: label chunks of the sensitivity pass (GL_ADJ_LT = 8 labels per launch),
meshes with more cells than its fixed grid has threads (2048 x 256 = 524 288), a Delaunay mesh under a shuffled numbering,
displacement terms at several steps with clamp values and a mechanical load, the forward variants ForwardGuard swaps around,
degenerate term sets, the output sizes of Handle.adjoint_gradient and the public parameter maps end to end.  The reference is
the numpy adjoint of tests/adjoint_common.py on the GPU's own trajectory (itself checked by finite differences in
tests/test_adjoint_cpu.py).
"""
import numpy as np
import pytest

from adjoint_common import adjoint, many_tissues, renumber, u_terms
from test_gpu_adjoint import _SKIP, _record, _rel

pytestmark = pytest.mark.gpu


def _handle(backend, prob, mechanics=True, **opts):
    h = backend.Handle(prob.points, prob.cells, prob.labels)
    h.set_materials(prob.D, prob.rho, prob.gamma, prob.E, prob.nu)
    h.set_options(dt=prob.dt, newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12, **opts)
    if prob.dir_c is not None:
        h.set_dirichlet_c(prob.dir_c[0], prob.dir_c[1])
    if mechanics:
        h.set_dirichlet_u(prob.dir_u[0], prob.dir_u[1])
        if prob.mech_load is not None:
            h.set_mech_load(prob.mech_load)
    if prob.rd_load is not None:
        h.set_rd_load(prob.rd_load)
    h.setup(with_mechanics=mechanics)
    h.set_state(prob.c0)
    return h


def _compare(h, prob, traj, terms, tol=1e-8):
    """Gradient of the recorded run against the numpy adjoint on the same trajectory; returns the GPU result."""
    out = h.adjoint_gradient(terms)
    ref = adjoint(prob, prob.oracle(), traj, terms)
    rel = {what: _rel(a, b) for a, b, what in zip(out, ref, ("J", "dD", "drho", "dgamma", "dc0"))}
    print("relative error vs numpy:", " ".join("%s %.2e" % kv for kv in rel.items()))
    for a, b, what in zip(out, ref, ("J", "dD", "drho", "dgamma", "dc0")):
        assert rel[what] <= tol, (what, rel[what], a, b)
    return out


# ---- 1. label chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,L,n,empty,zero", [(2, 9, 16, 3, 5), (3, 17, 6, 12, 9)])
def test_label_chunks(backend, dim, L, n, empty, zero):
    """9 labels: one past the first chunk of 8; 17: a third chunk holding one label.  One id no cell carries, one tissue with
    D = rho = gamma = 0; a displacement term, so the coupling pass runs over the chunks as well."""
    prob = many_tissues(dim, L, n=n, empty=(empty,), zero=(zero,), zero_gamma=(zero,), seed=L)
    count = np.bincount(prob.labels, minlength=L)
    assert count[empty] == 0 and np.all(np.delete(count, empty) > 0)
    N = 5
    terms = prob.terms(N)
    h = _handle(backend, prob)
    J, dD, drho, dgam, dc0 = _compare(h, prob, _record(h, N), terms)
    assert dD.shape == (L,) and dD[empty] == 0 and drho[empty] == 0 and dgam[empty] == 0
    assert dD[L - 1] != 0 and drho[L - 1] != 0 and dgam[L - 1] != 0   # the last (partial) chunk is reached
    assert dD[zero] != 0 and drho[zero] != 0 and dgam[zero] != 0      # sensitivities of a passive tissue
    h.close()


# ---- 2. more cells than the sensitivity grid has threads ------------------------------------------------------------------
def test_mesh_beyond_the_fixed_grid(backend):
    """530 x 530 rectangle: 561 800 cells > 2048 x 256 = 524 288, so some threads of the grid-stride loop take a second cell.
    The labels are scrambled bands, so the second cells of a thread carry other labels than its first ones."""
    prob = many_tissues(2, 10, n=530, seed=11)
    assert prob.cells.shape[0] == 561800 > 2048 * 256
    N = 2
    rng = np.random.default_rng(12)
    n = len(prob.points)
    terms = [dict(step=N, kind="c_thresh", level=0.3, smooth=0.1, weight=1.0, target=rng.uniform(0, 1, n)),
             dict(step=1, kind="c_l2", weight=2.0, target=rng.uniform(0, 0.5, n))]
    h = _handle(backend, prob, mechanics=False)
    g = _compare(h, prob, _record(h, N), terms)
    h.close()
    # the same trajectory on two fresh handles: the same bits
    again = []
    for _ in range(2):
        h = _handle(backend, prob, mechanics=False)
        h.adjoint_record(True)
        for _ in range(N):
            assert h.step(1) == 0
        again.append(h.adjoint_gradient(terms))
        h.close()
    for a in again:
        assert a[0] == g[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], g[1:]))


# ---- 3. unstructured mesh, shuffled numbering -----------------------------------------------------------------------------
def test_unstructured_mesh_in_a_shuffled_numbering(backend):
    """Delaunay mesh of random points, node ids randomly permuted: the targets (scalar and [n][dim]) go in and dc0 comes out
    through k_perm in the caller's numbering; k_cell_nodes / k_gt_rows see rows of ~6 to ~45 entries."""
    from glimslib_amd import workloads
    w = workloads.config_unstructured(n_points=6000, seed=1)
    pts, cells, _ = renumber(w.mesh.points, w.mesh.cells, 5)
    prob = many_tissues(3, 6, mesh=(pts, cells), u_clamp=0.01, seed=13)
    N = 4
    terms = prob.terms(N) + u_terms(prob, [2], seed=14)
    h = _handle(backend, prob)
    _compare(h, prob, _record(h, N), terms)
    h.close()


# ---- 4. displacement terms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["BLOCK_JACOBI", "MULTIGRID"])
@pytest.mark.parametrize("dim", [2, 3])
def test_displacement_terms_with_clamp_values_and_load(backend, dim, precond):
    """u_l2 at step 0, midway and twice at the last step; non-zero Dirichlet displacement (the xD branch of the elastic
    solve) and a mechanical load (gl_apply_G with the load)."""
    prob = many_tissues(dim, 3, n=16 if dim == 2 else 6, u_clamp=0.02, mech_load=1.0, seed=20 + dim)
    N = 4
    terms = u_terms(prob, [0, 2, N, N], seed=21) + [dict(step=N, kind="c_l2", weight=1.0,
                                                         target=np.full(len(prob.points), 0.2))]
    h = _handle(backend, prob, mech_precond=getattr(backend, "PRECOND_" + precond))
    _compare(h, prob, _record(h, N), terms)
    assert h.adjoint_stats()["mech_solves"] == 2 * 3   # u_k and mu_k at steps 0, 2 and N: one u_k for the two terms at N
    h.close()


# ---- 5. forward variants --------------------------------------------------------------------------------------------------
_VARIANTS = {
    "rd_pcg": lambda b: dict(rd_linear=b.RD_LINEAR_PCG),
    "rd_chebyshev": lambda b: dict(rd_linear=b.RD_LINEAR_CHEBYSHEV),
    "fp32_jacobian": lambda b: dict(flags=b.FLAG_FP32_JACOBIAN),
    "full_newton": lambda b: dict(flags=b.FLAG_FULL_NEWTON),
    "rd_multigrid_fp32_smoother": lambda b: dict(rd_precond=b.RD_PRECOND_MULTIGRID, flags=b.FLAG_MG_FP32_SMOOTHER),
    "mech_block_jacobi": lambda b: dict(mech_precond=b.PRECOND_BLOCK_JACOBI),
    "rd_load_and_moving_dirichlet_c": lambda b: dict(),
}


def _nostat(h):
    return {k: v for k, v in h.stats().items() if k not in _SKIP}


@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_forward_variants(backend, variant):
    """(a) the gradient of a run under each variant matches the numpy adjoint of its trajectory; (b) a handle that recorded
    and computed a gradient steps on and solves mechanics to the bits and stats of a twin that never did."""
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
    if moving:
        assert not np.allclose(traj[1][prob.dir_c[0]], traj[N][prob.dir_c[0]])
    assert np.array_equal(traj[-1], b.get_state(want_u=False)[0]) and _nostat(a) == _nostat(b)
    _compare(a, prob, traj, terms)
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


# ---- 6. degenerate term sets ----------------------------------------------------------------------------------------------
def test_degenerate_term_sets(backend):
    prob = many_tissues(2, 3, n=12, u_clamp=0.01, seed=40)
    n = len(prob.points)
    rng = np.random.default_rng(41)
    at0 = [dict(step=0, kind="c_thresh", level=0.3, smooth=0.1, weight=1.5, target=rng.uniform(0, 1, n)),
           dict(step=0, kind="c_l2", weight=0.5, target=rng.uniform(0, 0.5, n))] + u_terms(prob, [0], seed=42)
    N = 3
    h = _handle(backend, prob)
    traj = _record(h, N)
    # no terms: J = 0 and every gradient exactly 0
    J, dD, drho, dgam, dc0 = h.adjoint_gradient([])
    assert J == 0.0 and not dD.any() and not drho.any() and not dgam.any() and not dc0.any()
    # terms at step 0 only: no backward step contributes to dD, drho
    J, dD, drho, dgam, dc0 = _compare(h, prob, traj, at0)
    assert not dD.any() and not drho.any() and dgam.any()
    # a zero weight is the term omitted
    terms = prob.terms(N)
    ref = h.adjoint_gradient(terms)
    for extra in (dict(terms[2], weight=0.0), dict(u_terms(prob, [1], seed=43)[0], weight=0.0)):
        got = h.adjoint_gradient(terms + [extra])
        assert got[0] == ref[0] and all(np.array_equal(x, y) for x, y in zip(got[1:], ref[1:]))
    h.close()
    # N = 0: dc0 from the copy branch
    h = _handle(backend, prob)
    traj = _record(h, 0)
    J, dD, drho, dgam, dc0 = _compare(h, prob, traj, at0)
    assert not dD.any() and not drho.any()
    assert h.adjoint_stats()["backward_steps"] == 0
    h.close()


# ---- 3 (fix). output sizes of Handle.adjoint_gradient ---------------------------------------------------------------------
def test_adjoint_gradient_outputs_follow_set_materials(backend):
    prob = many_tissues(2, 5, n=8, seed=50)
    h = _handle(backend, prob, mechanics=False)
    _record(h, 2)
    terms = prob.terms(2, with_u=False)
    st = h.adjoint_stats()
    for wrong in (2, 4, 6):
        with pytest.raises(ValueError):
            h.adjoint_gradient(terms, wrong)
    assert h.adjoint_stats() == st   # refused before the library ran
    g = h.adjoint_gradient(terms, 5)
    assert all(len(x) == 5 for x in g[1:4])
    g2 = h.adjoint_gradient(terms)
    assert all(np.array_equal(x, y) for x, y in zip(g[1:], g2[1:]))
    h.set_materials(*(np.append(x, x[-1]) for x in (prob.D, prob.rho, prob.gamma, prob.E, prob.nu)))
    assert h.n_labels == 6
    h.close()


# ---- 7. public API ----------------------------------------------------------------------------------------------------------
def _brain_sim(tmp_path, cls, n_params):
    from glimslib_amd import fenics_local as fenics

    class Boundary(fenics.SubDomain):
        def inside(self, x, on_boundary):
            return on_boundary

    mesh = fenics.RectangleMesh(fenics.Point(-5, -5), fenics.Point(5, 5), 20, 20)
    r = np.linalg.norm(mesh.cell_midpoints(), axis=1)
    lab = np.where(r < 1.2, 4, np.where(r < 2.8, 3, np.where(r < 4.2, 2, 1)))   # Ventricles, WM = 3, GM = 2, CSF = 1
    opts = dict(newton_rtol=1e-13, newton_atol=1e-16, mech_rtol=1e-12)
    sim = cls(mesh, solver_options=opts)
    sim.setup_global_parameters(subdomains=lab, domain_names={1: 'CSF', 3: 'WM', 2: 'GM', 4: 'Ventricles'},
                                boundaries={'boundary_all': Boundary()},
                                dirichlet_bcs={'clamped': {'bc_value': fenics.Constant((0.0, 0.0)),
                                                           'named_boundary': 'boundary_all', 'subspace_id': 0}},
                                von_neumann_bcs={})
    iv = fenics.Expression('exp(-(pow(x[0]-2.4,2)+pow(x[1]-0.5,2))/1.5)', degree=1)
    common = dict(iv_expression={0: fenics.Constant((0.0, 0.0)), 1: iv}, sim_time=4, sim_time_step=1)
    if cls.__name__ == "TumorGrowthBrain":
        sim.setup_model_parameters(E_GM=3e-3, E_WM=2e-3, E_CSF=1e-3, E_VENT=1e-3, nu_GM=0.45, nu_WM=0.4, nu_CSF=0.45,
                                   nu_VENT=0.3, D_GM=0.02, D_WM=0.1, rho_GM=0.05, rho_WM=0.1, coupling=0.1, **common)
    else:
        sim.setup_model_parameters(diffusion=0.05, proliferation=0.1, coupling=0.1, E=2e-3, poisson=0.4, **common)
    x = mesh.points
    n = len(x)
    ct = 0.6 * np.exp(-((x - np.array([2.0, 1.0])) ** 2).sum(axis=1) / 2.0)
    ut = 0.05 * np.stack([np.sin(x[:, 1]), np.cos(x[:, 0])], axis=1)

    def terms(s, n_steps):
        return [dict(step=n_steps, kind="c_l2", weight=1.0, target=ct),
                dict(step=2, kind="c_thresh", level=0.4, smooth=0.1, weight=0.5, target=(ct > 0.4).astype(float)),
                dict(step=n_steps, kind="u_l2", weight=1.0, target=ut)]
    assert n == sim.mesh.points.shape[0]
    from glimslib_amd.optimization import ReducedFunctional
    return sim, ReducedFunctional(sim, n_params, terms, run_kwargs=dict(output_dir=str(tmp_path)))


@pytest.mark.parametrize("cls,m0", [("TumorGrowthBrain", [0.1, 0.02, 0.1, 0.05, 0.1]), ("TumorGrowth", [0.05, 0.1, 0.1])])
def test_reduced_functional_matches_central_differences(tmp_path, cls, m0):
    """TumorGrowthBrain with WM = 3 before GM = 2 (ids not sorted): dJ/d(D_WM, D_GM, rho_WM, rho_GM, coupling) through
    tissue_name_id_map and the label sum of dgamma; TumorGrowth with (diffusion, proliferation, coupling)."""
    from glimslib_amd import simulation
    sim, rf = _brain_sim(tmp_path, getattr(simulation, cls), len(m0))
    m0 = np.array(m0)
    g = rf.derivative(m0)
    eps = 1e-4
    for i in range(len(m0)):
        e = np.zeros_like(m0)
        e[i] = eps * m0[i]
        num = (rf(m0 + e) - rf(m0 - e)) / (2 * e[i])
        assert abs(g[i] - num) <= 1e-5 * abs(num), (i, g, num)
    sim.close()
