"""
The assembly sweep (kernels.hip: k_rd_assemble, k_rd_assemble_s, k_rd_assemble_sg) stated in numpy, with its error model.

The sweep at an iterate c forms, per row i,
    A(c) = S + 2 dt N(c)  (stored, fp64 or fp32),   S = M - dt M_rho + dt K_D,   N(c)_ik = sum_T rho_T int_T c_h phi_i phi_k,
    -R_i = b_i - (1/2 (A + S) c)_i  with  b = M c_prev + load  (R = 1/2 (A + S) c - M c_prev - load: the Newton residual),
    dinv_i = 1 / A_ii  (1 on a row with a Dirichlet value), the slice sums of R_i^2, and the flag `lin` of a slice whose stored
    entries all have the bits of S.

  SweepRef        the reference, entry by entry on the CSR pattern of slot_words16_common.row_slots: S, M and N(c) from the
                  oracle's element formulas (reference_mass, reference_triple, barycentric gradients) with the geometry and every
                  sum in np.longdouble, and the absolute-value companions the bounds need:
                    Sabs = |M| + dt |M_rho| + dt |K_D| cell by cell,  Nabs = N(|c|) with |w_T|,
                    rec  = the number of (row, cell) records behind an entry (its cells), R_i = the records of row i,
                    Sgeo, Ngeo, Mgeo = the same sums with every cell weighted by its geometric amplification (below).
  entry_bound, product_bound, residual_bound, dinv_bound, sums_bound     the bounds (derived below, not measured);
                  m_product_bound: the same construction for M z + load (hooks 2 and 10).
  sweep_emulate   the kernel's formula record by record in float64, in the kernel's record order, with the six defects the CPU
                  test must see outside the bound of the output each corrupts (tests/test_sweep_cpu.py).
  lin_reference   which slices of 64 rows (internal numbering) are exactly linear, and how many entries are too close to call.

Error model (first order in u = 2^-53).  One float64 evaluation of an entry of A(c) differs from the exact value by at most

    E_ik = (rec_ik + k0) u (Sabs_ik + 2 dt Nabs_ik)  +  KG u (Sgeo_ik + 2 dt Ngeo_ik),          k0 = 2 NV + 10,  KG = 3 (2 d + d!).

  First term, the sweep's operation count (rd_assemble_s_slice).  The `corner` lambda forms a record's term w (c_i + c_m + s) or
  w (4 c_i + 2 s) in NV - 1 additions for s, two more and one product: NV + 2 roundings, and w = rho |T| d!/(d+3)! carries two
  more (k_corner_weights): NV + 4.  An accumulator takes rec_ik additions.  Phase 3 forms S + two_dt * a in two roundings.  The
  entry of S was summed over the same rec_ik cells at set-up from local values of at most d + 5 roundings each (a d-term dot
  product, the volume, D, dt, and the three terms added).  In all rec_ik + (NV + 4) + 2 + (d + 5) = rec_ik + 2 NV + 10 roundings,
  each relative to a partial result bounded by Sabs_ik + 2 dt Nabs_ik.
  Second term, the geometry.  |T| and the gradients come from the cofactors and the determinant of the edge matrix in float64
  (k_egeo; numpy's inverse in the oracle): the determinant is a sum of d! products of rounded edge components, off by at most
  (2 d + d!) u times the sum P_T of the products' absolute values, i.e. relative kappa_T (2 d + d!) u with kappa_T = P_T / |det|
  >= 1, which a flat cell makes large.  A gradient is a cofactor (an error of at most (2 d + d!) u relative to the product of
  the other edges' lengths: gn_m = [2] |r_p| |r_q| / |det| >= |grad lambda_m|, and gn_0 = sum of the others, as both
  implementations form grad lambda_0 = - sum) over that determinant.  A local entry is a product of |T| and (for K_D) two
  gradients: three such factors, hence KG = 3 (2 d + d!), with Sgeo = sum_T kappa_T (|T| Mr (1 + dt |rho|) + dt D |T| gn_i gn_k)
  and Ngeo = sum_T kappa_T |N_T(|c|)|.  On a well-shaped cell kappa_T is of order one and this term is a few dozen u.
The reference is exact to 2^-64 where np.longdouble is wider than float64 and one such evaluation where it is not; the bounds
below always carry one E for the reference next to the kernel's own, so they hold on either machine:

    stored fp64 entry     |A_ik - ref_ik|  <=  E_ik (kernel) + E_ik (reference)                              [entry_bound]
    stored fp32 entry     ... + 2^-24 (|ref_ik| + that bound)
    product via k_spmv    |y_i - (A_ref z)_i|  <=  sum_k entry_bound_ik |z_k| + (len_i + k1) u (|A_ref| |z|)_i,   k1 = 2:
                          one fused multiply-add per slot and the final store                                 [product_bound]
    residual              sum_k entry_bound_ik |c_k|                      (Av and S each within E; their mean too)
                          + (len_i + 4) u (1/2 (Aabs + Sabs) |c|)_i        (Av + S, the product, len_i additions, b - r)
                          + sum_k EM_ik |c_prev,k| + (len_i + k1 + 2) u ((|M| |c_prev|)_i + |load_i|)         [residual_bound]
                          with EM the entry bound of M alone.  No fp32 term on an fp32 handle: the residual is formed from
                          the unrounded Av.
    dinv                  |dinv_i A_ref,ii - 1|  <=  entry_bound_ii / |A_ref,ii| + 2 u   (fp64 bound also on an fp32 handle:
                          the diagonal is taken before the store)                                             [dinv_bound]
    slice sums            |p - sum R_i^2|  <=  n u sum R_i^2: the same non-negative terms in another order     [sums_bound]

Out of scope here: the folded guess pass (FG = 1, 2) and the second right-hand side.  No hook reaches them; they stay with
tests/test_gpu_fused_guess_pass.py, which compares them bit for bit with the separate k_cheb launch, and that launch is held
to a reference in tests/test_gpu_chebyshev.py and tests/test_gpu_cheb_streams.py.
"""
import math

import numpy as np

from oracle.glims_oracle import p1_geometry, reference_mass, reference_triple

from quad_pass_common import (CASES, FAN_K, LOOPED, TABLES, case, cell_weights, fan_mesh, rho_of,      # noqa: F401  (re-exported:
                              three_tissues)                                                           # one set of meshes)
from slot_words16_common import row_slots

LD = np.longdouble
WIDE = np.finfo(LD).eps < np.finfo(np.float64).eps
REF_EVALS = 1 if WIDE else 2      # float64 evaluations between the oracle (one) and the reference (none, or one)
U32 = 2.0 ** -24
U64 = 2.0 ** -53
K1 = 2
MUTATIONS = ('drop_last', 'diag3', 'slot_shift', 'stored_dt', 'dinv_from_S', 'residual_from_rounded')
# which outputs a defect corrupts (A: the stored matrix through a product; R: the residual; dinv) -- the others must stay inside
# their bounds, or the GPU test could not tell the outputs apart
CORRUPTS = {'drop_last': {'A', 'R', 'dinv'}, 'diag3': {'A', 'R', 'dinv'}, 'slot_shift': {'A', 'R', 'dinv'},
            'stored_dt': {'A'}, 'dinv_from_S': {'dinv'}, 'residual_from_rounded': {'R'}}


def k0_of(nv):
    return 2 * nv + 10


def kg_of(d):
    return 3 * (2 * d + math.factorial(d))


# ---- structure ----------------------------------------------------------------------------------------------------------------

class Pattern:
    """CSR pattern with the diagonal, columns ascending; pos[T, a, b] = the entry of (cells[T, a], cells[T, b])."""

    def __init__(self, cells, n):
        cells = np.asarray(cells).astype(np.int64)
        self.n, self.nv, self.cells = n, cells.shape[1], cells
        self.ptr, self.cols = row_slots(cells, n)
        self.len = np.diff(self.ptr)
        self.rows = np.repeat(np.arange(n, dtype=np.int64), self.len)
        key = self.rows * n + self.cols
        i = np.repeat(cells, self.nv, axis=1)
        j = np.tile(cells, (1, self.nv))
        self.pos = np.searchsorted(key, i * n + j).reshape(len(cells), self.nv, self.nv)
        self.rec = np.bincount(self.pos.ravel(), minlength=len(self.cols))          # records (cells) behind an entry
        self.diag = np.searchsorted(key, np.arange(n, dtype=np.int64) * (n + 1))
        self.R = self.rec[self.diag]                                                 # records of a row

    def scatter(self, local, dtype=LD):
        out = np.zeros(len(self.cols), dtype=dtype)
        np.add.at(out, self.pos.ravel(), np.asarray(local, dtype=dtype).ravel())
        return out

    def matvec(self, vals, x, dtype=LD):
        y = np.zeros(self.n, dtype=dtype)
        np.add.at(y, self.rows, np.asarray(vals, dtype=dtype) * np.asarray(x, dtype=dtype)[self.cols])
        return y


def geometry_ld(points, cells):
    """(vol, grads [M, nv, d], kappa, gn [M, nv]) from the cofactors of the edge matrix in np.longdouble."""
    X = np.asarray(points, dtype=np.float64).astype(LD)[np.asarray(cells)]
    d = X.shape[2]
    r = X[:, 1:, :] - X[:, :1, :]                                   # [M, d, d], rows = edges
    M = len(r)
    g = np.zeros((M, d + 1, d), dtype=LD)
    ln = np.sqrt((r * r).sum(axis=2))                               # edge lengths
    if d == 2:
        a, b, c, e = r[:, 0, 0], r[:, 0, 1], r[:, 1, 0], r[:, 1, 1]
        det = a * e - b * c
        P = np.abs(a * e) + np.abs(b * c)
        g[:, 1, 0], g[:, 1, 1], g[:, 2, 0], g[:, 2, 1] = e / det, -c / det, -b / det, a / det
        gn = np.stack([ln[:, 1], ln[:, 0]], axis=1) / np.abs(det)[:, None]
    else:
        c12, c20, c01 = np.cross(r[:, 1], r[:, 2]), np.cross(r[:, 2], r[:, 0]), np.cross(r[:, 0], r[:, 1])
        det = (r[:, 0] * c12).sum(axis=1)
        a12 = np.stack([np.abs(r[:, 1, (k + 1) % 3] * r[:, 2, (k + 2) % 3]) + np.abs(r[:, 1, (k + 2) % 3] * r[:, 2, (k + 1) % 3])
                        for k in range(3)], axis=1)
        P = (np.abs(r[:, 0]) * a12).sum(axis=1)
        for m, cf in enumerate((c12, c20, c01)):
            g[:, m + 1, :] = cf / det[:, None]
        gn = 2.0 * np.stack([ln[:, 1] * ln[:, 2], ln[:, 2] * ln[:, 0], ln[:, 0] * ln[:, 1]], axis=1) / np.abs(det)[:, None]
    g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
    gn = np.concatenate([gn.sum(axis=1, keepdims=True), gn], axis=1)
    vol = np.abs(det) / math.factorial(d)
    return vol, g, P / np.abs(det), gn


class SweepRef:
    """The c-independent part of the reference of one workload (pattern, S, M and their companions), in np.longdouble."""

    def __init__(self, w):
        p, cells = w.mesh.points, np.asarray(w.mesh.cells)
        self.w, self.n, self.d, self.nv, self.dt = w, len(p), p.shape[1], cells.shape[1], float(w.dt)
        self.pat = pat = Pattern(cells, self.n)
        D, rho = w.per_cell('D').astype(LD), w.per_cell('rho').astype(LD)
        vol, g, kappa, gn = geometry_ld(p, cells)
        dt = LD(self.dt)
        Mr = reference_mass(self.d).astype(LD)
        self.Tr = reference_triple(self.d).astype(LD)
        m_loc = vol[:, None, None] * Mr[None]
        k_loc = (D * vol)[:, None, None] * np.einsum('mad,mbd->mab', g, g)
        kn_loc = (np.abs(D) * vol)[:, None, None] * gn[:, :, None] * gn[:, None, :]
        self.rho_vol, self.kappa = rho * vol, kappa
        self.M = pat.scatter(m_loc)
        self.S = pat.scatter(m_loc - dt * rho[:, None, None] * m_loc + dt * k_loc)
        self.Sabs = pat.scatter(m_loc + dt * np.abs(rho)[:, None, None] * m_loc + dt * np.abs(k_loc))
        self.Mgeo = pat.scatter(kappa[:, None, None] * m_loc)
        self.Sgeo = pat.scatter(kappa[:, None, None] * (m_loc * (1.0 + dt * np.abs(rho))[:, None, None] + dt * kn_loc))
        self.k0, self.kg = k0_of(self.nv), kg_of(self.d)
        self.EM = (pat.rec + self.k0) * U64 * self.M + self.kg * U64 * self.Mgeo        # one float64 evaluation of M_ik

    def at(self, c):
        return SweepRefAt(self, c)

    def m_product(self, z):
        return self.pat.matvec(self.M, z)

    def m_product_bound(self, z, load=None):
        """M z + load through k_spmv (len_i + k1 roundings) or from the sweep's incidence loop (MB = 1: q_i sum_T w_T (s_T + z_i),
        R_i fused multiply-adds on terms of NV + 4 roundings and two more for q and the load): the larger count, relative to
        (M |z|)_i + |load_i|, next to the two evaluations of M's entries."""
        za = np.abs(z)
        la = 0.0 if load is None else np.abs(np.asarray(load, dtype=np.float64))
        return (self.pat.matvec(2.0 * self.EM, za)
                + (np.maximum(self.pat.len, self.pat.R) + self.nv + 8) * U64 * (self.pat.matvec(self.M, za) + la))


class SweepRefAt:
    """The reference at an iterate c: N(c), A(c) and the bounds."""

    def __init__(self, base, c):
        self.base, self.c = base, np.asarray(c, dtype=np.float64)
        b, pat = base, base.pat
        cl = self.c.astype(LD)[pat.cells]
        n_loc = b.rho_vol[:, None, None] * np.einsum('ijk,mk->mij', b.Tr, cl)
        nabs_loc = np.abs(b.rho_vol)[:, None, None] * np.einsum('ijk,mk->mij', b.Tr, np.abs(cl))
        two_dt = LD(2.0 * b.dt)
        self.N = pat.scatter(n_loc)
        self.A = b.S + two_dt * self.N
        self.Aabs = b.Sabs + two_dt * pat.scatter(nabs_loc)
        self.Ageo = b.Sgeo + two_dt * pat.scatter(b.kappa[:, None, None] * nabs_loc)
        self.E = (pat.rec + b.k0) * U64 * self.Aabs + b.kg * U64 * self.Ageo             # one float64 evaluation of A_ik

    # -- references (float64 views of the longdouble values) ---------------------------------------------------------------------
    def product(self, z):
        return self.base.pat.matvec(self.A, z)

    def residual(self, c_prev, load=None):
        b, pat = self.base, self.base.pat
        r = pat.matvec(LD(0.5) * (self.A + b.S), self.c) - pat.matvec(b.M, c_prev)
        return r if load is None else r - np.asarray(load, dtype=np.float64).astype(LD)

    def diag(self):
        return self.A[self.base.pat.diag]

    # -- bounds ----------------------------------------------------------------------------------------------------------------
    # evals: how many float64 evaluations stand between the two sides -- 2 for a kernel against the reference (the kernel's
    # own and the reference's), REF_EVALS for another float64 statement of the same formulas against the reference (the
    # reference-rounding term alone)
    def entry_bound(self, fp32=False, evals=2):
        e = evals * self.E
        return e + U32 * (np.abs(self.A) + e) if fp32 else e

    def product_bound(self, z, fp32=False, evals=2):
        pat = self.base.pat
        za = np.abs(z)
        return pat.matvec(self.entry_bound(fp32, evals), za) + (pat.len + K1) * U64 * pat.matvec(np.abs(self.A), za)

    def residual_bound(self, c_prev, load=None, evals=2):
        b, pat = self.base, self.base.pat
        ca, pa = np.abs(self.c), np.abs(c_prev)
        la = 0.0 if load is None else np.abs(np.asarray(load, dtype=np.float64))
        return (pat.matvec(self.entry_bound(False, evals), ca)
                + (pat.len + 4) * U64 * pat.matvec(LD(0.5) * (self.Aabs + b.Sabs), ca)
                + pat.matvec(evals * b.EM, pa) + (pat.len + K1 + 2) * U64 * (pat.matvec(b.M, pa) + la))

    def dinv_bound(self, evals=2):
        d = self.base.pat.diag
        return self.entry_bound(False, evals)[d] / np.abs(self.A[d]) + 2.0 * U64


def sums_bound(n, s):
    return n * U64 * s


def f64(v):
    return np.asarray(v, dtype=np.float64)


def inside(err, bound):
    """Row by row (entry by entry): never a norm."""
    return bool(np.all(np.asarray(err, dtype=LD) <= np.asarray(bound, dtype=LD)))


def worst(err, bound):
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


# ---- fields ---------------------------------------------------------------------------------------------------------------------

BALL_CENTRES = (0.22, 0.5, 0.78)      # near one corner, the centre, near the opposite corner (fractions of the extent)


def ball_field(w, k):
    """c = 0 outside a ball of 0.3 of the largest extent around centre k, the case's bump (at least 0.02) inside."""
    p = w.mesh.points
    lo, hi = p.min(axis=0), p.max(axis=0)
    ctr = lo + BALL_CENTRES[k] * (hi - lo)
    r = 0.3 * (hi - lo).max()
    return np.where(((p - ctr) ** 2).sum(axis=1) < r * r, np.maximum(w.c0, 0.02), 0.0)


def fields(w):
    """The three iterates of the CPU test: the case's bump, a random field in [0.02, 1], the ball at the centre."""
    rng = np.random.default_rng(5)
    return {'bump': np.asarray(w.c0, dtype=np.float64), 'random': rng.uniform(0.02, 1.0, len(w.mesh.points)),
            'ball': ball_field(w, 1)}


# ---- the kernel's formula in float64 --------------------------------------------------------------------------------------------

def float64_operators(w, pat):
    """S and M as ONE float64 evaluation of the element formulas (the oracle's geometry, float64 sums in cell order)."""
    p, cells = w.mesh.points, pat.cells
    vol, g = p1_geometry(p, cells)
    D, rho, dt = w.per_cell('D'), w.per_cell('rho'), float(w.dt)
    m_loc = vol[:, None, None] * reference_mass(p.shape[1])[None]
    k_loc = (D * vol)[:, None, None] * np.einsum('mad,mbd->mab', g, g)
    return pat.scatter(m_loc - dt * rho[:, None, None] * m_loc + dt * k_loc, np.float64), pat.scatter(m_loc, np.float64)


def sweep_emulate(w, pat, c, c_prev, load=None, fp32=False, mutation=None):
    """The sweep record by record in float64: a row's records in cell order (the order of the incidence lists), a record's term
    as the `corner` lambda forms it, phase 3 slot by slot (the slots of slot_words16_common.row_slots).  Returns a dict:
    A (the stored entries, CSR order, as float64), R, dinv, sumsq.  mutation: see MUTATIONS; 'slot_shift' reads the first record's
    first other vertex one slot on in the row (cyclically), 'residual_from_rounded' needs fp32."""
    assert mutation is None or mutation in MUTATIONS
    assert mutation != 'residual_from_rounded' or fp32
    n, nv, cells = pat.n, pat.nv, pat.cells
    c = np.asarray(c, dtype=np.float64)
    dt = float(w.dt)
    two_dt = 2.0 * dt
    S, M = float64_operators(w, pat)
    wT = cell_weights(w.mesh.points, cells, rho_of(w))
    rows = cells.T.ravel()
    cell_of = np.tile(np.arange(len(cells)), nv)
    others = np.concatenate([np.delete(cells, p, axis=1) for p in range(nv)])
    order = np.lexsort((cell_of, rows))
    rows, cell_of, others = rows[order], cell_of[order], others[order].copy()
    first = np.ones(len(rows), dtype=bool)
    first[1:] = rows[1:] != rows[:-1]
    last = np.ones(len(rows), dtype=bool)
    last[:-1] = rows[1:] != rows[:-1]
    key = pat.rows * n + pat.cols
    if mutation == 'slot_shift':
        r = rows[first]
        slot = np.searchsorted(key, r * n + others[first, 0]) - pat.ptr[r]
        others[first, 0] = pat.cols[pat.ptr[r] + (slot + 1) % pat.len[r]]
    if mutation == 'drop_last':
        rows, cell_of, others = rows[~last], cell_of[~last], others[~last]
    ci = c[rows]
    cv = c[others]
    st = ci.copy()
    for m in range(nv - 1):
        st = st + cv[:, m]
    wr = wT[cell_of]
    acc = np.zeros(len(pat.cols))
    np.add.at(acc, pat.diag[rows], wr * ((3.0 if mutation == 'diag3' else 4.0) * ci + 2.0 * st))
    # record-major, so that an accumulator's terms arrive in record order (unbuffered: one float64 addition per term)
    np.add.at(acc, np.searchsorted(key, rows[:, None] * n + others).ravel(), (wr[:, None] * ((ci[:, None] + cv) + st[:, None])).ravel())
    Av = S + two_dt * acc
    stored = S + dt * acc if mutation == 'stored_dt' else Av
    if fp32:
        stored = stored.astype(np.float32).astype(np.float64)
    Ar = stored if mutation == 'residual_from_rounded' else Av
    r = np.zeros(n)
    np.add.at(r, pat.rows, 0.5 * (Ar + S) * c[pat.cols])
    b = np.zeros(n)
    np.add.at(b, pat.rows, M * np.asarray(c_prev, dtype=np.float64)[pat.cols])
    if load is not None:
        b = b + load
    R = -(b - r)
    dinv = 1.0 / (S if mutation == 'dinv_from_S' else Av)[pat.diag]
    return dict(A=stored, R=R, dinv=dinv, sumsq=float(np.sum(R * R)))


# ---- exactly-linear slices ---------------------------------------------------------------------------------------------------------

def lin_reference(w, c, numbering, ref=None):
    """(flags, ambiguous): flags[s] = every stored entry of the 64 rows of slice s (row i sits in slice numbering[i] // 64) has
    the bits of S, by the kernel's definition bits(fl(S + 2 dt a)) == bits(S) evaluated in float64 on the reference's values;
    ambiguous = the number of entries with 0 < 2 dt |N_ik| <= 2^-50 Sabs_ik, where a rounding could decide."""
    at = (ref or SweepRef(w)).at(c)
    b, pat = at.base, at.base.pat
    two_dt = 2.0 * b.dt
    S, N = f64(b.S), f64(at.N)
    changed = (S + two_dt * N).view(np.uint64) != S.view(np.uint64)
    t = two_dt * np.abs(N)
    ambiguous = int(np.sum((t > 0.0) & (t <= 2.0 ** -50 * f64(b.Sabs))))
    numbering = np.asarray(numbering, dtype=np.int64)
    n_slices = (pat.n + 63) // 64
    bad = np.zeros(n_slices, dtype=bool)
    bad[numbering[pat.rows[changed]] // 64] = True
    return ~bad, ambiguous
