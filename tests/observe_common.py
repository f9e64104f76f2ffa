"""
Reference for the observables (glims_observe; csrc/observe_clip.h, csrc/observe.hip), written independently of the package's
vectorised code: a plain loop over the cells that works on vertex POSITIONS.

  observe_cell(p, c, kind, level, smooth) -> (V, M_0 .. M_{d-1}) of one simplex with the signed volume of the positions p
  observe_mesh(points, cells, labels, c, queries, n_labels, u, scale) -> [n_q, n_labels, 1 + d]

SHARP clips the simplex at the level set: the cut point on an edge from an in-vertex a to an out-vertex b is
p_a + (c_a - level) / (c_a - c_b) (p_b - p_a); 0 in -> zeros, all in -> the cell, 1 in -> the corner simplex, 1 out -> the cell
minus the corner simplex at the out-vertex, 3-D 2 in / 2 out -> the prism {a, P_ae, P_af | b, P_be, P_bf} as the tetrahedra
(A0,A1,A2,B0), (A1,A2,B0,B1), (A2,B0,B1,B2).  A sub-simplex contributes |v| and |v| times the mean of its vertices (volumes from
determinants of position differences); the sign of the cell's own signed volume multiplies the result.  MASS is the closed
form, SMOOTH the rule simplex_quadrature(d, 4) point by point.

Plus the meshes, labels and fields the CPU and GPU tests share.
"""
import math

import numpy as np

from glimslib_amd.simulation_helpers.postprocess import simplex_quadrature

EPS = 2.0 ** -52
KIND_ID = {"mass": 0, "sharp": 1, "smooth": 2}


def _vol(P):
    """signed volume of a simplex given as d + 1 sequences of d floats (plain Python arithmetic)"""
    if len(P) == 3:
        (x0, y0), (x1, y1), (x2, y2) = P
        return ((x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)) / 2.0
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2), (x3, y3, z3) = P
    a0, a1, a2 = x1 - x0, y1 - y0, z1 - z0
    b0, b1, b2 = x2 - x0, y2 - y0, z2 - z0
    c0, c1, c2 = x3 - x0, y3 - y0, z3 - z0
    return (a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0)) / 6.0


def _simplex_terms(P):
    """[|v|, |v| * centroid] of a sub-simplex"""
    v = abs(_vol(P))
    n, d = len(P), len(P[0])
    return [v] + [v * (sum(P[i][a] for i in range(n)) / n) for a in range(d)]


def in_count(c, level):
    return int(sum(1 for v in c if v >= level))


_RULE = {}


def _rule(d):
    if d not in _RULE:
        _RULE[d] = simplex_quadrature(d, 4)
    return _RULE[d]


def observe_cell(p, c, kind, level=0.0, smooth=1.0):
    """(V, M_0 .. M_{d-1}) of one simplex; p: d + 1 positions, c: d + 1 values.  The volume is the SIGNED one of p."""
    return np.array(_observe_lists([[float(x) for x in row] for row in p], [float(v) for v in c], kind, level, smooth))


def _observe_lists(p, c, kind, level, smooth, T=None):
    """observe_cell on lists of Python floats, returning a list (T: the signed volume of p where the caller has it)"""
    nv, d = len(p), len(p[0])
    if T is None:
        T = _vol(p)
    if kind == "mass":
        M = [0.0] * d
        for i in range(nv):
            for j in range(nv):
                f = (2.0 if i == j else 1.0) * c[i]
                pj = p[j]
                M = [M[a] + f * pj[a] for a in range(d)]
        return [T * sum(c) / nv] + [T / (nv * (nv + 1)) * m for m in M]
    if kind == "smooth":
        lam, w = _rule(d)
        f = w * (0.5 * (np.tanh((lam @ np.array(c) - level) / smooth) + 1.0))     # the integrand at the points of the rule
        return [T * float(f.sum())] + (T * (f @ (lam @ np.array(p)))).tolist()
    assert kind == "sharp"
    ins = [i for i in range(nv) if c[i] >= level]
    if not ins:
        return [0.0] * (1 + d)
    outs = [i for i in range(nv) if not c[i] >= level]
    sign = 1.0 if T >= 0.0 else -1.0
    whole = [abs(T)] + [abs(T) * (sum(p[i][a] for i in range(nv)) / nv) for a in range(d)]

    def cut(a, b):
        t = (c[a] - level) / (c[a] - c[b])
        return [p[a][k] + t * (p[b][k] - p[a][k]) for k in range(d)]

    if not outs:
        tot = whole
    elif len(ins) == 1:
        a = ins[0]
        tot = _simplex_terms([p[a]] + [cut(a, b) for b in outs])
    elif len(outs) == 1:
        b = outs[0]
        corner = _simplex_terms([p[b]] + [cut(a, b) for a in ins])
        tot = [whole[k] - corner[k] for k in range(1 + d)]
    else:
        a, b = ins
        e, f = outs
        A = [p[a], cut(a, e), cut(a, f)]
        B = [p[b], cut(b, e), cut(b, f)]
        t1, t2, t3 = (_simplex_terms(q) for q in ([A[0], A[1], A[2], B[0]], [A[1], A[2], B[0], B[1]], [A[2], B[0], B[1], B[2]]))
        tot = [t1[k] + t2[k] + t3[k] for k in range(1 + d)]
    return [sign * v for v in tot]


def observe_mesh(points, cells, labels, c, queries, n_labels, u=None, scale=1.0):
    """Loop over the cells; per label the contributions are added with math.fsum (the exactly rounded sum).  Also returns the
    in-counts seen per SHARP query and sum |T| (of the configuration integrated over), for the tests' bounds."""
    X = np.asarray(points, dtype=np.float64)
    d = X.shape[1]
    Y = X if u is None else X + scale * np.asarray(u, dtype=np.float64).reshape(len(X), d)
    cells = np.asarray(cells)
    PX, PY, CV, lab = X[cells].tolist(), Y[cells].tolist(), np.asarray(c, dtype=np.float64)[cells].tolist(), list(labels)
    terms = [[[[] for _ in range(1 + d)] for _ in range(n_labels)] for _ in queries]
    counts = [set() for _ in queries]
    sum_abs = 0.0
    for e in range(len(cells)):
        p, cv = PY[e], CV[e]
        orient = 1.0 if _vol(PX[e]) >= 0.0 else -1.0          # a cell counts positively where it is not folded
        T = _vol(p)
        sum_abs += abs(T)
        for k, (kind, level, smooth) in enumerate(queries):
            if kind == "sharp":
                n_in = in_count(cv, level)
                counts[k].add(n_in)
                if n_in == 0:
                    continue
            val = _observe_lists(p, cv, kind, level, smooth, T)
            row = terms[k][int(lab[e])]
            for a in range(1 + d):
                row[a].append(orient * val[a])
    out = np.array([[[math.fsum(terms[k][l][a]) for a in range(1 + d)] for l in range(n_labels)]
                    for k in range(len(queries))])
    return out, counts, sum_abs


def normalise(queries):
    """(kind[, level[, smooth]]) -> (kind, level, smooth)"""
    return [(q[0], float(q[1]) if len(q) > 1 else 0.0, float(q[2]) if len(q) > 2 else 1.0) for q in queries]


def bound(n_cells, sum_abs_T, max_abs_x):
    """|got - want| of the GPU tests: (2 N 2^-53 + 64 2^-52) sum|T| for the measure, times max|x| for the moments -- the worst-case
    difference of two fp64 sums of the same terms in different orders plus the per-cell bound."""
    b = (2.0 * n_cells * 2.0 ** -53 + 64.0 * EPS) * sum_abs_T
    return b, b * max_abs_x


def assert_close(got, want, n_cells, sum_abs_T, max_abs_x, what=""):
    bv, bm = bound(n_cells, sum_abs_T, max_abs_x)
    ev = np.abs(got[..., 0] - want[..., 0]).max()
    em = np.abs(got[..., 1:] - want[..., 1:]).max()
    print("%s: measure err %.3e (bound %.3e)  moment err %.3e (bound %.3e)" % (what, ev, bv, em, bm))
    assert ev <= bv, (what, ev, bv)
    assert em <= bm, (what, em, bm)


# ---- meshes, labels, fields -----------------------------------------------------------------------------------------------
def rectangle():
    from glimslib_amd import fenics_local as fenics
    return fenics.RectangleMesh((0, 0), (2, 1), 12, 9)


def box():
    from glimslib_amd import fenics_local as fenics
    return fenics.BoxMesh((0, 0, 0), (2, 1, 1.5), 5, 4, 4)


def half_labels(mesh, cut=0.9):
    """label 1 left of x_0 = cut (a cell midpoint criterion), label 2 right of it"""
    return np.where(mesh.cell_midpoints()[:, 0] < cut, 1, 2).astype(np.int32)


def sparse_labels(mesh):
    """labels {0, 7, 255} changing from cell to cell: gaps, the top label, three labels inside one wave"""
    return np.array([0, 7, 255], dtype=np.int32)[np.arange(len(mesh.cells)) % 3]


def tables(n_labels):
    r = np.arange(n_labels)
    return dict(D=0.05 + 0.001 * r, rho=0.1 + 0.001 * r, gamma=0.1 + 0.0005 * r, E=np.full(n_labels, 3e-3),
                nu=np.full(n_labels, 0.3))


def bump(points, centre=None, width=0.6, height=0.9):
    """a smooth bump in [0, height], wide enough that every in-count of the levels of QUERIES occurs on the test meshes"""
    X = np.asarray(points, dtype=np.float64)
    lo, hi = X.min(axis=0), X.max(axis=0)
    ctr = lo + 0.45 * (hi - lo) if centre is None else np.asarray(centre)
    r2 = ((X - ctr) ** 2).sum(axis=1) / (width * (hi - lo).min()) ** 2
    return height * np.exp(-r2)


# (0.12 is the reference's T2 threshold; its T1 = 0.80 has no all-in cell on the coarse box, 0.5 has)
QUERIES_BRAIN = [("sharp", 0.12, 1.0), ("sharp", 0.5, 1.0), ("mass", 0.0, 1.0), ("smooth", 0.12, 0.05)]   # (one query less: 140 k cells)
QUERIES = [("sharp", 0.12, 1.0), ("sharp", 0.5, 1.0), ("mass", 0.0, 1.0), ("smooth", 0.12, 0.05), ("smooth", 0.5, 0.05)]


# ---- the problems shared by the CPU and GPU tests: built once per session, never modified ------------------------------------
_problems = {}
_references = {}


def problem(name):
    """(mesh, labels, n_labels, c, u).  'rect': 216 cells, less than one block of the cell pass; 'box': 480 cells, more than one
    block and no multiple of 64; 'brain': the unstructured brain-like mesh, curved interface, cell volumes over decades -- each
    with the two labels of derive_common.two_labels; 'box_sparse': labels {0, 7, 255}; 'box_many': 40 labels (the per-wave
    tables of the cell pass no longer fit in LDS).  c is the bump below (height 0.9), u the field of derive_common.sample_fields."""
    import derive_common as dc
    if name not in _problems:
        if name == "rect":
            mesh = rectangle()
        elif name.startswith("box"):
            mesh = box()
        else:
            from glimslib_amd import workloads
            mesh = workloads.config_brain_like(24000, isolate=True).mesh
        if name == "box_sparse":
            lab = sparse_labels(mesh)
        elif name == "box_many":
            lab = (np.arange(len(mesh.cells)) % 40).astype(np.int32)
        else:
            lab = dc.two_labels(mesh)
            assert set(np.unique(lab)) == {1, 2}
        _, u = dc.sample_fields(mesh.points, seed=len(mesh.points))
        _problems[name] = (mesh, lab, int(lab.max()) + 1, bump(mesh.points), u)
    return _problems[name]


def queries(name):
    return QUERIES_BRAIN if name == "brain" else QUERIES


def reference(name, deformed):
    """The loop reference of a problem: (table [n_q, n_labels, 1 + d], in-counts per query, sum |T|); computed once (the brain-like
    mesh has 161 k cells: some ten seconds per configuration)."""
    key = (name, bool(deformed))
    if key not in _references:
        mesh, lab, n_labels, c, u = problem(name)
        _references[key] = observe_mesh(mesh.points, mesh.cells, lab, c, queries(name), n_labels, u=u if deformed else None)
    return _references[key]
