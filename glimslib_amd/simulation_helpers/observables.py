"""
Tumour volumes and centres of mass per tissue (the numpy statement of ``glims_observe``; csrc/observe.hip, csrc/observe_clip.h).

For a P1 concentration c_h on a simplex mesh with one label per cell, a query q is integrated over the cells of every label:
the measure V = int q dx and the first moments M_a = int x_a q dx, with

  'mass'    q = c_h                                        exact
  'sharp'   q = 1 where c_h >= level (a tie is in)         exact: every cell is clipped at the level set
  'smooth'  q = 1/2 (tanh((c_h - level) / smooth) + 1)     the degree-7 rule simplex_quadrature(d, 4) (thresh(); the discrete
                                                           statement of that rule, not a converged integral for small smooth)

-- what the reference's compute_from_conc_for_each_time_step / compute_volume_thresholded / compute_com_all compute with
``conditional(c >= threshold, 1, 0)`` and ``thresh()`` over dx and dx(subdomain_id)
(optimization_workflow/image_based_optimization.py:1333-1397, :1262-1301, :1416-1430, :1470-1472); the reference's extra L2
projection of q before the per-subdomain integrals is left out (it changes nothing over the whole domain).

Every query is evaluated per cell in barycentric terms, b0 = V / |T| and b_k = int lambda_k q / |T|, vectorised over the cells;
then V = |T| b0 and M = |T| sum_k b_k p_k with the vertex positions p_k = X_k (reference configuration) or X_k + scale u_k
(deformed: |T| is the signed volume of the displaced cell times the orientation of the cell in X, so the measure is
int q det(I + grad u) dX and a folded cell counts negatively).  The device computes the same per cell; this module serves
host-resident results, ``device=False`` and partitioned runs.
"""
import math

import numpy as np

from .postprocess import simplex_quadrature

KINDS = ("mass", "sharp", "smooth")


def _kind(k):
    return KINDS[k] if isinstance(k, (int, np.integer)) else str(k)


def normalise_queries(queries):
    """[(kind name, level, smooth)] from (kind[, level[, smooth]]) tuples with names or numbers."""
    out = []
    for q in queries:
        q = tuple(q) if isinstance(q, (tuple, list)) else (q,)
        kind = _kind(q[0])
        if kind not in KINDS:
            raise ValueError("unknown observable kind %r" % (q[0],))
        level = float(q[1]) if len(q) > 1 else 0.0
        smooth = float(q[2]) if len(q) > 2 else 1.0
        if kind == "smooth" and not smooth > 0.0:
            raise ValueError("smooth must be positive")
        out.append((kind, level, smooth))
    return out


def signed_volumes(P):
    """[M, d+1, d] vertex positions -> signed volumes det(p_1 - p_0, ..) / d!"""
    d = P.shape[2]
    return np.linalg.det(P[:, 1:, :] - P[:, :1, :]) / math.factorial(d)


def _det3(a, b, c):
    return (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0])
            + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]))


def _sharp(cv, level):
    """b [M, d+2] of q = [c_h >= level]"""
    M, nv = cv.shape
    b = np.zeros((M, nv + 1))
    inside = cv >= level
    n_in = inside.sum(axis=1)
    full = n_in == nv
    b[full, 0] = 1.0
    b[full, 1:] = 1.0 / nv
    for corner_in in (True, False):
        rows = np.nonzero(n_in == (1 if corner_in else nv - 1))[0]
        if len(rows) == 0:
            continue
        c = cv[rows]
        v = np.argmax(inside[rows] if corner_in else ~inside[rows], axis=1)
        r = np.arange(len(rows))
        cvv = c[r, v][:, None]
        with np.errstate(divide='ignore', invalid='ignore'):
            s = (cvv - level) / (cvv - c) if corner_in else 1.0 - (c - level) / (c - cvv)
        s[r, v] = 1.0
        frac = s.prod(axis=1)
        rest = (1.0 - s).sum(axis=1)                     # (the entry of v adds 0)
        m = s / nv
        m[r, v] = (1.0 + rest) / nv
        if corner_in:
            b[rows, 0] = frac
            b[rows, 1:] = frac[:, None] * m
        else:
            b[rows, 0] = 1.0 - frac
            b[rows, 1:] = 1.0 / nv - frac[:, None] * m
    if nv == 4:
        rows = np.nonzero(n_in == 2)[0]
        if len(rows):
            c = cv[rows]
            order = np.argsort(~inside[rows], axis=1, kind='stable')      # in-vertices first, each group in vertex order
            r = np.arange(len(rows))
            A = np.zeros((len(rows), 3, 4))
            B = np.zeros((len(rows), 3, 4))
            ia, ib = order[:, 0], order[:, 1]
            A[r, 0, ia] = 1.0
            B[r, 0, ib] = 1.0
            for k in range(2):
                o = order[:, 2 + k]
                ta = (c[r, ia] - level) / (c[r, ia] - c[r, o])
                tb = (c[r, ib] - level) / (c[r, ib] - c[r, o])
                A[r, 1 + k, ia] = 1.0 - ta
                A[r, 1 + k, o] = ta
                B[r, 1 + k, ib] = 1.0 - tb
                B[r, 1 + k, o] = tb
            acc = np.zeros((len(rows), 5))
            for tet in ((A[:, 0], A[:, 1], A[:, 2], B[:, 0]), (A[:, 1], A[:, 2], B[:, 0], B[:, 1]),
                        (A[:, 2], B[:, 0], B[:, 1], B[:, 2])):
                q0 = tet[0]
                f = np.abs(_det3(*(t[:, 1:] - q0[:, 1:] for t in tet[1:])))
                acc[:, 0] += f
                acc[:, 1:] += f[:, None] * (0.25 * (tet[0] + tet[1] + tet[2] + tet[3]))
            b[rows] = acc
    return b


def cell_terms(cv, kind, level=0.0, smooth=1.0):
    """b [M, d+2]: b[:, 0] = int_T q / |T|, b[:, 1 + k] = int_T lambda_k q / |T| for the vertex values cv [M, d+1]"""
    cv = np.asarray(cv, dtype=np.float64)
    M, nv = cv.shape
    kind = _kind(kind)
    if kind == "mass":
        s = cv.sum(axis=1)
        return np.concatenate([(s / nv)[:, None], (s[:, None] + cv) / (nv * (nv + 1))], axis=1)
    if kind == "sharp":
        return _sharp(cv, level)
    if kind == "smooth":
        lam, w = simplex_quadrature(nv - 1, 4)
        f = w[None, :] * (0.5 * (np.tanh((cv @ lam.T - level) / smooth) + 1.0))          # [M, Q]
        return np.concatenate([f.sum(axis=1)[:, None], f @ lam], axis=1)
    raise ValueError("unknown observable kind %r" % (kind,))


def observe(points, cells, labels, c, queries, n_labels=None, u=None, scale=1.0):
    """
    [n_q, n_labels, 1 + d] = (V, M_0 ..) of every query and label for the nodal concentration c [N]; ``u`` [N, d] gives the
    deformed configuration x = X + scale u.  ``queries``: (kind[, level[, smooth]]) tuples.
    """
    X = np.asarray(points, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    d = X.shape[1]
    n_labels = int(labels.max()) + 1 if n_labels is None else int(n_labels)
    qs = normalise_queries(queries)
    PX = X[cells]
    TX = signed_volumes(PX)
    if u is None:
        P, T = PX, np.abs(TX)
    else:
        P = PX + float(scale) * np.asarray(u, dtype=np.float64).reshape(len(X), d)[cells]
        T = signed_volumes(P) * np.where(TX < 0.0, -1.0, 1.0)
    cv = np.asarray(c, dtype=np.float64)[cells]
    out = np.zeros((len(qs), n_labels, 1 + d))
    for k, (kind, level, smooth) in enumerate(qs):
        b = cell_terms(cv, kind, level, smooth)
        vals = np.concatenate([(T * b[:, 0])[:, None], T[:, None] * np.einsum('mk,mka->ma', b[:, 1:], P)], axis=1)
        for a in range(1 + d):
            out[k, :, a] = np.bincount(labels, weights=vals[:, a], minlength=n_labels)[:n_labels]
    return out


def totals_and_com(table):
    """[..., n_labels, 1 + d] -> (per-label and whole-domain measures [..., 1 + n_labels], centres of mass [..., 1 + n_labels, d]):
    entry 0 is the whole domain, the sum over the labels in label order; the centre of mass is NaN where the measure is not > 0
    (compute_com)."""
    table = np.asarray(table, dtype=np.float64)
    whole = np.zeros(table.shape[:-2] + (table.shape[-1],))
    for l in range(table.shape[-2]):
        whole = whole + table[..., l, :]
    full = np.concatenate([whole[..., None, :], table], axis=-2)
    V = full[..., 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        com = np.where((V > 0.0)[..., None], full[..., 1:] / V[..., None], np.nan)
    return V, com
