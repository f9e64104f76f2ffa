"""Resolved samplers of partitioned runs without a GPU: the numpy rule of tests/sampler_partition_common.py (keep the global
winner, count on the smallest keeping rank, P^T by owned rows) against the single-mesh locate / apply_t, and the C-ABI surface
of glims_sampler_resolve."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sampler_common as sc
import sampler_partition_common as spc
from adjoint_common import Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[(2, 12, (15, 14)), (3, 6, (9, 8, 7))], ids=["2d-12x12", "3d-6x6x6"])
def lattice(request):
    dim, n, size = request.param
    prob = Problem(dim, n)
    x = spc.vertex_and_overhanging_points(prob.points, size)
    cell, w, margin, n_acc = sc.locate(prob.points, prob.cells, x)
    sc.assert_decisive(margin)
    nv = len(prob.points)
    # a tie at every vertex but a few corners of the domain; the grid overhangs
    assert (n_acc[:nv] >= 1).all() and (n_acc[:nv] >= 2).sum() >= nv - 2 ** dim
    assert (cell[nv:] < 0).any() and (cell[nv:] >= 0).any()
    return prob, x, cell, w


@pytest.mark.parametrize("world", [2, 3, 4, 5])
def test_numpy_rule_equals_the_single_mesh_sampler(lattice, world):
    prob, x, cell, w = lattice
    n_nodes = len(prob.points)
    parts, loc = spc.locate_on_parts(prob.points, prob.cells, world, x)
    win, keep, counted = spc.resolve(parts, loc)
    found = cell >= 0
    # every found point is counted on exactly one rank, the others on none
    assert np.array_equal(counted.sum(axis=0), found.astype(np.int64))
    assert (counted <= keep).all()
    # the global winner is the single-mesh winner, and the kept winner is it on every keeping rank
    assert np.array_equal(win, cell.astype(np.int64))
    shared = 0
    for p, (lc, lw), kr in zip(parts, loc, keep):
        assert np.array_equal(np.asarray(p.cell_ids)[lc[kr]], cell[kr])
        # (the local cell has the global cell's vertices in the same order: the same weights up to the rounding of the solve)
        assert np.abs(lw[kr] - w[kr]).max() <= 1e-13
        shared += int(kr.sum())
    assert shared > int(found.sum())              # some winners are held by several ranks: cells on the cut
    # without the rule a rank's own winner differs from the global one somewhere (the ties on the cut)
    assert any(((lc >= 0) & ~kr).any() for (lc, _), kr in zip(loc, keep))
    rng = np.random.default_rng(3)
    for k in (1, 3):
        r = rng.standard_normal((len(x), k)) if k > 1 else rng.standard_normal(len(x))
        ref = sc.apply_t(prob.cells, cell, w, r, n_nodes)
        got = spc.apply_t_by_owned_rows(parts, loc, keep, r, n_nodes)
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    f = rng.uniform(0, 1, n_nodes)
    t = rng.uniform(0, 1, len(x))
    t[rng.random(len(x)) < 0.1] = np.nan
    q = rng.uniform(0.5, 2.0, len(x))
    v = sc.apply(prob.cells, cell, w, f, fill=0.0)
    ok = found & ~np.isnan(t)
    J = float(np.sum(q[ok] * (v[ok] - t[ok]) ** 2))
    sums = spc.counted_sums(parts, loc, counted, f, t, q)
    assert abs(sum(sums) - J) <= 1e-13 * J


def test_library_exports_resolve_and_the_image_misfit_struct_keeps_its_layout():
    from glimslib_amd import _backend
    src = open(os.path.join(ROOT, "include", "glims_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(glims_[a-z_0-9]+)\s*\(", code))
    lib = _backend.load_library()
    assert lib.glims_abi_version() == 6
    for name in ("glims_sampler_resolve", "glims_sampler_get_counted"):
        assert name in declared, "%s is not declared in glims_hip.h" % name
        assert hasattr(lib, name), "libglimship.so does not export %s" % name
        assert name in _backend.SIGNATURES
    assert _backend.SIGNATURES["glims_sampler_resolve"][1][1:] == [C.c_int64, C.POINTER(C.c_int64)]
    body = re.search(r"typedef struct glims_image_misfit \{(.*?)\} glims_image_misfit;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*?\s*([a-z_]+)\s*[;,]", body) == ["step", "sampler", "kind", "level", "smooth", "weight", "target",
                                                           "pweight"]
    assert C.sizeof(_backend.ImageMisfit) == 64
    assert [getattr(_backend.ImageMisfit, f).offset for f, _ in _backend.ImageMisfit._fields_] == [0, 8, 16, 24, 32, 40, 48, 56]
