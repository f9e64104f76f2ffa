"""
Hessian-vector products on partitioned handles, without a GPU: the ABI surface of glims_adjoint_hessian_spmd, the Python entry
points, and a numpy statement of the counting rule of the per-label Hessian sums ("Second order",
"Partitioned handles"): a cell is counted by the smallest rank that owns one of its vertices, the ranks' sums are added in
rank order.
"""
import inspect

import numpy as np
import pytest

from adjoint_common import Problem
from adjoint_hessian_common import _Cells


def test_spmd_symbol_is_exported_with_the_signature_of_the_single_gpu_call():
    from glimslib_amd import _backend
    lib = _backend.load_library()
    assert hasattr(lib, "glims_adjoint_hessian_spmd")
    assert "glims_adjoint_hessian_spmd" in _backend.SIGNATURES
    assert _backend.SIGNATURES["glims_adjoint_hessian_spmd"] == _backend.SIGNATURES["glims_adjoint_hessian"]


def test_python_entry_points():
    from glimslib_amd import _backend
    from glimslib_amd.parallel import DistributedHandle
    sig = inspect.signature(_backend.Handle.adjoint_hessian)
    assert list(sig.parameters) == ["self", "terms", "directions", "n_labels", "collective"]
    assert sig.parameters["collective"].default is False
    assert list(inspect.signature(DistributedHandle.adjoint_hessian).parameters) == ["self", "terms", "directions", "n_labels"]
    assert "NotImplementedError" not in inspect.getsource(DistributedHandle.adjoint_hessian)


def _counted(part):
    """The device rule (k_cell_counted) in the rank's local numbering: owner of a local node = the rank for the owned ones,
    the peer of its group for the ghosts (grouped by peer in peer_rank order)."""
    own = np.full(len(part.global_ids), part.rank, dtype=np.int64)
    own[part.n_own:] = np.repeat(np.asarray(part.peer_rank, dtype=np.int64), np.asarray(part.recv_count, dtype=np.int64))
    return own[np.asarray(part.cells, dtype=np.int64)].min(axis=1) == part.rank


class _Local:
    def __init__(self, prob, part):
        self.points, self.cells, self.dim = part.points, part.cells, prob.dim


def _label_sums(geo, lab, L, c, lam, dc, nu):
    """[L][2]: the D and rho Hessian sums of one step (k_hsens) from adjoint_hessian_common's cell integrals"""
    q0 = geo.gg(nu, c) + geo.gg(lam, dc)
    q1 = geo.xyz(nu, c, c) - geo.xy(nu, c) + 2.0 * geo.xyz(lam, c, dc) - geo.xy(lam, dc)
    return np.stack([np.bincount(lab, q0, minlength=L), np.bincount(lab, q1, minlength=L)], axis=1)


@pytest.mark.parametrize("dim,n", [(2, 12), (3, 5)])
@pytest.mark.parametrize("world", [2, 3, 4, 5])
def test_every_cell_is_counted_once_and_the_rank_sums_add_up(dim, n, world):
    from glimslib_amd.partition import partition_mesh
    prob = Problem(dim, n)
    rng = np.random.default_rng(100 * dim + world)
    nn, L = len(prob.points), prob.n_labels
    c, lam, dc, nu = (rng.uniform(-1, 1, nn) for _ in range(4))
    ref = _label_sums(_Cells(prob), prob.labels, L, c, lam, dc, nu)
    times = np.zeros(len(prob.cells), dtype=np.int64)
    total = np.zeros((L, 2))
    for rank in range(world):   # rank order, as the host adds the gathered rows
        part = partition_mesh(prob.points, prob.cells, world, rank)
        cnt = _counted(part)
        times[np.asarray(part.cell_ids)[cnt]] += 1
        geo = _Cells(_Local(prob, part))
        gid = part.global_ids
        lab = np.where(cnt, prob.labels[part.cell_ids], L)   # the cells of other ranks: a bin that is dropped
        total += _label_sums(geo, lab, L + 1, c[gid], lam[gid], dc[gid], nu[gid])[:L]
    assert np.array_equal(times, np.ones(len(prob.cells), dtype=np.int64))
    assert np.abs(total - ref).max() <= 1e-13 * np.abs(ref).max()
