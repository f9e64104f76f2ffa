"""
SPMD support for the simulation classes: one process per GPU (``torchrun`` / ``torch.distributed``), the mesh
partitioned by ``glimslib_amd.partition``, halos and reductions inside libglimship over RCCL.

The reference's counterpart is "run the same script under ``mpirun -np N``" (README.md:142-183): DOLFIN distributes
the mesh and PETSc does the communication.  Here every rank holds the full (host) mesh, owns a Morton range of the
nodes on its GPU, and ``sync_solution`` all-gathers the owned values so that ``sim.solution`` is the global field
on every rank.

``HostStagedTransport`` is an alternative to RCCL that plugs into ``glims_set_transport``: device buffers are
staged through the host and exchanged with the process group's CPU backend (gloo).  It exists for boxes where RCCL
cannot be used -- e.g. several ranks sharing one GPU, which RCCL rejects ("Duplicate GPU detected") -- and is what
the 2-rank single-GPU tests use.  Select it with ``GLIMS_TRANSPORT=gloo``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _backend
from .partition import partition_mesh


def dist_info():
    """(dist module or None, rank, world).  torch is only imported when a launcher environment is present or the
    caller has imported it already (a single-process run should not pay ~1 s for it)."""
    import sys
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 and "torch" not in sys.modules:
        return None, 0, 1
    try:
        import torch.distributed as dist
    except Exception:   # pragma: no cover
        return None, 0, 1
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def broadcast_unique_id(dist, rank):
    """RCCL unique id of rank 0 to every rank, as a CPU uint8 tensor (gloo side of a 'cpu:gloo,cuda:nccl' group)."""
    import torch
    buf = torch.zeros(_backend.GLIMS_UNIQUE_ID_BYTES, dtype=torch.uint8)
    if rank == 0:
        buf = torch.frombuffer(bytearray(_backend.Handle.comm_unique_id()), dtype=torch.uint8).clone()
    try:
        dist.broadcast(buf, src=0)
    except Exception:
        # process group without a CPU backend (plain 'nccl'): go through the GPU
        dev = torch.device("cuda", torch.cuda.current_device())
        gbuf = buf.to(dev)
        dist.broadcast(gbuf, src=0)
        buf = gbuf.cpu()
    return bytes(buf.numpy().tobytes())


def setup_node_mailbox(h, dist, rank):
    """
    Switches the scalar all-reduces of `h` (a _backend.Handle with rank / world already set) to the node-local
    shared-memory mailbox (glims_comm_mailbox), checks it collectively and falls back to RCCL / the transport callback
    on every rank if any rank's check fails.  GLIMS_ALLREDUCE=rccl skips it.  Returns True when the mailbox is in use.
    """
    import torch
    if os.environ.get("GLIMS_ALLREDUCE", "mailbox").lower() in ("rccl", "nccl", "callback"):
        return False
    name = ["/glims_%d_%s" % (os.getpid(), os.urandom(4).hex())] if rank == 0 else [None]
    dist.broadcast_object_list(name, src=0)
    ok = 1
    try:
        h.comm_mailbox(name[0])
    except Exception as e:   # noqa: BLE001
        print("glimslib_amd: node mailbox unavailable on rank %d (%s)" % (rank, e), flush=True)
        ok = 0
    flag = torch.tensor([ok], dtype=torch.int32)
    _all_reduce_cpu(dist, flag, dist.ReduceOp.MIN)
    if int(flag.item()) == 1:
        try:
            h.comm_mailbox_selftest()
        except Exception as e:   # noqa: BLE001
            print("glimslib_amd: node mailbox self-test failed on rank %d (%s)" % (rank, e), flush=True)
            ok = 0
        flag = torch.tensor([ok], dtype=torch.int32)
        _all_reduce_cpu(dist, flag, dist.ReduceOp.MIN)
    if rank == 0:
        try:
            os.unlink("/dev/shm" + name[0])   # every rank has mapped it (or given up) by now
        except OSError:
            pass
    if int(flag.item()) != 1:
        h.comm_mailbox(None)
        return False
    return True


def _all_reduce_cpu(dist, t, op):
    try:
        dist.all_reduce(t, op=op)
    except Exception:   # process group without a CPU backend
        import torch
        g = t.to(torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(g, op=op)
        t.copy_(g.cpu())


class HostStagedTransport:
    """glims_halo_fn / glims_allreduce_fn implemented with hipMemcpy staging + torch.distributed CPU collectives."""

    def __init__(self, dist, group=None):
        import torch
        self.torch = torch
        self.dist = dist
        self.group = group
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
        self.hip = hip
        self.halo_cb = _backend.HALO_FN(self._halo)
        self.allreduce_cb = _backend.ALLREDUCE_FN(self._allreduce)
        # GLIMS_TRANSPORT_TRACE=<prefix>: every collective this rank enters, one line each, in <prefix><rank>.txt -- ranks whose
        # call sequences differ show where a partitioned run went out of step
        pre = os.environ.get("GLIMS_TRANSPORT_TRACE")
        self._trace = open("%s%d.txt" % (pre, dist.get_rank()), "w") if pre else None
        self._n = 0

    def _note(self, what):
        if self._trace:
            self._n += 1
            self._trace.write("%d %s\n" % (self._n, what))
            self._trace.flush()

    def _d2h(self, ptr, n):
        a = np.empty(n)
        if self.hip.hipMemcpy(a.ctypes.data, ptr, n * 8, 2) != 0:
            raise RuntimeError("hipMemcpy D2H failed")
        return a

    def _h2d(self, ptr, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if self.hip.hipMemcpy(ptr, a.ctypes.data, a.size * 8, 1) != 0:
            raise RuntimeError("hipMemcpy H2D failed")

    def _halo(self, user, sendbuf, send_ptr, ghosts, recv_ptr, n_peers, peers, bs, stream):
        try:
            self._note("halo bs=%d peers=%s" % (bs, [int(peers[p]) for p in range(n_peers)]))
            self.hip.hipStreamSynchronize(stream)
            reqs, rbufs = [], []
            for p in range(n_peers):
                lo, hi = send_ptr[p] * bs, send_ptr[p + 1] * bs
                if hi > lo:      # (an empty direction is skipped on both sides: the two ranks derive the same counts)
                    sb = self.torch.from_numpy(self._d2h(sendbuf + lo * 8, hi - lo))
                    reqs.append(self.dist.isend(sb, int(peers[p]), group=self.group))
                nr = int((recv_ptr[p + 1] - recv_ptr[p]) * bs)
                if nr > 0:
                    rb = self.torch.empty(nr, dtype=self.torch.float64)
                    reqs.append(self.dist.irecv(rb, int(peers[p]), group=self.group))
                    rbufs.append((recv_ptr[p] * bs, rb))
            for r in reqs:
                r.wait()
            for off, rb in rbufs:
                self._h2d(ghosts + off * 8, rb.numpy())
            return 0
        except Exception as e:   # noqa: BLE001 -- must not unwind through the C frame
            print("glimslib_amd: halo transport failed: %r" % (e,), flush=True)
            return 1

    def _allreduce(self, user, values, n, stream):
        try:
            self._note("allreduce n=%d" % n)
            self.hip.hipStreamSynchronize(stream)
            t = self.torch.from_numpy(self._d2h(values, n))
            self.dist.all_reduce(t, group=self.group)
            self._h2d(values, t.numpy())
            return 0
        except Exception as e:   # noqa: BLE001
            print("glimslib_amd: allreduce transport failed: %r" % (e,), flush=True)
            return 1


class ThreadGroup:
    """Meeting point of ThreadedTransport's ranks (one process, one thread per rank)."""

    def __init__(self, world):
        import queue
        import threading
        self.world = world
        self.barrier = threading.Barrier(world)
        self.pipes = {(a, b): queue.Queue() for a in range(world) for b in range(world) if a != b}
        self.values = [None] * world


class ThreadedTransport:
    """glims_halo_fn / glims_allreduce_fn for ranks that are THREADS of one process sharing one GPU -- a rehearsal transport:
    the GPU boxes allow a handful of processes on a card, so rank counts like 8 cannot be rehearsed with one process per rank
    (tests/test_gpu_multirank.py, tools/rehearse_partition.py).  Everything else is the product path: each rank its own handle
    and streams, its own sub-mesh, the library's halo packing, slice split and reduction points.  Messages travel through
    FIFO queues per ordered rank pair (both sides derive the same sequence of exchanges), all-reduces through a barrier and
    a sum in rank order."""

    def __init__(self, group, rank):
        self.g, self.rank = group, rank
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
        self.hip = hip
        self.halo_cb = _backend.HALO_FN(self._halo)
        self.allreduce_cb = _backend.ALLREDUCE_FN(self._allreduce)
        self.failed = None

    def _d2h(self, ptr, n):
        a = np.empty(n)
        if self.hip.hipMemcpy(a.ctypes.data, ptr, n * 8, 2) != 0:
            raise RuntimeError("hipMemcpy D2H failed")
        return a

    def _h2d(self, ptr, a):
        if self.hip.hipMemcpy(ptr, a.ctypes.data, a.size * 8, 1) != 0:
            raise RuntimeError("hipMemcpy H2D failed")

    def _halo(self, user, sendbuf, send_ptr, ghosts, recv_ptr, n_peers, peers, bs, stream):
        try:
            self.hip.hipStreamSynchronize(stream)
            for p in range(n_peers):
                lo, hi = send_ptr[p] * bs, send_ptr[p + 1] * bs
                if hi > lo:
                    self.g.pipes[(self.rank, int(peers[p]))].put(self._d2h(sendbuf + lo * 8, hi - lo))
            for p in range(n_peers):
                nr = int((recv_ptr[p + 1] - recv_ptr[p]) * bs)
                if nr > 0:
                    a = self.g.pipes[(int(peers[p]), self.rank)].get(timeout=120)
                    assert a.size == nr, (a.size, nr)
                    self._h2d(ghosts + recv_ptr[p] * bs * 8, a)
            return 0
        except Exception as e:   # noqa: BLE001 -- must not unwind through the C frame
            self.failed = e
            print("glimslib_amd: threaded halo transport failed on rank %d: %r" % (self.rank, e), flush=True)
            return 1

    def _allreduce(self, user, values, n, stream):
        try:
            self.hip.hipStreamSynchronize(stream)
            self.g.values[self.rank] = self._d2h(values, n)
            self.g.barrier.wait(timeout=120)
            t = np.zeros(n)
            for r in range(self.g.world):       # rank order: the same bits on every rank
                t += self.g.values[r]
            self.g.barrier.wait(timeout=120)    # nobody overwrites its slot before everybody has read it
            self._h2d(values, t)
            return 0
        except Exception as e:   # noqa: BLE001
            self.failed = e
            print("glimslib_amd: threaded allreduce transport failed on rank %d: %r" % (self.rank, e), flush=True)
            return 1


def run_threaded_ranks(world, fn):
    """Runs fn(rank, ThreadedTransport) on `world` threads and returns their results in rank order (exceptions re-raised)."""
    import threading
    group = ThreadGroup(world)
    res, err = [None] * world, [None] * world

    def body(r):
        try:
            res[r] = fn(r, ThreadedTransport(group, r))
        except BaseException as e:   # noqa: BLE001
            err[r] = e
            group.barrier.abort()

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in err:
        if e is not None:
            raise e
    return res


class DistributedHandle:
    """
    Rank-local ``_backend.Handle`` + the index maps between global (mesh) and local (owned | ghost) numbering.
    Presents the same methods the simulation classes use on a plain Handle, with *global* arrays at the interface.
    """

    def __init__(self, points, cells, cell_label, dist, rank, world, device):
        import torch
        self.dist, self.rank, self.world = dist, rank, world
        self.n_global = len(points)
        self.dim = np.asarray(points).shape[1]
        self.n_cells_global = len(cells)
        self.part = partition_mesh(points, cells, world, rank)
        p = self.part
        self.h = _backend.Handle(p.points, p.cells, np.asarray(cell_label)[p.cell_ids], n_own=p.n_own, device=device)
        self.cpu_group = None
        use_gloo = os.environ.get("GLIMS_TRANSPORT", "rccl").lower() == "gloo"
        if use_gloo:
            self._transport = HostStagedTransport(dist)
            self.h.set_transport(rank, world, self._transport.halo_cb, self._transport.allreduce_cb)
        else:
            self.h.comm_init(rank, world, broadcast_unique_id(dist, rank))
        self.h.set_halo(p.peer_rank, p.send_ptr, p.send_idx, p.recv_count)
        pts = np.asarray(points)
        self.h.set_mg_frame(pts.min(axis=0), pts.max(axis=0))   # every rank holds the whole host mesh: global box
        self.node_mailbox = setup_node_mailbox(self.h, dist, rank)
        self.g2l_owned = np.full(self.n_global, -1, dtype=np.int64)
        self.g2l_owned[p.global_ids[:p.n_own]] = np.arange(p.n_own)
        self.options = self.h.options

    # -- pass-through -----------------------------------------------------------------------------------------
    def set_materials(self, *a):
        self.h.set_materials(*a)

    def set_diffusion_tensor(self, T):
        """``Handle.set_diffusion_tensor`` with the field in the GLOBAL cell order (or one [d, d] matrix, or None): every rank
        keeps the tensors of its own cells.  Rank-local, no communication."""
        if T is None:
            self.h.set_diffusion_tensor(None)
            return
        T = _backend.pack_diffusion_tensor(T, self.n_cells_global, self.dim)
        self.h.set_diffusion_tensor(T[self.part.cell_ids])

    def diffusion_tensor_info(self):
        return self.h.diffusion_tensor_info()

    def set_diffusion_tensor_tangents(self, dT):
        """``Handle.set_diffusion_tensor_tangents`` with the fields in the GLOBAL cell order (or None): every rank keeps the
        tangents of its own cells.  Rank-local, no communication; every rank stores the same number of fields."""
        if dT is None:
            self.h.set_diffusion_tensor_tangents(None)
            return
        dT = _backend.pack_diffusion_tensor_tangents(dT, self.n_cells_global, self.dim)
        self.h.set_diffusion_tensor_tangents(dT[:, self.part.cell_ids])

    @property
    def n_tangents(self):
        return self.h.n_tangents

    def adjoint_tensor_gradient(self):
        """``Handle.adjoint_tensor_gradient``: gathered over the ranks in the last sweep, the same bits on every rank."""
        return self.h.adjoint_tensor_gradient()

    def set_options(self, **kw):
        self.h.set_options(**kw)

    def setup(self, with_mechanics=True):
        self.h.setup(with_mechanics)

    def step(self, n=1):
        return self.h.step(n)

    def solve_mechanics(self):
        return self.h.solve_mechanics()

    def stats(self):
        return self.h.stats()

    def reset_stats(self):
        self.h.reset_stats()

    def close(self):
        self.h.close()

    def project(self, rhs, rtol=1e-12):
        rhs = np.asarray(rhs, dtype=np.float64)
        loc = self.h.project(rhs[self.part.global_ids], rtol)
        n_own = self.part.n_own
        parts = [None] * self.world
        self.dist.all_gather_object(parts, (self.part.global_ids[:n_own], loc[:n_own]))
        out = np.empty_like(rhs)
        for gid, v in parts:
            out[gid] = v
        return out

    # -- discrete adjoint (collective: every rank calls adjoint_gradient with the same terms) ---------------------------
    @property
    def n_labels(self):
        return self.h.n_labels

    def adjoint_record(self, on=True):
        self.h.adjoint_record(on)

    def _local_terms(self, terms):
        """The term dicts with their nodal targets localised (GLOBAL node order in) and their image terms on the rank-local
        sampler."""
        loc = []
        for t in terms:
            if t["kind"] in ("obs_volume", "obs_com"):
                self._no_volume_terms()
            if t["kind"] == "img_u_l2":
                self._no_displacement_image_terms()
            if t["kind"] in _backend._IMAGE_KINDS:
                loc.append(self._image_term(t))
                continue
            t = dict(t)
            bs = self.dim if t["kind"] in ("u_l2", _backend.MISFIT_U_L2) else 1
            t["target"] = self._local(t["target"], bs).reshape(-1)
            loc.append(t)
        return loc

    def _gather_owned(self, v):
        """Rank-local node vectors [..., n_local] -> the GLOBAL order, from every rank's owned entries (as get_state)."""
        n_own = self.part.n_own
        parts = [None] * self.world
        self.dist.all_gather_object(parts, (self.part.global_ids[:n_own], np.ascontiguousarray(v[..., :n_own])))
        out = np.empty(v.shape[:-1] + (self.n_global,))
        for gid, a in parts:
            out[..., gid] = a
        return out

    def adjoint_hessian_full(self, terms, directions, n_labels=None):
        """Second order in E / nu (Handle.adjoint_hessian_full, glims_adjoint_hessian_full) runs on one GPU only: raised
        here, before any collective."""
        raise NotImplementedError("adjoint_hessian_full (second order in E / nu, elastic=True) is not available on "
                                  "partitioned runs")

    def adjoint_hessian(self, terms, directions, n_labels=None):
        """Handle.adjoint_hessian on the partitioned run (glims_adjoint_hessian_spmd, collective: every rank calls it with
        the same terms and directions).  Targets and 'c0' directions in GLOBAL node order, localised here; J and every
        per-label array come back bitwise the same on every rank; 'c0' and 'hv_c0' are all-gathered into the global order."""
        dirs = []
        for d in directions:
            d = dict(d)
            if d.get("c0") is not None:
                d["c0"] = self._local(np.broadcast_to(np.asarray(d["c0"], dtype=np.float64), (self.n_global,)))
            dirs.append(d)
        r = self.h.adjoint_hessian(self._local_terms(terms), dirs, n_labels=n_labels, collective=True)
        r["c0"] = self._gather_owned(r["c0"])
        r["hv_c0"] = self._gather_owned(r["hv_c0"])
        return r

    def adjoint_gradient(self, terms, n_labels=None, want_dc0=True, elastic=False):
        """Handle.adjoint_gradient on the partitioned run: targets in GLOBAL node order ([n_global] or [n_global, dim]),
        localised here; J and the per-label arrays come back bitwise the same on every rank, dJ/dc0 all-gathered into the
        global order (as get_state does).  elastic=True (on every rank alike) appends dJ/dE and dJ/dnu."""
        res = self.h.adjoint_gradient(self._local_terms(terms), n_labels=n_labels, want_dc0=want_dc0, elastic=elastic)
        J, dD, drho, dgamma, dc0 = res[:5]
        if want_dc0:
            n_own = self.part.n_own
            parts = [None] * self.world
            self.dist.all_gather_object(parts, (self.part.global_ids[:n_own], dc0[:n_own]))
            dc0 = np.empty(self.n_global)
            for gid, v in parts:
                dc0[gid] = v
        return (J, dD, drho, dgamma, dc0) + tuple(res[5:])

    def adjoint_stats(self):
        return self.h.adjoint_stats()

    # -- image-space misfit terms: the sampler is a DistributedSampler, target / pweight are in POINT order (the same on every
    #    rank, not localised); the rank-local handle stores them against the resolved rank-local sampler
    def _image_term(self, t):
        sm = t["sampler"]
        if not isinstance(sm, DistributedSampler) or sm.dh is not self:
            raise ValueError("image term: its sampler is not a DistributedSampler of this handle")
        # (the caller's target / pweight objects stay: their identity is what Handle._split_terms compares)
        return dict(t, sampler=sm.local)

    def set_image_terms(self, terms):
        """Handle.set_image_terms on every rank (an empty list clears them)."""
        self.h.set_image_terms([self._image_term(t) for t in terms])

    def image_term_info(self, k):
        """(rank-local sampler id, number of points, number of observed points summed over the ranks) of stored term k."""
        sid, n, n_obs = self.h.image_term_info(k)
        parts = [None] * self.world
        self.dist.all_gather_object(parts, int(n_obs))
        return sid, n, int(sum(parts))

    # -- displacement-image misfit terms: single-rank handles only (the library refuses them on a partitioned handle) --------
    @staticmethod
    def _no_displacement_image_terms():
        raise NotImplementedError("displacement image misfit terms (set_displacement_image_terms, kind 'img_u_l2') are not "
                                  "available on partitioned runs")

    def set_displacement_image_terms(self, terms):
        self._no_displacement_image_terms()

    def displacement_image_term_info(self, k):
        self._no_displacement_image_terms()

    # -- volume misfit terms: single-rank handles only (the library refuses them on a partitioned handle, as glims_observe) --
    @staticmethod
    def _no_volume_terms():
        raise NotImplementedError("volume and centre-of-mass misfit terms (set_observable_terms, kinds 'obs_volume' and "
                                  "'obs_com') are not available on partitioned runs")

    def set_observable_terms(self, terms):
        self._no_volume_terms()

    def observable_term_info(self, k):
        self._no_volume_terms()

    def observable_term_info2(self, k):
        self._no_volume_terms()

    def observable_term_info3(self, k):
        self._no_volume_terms()

    # -- samplers (collective: every rank passes the same points) --------------------------------------------------------
    def sampler_points(self, xyz, deformed_by=None, scale=1.0):
        self._no_deformed(deformed_by)
        return DistributedSampler(self, self.h.sampler_points(xyz))

    def sampler_grid(self, origin, spacing, size, deformed_by=None, scale=1.0):
        self._no_deformed(deformed_by)
        return DistributedSampler(self, self.h.sampler_grid(origin, spacing, size))

    @staticmethod
    def _no_deformed(deformed_by):
        if deformed_by is not None:
            raise NotImplementedError("deformed-configuration samplers are not available on partitioned runs (the points "
                                      "would have to be located in every rank's displaced cells); run on one GPU")

    # -- global <-> local -----------------------------------------------------------------------------------------
    def _local(self, v, bs=1):
        v = np.asarray(v, dtype=np.float64).reshape(self.n_global, bs) if bs > 1 else np.asarray(v, dtype=np.float64)
        return v[self.part.global_ids]

    def set_rd_load(self, f):
        self.h.set_rd_load(None if f is None else self._local(f))

    def set_mech_load(self, f):
        self.h.set_mech_load(None if f is None else self._local(f, self.dim).reshape(-1))

    def set_dirichlet_c(self, nodes, values):
        nodes = np.asarray(nodes, dtype=np.int64)
        loc = self.g2l_owned[nodes] if len(nodes) else nodes
        keep = loc >= 0
        self.h.set_dirichlet_c(loc[keep], np.asarray(values, dtype=np.float64)[keep] if len(nodes) else values)

    def set_dirichlet_u(self, dofs, values):
        dofs = np.asarray(dofs, dtype=np.int64)
        if len(dofs) == 0:
            self.h.set_dirichlet_u(dofs, values)
            return
        node, comp = dofs // self.dim, dofs % self.dim
        loc = self.g2l_owned[node]
        keep = loc >= 0
        self.h.set_dirichlet_u(loc[keep] * self.dim + comp[keep], np.asarray(values, dtype=np.float64)[keep])

    def set_state(self, c, u=None):
        self.h.set_state(self._local(c), None if u is None else self._local(u, self.dim).reshape(-1))

    def get_state(self, want_u=True):
        """All-gathers the owned values: every rank returns the global fields."""
        c, u = self.h.get_state(want_u=want_u)
        n_own = self.part.n_own
        mine = (self.part.global_ids[:n_own], c[:n_own], None if u is None else u.reshape(-1, self.dim)[:n_own])
        parts = [None] * self.world
        self.dist.all_gather_object(parts, mine)
        cg = np.empty(self.n_global)
        ug = np.empty((self.n_global, self.dim)) if want_u else None
        for gid, cc, uu in parts:
            cg[gid] = cc
            if want_u:
                ug[gid] = uu
        return cg, (ug.reshape(-1) if want_u else None)


class DistributedSampler:
    """
    ``_backend.Sampler`` of a partitioned run.  Every rank locates the (same) points in its own cells and translates its
    winners to global cell ids; per point the SMALLEST GLOBAL CELL ID over the ranks wins -- the cell a single-GPU sampler
    picks, because every cell is local to some rank and each rank has already taken the minimum over its own -- and among the
    ranks that hold that cell the smallest rank supplies the value.  Every rank returns the same bits.

    The rank-local sampler is then RESOLVED (``glims_sampler_resolve``): it keeps only the points whose local winner is the
    global winner and counts a point on the smallest rank that keeps it -- the supplier above.  That makes ``apply_t`` and the
    image-space misfit terms available; ``apply`` returns the bits it returned before.
    """

    def __init__(self, dh, local):
        self.dh, self.local = dh, local
        self.n_points, self.grid_size = local.n_points, local.grid_size
        lc = local.cells
        g = np.where(lc >= 0, dh.part.cell_ids[np.maximum(lc, 0)], -1).astype(np.int64)
        parts = [None] * dh.world
        dh.dist.all_gather_object(parts, g)
        big = np.iinfo(np.int64).max
        allg = np.stack([np.where(a >= 0, a, big) for a in parts])          # [world, n]
        win = allg.min(axis=0)
        self.cells = np.where(win < big, win, -1).astype(np.int64)           # global cell ids
        self.n_found = int((self.cells >= 0).sum())
        holds = (allg == win[None, :]) & (win < big)[None, :]
        self.supplier = np.where(self.cells >= 0, holds.argmax(axis=0), -1)  # smallest rank that holds the winner
        self._mine = np.flatnonzero(self.supplier == dh.rank)
        local.resolve(dh.part.cell_ids)

    def apply(self, field, snapshot=None, fill=np.nan):
        """As ``Sampler.apply``; a nodal array is given in the GLOBAL node order.  The fields' ghost values must be current
        (they are after step / solve_mechanics)."""
        dh = self.dh
        if snapshot is not None:
            raise ValueError("partitioned runs keep no device snapshots")
        if isinstance(field, str):
            loc = self.local.apply(field, fill=fill)
        else:
            a = np.asarray(field, dtype=np.float64)
            loc = self.local.apply(a[dh.part.global_ids], fill=fill)
        parts = [None] * dh.world
        dh.dist.all_gather_object(parts, (self._mine, loc[self._mine]))
        out = np.full(loc.shape, fill, dtype=np.float64)
        for idx, v in parts:
            out[idx] = v
        return out

    def apply_t(self, r):
        """P^T r: r [n_points] or [n_points, k] in point order, the same on every rank; the owned rows of every rank
        all-gathered into the GLOBAL node order (as ``get_state`` does).  Every rank returns the same array."""
        dh = self.dh
        g = self.local.apply_t(r)
        n_own = dh.part.n_own
        parts = [None] * dh.world
        dh.dist.all_gather_object(parts, (dh.part.global_ids[:n_own], g[:n_own]))
        out = np.zeros((dh.n_global,) + g.shape[1:])
        for gid, v in parts:
            out[gid] = v
        return out

    def close(self):
        self.local.close()
