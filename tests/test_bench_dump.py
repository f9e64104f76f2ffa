"""bench.py --dump-outputs: the arrays written for the last timed step, assembled from a stand-in handle (no GPU).
Full arrays when they fit the budget, a fixed seeded node sample when they do not, and the same files from one rank
as from several."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Handle:
    def __init__(self, c, u):
        self.c, self.u = c, u

    def get_state(self, want_u=True):
        return self.c.copy(), (self.u.copy() if want_u else None)


class _Part:
    def __init__(self, global_ids, n_own):
        self.global_ids, self.n_own = global_ids, n_own


class _Dist:
    """all_gather_object of one rank, the other ranks' objects given."""
    def __init__(self, rank, others):
        self.rank, self.others, self.sent = rank, others, None

    def all_gather_object(self, out, obj):
        self.sent = obj
        for r in range(len(out)):
            out[r] = obj if r == self.rank else self.others.get(r)


def _state(n, dim, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(n * dim)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _dump_ranks(b, out_dir, c, u, dim, coupled, world):
    """Split the nodes over `world` ranks (owned nodes permuted, a few ghosts after them) and dump as the ranks would."""
    n = len(c)
    rng = np.random.default_rng(7)
    owners = np.array_split(rng.permutation(n), world)
    parts, sent = [], {}
    for r, own in enumerate(owners):
        ghosts = rng.choice(np.setdiff1d(np.arange(n), own), 5, replace=False)
        gid = np.concatenate([own, ghosts]).astype(np.int64)
        parts.append((gid, len(own)))
    for r in range(1, world):
        gid, n_own = parts[r]
        lu = u.reshape(n, dim)[gid].ravel() if coupled else None
        d = _Dist(r, {})
        b.dump_outputs(out_dir, _Handle(c[gid], lu), coupled, dim, n, _Part(gid, n_own), d, r, world)
        sent[r] = d.sent
    gid, n_own = parts[0]
    lu = u.reshape(n, dim)[gid].ravel() if coupled else None
    b.dump_outputs(out_dir, _Handle(c[gid], lu), coupled, dim, n, _Part(gid, n_own), _Dist(0, sent), 0, world)


def test_dump_full_arrays_coupled(tmp_path):
    b = _bench()
    n, dim = 300, 3
    c, u = _state(n, dim)
    b.dump_outputs(str(tmp_path), _Handle(c, u), True, dim, n, None, None, 0, 1)
    got = _load(str(tmp_path))
    assert sorted(got) == ["concentration", "displacement"]
    assert got["concentration"].dtype == np.float64 and np.array_equal(got["concentration"], c)
    assert got["displacement"].shape == (n, dim) and np.array_equal(got["displacement"], u.reshape(n, dim))


def test_dump_concentration_only_when_not_coupled(tmp_path):
    b = _bench()
    c, _ = _state(100, 3)
    b.dump_outputs(str(tmp_path), _Handle(c, None), False, 3, 100, None, None, 0, 1)
    got = _load(str(tmp_path))
    assert sorted(got) == ["concentration"] and np.array_equal(got["concentration"], c)


def test_dump_fixed_sample_above_the_budget(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 4096 + 16 * 1000)
    n = 5000
    c, _ = _state(n, 3)
    for sub in ("a", "b"):
        b.dump_outputs(str(tmp_path / sub), _Handle(c, None), False, 3, n, None, None, 0, 1)
    a, a2 = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["concentration", "sample_node_ids"]
    ids = a["sample_node_ids"]
    assert len(ids) == 1000 and np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < n
    assert np.array_equal(ids, np.round(ids))
    assert np.array_equal(a["concentration"], c[ids.astype(np.int64)])
    for k in a:                                                      # the same sample every run
        assert np.array_equal(a[k], a2[k])
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= b.DUMP_BUDGET_BYTES


def test_dump_partitioned_equals_single_rank(tmp_path, monkeypatch):
    b = _bench()
    n, dim = 2000, 3
    c, u = _state(n, dim)
    b.dump_outputs(str(tmp_path / "one"), _Handle(c, u), True, dim, n, None, None, 0, 1)
    _dump_ranks(b, str(tmp_path / "four"), c, u, dim, True, 4)
    one, four = _load(str(tmp_path / "one")), _load(str(tmp_path / "four"))
    assert sorted(one) == sorted(four) == ["concentration", "displacement"]
    for k in one:
        assert np.array_equal(one[k], four[k])
    # and with the sample
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 4096 + 8 * 5 * 300)
    b.dump_outputs(str(tmp_path / "one_s"), _Handle(c, u), True, dim, n, None, None, 0, 1)
    _dump_ranks(b, str(tmp_path / "four_s"), c, u, dim, True, 4)
    one, four = _load(str(tmp_path / "one_s")), _load(str(tmp_path / "four_s"))
    assert sorted(one) == sorted(four) == ["concentration", "displacement", "sample_node_ids"]
    assert len(one["sample_node_ids"]) == 300
    for k in one:
        assert np.array_equal(one[k], four[k])


def _api_run(name, n, warmup, steps):
    """The same workload through the C-ABI handle, as bench.py sets it up: warm-up + timed steps back to back."""
    from glimslib_amd import workloads
    from glimslib_amd._backend import Handle
    w = workloads.by_name(name, n)
    h = Handle(w.mesh.points, w.mesh.cells, w.cell_label, device=0)
    t = w.tables
    h.set_materials(t['D'], t['rho'], t['gamma'], t['E'], t['nu'])
    h.set_options(dt=w.dt, flags=h.options.flags, time_kernels=1)
    coupled = bool(w.mechanics)
    dim = w.mesh.points.shape[1]
    if coupled:
        nodes = np.asarray(w.dirichlet_nodes, dtype=np.int64)
        dofs = (nodes[:, None] * dim + np.arange(dim)).ravel()
        h.set_dirichlet_u(dofs, np.zeros(len(dofs)))
    h.setup(with_mechanics=coupled)
    h.set_state(w.c0)
    if coupled:
        h.solve_mechanics()
    for _ in range(warmup + steps):
        assert h.step(1) == 0
        if coupled:
            assert h.solve_mechanics() == 0
    c, u = h.get_state(want_u=coupled)
    h.close()
    return c, (u.reshape(-1, dim) if coupled else None)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("c3", 24), ("c5", 12)])
def test_bench_dump_is_the_state_after_warmup_plus_steps(tmp_path, name, n):
    """`bench.py --steps K --warmup W --dump-outputs DIR` runs exactly K timed steps and writes the state a caller of the
    C-ABI would hold after W + K steps of the same workload."""
    import json
    import subprocess
    import sys
    out_dir = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", name, "--size", str(n),
                        "--steps", "3", "--warmup", "2", "--no-cpu-baseline", "--no-alt", "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert line["steps"] == 3 and line["steps_completed"] == 3 and line["solver_status"] == 0
    got = _load(out_dir)
    c, u = _api_run(name, n, 2, 3)
    assert sorted(got) == (["concentration", "displacement"] if u is not None else ["concentration"])
    assert got["concentration"].dtype == np.float64
    assert np.linalg.norm(got["concentration"] - c) <= 1e-12 * np.linalg.norm(c)
    if u is not None:
        assert np.linalg.norm(got["displacement"] - u) <= 1e-12 * np.linalg.norm(u)
