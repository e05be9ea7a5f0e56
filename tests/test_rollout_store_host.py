"""Host side of the async-PPO rollout store, without a GPU: this package's PriorityStore (statistics taken by a torch function in
place of rlx_version_stats) driven side by side with the reference's class; the learner's drop / evict / ready / on-policy-ratio
logic against the reference's ``_drain_received_trajectories`` / ``_wait_for_rollout_store_ready``; the configuration keys; and
the argument validation of the two ABI entries."""

import ctypes
import queue
import random
from contextlib import contextmanager
from types import SimpleNamespace

import pytest
import torch

from helpers.sorted_list import SortedList as StandInSortedList
from helpers.sorted_list import sorted_list_class
from oracle import reference_loader
from rlinf_amd.data.embodied_types import Trajectory
from rlinf_amd.data.rollout_store import PriorityStore, VersionSummary

needs_reference = pytest.mark.skipif(not reference_loader.available(), reason="reference tree not present on this machine")

T, B, A, D = 4, 2, 8, 5
CELLS = T * B * A


def torch_summary(versions: torch.Tensor) -> VersionSummary:
    """What rlx_version_stats delivers, in torch (the reference's own expressions: buffer.py:1185-1189)."""
    flat = torch.round(versions.reshape(-1)).to(torch.int64)
    uniq, cnt = torch.unique(flat, return_counts=True)
    return VersionSummary(min=float(versions.min().item()), total=int(flat.sum()), n=flat.numel(),
                          counts=dict(zip(uniq.tolist(), cnt.tolist())))


def make_traj(versions: torch.Tensor, tag: int = 0) -> Trajectory:
    z = lambda *s, dt=torch.float32: torch.full(s, float(tag), dtype=dt) if dt != torch.bool else torch.zeros(s, dtype=dt)  # noqa: E731
    actions = z(T, B, A)
    return Trajectory(actions=actions, rewards=z(T, B, 1), terminations=z(T + 1, B, 1, dt=torch.bool),
                      truncations=z(T + 1, B, 1, dt=torch.bool), dones=z(T + 1, B, 1, dt=torch.bool), prev_logprobs=z(T, B, A),
                      prev_values=z(T + 1, B, 1), versions=versions.clone(),
                      forward_inputs={"states": z(T, B, D), "action": actions, "model_action": actions})


def random_versions(rng: random.Random, lo: int, used: set) -> torch.Tensor:
    """Integer-valued versions with minimum ``lo`` whose (min, sum) is new: two trajectories of equal minimum then differ in mean
    by at least 1 / CELLS."""
    for _ in range(1000):
        extra = [rng.choice((0, 0, 1, 2, 3)) for _ in range(CELLS)]
        extra[rng.randrange(CELLS)] = 0  # the minimum is attained
        if (lo, sum(extra)) not in used:
            used.add((lo, sum(extra)))
            v = torch.tensor([lo + e for e in extra], dtype=torch.float32)
            return v[torch.randperm(CELLS, generator=torch.Generator().manual_seed(rng.randrange(1 << 30)))].view(T, B, A)
    raise AssertionError("no unused (min, sum) left")


def reference_store_class():
    return reference_loader.load_class("rlinf/data/storage/replay/buffer.py", "PriorityStore", SortedList=sorted_list_class(),
                                       torch=torch)


def reference_priority(traj) -> tuple:
    return (float(traj.versions.min().item()), float(traj.versions.float().mean().item()))  # async_ppo_fsdp_worker.py:126-128


def test_sorted_list_stand_in():
    sl = StandInSortedList(key=lambda x: (x[0], x[1]))
    items = [((1.0, 1.0), 0, "a"), ((0.0, 2.0), 1, "b"), ((1.0, 1.0), 2, "c"), ((0.0, 1.0), 3, "d")]
    for it in items:
        sl.add(it)
    assert [x[2] for x in sl] == ["d", "b", "a", "c"] and len(sl) == 4 and sl[0][2] == "d"
    assert [x[2] for x in sl[-2:]] == ["a", "c"]
    sl.remove(items[0])
    assert sl.pop(0)[2] == "d" and [x[2] for x in sl] == ["b", "c"]


@needs_reference
@pytest.mark.parametrize("maxsize", [1, 2, 3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_priority_store_side_by_side_with_the_reference(maxsize, seed):
    rng = random.Random(1000 * maxsize + seed)
    ref, mine = reference_store_class()(maxsize), PriorityStore(maxsize, stats_fn=torch_summary, device="cpu")
    used, made, version = set(), [], 0
    calls = 0

    def compare():
        assert len(mine) == len(ref)
        assert mine._discarded_unused == ref._discarded_unused
        assert mine.get_metric() == ref.get_metric()

    while calls < 240:
        op = rng.choice(("add", "add", "add", "topn", "remove_below", "get_metric"))
        calls += 1
        if op == "add":
            if rng.random() < 0.3:
                version += 1
            traj = make_traj(random_versions(rng, max(0, version - rng.choice((0, 0, 1, 1, 2, 3))), used), tag=len(made))
            made.append(traj)
            p = reference_priority(traj)
            assert mine.add(None, traj) == ref.add(p, traj)
        elif op == "topn":
            n = rng.randrange(1, maxsize + 2)
            got, want = mine.topn(n), ref.topn(n)
            assert len(got) == len(want) and all(g.source is w for g, w in zip(got, want)), "order, by trajectory identity"
            for g in got:  # a stored trajectory is a snapshot of its source, not a view of it
                assert torch.equal(g.versions, g.source.versions) and g.versions.data_ptr() != g.source.versions.data_ptr()
                assert torch.equal(g.rewards, g.source.rewards) and torch.equal(g.forward_inputs["states"], g.source.forward_inputs["states"])
        elif op == "remove_below":
            thr = version - rng.choice((0, 1, 2, 3))
            mine.remove_below(thr), ref.remove_below(thr)
        compare()
        assert mine._shape is None or len(mine._free) + len(mine) == maxsize + 1, "every slot buffer is either stored or free"
    # the property of the generated inputs the comparison relies on: integer versions, and equal minima => means >= 1e-3 apart
    pri = [torch_summary(t.versions) for t in made]
    assert len(made) >= 60
    for t in made:
        assert torch.equal(t.versions, torch.round(t.versions))
    for i in range(len(pri)):
        for j in range(i):
            if pri[i].min == pri[j].min:
                assert abs(pri[i].mean - pri[j].mean) >= 1e-3
                assert (reference_priority(made[i]) < reference_priority(made[j])) == (pri[i].priority < pri[j].priority)


@needs_reference
def test_equal_priorities_evict_the_oldest_first_like_the_reference():
    """Constant integer versions: equal priorities are exactly equal in both stores."""
    ref, mine = reference_store_class()(3), PriorityStore(3, stats_fn=torch_summary, device="cpu")
    trajs = [make_traj(torch.full((T, B, A), float(v)), tag=i) for i, v in enumerate((2, 2, 1, 2, 2, 1, 3, 0, 2))]
    for i, t in enumerate(trajs):
        assert mine.add(None, t) == ref.add(reference_priority(t), t), i
        if i in (3, 6):
            assert all(g.source is w for g, w in zip(mine.topn(2), ref.topn(2)))
        assert len(mine) == len(ref) and mine.get_metric() == ref.get_metric()
    assert all(g.source is w for g, w in zip(mine.topn(3), ref.topn(3)))


def test_priority_store_rules_without_the_reference():
    """The documented rules, checked on their own: lexicographic (min, mean); highest first; a full store refuses a lower
    priority; the oldest of equal priorities goes first; discarded_unused counts what left without having been returned."""
    s = PriorityStore(2, stats_fn=torch_summary, device="cpu")
    const = lambda v, tag: make_traj(torch.full((T, B, A), float(v)), tag)  # noqa: E731
    a, b, c, d = const(1, 0), const(1, 1), const(0, 2), const(2, 3)
    mixed = torch.full((T, B, A), 1.0)
    mixed[0, 0, 0] = 3.0
    e = make_traj(mixed, 4)  # min 1, mean above 1: outranks a and b
    assert s.add(None, a) and s.add(None, b) and len(s) == 2
    assert not s.add(None, c) and s._discarded_unused == 1, "lower than the lowest entry of a full store"
    assert [x.source for x in s.topn(1)] == [b], "equal priorities: the newer one ranks higher"
    assert s.add(None, e) and [x.source for x in s.topn(2)] == [e, b], "a (oldest of the equal pair, never returned) was evicted"
    assert s._discarded_unused == 2
    assert s.add(None, d) and [x.source for x in s.topn(2)] == [d, e] and s._discarded_unused == 2, "b had been used"
    assert s.get_metric() == {1: {"ratio": (CELLS - 1) / (2 * CELLS)}, 2: {"ratio": 0.5}, 3: {"ratio": 1 / (2 * CELLS)},
                              "discarded_unused": 2}
    s.remove_below(2)
    assert [x.source for x in s.topn(5)] == [d] and s._discarded_unused == 2 and len(s._free) == 2
    s.remove_below(3)
    assert len(s) == 0 and s.get_metric() == {"discarded_unused": 2}
    wide = make_traj(torch.zeros(T, B, A))
    wide.forward_inputs = {k: torch.zeros(T, B + 1, v.shape[-1]) for k, v in wide.forward_inputs.items()}
    with pytest.raises(ValueError, match="same env count"):
        s.add(None, wide)


# ---- the learner's drop / evict / ready logic ------------------------------------------------------------------------------------
def _learner(store_size, threshold, ratio):
    from test_end_to_end import make_cfg
    from rlinf_amd.config import validate_cfg
    from rlinf_amd.scheduler import init_distributed
    from rlinf_amd.workers.actor.async_ppo_fsdp_worker import AsyncPPOEmbodiedFSDPActor
    cfg = make_cfg()
    cfg.algorithm.loss_type = "decoupled_actor_critic"
    cfg.algorithm.rollout_store_size_per_rank, cfg.algorithm.staleness_threshold = store_size, threshold
    cfg.algorithm.on_policy_min_ratio = ratio
    w = AsyncPPOEmbodiedFSDPActor(validate_cfg(cfg), init_distributed())
    assert w.use_rollout_store and w.rollout_store.maxsize == store_size
    w.rollout_store = PriorityStore(store_size, stats_fn=torch_summary, device="cpu")
    return cfg, w


class _NotReady(Exception):
    pass


def _reference_learner(cfg, store_size):
    path = "rlinf/workers/actor/async_ppo_fsdp_worker.py"

    def sleep(_):
        raise _NotReady

    @contextmanager
    def worker_timer(_):
        yield

    drain = reference_loader.load_function(path, "AsyncPPOEmbodiedFSDPActor._drain_received_trajectories", queue=queue)
    wait = reference_loader.load_function(path, "AsyncPPOEmbodiedFSDPActor._wait_for_rollout_store_ready",
                                          asyncio=SimpleNamespace(sleep=sleep))
    me = SimpleNamespace(cfg=cfg, version=0, rollout_store=reference_store_class()(store_size), rollout_store_size=store_size,
                         _recv_queue=queue.Queue(), log_info=lambda *_: None, worker_timer=worker_timer)
    me._drain_received_trajectories = lambda: drain(me)

    def ready() -> bool:
        try:
            wait(me).send(None)
        except StopIteration:
            return True
        except _NotReady:
            return False
        raise AssertionError("the coroutine neither finished nor slept")

    return me, ready


@needs_reference
@pytest.mark.parametrize("store_size,threshold,ratio", [(1, 0, 0.0), (2, 1, 0.0), (2, 1, 0.5), (3, 2, 0.4), (2, 0, 1.0), (5, 3, 0.25)])
def test_learner_drop_evict_ready_match_the_reference(store_size, threshold, ratio):
    cfg, w = _learner(store_size, threshold, ratio)
    ref, ref_ready = _reference_learner(cfg, store_size)
    rng = random.Random(7 * store_size + threshold)
    used, readies, drops = set(), 0, 0
    for step in range(160):
        if rng.random() < 0.35:
            w.set_global_step(w.version + 1)
            ref.version = w.version
        for _ in range(rng.choice((0, 1, 1, 2))):
            if rng.random() < 0.4:  # sampled with one version throughout, usually the current one (priorities tie exactly)
                traj = make_traj(torch.full((T, B, A), float(max(0, w.version - rng.choice((0, 0, 0, 1))))), tag=step)
            else:
                traj = make_traj(random_versions(rng, max(0, w.version - rng.choice((0, 0, 0, 1, 1, 2, 4))), used), tag=step)
            before = w.dropped_on_receipt
            w.recv_rollout_trajectories([traj])
            drops += w.dropped_on_receipt - before
            ref._recv_queue.put(traj)
        got, want = w.rollout_store_ready(), ref_ready()
        assert got == want, step
        assert len(w.rollout_store) == len(ref.rollout_store) and w.rollout_store.get_metric() == ref.rollout_store.get_metric()
        if got:  # construct_rollout_batch: topn(store_size), then the staleness metrics (:167-177)
            readies += 1
            a, b = w.rollout_store.topn(store_size), ref.rollout_store.topn(store_size)
            assert all(x.source is y for x, y in zip(a, b)) and len(a) == len(b) == store_size
            assert all(x.summary.min >= w.version - threshold for x in a)
    assert readies > 5 and drops > 0 and w.rollout_store._discarded_unused > 0, (readies, drops)
    assert readies < 160 or ratio == 0.0, "the on-policy ratio held some rounds back"
    assert len(w.rollout_store._free) + len(w.rollout_store) == store_size + 1


def test_learner_without_the_keys_builds_no_store():
    from test_end_to_end import make_cfg
    from rlinf_amd.config import validate_cfg
    from rlinf_amd.scheduler import init_distributed
    from rlinf_amd.workers.actor.async_ppo_fsdp_worker import AsyncPPOEmbodiedFSDPActor
    cfg = make_cfg()
    cfg.algorithm.loss_type = "decoupled_actor_critic"
    w = AsyncPPOEmbodiedFSDPActor(validate_cfg(cfg), init_distributed())
    assert not w.use_rollout_store and w.rollout_store is None
    with pytest.raises(AssertionError, match="staleness_threshold"):
        w.construct_rollout_batch()


def test_validate_cfg_defaults_and_refusals():
    from test_end_to_end import make_cfg
    from rlinf_amd.config import validate_cfg
    cfg = validate_cfg(make_cfg())
    alg = cfg.algorithm
    assert alg.rollout_store_size_per_rank == 1 and alg.get("staleness_threshold") is None and alg.on_policy_min_ratio == 0.0

    def bad(**keys):
        c = make_cfg()
        c.algorithm.loss_type = "decoupled_actor_critic"
        for k, v in keys.items():
            c.algorithm[k] = v
        return c

    ok = validate_cfg(bad(rollout_store_size_per_rank=2, staleness_threshold=0, on_policy_min_ratio=1.0))
    assert ok.algorithm.rollout_store_size_per_rank == 2 and ok.algorithm.staleness_threshold == 0
    with pytest.raises(AssertionError, match="algorithm.staleness_threshold must not be negative"):
        validate_cfg(bad(staleness_threshold=-1))
    for r in (-0.1, 1.5):
        with pytest.raises(AssertionError, match=r"algorithm.on_policy_min_ratio must lie in \[0, 1\]"):
            validate_cfg(bad(staleness_threshold=1, on_policy_min_ratio=r))
    with pytest.raises(AssertionError, match="algorithm.staleness_threshold is required"):
        validate_cfg(bad(rollout_store_size_per_rank=2))
    with pytest.raises(AssertionError, match="rollout_store_size_per_rank must be at least 1"):
        validate_cfg(bad(rollout_store_size_per_rank=0))
    with pytest.raises(AssertionError, match="at most 16"):
        validate_cfg(bad(rollout_store_size_per_rank=17, staleness_threshold=1))
    sync = make_cfg()
    sync.algorithm.staleness_threshold = 1
    with pytest.raises(AssertionError, match="decoupled_actor_critic"):
        validate_cfg(sync)


def test_shipped_async_config_keeps_the_store_off():
    import os
    from conftest import ROOT
    from rlinf_amd.config import load_config, validate_cfg
    d = os.path.join(ROOT, "examples", "embodiment", "config")
    cfg = validate_cfg(load_config(os.path.join(d, "maniskill_async_ppo_mlp.yaml"), search_paths=[d]))
    alg = cfg.algorithm
    assert alg.rollout_store_size_per_rank == 1 and alg.get("staleness_threshold") is None and alg.on_policy_min_ratio == 0.0


# ---- argument validation of the ABI entries, without a GPU -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from rlinf_amd import _lib
    return _lib.load()


def test_version_stats_argument_validation(lib):
    from rlinf_amd._lib import VersionStats
    fake = 4096  # never dereferenced: validation fails first
    need = lib.rlx_version_stats_workspace_bytes(1 << 20)
    assert need >= 1024 * (4 + 64) * 8
    assert lib.rlx_version_stats(None, 8, 0, 64, fake, fake, need, None) == -22 and b"NULL" in lib.rlx_last_error()
    assert lib.rlx_version_stats(fake, 8, 0, 64, None, fake, need, None) == -22
    assert lib.rlx_version_stats(fake, 8, 0, 64, fake, None, need, None) == -22
    assert lib.rlx_version_stats(fake, 0, 0, 64, fake, fake, need, None) == -22 and b"n=0" in lib.rlx_last_error()
    for bins in (0, 65):
        assert lib.rlx_version_stats(fake, 8, 0, bins, fake, fake, need, None) == -22 and b"n_bins" in lib.rlx_last_error()
    assert lib.rlx_version_stats(fake + 2, 8, 0, 64, fake, fake, need, None) == -22 and b"misaligned" in lib.rlx_last_error()
    assert lib.rlx_version_stats(fake, 8, 0, 64, fake, fake, 8, None) == -28 and b"workspace" in lib.rlx_last_error()
    assert ctypes.sizeof(VersionStats) == 8 + 5 * 8 + 64 * 8


def test_gather_rows_segmented_argument_validation(lib):
    from rlinf_amd._lib import SegField
    fake = 4096
    envs = (ctypes.c_int64 * 2)(4, 4)
    table = (ctypes.c_void_p * 2)(fake, fake)
    f = (SegField * 1)()
    f[0].srcs, f[0].dst, f[0].row_bytes, f[0].t_rows = table, fake, 32, 3
    call = lambda fields, nf, ns, e, idx=fake, n=8: lib.rlx_gather_rows_segmented(fields, nf, ns, e, idx, n, None)  # noqa: E731
    assert call(f, 1, 0, envs) == -22 and b"n_slots=0" in lib.rlx_last_error()
    assert call(f, 1, 17, envs) == -22 and b"n_slots=17" in lib.rlx_last_error()
    assert call(f, 17, 2, envs) == -22 and b"n_fields=17" in lib.rlx_last_error()
    assert call(f, 1, 2, None) == -22 and b"slot_envs" in lib.rlx_last_error()
    assert call(None, 1, 2, envs) == -22 and b"NULL field table" in lib.rlx_last_error()
    assert call(f, 1, 2, envs, n=-1) == -22 and b"negative" in lib.rlx_last_error()
    for bad in (0, -3):
        assert call(f, 1, 2, (ctypes.c_int64 * 2)(4, bad)) == -22 and b"B_s=" in lib.rlx_last_error()
    f[0].row_bytes = 0
    assert call(f, 1, 2, envs) == -22 and b"row_bytes=0" in lib.rlx_last_error()
    f[0].row_bytes, f[0].t_rows = 32, 0
    assert call(f, 1, 2, envs) == -22 and b"t_rows=0" in lib.rlx_last_error()
    f[0].t_rows, f[0].srcs = 3, ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p))
    assert call(f, 1, 2, envs) == -22 and b"NULL table" in lib.rlx_last_error()
    f[0].srcs, f[0].dst = table, None
    assert call(f, 1, 2, envs) == -22
    f[0].dst = fake
    hole = (ctypes.c_void_p * 2)(fake, None)
    f[0].srcs = hole
    assert call(f, 1, 2, envs) == -22 and b"slot 1 is NULL" in lib.rlx_last_error()
    # nothing to do: no fields, or an index without rows
    f[0].srcs = table
    assert call(f, 0, 2, envs) == 0 and call(f, 1, 2, envs, n=0) == 0
