"""The rollout store of asynchronous PPO: ``PriorityStore`` with the semantics of rlinf/data/storage/replay/buffer.py:1129-1199
(``add`` / ``topn`` / ``remove_below`` / ``get_metric`` / ``__len__``), holding device-resident snapshots.

Priority is the lexicographic pair (min version, mean version) of a trajectory; among equal priorities the oldest entry is
evicted first; a full store refuses a trajectory whose priority is lower than its lowest entry; ``topn`` returns the highest
priority first; ``discarded_unused`` counts the entries that left (or were refused) without ever having been returned by
``topn``.  With ``maxsize`` a handful, a sorted Python list stands in for the reference's SortedList.

What differs is where the data lives and who looks at it:
  * a stored trajectory is a SNAPSHOT -- the rollout worker overwrites its resident buffer with the next rollout -- taken into one
    of ``maxsize + 1`` preallocated slot buffers by one device copy per field (no allocation per iteration; the spare slot is
    where a candidate lands before the store decides whether it stays);
  * min, mean and the version histogram come from ONE device pass per added trajectory (``rlx_version_stats``) read back once:
    the mean is the exact integer sum over n taken in f64, and ``get_metric`` adds up the cached histograms instead of running
    ``torch.unique`` over every stored trajectory on every call.
"""

from __future__ import annotations

import bisect
from dataclasses import dataclass, field
from typing import Callable, Optional

import torch

from .embodied_types import Trajectory, TrajectoryBuffer

SLOT_FIELDS = ("states", "actions", "prev_logprobs", "versions", "prev_values", "rewards", "dones", "terminations", "truncations")


@dataclass
class VersionSummary:
    """What the store needs to know about a trajectory's ``versions``."""
    min: float
    total: int                      # exact sum of the rounded versions
    n: int
    counts: dict = field(default_factory=dict)  # rounded version -> cells

    @property
    def mean(self) -> float:
        return self.total / self.n

    @property
    def priority(self) -> tuple:
        return (float(self.min), self.mean)


def device_version_summary(workspace_cache: dict) -> Callable:
    """The product's statistics function: rlx_version_stats over the slot's contiguous ``versions``.  The bin range follows the
    data: a first pass with the base of the previous call; when anything falls outside, a second pass based at the rounded
    minimum (which the first pass delivered).  A trajectory that spans more versions than the kernel has bins is refused."""
    from .. import ops
    from .._lib import VERSION_STATS_MAX_BINS, RlxError

    def summary(versions: torch.Tensor) -> VersionSummary:
        key = ("version_stats", versions.device)
        if key not in workspace_cache:
            workspace_cache[key] = ops.version_stats_workspace(versions.device)
        base = workspace_cache.get("version_stats_base", 0)
        st = ops.version_stats(versions, base, VERSION_STATS_MAX_BINS, workspace_cache[key])
        if st.below or st.above:
            base = int(round(st.min))  # Python rounds half to even, like the kernel
            st = ops.version_stats(versions, base, VERSION_STATS_MAX_BINS, workspace_cache[key])
            if st.below or st.above:
                raise RlxError(f"a trajectory spans more than {VERSION_STATS_MAX_BINS} policy versions "
                               f"(min {st.min}, {st.above} cells above version {base + VERSION_STATS_MAX_BINS - 1})")
            workspace_cache["version_stats_base"] = base
        return VersionSummary(min=float(st.min), total=int(st.sum), n=int(st.n),
                              counts={base + k: int(c) for k, c in enumerate(st.count[:st.n_bins]) if c})

    return summary


class StoredTrajectory(Trajectory):
    """A slot of the store seen as a Trajectory; ``source`` is the trajectory it was copied from, ``summary`` its statistics."""
    slot: Optional[TrajectoryBuffer] = None
    source: Optional[Trajectory] = None
    summary: Optional[VersionSummary] = None


class PriorityStore:
    def __init__(self, maxsize: int, stats_fn: Optional[Callable] = None, device=None):
        self.maxsize = int(maxsize)
        self._seq = 0
        self._items: list = []  # ((priority, seq), StoredTrajectory), ascending: index 0 is the lowest priority, oldest first
        self._used_seqs: set = set()
        self._discarded_unused = 0
        self.device = device
        self._ws: dict = {}
        self._stats_fn = stats_fn if stats_fn is not None else device_version_summary(self._ws)
        self._free: list = []   # slot buffers not holding a stored trajectory
        self._shape = None

    # ---- slots ----------------------------------------------------------------------------------------------------------------
    def _allocate(self, traj: Trajectory) -> None:
        states = traj.forward_inputs["states"]
        T, B, D = states.shape
        C = traj.rewards.shape[-1]
        A = traj.actions.shape[-1]
        V = traj.prev_values.shape[-1]
        dev = self.device if self.device is not None else states.device
        self._shape = (T, B, D, A, C, V)
        self._free = [TrajectoryBuffer(T, B, D, A // C, C, value_dim=V, device=dev, max_episode_length=traj.max_episode_length)
                      for _ in range(self.maxsize + 1)]

    def _snapshot(self, traj: Trajectory) -> StoredTrajectory:
        """One device copy per field into a free slot."""
        if self._shape is None:
            self._allocate(traj)
        T, B, D, A, C, V = self._shape
        got = (*traj.forward_inputs["states"].shape, traj.actions.shape[-1], traj.rewards.shape[-1], traj.prev_values.shape[-1])
        if got != self._shape:
            raise ValueError(f"the rollout store holds trajectories of shape (T, B, obs, act, chunks, val) = {self._shape}; got {got} "
                             "(every stored trajectory has the same env count: the assembled batch then has a constant size)")
        slot = self._free.pop()
        for name in SLOT_FIELDS:
            src = traj.forward_inputs["states"] if name == "states" else getattr(traj, name)
            getattr(slot, name).copy_(src)
        view = slot.to_trajectory()
        st = StoredTrajectory(**{k: getattr(view, k) for k in Trajectory._TENSOR_FIELDS}, forward_inputs=view.forward_inputs,
                              max_episode_length=view.max_episode_length)
        st.slot, st.source = slot, traj
        return st

    def _release(self, st: StoredTrajectory) -> None:
        self._free.append(st.slot)

    # ---- the reference's interface ----------------------------------------------------------------------------------------------
    def stage(self, traj: Trajectory) -> StoredTrajectory:
        """Snapshot ``traj`` into the spare slot and take its version statistics; the caller then ``add``s or ``discard``s it."""
        st = self._snapshot(traj)
        st.summary = self._stats_fn(st.versions)
        return st

    def discard(self, st: StoredTrajectory) -> None:
        """A staged trajectory that never enters the store (dropped on receipt: too stale)."""
        self._release(st)

    def add(self, priority: Optional[tuple], data) -> bool:
        """buffer.py:1143-1160.  ``data``: a staged trajectory, or any Trajectory (staged here).  ``priority`` None: the
        trajectory's own (min, mean)."""
        st = data if isinstance(data, StoredTrajectory) else self.stage(data)
        if priority is None:
            priority = st.summary.priority
        priority = tuple(priority)
        if len(self._items) == self.maxsize and priority < self._items[0][0][0]:
            self._discarded_unused += 1
            self._release(st)
            return False
        key = (priority, self._seq)
        self._items.insert(bisect.bisect_left([k for k, _ in self._items], key), (key, st))
        self._seq += 1
        if len(self._items) > self.maxsize:
            (_, seq), evicted = self._items.pop(0)
            if seq not in self._used_seqs:
                self._discarded_unused += 1
            else:
                self._used_seqs.discard(seq)
            self._release(evicted)
        return True

    def topn(self, n: int) -> list:
        items = self._items[-n:]  # (n = 0 is the whole store, as with the reference's slice)
        for (_, seq), _ in items:
            self._used_seqs.add(seq)
        return [st for _, st in reversed(items)]

    def remove_below(self, threshold) -> None:
        keep = []
        for (priority, seq), st in self._items:
            if priority[0] < threshold:
                if seq not in self._used_seqs:
                    self._discarded_unused += 1
                else:
                    self._used_seqs.discard(seq)
                self._release(st)
            else:
                keep.append(((priority, seq), st))
        self._items = keep

    def get_metric(self) -> dict:
        total_cells, counts = 0, {}
        for _, st in self._items:
            for v, c in st.summary.counts.items():
                counts[v] = counts.get(v, 0) + c
            total_cells += st.summary.n
        if total_cells == 0:
            return {"discarded_unused": self._discarded_unused}
        result = {v: {"ratio": c / total_cells} for v, c in sorted(counts.items())}
        result["discarded_unused"] = self._discarded_unused
        return result

    def __len__(self) -> int:
        return len(self._items)
