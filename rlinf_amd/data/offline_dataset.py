"""Device-resident transition set for offline training (IQL): the five D4RL fields as float32 tensors on the GPU, batches drawn by
a per-epoch permutation and gathered on the device with the row-gather kernel (rlx_gather_rows).

Takes the place of the reference's per-rank ``DataLoader`` over ``build_d4rl_dataset_from_cfg``
(rlinf/workers/actor/fsdp_iql_policy_worker.py:78-139, :500-542) at world size 1: shuffle, ``drop_last=True``, a new order every
epoch, and a position (epoch, batches taken) that a checkpoint restores.  The permutation comes from a CPU generator seeded by
``data.seed`` and the epoch, so it does not depend on the device.  HDF5 / ``d4rl`` loading and D4RL's reward post-processing are
not here: arrays or an ``.npz`` file with D4RL's key names are.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import ops

FIELDS = ("observations", "actions", "rewards", "masks", "next_observations")


class OfflineTransitionDataset:
    def __init__(self, observations, actions, rewards, masks, next_observations, device="cuda"):
        arrays = dict(zip(FIELDS, (observations, actions, rewards, masks, next_observations)))
        n = int(np.shape(arrays["observations"])[0])
        self._host_shapes = {}
        self.device = torch.device(device)
        self.fields = {}
        for k, v in arrays.items():
            t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(torch.float32)
            if t.shape[0] != n:
                raise ValueError(f"offline data set: {k} has {t.shape[0]} rows, observations {n}")
            if k in ("rewards", "masks"):
                t = t.reshape(n)
            elif t.dim() != 2:
                raise ValueError(f"offline data set: {k} must be [N, dim], got {tuple(t.shape)}")
            self.fields[k] = t.contiguous().to(self.device)
        if self.fields["next_observations"].shape != self.fields["observations"].shape:
            raise ValueError("offline data set: next_observations and observations differ in shape")
        self._n = n
        self.batch_size, self.seed, self.shuffle = None, 42, True
        self.epoch, self.iter_offset = 0, 0
        self._order = None

    # ---- construction ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, observations, actions, rewards, masks, next_observations, device="cuda"):
        return cls(observations, actions, rewards, masks, next_observations, device=device)

    @classmethod
    def from_npz(cls, path: str, device="cuda"):
        """D4RL's key names: observations, actions, rewards, terminals, next_observations (masks = 1 - terminals; a ``masks`` array,
        when the file has one, is taken as it is)."""
        with np.load(path) as z:
            masks = z["masks"] if "masks" in z.files else 1.0 - z["terminals"].astype(np.float32)
            return cls(z["observations"], z["actions"], z["rewards"], masks, z["next_observations"], device=device)

    @classmethod
    def synthetic(cls, size: int, obs_dim: int, action_dim: int, seed: int = 0, device="cuda"):
        """A seeded random transition set for smoke runs: actions inside (-1, 1), about one terminal in ten."""
        rng = np.random.default_rng(seed)
        obs = rng.standard_normal((size, obs_dim)).astype(np.float32)
        act = np.tanh(rng.standard_normal((size, action_dim))).astype(np.float32)
        rew = rng.standard_normal(size).astype(np.float32)
        masks = (rng.random(size) > 0.1).astype(np.float32)
        nxt = (obs + 0.1 * rng.standard_normal((size, obs_dim))).astype(np.float32)
        return cls(obs, act, rew, masks, nxt, device=device)

    # ---- the reference data set's queries ---------------------------------------------------------------------------------
    def get_obs_action_dims(self):
        return int(self.fields["observations"].shape[1]), int(self.fields["actions"].shape[1])

    def get_dataset_size(self) -> int:
        return self._n

    def __len__(self):
        return self._n

    # ---- batches ------------------------------------------------------------------------------------------------------------
    def configure(self, batch_size: int, seed: int = 42, shuffle: bool = True) -> None:
        if self._n < int(batch_size):
            raise ValueError(f"Dataset size ({self._n}) must be >= batch_size ({int(batch_size)}).")
        self.batch_size, self.seed, self.shuffle = int(batch_size), int(seed), bool(shuffle)
        self.set_position(0, 0)

    def batches_per_epoch(self) -> int:
        return self._n // self.batch_size  # the last partial batch is dropped

    def epoch_order(self, epoch: int) -> torch.Tensor:
        """The epoch's row order on the CPU (int64)."""
        if not self.shuffle:
            return torch.arange(self._n, dtype=torch.int64)
        g = torch.Generator()
        g.manual_seed(self.seed + int(epoch))
        return torch.randperm(self._n, generator=g)

    def set_position(self, epoch: int, iter_offset: int) -> None:
        """``iter_offset`` batches of ``epoch`` have been taken (what a checkpoint stores)."""
        self.epoch, self.iter_offset = int(epoch), int(iter_offset)
        self._order = self.epoch_order(self.epoch).to(self.device)

    def next_indices(self) -> torch.Tensor:
        if self.batch_size is None:
            raise RuntimeError("offline data set: configure(batch_size, ...) first")
        if self.iter_offset >= self.batches_per_epoch():
            self.set_position(self.epoch + 1, 0)
        lo = self.iter_offset * self.batch_size
        self.iter_offset += 1
        return self._order[lo:lo + self.batch_size]

    def next_batch(self):
        """-> (observations, actions, rewards, masks, next_observations) rows of the next batch, gathered on the device."""
        idx = self.next_indices()
        return tuple(ops.gather_rows([self.fields[k] for k in FIELDS], idx))
