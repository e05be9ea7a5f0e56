"""Offline IQL learner for the MLP policy on HIP: flat parameter buffers, no autograd graph, no torch optimizer.

Takes the place of ``EmbodiedIQLFSDPPolicy`` (rlinf/workers/actor/fsdp_iql_policy_worker.py) at world size 1, with its method names
and result keys.  One update is the reference's ``update_step_forward`` as a fixed chain of launches on one stream, in order
(the launch list is in DESIGN.md):

    value leg    target twin forward (no grad) -> value forward -> value loss leg -> value backward -> Adam(value)
    actor leg    ONE value forward over obs || next_obs with the UPDATED value parameters (new_v and next_v) -> actor forward with
                 the log-prob -> actor loss leg -> actor backward -> Adam(actor); then the cosine schedule steps
    critic leg   twin forward -> critic loss leg -> twin backward -> Adam(critic)
    soft update  target <- (1 - tau) target + tau critic

The three optimizers are ``rlx_clip_adamw_step`` as it is: torch.optim.Adam is its formula with weight_decay = 0, no clipping,
the slab count in grad_partials and the step count on the device.  The eight metrics of every update go into one device matrix
that the host reads once per ``run_training``.  Checkpoints are this learner's own format (one file: the four flat buffers, the
moments, the step counts, the scheduler state, the data position), not the reference's sharded one.
"""

from __future__ import annotations

import ctypes
import os
from typing import Any, Optional

import torch

from ... import _lib, ops
from ...data.offline_dataset import OfflineTransitionDataset
from ...models.embodiment.iql_mlp import IqlNetworks

METRIC_KEYS = _lib.IQL_METRIC_NAMES
_OPTIMS = (("actor", "optim"), ("value", "value_optim"), ("critic", "critic_optim"))


class _Adam:
    """One flat parameter buffer under rlx_clip_adamw_step: the argument struct is prepared once; only ``lr`` may change."""

    def __init__(self, flat: torch.Tensor, optim_cfg, slabs: int):
        dev, n = flat.device, flat.numel()
        self.flat, self.n = flat, n
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
        self.step_state = torch.zeros(2, dtype=torch.int32, device=dev)  # the step count lives on the device
        self.stats = torch.zeros(2, dtype=torch.float32, device=dev)
        self.lr = float(optim_cfg.lr)
        self.args = ops._adamw_params([(0, n, self.lr)], slabs, 0, betas=(float(optim_cfg.adam_beta1), float(optim_cfg.adam_beta2)),
                                      eps=float(optim_cfg.adam_eps), weight_decay=0.0, max_grad_norm=0.0, grad_scale=1.0,
                                      tile_layout=None, tiles=None, deferred=None, sync=None)
        self.workspace = _lib.workspace(dev, _lib.load().rlx_adamw_workspace_bytes(n))

    def set_lr(self, lr: float) -> None:
        self.lr = float(lr)
        self.args.groups[0].lr = self.lr

    def step(self, grads: torch.Tensor) -> None:
        _lib.launch("rlx_clip_adamw_step", self.flat.device, self.flat, grads, self.exp_avg, self.exp_avg_sq, self.n, self.args,
                    self.stats, self.step_state, self.workspace, self.workspace.numel())

    def state(self) -> dict:
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "step_state": self.step_state.clone(),
                "lr": self.lr}

    def load_state(self, st: dict) -> None:
        self.exp_avg.copy_(st["exp_avg"]), self.exp_avg_sq.copy_(st["exp_avg_sq"]), self.step_state.copy_(st["step_state"])
        self.set_lr(st["lr"])


class EmbodiedIQLFSDPPolicy:
    def __init__(self, cfg, dataset: Optional[OfflineTransitionDataset] = None, device=None):
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda")
        self._offline_dataset = dataset
        self._obs_dim = self._action_dim = None
        self._dataset_size = 0
        self._global_step = 0
        self.nets: Optional[IqlNetworks] = None
        self._adam: dict = {}
        self.lr_scheduler = None
        self._use_fsdp_wrap = False  # accepted in the configuration; one process has nothing to wrap
        self._metrics = None
        self._metric_row = 0

    # ---- set-up -----------------------------------------------------------------------------------------------------------
    def build_offline_dataloader(self) -> None:
        data_cfg = self.cfg.get("data", None) or {}
        if self._offline_dataset is None:
            kind = data_cfg.get("dataset_type", None)
            if kind is None:
                raise ValueError("data.dataset_type is required for offline IQL (e.g. data.dataset_type: npz).")
            kind = str(kind).lower()
            if kind == "npz":
                self._offline_dataset = OfflineTransitionDataset.from_npz(data_cfg["dataset_path"], device=self.device)
            elif kind == "synthetic":
                m = self.cfg.actor.model
                self._offline_dataset = OfflineTransitionDataset.synthetic(int(data_cfg.get("size", 4096)), int(m.obs_dim),
                                                                         int(m.action_dim), seed=int(data_cfg.get("seed", 42)),
                                                                         device=self.device)
            else:
                raise AssertionError(f"offline IQL on HIP supports dataset_type 'npz' or 'synthetic', got {kind!r} (HDF5 / d4rl "
                                     "loading is not part of this build).")
        self._offline_dataset.configure(self.batch_size, seed=int(data_cfg.get("seed", 42)), shuffle=bool(data_cfg.get("shuffle", True)))
        self._obs_dim, self._action_dim = self._offline_dataset.get_obs_action_dims()
        self._dataset_size = self._offline_dataset.get_dataset_size()

    def setup_iql_components(self) -> None:
        cfg, actor_cfg = self.cfg, self.cfg.actor
        self._seed = int(actor_cfg.seed)
        self._save_dir = cfg.runner.get("save_dir", None) or "."
        torch.manual_seed(self._seed)
        self.discount, self.tau = float(cfg.algorithm.gamma), float(cfg.algorithm.tau)
        self.expectile, self.temperature = float(cfg.algorithm.expectile), float(cfg.algorithm.temperature)
        self.batch_size = int(actor_cfg.global_batch_size)
        if int(actor_cfg.micro_batch_size) != self.batch_size:
            raise ValueError("actor.micro_batch_size must equal per-rank batch size (actor.global_batch_size // world_size); got "
                             f"micro_batch_size={actor_cfg.micro_batch_size}, expected {self.batch_size}.")
        self.build_offline_dataloader()

    def init_worker(self) -> None:
        self.setup_iql_components()
        self.setup_model_and_optimizer(initialize_target=True)

    def setup_model_and_optimizer(self, initialize_target: bool = True) -> None:
        if self._obs_dim is None or self._action_dim is None:
            raise ValueError("actor.model.obs_dim/action_dim must be set before actor init.")
        model_cfg, alg = self.cfg.actor.model, self.cfg.algorithm
        if alg.get("hidden_dims", None) is None:
            raise ValueError("algorithm.hidden_dims is required for IQL offline training.")
        ic = model_cfg.get("iql_config", None) or {}
        self.nets = IqlNetworks(self._obs_dim, self._action_dim, self.device, num_action_chunks=int(model_cfg.get("num_action_chunks", 1)),
                                hidden_dims=tuple(alg.hidden_dims), log_std_min=float(ic.get("log_std_min", -5.0)),
                                log_std_max=float(ic.get("log_std_max", 2.0)))
        slabs = _lib.load().rlx_iql_mlp_bwd_slabs(self.batch_size)
        self._slabs = slabs
        flats = {"actor": self.nets.actor.flat, "value": self.nets.value.flat, "critic": self.nets.critic.flat}
        self._adam = {name: _Adam(flats[name], self.cfg.actor[key], slabs) for name, key in _OPTIMS}
        self.build_lr_schedulers()
        self._grads = {n: torch.empty((slabs, f.numel()), dtype=torch.float32, device=self.device) for n, f in flats.items()}
        ws = max(_lib.load().rlx_iql_mlp_bwd_workspace_bytes(ctypes.byref(net.layout), self.batch_size)
                 for net in (self.nets.actor, self.nets.value, self.nets.critic))
        self._bwd_ws = _lib.workspace(self.device, ws)
        self._metrics = torch.zeros((max(1, int(self.cfg.runner.get("local_update_steps", 1))), len(METRIC_KEYS)), dtype=torch.float32,
                                    device=self.device)

    def build_lr_schedulers(self) -> None:
        """The actor's cosine schedule is torch's own class over a one-parameter stand-in optimizer, so the sequence of learning
        rates is bit-equal to the reference's; the value and critic rates are constant."""
        self._lr_dummy = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=self._adam["actor"].lr)
        self.lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self._lr_dummy, T_max=max(1, int(self.cfg.runner.max_steps)),
                                                                       eta_min=0.0)

    # ---- one update ---------------------------------------------------------------------------------------------------------
    def update_one_epoch(self, batch) -> dict:
        obs, actions, rewards, masks, next_obs = batch
        M = int(obs.shape[0])
        if M != self.batch_size:
            raise ValueError(f"Offline IQL requires static batch size. Got {M}, expected {self.batch_size}. Use a fixed-size sampler "
                             "(e.g., drop_last=True).")
        N, row, ad = self.nets, self._metrics[self._metric_row], self._adam
        # value leg
        q_target, _, _ = N.target.forward(obs, actions=actions)
        v, v_acts, _ = N.value.forward(obs, train=True)
        d_v, q_min = ops.iql_value_loss(q_target, v, self.expectile, row)
        ad["value"].step(N.value.backward(obs, None, v_acts, d_v, grads=self._grads["value"], workspace=self._bwd_ws))
        # actor leg.  q_min is reused: the reference evaluates the target twin again here, on parameters that have not changed
        # since the value leg (the soft update comes last), so the second evaluation returns the same numbers.
        vv, _, _ = N.value.forward(obs, obs2=next_obs)
        new_v, next_v = vv.view(-1)[:M], vv.view(-1)[M:]
        mean, a_acts, logprob = N.actor.forward(obs, train=True, logprob_of=actions)
        d_mean, d_logstd, _ = ops.iql_actor_loss(N.actor.flat, N.actor.layout, q_min, new_v, logprob, mean, actions, self.temperature, row)
        ad["actor"].step(N.actor.backward(obs, None, a_acts, d_mean, d_logstd, grads=self._grads["actor"], workspace=self._bwd_ws))
        self._lr_dummy.step()
        self.lr_scheduler.step()
        ad["actor"].set_lr(self._lr_dummy.param_groups[0]["lr"])
        # critic leg
        q, q_acts, _ = N.critic.forward(obs, actions=actions, train=True)
        d_q = ops.iql_critic_loss(q, next_v, rewards, masks, self.discount, row)
        ad["critic"].step(N.critic.backward(obs, actions, q_acts, d_q, grads=self._grads["critic"], workspace=self._bwd_ws))
        self.soft_update_target_model()
        result: dict[str, Any] = {k: row[i] for i, k in enumerate(METRIC_KEYS)}  # device scalars: nothing is read back here
        result.update(lr_actor=ad["actor"].lr, lr_value=ad["value"].lr, lr_critic=ad["critic"].lr, use_fsdp_wrap=self._use_fsdp_wrap)
        return result

    def soft_update_target_model(self) -> None:
        ops.soft_update_(self.nets.target.flat, self.nets.critic.flat, self.tau)

    def run_training(self) -> dict:
        assert self.nets is not None, "init_worker() must be called before run_training()."
        local_update_steps = max(1, int(self.cfg.runner.local_update_steps))
        if self._global_step < 0:
            self._global_step = 0
        remaining_steps = int(self.cfg.runner.max_steps) - int(self._global_step)
        local_update_steps = min(local_update_steps, max(1, remaining_steps))
        lr_sums = {"lr_actor": 0.0, "lr_value": 0.0, "lr_critic": 0.0}
        for i in range(local_update_steps):
            self._metric_row = i
            info = self.update_one_epoch(self._offline_dataset.next_batch())
            for k in lr_sums:
                lr_sums[k] += info[k]
            self._global_step += 1
        self._metric_row = 0
        means = (self._metrics[:local_update_steps].sum(0) / local_update_steps).cpu()  # the one read-back
        out: dict[str, Any] = {k: float(means[i]) for i, k in enumerate(METRIC_KEYS)}
        out.update({k: v / local_update_steps for k, v in lr_sums.items()})
        out["__global_step"] = int(self._global_step)
        return out

    def compute_advantages_and_returns(self) -> dict:
        return {}

    def set_global_step(self, step: int) -> None:
        self._global_step = int(step)

    def get_policy_state_dict(self) -> dict:
        assert self.nets is not None, "init_worker() must be called before get_policy_state_dict()."
        return self.nets.get_policy_state_dict()

    # ---- checkpoints (own format) ---------------------------------------------------------------------------------------------
    def save_checkpoint(self, save_base_path: str, step: int) -> None:
        assert self.nets is not None, "init_worker() must initialize the networks first."
        os.makedirs(save_base_path, exist_ok=True)
        N = self.nets
        payload = {
            "format": "rlinf_amd.iql.v1",
            "flat": {k: getattr(N, k).flat.cpu() for k in ("actor", "critic", "target", "value")},
            "optim": {k: {n: (t.cpu() if isinstance(t, torch.Tensor) else t) for n, t in a.state().items()} for k, a in self._adam.items()},
            "lr_scheduler": self.lr_scheduler.state_dict(), "lr_dummy": self._lr_dummy.state_dict(),
            "step": int(step), "global_step": int(self._global_step),
            "data_epoch": int(self._offline_dataset.epoch), "data_iter_offset": int(self._offline_dataset.iter_offset),
        }
        torch.save(payload, os.path.join(save_base_path, "iql_learner.pt"))

    def load_checkpoint(self, load_base_path: str) -> None:
        assert self.nets is not None, "init_worker() must initialize the networks first."
        payload = torch.load(os.path.join(load_base_path, "iql_learner.pt"), map_location="cpu", weights_only=False)
        if payload.get("format") != "rlinf_amd.iql.v1":
            raise ValueError(f"{load_base_path}: not an rlinf_amd IQL checkpoint (the reference's sharded format is not read here)")
        for k, t in payload["flat"].items():
            getattr(self.nets, k).flat.copy_(t)
        for k, st in payload["optim"].items():
            self._adam[k].load_state(st)
        self._lr_dummy.load_state_dict(payload["lr_dummy"])
        self.lr_scheduler.load_state_dict(payload["lr_scheduler"])
        if "global_step" not in payload:
            raise KeyError("Checkpoint must contain key 'global_step' for offline IQL resume.")
        self._global_step = int(payload["global_step"])
        self._offline_dataset.set_position(payload["data_epoch"], payload["data_iter_offset"])

