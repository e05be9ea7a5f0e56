"""The learner of asynchronous (decoupled) PPO: same method names and data path as
rlinf/workers/actor/async_ppo_fsdp_worker.py -- ``compute_advantages_and_returns`` (:185-213), ``compute_proximal_logprobs``
(:215-272) and ``run_training`` (:274-497).

What differs from the synchronous learner (embodied_fsdp_actor_worker.py) is data, not machinery: trajectories carry the
policy ``versions`` they were sampled with; the loss is ``decoupled_actor_critic`` (clip against a proximal policy given,
recomputed, or interpolated from the version distance; importance-weight by exp(proximal - behaviour)); advantages are
normalised a second time over the whole shuffled buffer with cross-rank statistics (``masked_normalization``); dual clip is
on by default (clip_ratio_c 3.0).

The rollout store (:72-182) is mirrored when ``algorithm.rollout_store_size_per_rank > 1`` or ``algorithm.staleness_threshold``
is set: received trajectories are snapshot into a ``PriorityStore`` (data/rollout_store.py), dropped on receipt and evicted
before every round when staler than the threshold, and a round trains on ``topn(store_size)`` -- assembled by
``rlx_gather_rows_segmented`` straight from the store's slots, so ``versions`` genuinely varies per row.  Without those keys
``recv_rollout_trajectories`` of the base class fills ``rollout_batch`` directly and no store exists.  The reference's receive
thread and channel drain are Ray-side control plane and not mirrored: ``construct_rollout_batch`` returns None ("not ready")
instead of sleeping, and the runner answers with another rollout.
"""

from __future__ import annotations

import torch

from ... import ops
from ..._lib import DPPO_OUT_NAMES, PPO_ACTOR_GRAD_SCALE, PPO_OUT_FLOATS
from ...algorithms.losses import _CRITIC_KEYS, _DECOUPLED_KEYS, _EV_MAP, explained_variance_from_stats
from ...algorithms.registry import calculate_adv_and_returns
from ...scheduler import all_reduce_flat_
from .embodied_fsdp_actor_worker import CRITIC_EXPLAINED_VARIANCE_KEY, EmbodiedFSDPActor


class AsyncPPOEmbodiedFSDPActor(EmbodiedFSDPActor):
    """Embodied learner for async PPO / decoupled actor-critic training."""

    METRIC_ROW_FLOATS = PPO_OUT_FLOATS + 2  # + the entropy bonus's part of the loss, the entropy loss

    def __init__(self, cfg, ctx=None):
        super().__init__(cfg, ctx)
        alg = cfg.algorithm
        self.rollout_store_size = int(alg.get("rollout_store_size_per_rank", 1))  # :79-82
        self.staleness_threshold = alg.get("staleness_threshold", None)
        self.on_policy_min_ratio = float(alg.get("on_policy_min_ratio", 0.0))
        self.use_rollout_store = self.rollout_store_size > 1 or self.staleness_threshold is not None
        self.rollout_store = None
        self.dropped_on_receipt = 0
        if self.use_rollout_store:
            assert self.staleness_threshold is not None, (
                "algorithm.staleness_threshold is required when algorithm.rollout_store_size_per_rank > 1")
            assert self.pipeline_epochs == 1, "the rollout store is not served together with runner.use_training_pipeline epochs"
            from ...data.rollout_store import PriorityStore
            self.rollout_store = PriorityStore(maxsize=self.rollout_store_size)

    # ---- the rollout store (:84-182) ---------------------------------------------------------------------------------------------
    def recv_rollout_trajectories(self, input_channel=None):
        """:99-128 without the thread: every received trajectory is snapshot into the store's spare slot, its (min, mean, histogram)
        taken in one device pass, and it is dropped when its minimum version is below ``version - staleness_threshold``."""
        if not self.use_rollout_store:
            return super().recv_rollout_trajectories(input_channel)
        if isinstance(input_channel, (list, tuple)):
            trajectories = list(input_channel)
        else:
            trajectories = []
            while not input_channel.empty():
                trajectories.append(input_channel.get())
        for traj in trajectories:
            staged = self.rollout_store.stage(traj)
            if staged.summary.min < self.version - self.staleness_threshold:
                self.dropped_on_receipt += 1
                self.rollout_store.discard(staged)
                continue
            self.rollout_store.add(staged.summary.priority, staged)

    def rollout_store_ready(self) -> bool:
        """One pass of _wait_for_rollout_store_ready's loop body (:139-159): evict below the threshold, then enough trajectories
        and, with ``on_policy_min_ratio``, that share of the stored cells at the current version."""
        store = self.rollout_store
        store.remove_below(self.version - self.staleness_threshold)
        if len(store) < self.rollout_store_size:
            return False
        if self.on_policy_min_ratio <= 0.0:
            return True
        return store.get_metric().get(int(self.version), {}).get("ratio", 0.0) >= self.on_policy_min_ratio

    def construct_rollout_batch(self):
        """:161-182.  None when the store is not ready (the runner then rolls out again); else the staleness metrics of the
        store, with ``rollout_batch`` assembled from ``topn(store_size)``."""
        assert self.use_rollout_store, "construct_rollout_batch needs the rollout store (algorithm.staleness_threshold)"
        if not self.rollout_store_ready():
            return None
        slots = self.rollout_store.topn(self.rollout_store_size)
        staleness_metrics: dict = {}
        for version_val, stats in self.rollout_store.get_metric().items():
            if version_val == "discarded_unused":
                staleness_metrics["discarded_unused_trajs"] = stats
                continue
            staleness_metrics[f"data_staleness_{int(self.version) - int(version_val)}/ratio"] = stats["ratio"]
        self.rollout_batch = self._process_received_rollout_batch(self._assemble_store_batch(slots))
        return staleness_metrics

    def _assemble_store_batch(self, slots: list) -> dict:
        """convert_trajectories_to_batch (embodied_types.py:500-559) for the arrays the advantage and metric kernels want
        contiguous -- rewards [T, sum B], dones and prev_values [T + 1, sum B] -- in one segmented launch into persistent buffers.
        The large fields stay in the slots (``_store``): run_training gathers its shuffled rows straight from them."""
        T, B = slots[0].rewards.shape[:2]
        sum_b = B * len(slots)
        key = ("store_batch", T, sum_b)
        names = ("rewards", "dones", "prev_values")
        if key not in self._ws:
            self._ws[key] = [torch.empty((getattr(slots[0], n).shape[0], sum_b, *getattr(slots[0], n).shape[2:]),
                                         dtype=getattr(slots[0], n).dtype, device=self.device) for n in names]
        outs = ops.gather_rows_segmented([[getattr(s, n) for s in slots] for n in names], None, self._ws[key])
        batch = dict(zip(names, outs))
        batch["_store"] = {"slots": slots, "T": int(T), "B": int(sum_b)}
        return batch

    def compute_advantages_and_returns(self) -> dict:
        """:185-213 -- GAE against the proximal values when the batch carries them."""
        alg, b = self.cfg.algorithm, self.rollout_batch
        proximal_values = b.get("proximal_values")
        out = calculate_adv_and_returns(
            task_type=self.cfg.runner.task_type, adv_type=alg.adv_type, rewards=b["rewards"], dones=b["dones"],
            values=proximal_values if proximal_values is not None else b.get("prev_values"), gamma=alg.get("gamma", 1),
            gae_lambda=alg.get("gae_lambda", 1), group_size=alg.get("group_size", 8), reward_type=alg.reward_type,
            loss_mask=b.get("loss_mask"), loss_mask_sum=b.get("loss_mask_sum"))
        b.update(out)
        return self._rollout_metrics(b)

    @torch.no_grad()
    def compute_proximal_logprobs(self) -> None:
        """:215-272 -- log-probs of the stored actions under the CURRENT weights, in micro-batch sized pieces, un-shuffled."""
        b, m = self.rollout_batch, self.model
        if "_store" in b:  # per slot, into a slot-shaped buffer: it rides with the other large fields in the segmented gather
            step = int(self.cfg.actor.micro_batch_size)
            for i, s in enumerate(b["_store"]["slots"]):
                n = s.prev_logprobs.shape[0] * s.prev_logprobs.shape[1]
                key = ("store_prox", i, tuple(s.prev_logprobs.shape))
                if key not in self._ws:
                    self._ws[key] = torch.empty_like(s.prev_logprobs)
                out = self._ws[key].view(n, -1)
                states, action = s.forward_inputs["states"].view(n, -1), s.forward_inputs["action"].view(n, -1)
                for lo in range(0, n, step):
                    out[lo:lo + step] = ops.mlp_train_fwd(m.flat.data, m.packed(), m.layout, states[lo:lo + step], action[lo:lo + step])[0]
            b["_store"]["proximal_logprobs"] = [self._ws[("store_prox", i, tuple(s.prev_logprobs.shape))]
                                                for i, s in enumerate(b["_store"]["slots"])]
            return
        T, B = b["prev_logprobs"].shape[:2]
        states = b["forward_inputs"]["states"].reshape(T * B, -1)
        action = b["forward_inputs"]["action"].reshape(T * B, -1)
        out = torch.empty((T * B, m.layout.act_dim), dtype=torch.float32, device=self.device)
        step = int(self.cfg.actor.micro_batch_size)
        for lo in range(0, T * B, step):
            lp = ops.mlp_train_fwd(m.flat.data, m.packed(), m.layout, states[lo:lo + step], action[lo:lo + step])[0]
            out[lo:lo + lp.shape[0]] = lp
        b["proximal_logprobs"] = out.view(T, B, *b["prev_logprobs"].shape[2:])

    # ---- update ---------------------------------------------------------------------------------------------------
    def _flatten_shuffle_normalize(self):
        """flatten_rollout_batch_for_train (:42-69) with one randperm seeded actor.seed + rank (:283-285), then
        masked_normalization of the advantages over the whole buffer, statistics summed over ranks (:292-296)."""
        b = self.rollout_batch
        store = b.get("_store")
        T, B = (store["T"], store["B"]) if store is not None else b["prev_logprobs"].shape[:2]
        N = T * B
        pkey = ("perm", N)
        if pkey not in self._ws:
            g = torch.Generator()
            g.manual_seed(int(self.cfg.actor.seed) + self._rank)
            self._ws[pkey] = torch.randperm(N, generator=g).to(self.device)
        if store is not None:
            return self._flatten_shuffle_normalize_store(b, store, N, self._ws[pkey])
        fields = {"states": b["forward_inputs"]["states"], "action": b["forward_inputs"]["action"],
                  "prev_logprobs": b["prev_logprobs"], "advantages": b["advantages"], "prev_values": b["prev_values"][:-1],
                  "returns": b.get("returns"), "loss_mask": b.get("loss_mask"), "versions": b.get("versions"),
                  "proximal_logprobs": b.get("proximal_logprobs"), "proximal_values": b.get("proximal_values")}
        if b.get("loss_mask_sum") is not None:
            fields["loss_mask_sum"] = b["loss_mask_sum"].contiguous()
        fields = {k: v for k, v in fields.items() if v is not None}
        if "versions" in fields:
            fields["versions"] = fields["versions"].float()
        src = [v.reshape(N, *v.shape[2:]).contiguous() for v in fields.values()]
        # persistent destinations, keyed by every field's name, row shape and dtype: the prepared launches and the captured
        # hipGraph of the fused path read the same addresses every iteration
        key = ("ashuf", N, tuple((n, tuple(t.shape[1:]), t.dtype) for n, t in zip(fields, src)))
        if key not in self._ws:
            self._ws[key] = [torch.empty_like(t) for t in src] + [torch.empty(N, *src[list(fields).index("advantages")].shape[1:],
                                                                              dtype=torch.float32, device=self.device)]
        flat = dict(zip(fields, ops.gather_rows(src, self._ws[pkey], self._ws[key][:-1])))
        return self._normalize_flat_advantages(flat, self._ws[key][-1]), N

    def _flatten_shuffle_normalize_store(self, b: dict, store: dict, N: int, perm: torch.Tensor):
        """The same rows from a store batch: the fields that live in the slots (states, action, prev_logprobs, versions,
        prev_values, proximal log-probs when recomputed) come out of ONE segmented launch -- cat(dim=1) + flatten + gather without
        the concatenated copy; the arrays computed on the assembled batch (advantages, returns, masks) through rlx_gather_rows."""
        slots = store["slots"]
        seg = {"states": [s.forward_inputs["states"] for s in slots], "action": [s.forward_inputs["action"] for s in slots],
               "prev_logprobs": [s.prev_logprobs for s in slots], "versions": [s.versions for s in slots],
               "prev_values": [s.prev_values for s in slots]}  # (T + 1 rows: the closing row is never addressed)
        if store.get("proximal_logprobs") is not None:
            seg["proximal_logprobs"] = store["proximal_logprobs"]
        cont = {"advantages": b["advantages"], "returns": b.get("returns"), "loss_mask": b.get("loss_mask"),
                "proximal_values": b.get("proximal_values")[:-1] if b.get("proximal_values") is not None else None}
        if b.get("loss_mask_sum") is not None:
            cont["loss_mask_sum"] = b["loss_mask_sum"].contiguous()
        cont = {k: v for k, v in cont.items() if v is not None}
        src = [v.reshape(N, *v.shape[2:]).contiguous() for v in cont.values()]
        key = ("ashuf_store", N, tuple((n, tuple(f[0].shape[2:]), f[0].dtype) for n, f in seg.items()),
               tuple((n, tuple(t.shape[1:]), t.dtype) for n, t in zip(cont, src)))
        if key not in self._ws:
            adv = src[list(cont).index("advantages")]
            self._ws[key] = ([torch.empty((N, *f[0].shape[2:]), dtype=f[0].dtype, device=self.device) for f in seg.values()],
                             [torch.empty_like(t) for t in src], torch.empty(N, *adv.shape[1:], dtype=torch.float32, device=self.device))
        seg_out, cont_out, adv_out = self._ws[key]
        flat = dict(zip(seg, ops.gather_rows_segmented(list(seg.values()), perm, seg_out)))
        flat.update(zip(cont, ops.gather_rows(src, perm, cont_out)))
        return self._normalize_flat_advantages(flat, adv_out), N

    def _normalize_flat_advantages(self, flat: dict, out: torch.Tensor) -> dict:
        if self.cfg.algorithm.get("normalize_advantages", True):
            adv, mask = flat["advantages"], flat.get("loss_mask")
            if mask is not None:
                assert mask.dim() == adv.dim() and mask.shape == adv.shape, (mask.shape, adv.shape)
            stats = ops.masked_stats(adv, mask)
            all_reduce_flat_(stats, self.ctx)  # factor, x_sum, x_sum_sq in ONE call (the reference issues three)
            flat["advantages"] = ops.masked_normalize(adv, mask, stats, out=out)
        return flat

    # ---- the fused path: rlx_ppo_step with the decoupled loss + deferred actor scale, prepared launches, hipGraph -------
    def _fused_update_ok(self, flat: dict) -> bool:
        """No critic warm-up, loss-mask sums already at the advantage shape.  (Any world size: every rank applies its own
        micro-batches' actor scales where its slabs are collapsed -- the xGMI staging launch or the slab sum in front of RCCL.)"""
        msum = flat.get("loss_mask_sum")
        return (self.fused_step and self.critic_warmup_steps == 0
                and (msum is None or (msum.dtype == torch.int64 and msum.numel() == flat["advantages"].numel())))

    def _loss_params(self, critic_warmup: bool):
        alg, m = self.cfg.algorithm, self.cfg.actor.model
        return ops.make_ppo_params(
            logprob_type=alg.logprob_type, action_dim=int(m.get("action_dim", 7)), chunks=int(m.get("num_action_chunks", 1)),
            clip_ratio_low=alg.clip_ratio_low, clip_ratio_high=alg.clip_ratio_high, value_clip=alg.get("value_clip"),
            huber_delta=alg.get("huber_delta"), max_episode_steps=self.cfg.env.train.get("max_episode_steps"),
            clip_ratio_c=alg.get("clip_ratio_c", 3.0), critic_warmup=critic_warmup, has_critic=True,
            reward_type=alg.get("reward_type", "action_level"))

    def _entropy_bonus_deferred(self, mb: dict, g: torch.Tensor, row: torch.Tensor):
        """:449-462 behind a decoupled fused step: the decoupled row keeps slot 19 for the average version, so the bonus goes
        through a scratch row; the logstd slab is in sum form -> the bonus is pre-divided by the row's actor scale."""
        ent_row = self._ent_row
        ent_row.zero_()
        ent_row[18] = row[DPPO_OUT_NAMES["mask_count"]]
        self._entropy_bonus(mb, g, ent_row, actor_scale=row[PPO_ACTOR_GRAD_SCALE:PPO_ACTOR_GRAD_SCALE + 1])
        row[PPO_OUT_FLOATS] = ent_row[0]
        row[PPO_OUT_FLOATS + 1] = ent_row[19]

    def _micro_batch_calls(self, lp, mb: dict, g: torch.Tensor, row: torch.Tensor, step_ws: torch.Tensor) -> list:
        """The decoupled loss inside rlx_ppo_step; the actor network's gradients leave it in sum form (_step_deferred)."""
        m, alg = self.model, self.cfg.algorithm
        if mb.get("proximal_values") is not None:  # :419-421
            mb["prev_values"] = mb["proximal_values"]
        if mb.get("loss_mask") is not None:
            mb["loss_mask"] = mb["loss_mask"].view(torch.uint8)
        dec = ops.decoupled_step_args(lp, mb, current_version=int(self.version) + 1,
                                      behave_weight_threshold=alg.get("behave_weight_threshold"),
                                      current_version_dev=self._version_dev)
        calls = [ops.PreparedPpoStep(m.flat.data, m.layout, lp, mb, g, row[:PPO_OUT_FLOATS], step_ws, grad_out=self._grad_out_host,
                                     tiles=m.tiles() if self.optimizer_writes_tiles else None,
                                     bf16=m.compute_dtype == torch.bfloat16, decoupled=dec)]
        if float(alg.get("entropy_bonus", 0) or 0) > 0:
            calls.append(lambda _stream: self._entropy_bonus_deferred(mb, g, row))
        return calls

    def _step_deferred(self, step_rows: torch.Tensor, accum: int) -> dict:
        return ops.deferred_actor_scale(self.model.layout, step_rows[:, :PPO_OUT_FLOATS], accum)

    def _capturable(self) -> bool:
        """At world_size > 1 only over the xGMI exchange (pure kernels): this learner does not capture RCCL."""
        return not self._exchange or self._xgmi is not None

    def _run_training_fused(self, flat: dict, N: int, n_global: int, per_rank: int, accum: int, micro: int) -> dict:
        n_steps = n_global * int(self.cfg.algorithm.get("update_epoch", 1))
        _, grads, rows, norms = self._update_buffers(micro, accum, n_steps)
        if getattr(self, "_version_dev", None) is None:
            self._version_dev = torch.zeros(1, dtype=torch.float32, device=self.device)
            self._ent_row = torch.zeros(PPO_OUT_FLOATS, device=self.device)  # _entropy_bonus_deferred's scratch row
        self._version_dev.fill_(float(int(self.version) + 1))  # read by the launches when they EXECUTE: a replayed graph sees it
        plan = self._update_plan(flat, N, n_global, per_rank, accum)
        self._lr_log = []
        self._run_or_replay(self._plan_key, lambda: self._exec_plan(plan, grads), n_steps)
        out = self._collect_decoupled_metrics(rows, norms, accum, flat.get("versions") is not None)
        if self._xgmi is not None and not self.defer_host_reads:
            self._xgmi.check_status()  # a peer that never published its gradient: raise instead of training on garbage
        self._step_lr_scheduler()  # :467
        return out

    def run_training(self) -> dict:
        a, alg, m = self.cfg.actor, self.cfg.algorithm, self.model
        assert alg.adv_type == "gae", "decoupled_actor_critic needs values: compute_values = (adv_type == 'gae') (:374)"
        lay = m.layout
        with self.timer("run_training"):
            flat, N = self._flatten_shuffle_normalize()
            world, gbs, micro = self._world_size, int(a.global_batch_size), int(a.micro_batch_size)
            assert gbs % (micro * world) == 0, (f"global_batch_size {gbs} must be divisible by micro_batch_size {micro} * "
                                                f"world_size {world}")
            per_rank = gbs // world
            accum = per_rank // micro
            self.gradient_accumulation = accum
            assert N % per_rank == 0, f"Flattened rollout size {N} must be divisible by per-rank batch size {per_rank}"
            n_global = N // per_rank
            if self._fused_update_ok(flat):
                return self._run_training_fused(flat, N, n_global, per_rank, accum, micro)
            n_steps = n_global * int(alg.get("update_epoch", 1))
            slabs = ops.mlp_bwd_slabs(micro)
            grads = torch.zeros((slabs * accum, m.n_params), dtype=torch.float32, device=self.device)
            bwd_ws = torch.empty(ops._lib.load().rlx_mlp_bwd_workspace_bytes(ops.byref(lay), micro), dtype=torch.uint8,
                                 device=self.device)
            rows = torch.zeros(n_steps * accum, PPO_OUT_FLOATS + 2, device=self.device)  # + the bonus's part of the loss, entropy loss
            norms = torch.zeros(n_steps, 2, device=self.device)
            ent_row = torch.zeros(PPO_OUT_FLOATS, device=self.device)
            self._grad_out_host = 1.0 / accum
            bonus = float(alg.get("entropy_bonus", 0) or 0)
            step = 0
            for _ in range(int(alg.get("update_epoch", 1))):
                for i in range(n_global):
                    warm = self.optimizer_steps < self.critic_warmup_steps
                    for j in range(accum):
                        lo = i * per_rank + j * micro
                        mb = {k: v[lo:lo + micro] for k, v in flat.items()}
                        row = rows[step * accum + j]
                        g = grads[j * slabs:(j + 1) * slabs]
                        logprob, _, value, mean, acts = ops.mlp_train_fwd(m.flat.data, m.packed(), lay, mb["states"], mb["action"])
                        lp, v = logprob.requires_grad_(True), value.requires_grad_(True)
                        prox_v = mb.get("proximal_values")
                        loss, out = ops.ppo_loss(
                            lp, mb["prev_logprobs"], mb["advantages"], logprob_type=alg.logprob_type, reward_type=alg.reward_type,
                            action_dim=int(a.model.get("action_dim", 7)), clip_ratio_low=alg.clip_ratio_low,
                            clip_ratio_high=alg.clip_ratio_high, values=v,
                            prev_values=prox_v if prox_v is not None else mb["prev_values"], returns=mb["returns"],
                            value_clip=alg.get("value_clip"), huber_delta=alg.get("huber_delta"), loss_mask=mb.get("loss_mask"),
                            loss_mask_sum=mb.get("loss_mask_sum"), max_episode_steps=self.cfg.env.train.get("max_episode_steps"),
                            clip_ratio_c=alg.get("clip_ratio_c", 3.0), critic_warmup=warm, has_critic=True,
                            decoupled=dict(proximal_logprobs=mb.get("proximal_logprobs"), versions=mb.get("versions"),
                                           current_version=int(self.version) + 1,
                                           behave_weight_threshold=alg.get("behave_weight_threshold")))
                        (loss / accum).backward()
                        ops.mlp_train_bwd(m.flat.data, m.packed(), lay, mb["states"], mb["action"], mean, acts, lp.grad, None,
                                          v.grad, grads=g, workspace=bwd_ws)
                        row[:PPO_OUT_FLOATS] = out
                        if bonus > 0 and not warm:  # :449-462; the decoupled row keeps slot 19 for the average version
                            ent_row.zero_()
                            ent_row[18] = out[DPPO_OUT_NAMES["mask_count"]]
                            self._entropy_bonus(mb, g, ent_row)
                            row[PPO_OUT_FLOATS] = ent_row[0]
                            row[PPO_OUT_FLOATS + 1] = ent_row[19]
                    self.optimizer_step(grads, stats=norms[step], critic_warmup=warm)
                    step += 1
            out = self._collect_decoupled_metrics(rows, norms, accum, flat.get("versions") is not None)
            self._step_lr_scheduler()  # :467
            return out

    def _collect_decoupled_metrics(self, rows, norms, accum: int, has_versions: bool):
        """Means over micro-batches (the version metrics only over those that reported them: some element unmasked,
        losses.py:156-165), AVG over ranks; EV sufficient statistics summed (:477-496).  One D2H copy -- behind the queued
        launches and read one iteration late when the runner's run-ahead loop asks for that (utils/pending.py)."""
        m = rows.mean(dim=0)
        counted = (rows[:, DPPO_OUT_NAMES["mask_count"]] > 0).float()
        ver = (rows[:, DPPO_OUT_NAMES["actor/average_version"]] * counted).sum() / counted.sum().clamp_min(1.0)
        ev = rows[:, DPPO_OUT_NAMES["ev/count"]:DPPO_OUT_NAMES["ev/errors_sq_sum"] + 1].sum(dim=0)
        avg = torch.cat([m, ver.view(1), norms[:, 0].mean().view(1)])
        if self._world_size > 1:
            all_reduce_flat_(avg, self.ctx, average=True)
            all_reduce_flat_(ev, self.ctx)
        vec = torch.cat([avg, ev, counted.sum().view(1)])
        current, lrs = float(int(self.version) + 1), tuple(self._lrs)

        def finish(host: list) -> dict:
            any_counted = host[-1] > 0
            out = {k: host[DPPO_OUT_NAMES[k]] for k in _DECOUPLED_KEYS + _CRITIC_KEYS}
            if has_versions and any_counted:
                out["actor/average_version"] = host[PPO_OUT_FLOATS + 2]
                out["actor/current_version"] = current
            n0 = PPO_OUT_FLOATS + 4
            out[CRITIC_EXPLAINED_VARIANCE_KEY] = explained_variance_from_stats(
                {name: host[n0 + i] for i, name in enumerate(_EV_MAP.values())})
            out["actor/total_loss"] = (host[DPPO_OUT_NAMES["loss"]] + host[PPO_OUT_FLOATS]) / max(accum, 1)
            out["actor/entropy_loss"] = host[PPO_OUT_FLOATS + 1]
            out["actor/grad_norm"] = host[PPO_OUT_FLOATS + 3]
            self._one_launch_expired(host[PPO_OUT_FLOATS + 3])
            out["actor/lr"], out["critic/lr"] = lrs
            return out

        return self._read_update_metrics(vec, finish)
