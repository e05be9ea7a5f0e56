"""The async learner behind its rollout store: store size 2, staleness_threshold 1, weight_sync_interval 2 -- every round after
the first trains on two trajectories of two policy versions -- against the oracle loop (oracle/ppo_loop.py) fed the torch.cat of
the same stored trajectories; the staleness metrics against host-computed cell shares; eviction of what became stale; and the
unchanged path when the three keys are absent."""

import copy

import pytest
import torch

from oracle import ppo_loop as L
from oracle import ppo_oracle as O
from test_end_to_end import make_cfg

pytestmark = pytest.mark.gpu

T, B, GB, MB = 10, 16, 80, 40


def _runner(precision="32", hip_graph=False, store=True, explicit_defaults=False, entropy_bonus=0.0):
    from rlinf_amd.config import validate_cfg
    from rlinf_amd.runners import EmbodiedRunner
    from rlinf_amd.scheduler import init_distributed
    from rlinf_amd.workers.actor.async_ppo_fsdp_worker import AsyncPPOEmbodiedFSDPActor
    from rlinf_amd.workers.env import EnvWorker
    from rlinf_amd.workers.rollout.hf import MultiStepRolloutWorker
    cfg = make_cfg(total_envs=B, steps=T, global_batch=GB, micro_batch=MB, auto_reset=True, entropy_bonus=entropy_bonus,
                   hip_graph=hip_graph)
    cfg.algorithm.loss_type = "decoupled_actor_critic"
    cfg.algorithm.normalize_advantages = True
    cfg.actor.model.precision = precision
    if store:
        cfg.algorithm.rollout_store_size_per_rank = 2
        cfg.algorithm.staleness_threshold = 1
        cfg.runner.weight_sync_interval = 2
    elif explicit_defaults:
        cfg.algorithm.rollout_store_size_per_rank = 1
        cfg.algorithm.staleness_threshold = None
        cfg.algorithm.on_policy_min_ratio = 0.0
    cfg = validate_cfg(cfg)
    env = L.synthetic_env_tensors(0, T, B, 42, max_episode_steps=5)
    torch.manual_seed(11)
    ora = O.OracleMLPPolicy(42, 8, 1)
    sd = copy.deepcopy(ora.state_dict())
    ctx = init_distributed()
    actor = AsyncPPOEmbodiedFSDPActor.create_group(cfg, ctx).launch(None, name="ActorGroup")
    runner = EmbodiedRunner(cfg, actor, MultiStepRolloutWorker.create_group(cfg, ctx).launch(None, name="RolloutGroup"),
                            EnvWorker.create_group(cfg, ctx).launch(None, name="EnvGroup"))
    runner.init_workers(env_tensors=env)
    actor.worker.model.load_reference_state_dict(sd)
    return cfg, runner, actor.worker, ora


def _eps(k):
    return torch.randn(T, B, 8, generator=torch.Generator().manual_seed(100 + k)).cuda()


def _cat_stored(slots):
    """torch.cat(dim=1) of the stored trajectories, on the host: what convert_trajectories_to_batch (embodied_types.py:500-559)
    hands the reference's learner."""
    cat = lambda name: torch.cat([getattr(s, name).cpu() for s in slots], dim=1)  # noqa: E731
    return dict(rewards=cat("rewards"), dones=cat("dones"), prev_values=cat("prev_values"), prev_logprobs=cat("prev_logprobs"),
                versions=cat("versions"),
                forward_inputs=dict(states=torch.cat([s.forward_inputs["states"].cpu() for s in slots], dim=1),
                                    action=torch.cat([s.forward_inputs["action"].cpu() for s in slots], dim=1)))


@pytest.mark.parametrize("precision,hip_graph", [("32", False), ("32", True), ("bf16", False), ("bf16", True)])
def test_store_rounds_match_the_oracle_on_the_stored_trajectories(precision, hip_graph):
    """Four training rounds.  Tolerances: the ones tests/test_end_to_end.py::test_async_ppo_learner_matches_oracle uses for the same
    quantities (its ``check``, test_end_to_end.py:444-457: rel 2e-3 / abs 3e-4 in the first iteration, rel 2e-2 / abs 3e-3 later;
    grad norm rel 2e-3 / 2e-2; weights 2 * 3e-4 * steps + 1e-6 and fewer than 2 % of them off by more than 2e-5 * (it + 1)).
    bf16: the oracle's forward is the operand-rounding model of the bf16 launches (oracle/bf16_operand_model.py, the yardstick
    tests/test_gpu_fused_step.py and tests/test_end_to_end_bench_config.py pin them with): the reference arithmetic with the
    launches' bf16 operand roundings written out.  The oracle under torch.autocast only bounds a bf16 implementation from
    outside (two bf16 implementations land on different sides of the clip boundaries) and cannot meet f32-derived bounds."""
    cfg, runner, w, ora = _runner(precision, hip_graph)
    assert w.use_rollout_store and w.rollout_store is not None and runner.use_rollout_store
    opt = O.build_adamw(ora)
    if precision == "bf16":
        from oracle import bf16_operand_model as BM
        ora.evaluate = lambda states, action: BM.evaluate(ora, states, action)
    kw = dict(seed=1234, global_batch=GB, micro_batch=MB, update_epoch=2, entropy_bonus=0.0,
              max_episode_steps=cfg.env.train.get("max_episode_steps"))
    steps, mixed, failures = 0, 0, []
    for it in range(4):
        metrics = runner.run_step(_eps)
        assert w.version == it and runner.global_step == it + 1
        slots = w.rollout_batch["_store"]["slots"]
        assert len(slots) == 2
        batch = _cat_stored(slots)
        # ---- the batch: priority order, versions, staleness metrics ------------------------------------------------------
        vmin = [float(s.versions.min()) for s in slots]
        assert vmin == sorted(vmin, reverse=True), "topn: highest priority first"
        uniq, cnt = torch.unique(torch.round(batch["versions"].reshape(-1)).to(torch.int64), return_counts=True)
        mixed += len(uniq) > 1
        want = {f"rollout/data_staleness_{it - int(v)}/ratio": int(c) / batch["versions"].numel() for v, c in zip(uniq, cnt)}
        got = {k: v for k, v in metrics.items() if k.startswith("rollout/data_staleness_")}
        assert got == want and sum(got.values()) == 1.0, (got, want)
        assert all(0 <= it - int(v) <= 1 for v in uniq), "nothing staler than the threshold is trained on"
        assert metrics["rollout/discarded_unused_trajs"] == 0
        # ---- the assembled arrays and the training round against the oracle ------------------------------------------------
        rb = w.rollout_batch
        for name in ("rewards", "dones", "prev_values"):
            assert torch.equal(rb[name].cpu(), batch[name]), name
        batch = L.advantages(batch, 0.8, 0.9, True)
        torch.testing.assert_close(rb["advantages"].cpu(), batch["advantages"], rtol=1e-3 * (1 + 4 * min(it, 1)),
                                   atol=1e-4 * (1 + 4 * min(it, 1)))  # (test_end_to_end.py:468)
        om, norms = L.async_update(ora, opt, batch, version=it, **kw)
        steps += len(norms)
        mean = lambda k: sum(float(m[k]) for m in om) / len(om)  # noqa: E731
        tm = {k[len("train/"):]: v for k, v in metrics.items() if k.startswith("train/")}
        tol = dict(rel=2e-3, abs=3e-4) if it == 0 else dict(rel=2e-2, abs=3e-3)
        for k in ("actor/policy_loss", "actor/proximal_ratio", "actor/clipped_proximal_ratio", "actor/clip_fraction",
                  "actor/dual_clip_fraction", "actor/proximal_approx_kl", "actor/behav_approx_kl", "critic/value_loss",
                  "critic/value_clip_ratio", "actor/total_loss", "actor/entropy_loss", "actor/average_version",
                  "actor/current_version"):
            print(f"[{precision} graph={hip_graph} it={it}] {k}: got {tm[k]!r} want {mean(k)!r}")
            if tm[k] != pytest.approx(mean(k), **tol):
                failures.append((it, k, tm[k], mean(k)))
        gn = sum(norms) / len(norms)
        print(f"[{precision} graph={hip_graph} it={it}] actor/grad_norm: got {tm['actor/grad_norm']!r} want {gn!r}")
        if tm["actor/grad_norm"] != pytest.approx(gn, rel=2e-3 if it == 0 else 2e-2):
            failures.append((it, "actor/grad_norm", tm["actor/grad_norm"], gn))
        diff = (w.model.flat.detach().cpu() - torch.cat([p.detach().reshape(-1) for p in ora.parameters()])).abs()
        print(f"[{precision} graph={hip_graph} it={it}] weights: max diff {float(diff.max())!r}, "
              f"share above {2e-5 * (it + 1)}: {float((diff > 2e-5 * (it + 1)).float().mean())!r}")
        if not float(diff.max()) <= 2 * 3e-4 * steps + 1e-6:
            failures.append((it, "weights max", float(diff.max()), 2 * 3e-4 * steps + 1e-6))
        if not float((diff > 2e-5 * (it + 1)).float().mean()) < 0.02:
            failures.append((it, "weights share", float((diff > 2e-5 * (it + 1)).float().mean()), 0.02))
    assert mixed >= 1, "no trained batch held two distinct versions"
    assert mixed == 3, "weight_sync_interval 2 with a store of 2: every round after the first is mixed"
    assert w._plan is not None and ((w._graph is not None) == hip_graph), "which learner loop ran"
    runner.close()
    assert not failures, failures


def test_a_trajectory_made_stale_is_evicted_and_counted():
    cfg, runner, w, _ = _runner()
    runner._sync_rollout_weights()
    runner.env.interact(actor_channel=runner.actor_channel, eps=_eps(0))
    w.recv_rollout_trajectories(input_channel=runner.actor_channel)
    store = w.rollout_store
    assert len(store) == 1 and w.construct_rollout_batch() is None, "one of two trajectories: not ready"
    assert store.get_metric() == {0: {"ratio": 1.0}, "discarded_unused": 0}
    w.set_global_step(1)
    assert w.construct_rollout_batch() is None and len(store) == 1, "version 0 is within the threshold of version 1"
    w.set_global_step(2)  # version 0 < 2 - 1: evicted, never used
    assert w.construct_rollout_batch() is None and len(store) == 0
    assert store.get_metric() == {"discarded_unused": 1}
    # a stale trajectory is dropped on receipt: the rollout worker still stamps version 0
    runner.env.interact(actor_channel=runner.actor_channel, eps=_eps(1))
    w.recv_rollout_trajectories(input_channel=runner.actor_channel)
    assert len(store) == 0 and w.dropped_on_receipt == 1 and len(store._free) == 3, "every slot is back in the pool"
    # the next round reports the count
    runner.global_step = 2
    metrics = runner.run_step(_eps)
    assert metrics["rollout/discarded_unused_trajs"] == 1
    assert metrics["rollout/data_staleness_0/ratio"] == 1.0 and runner.rollout.worker.version == 2
    runner.close()


def test_on_policy_min_ratio_forces_current_version_data():
    """on_policy_min_ratio 1.0: a round waits until every stored cell carries the version being trained."""
    cfg, runner, w, _ = _runner()
    w.on_policy_min_ratio = 1.0
    for it in range(3):
        metrics = runner.run_step(_eps)
        assert metrics["rollout/data_staleness_0/ratio"] == 1.0, metrics
        assert float(torch.cat([s.versions.reshape(-1) for s in w.rollout_batch["_store"]["slots"]]).min()) == it
    runner.close()


def test_recomputed_proximal_logprobs_ride_in_the_segmented_gather():
    cfg, runner, w, _ = _runner()
    runner.run_step(_eps)
    runner.run_step(_eps)
    w.compute_proximal_logprobs()
    flat, n = w._flatten_shuffle_normalize()
    slots = w.rollout_batch["_store"]["slots"]
    perm = w._ws[("perm", n)]
    from rlinf_amd import ops
    m = w.model
    states = torch.cat([s.forward_inputs["states"] for s in slots], dim=1).reshape(n, -1)
    action = torch.cat([s.forward_inputs["action"] for s in slots], dim=1).reshape(n, -1)
    want = ops.mlp_train_fwd(m.flat.data, m.packed(), m.layout, states, action)[0][perm]
    torch.testing.assert_close(flat["proximal_logprobs"], want, rtol=1e-5, atol=1e-6)
    for name, src in (("states", states), ("action", action)):
        assert torch.equal(flat[name], src[perm])
    assert torch.equal(flat["versions"], torch.cat([s.versions for s in slots], dim=1).reshape(n, -1)[perm])
    assert torch.equal(flat["prev_values"], torch.cat([s.prev_values[:-1] for s in slots], dim=1).reshape(n, -1)[perm])
    runner.close()


def test_without_the_keys_the_store_is_never_built_and_nothing_changes(monkeypatch):
    from rlinf_amd.data import rollout_store

    def refuse(self, *a, **kw):
        raise AssertionError("PriorityStore constructed on the path without the rollout-store keys")

    monkeypatch.setattr(rollout_store.PriorityStore, "__init__", refuse)
    runs = []
    for explicit in (False, True):
        cfg, runner, w, _ = _runner(store=False, explicit_defaults=explicit)
        assert not w.use_rollout_store and w.rollout_store is None and not runner.use_rollout_store
        assert cfg.algorithm.rollout_store_size_per_rank == 1 and cfg.algorithm.get("staleness_threshold") is None
        out = []
        for it in range(3):
            m = runner.run_step(_eps(it))
            assert "_store" not in w.rollout_batch and torch.equal(w.rollout_batch["versions"], torch.full_like(w.rollout_batch["versions"], it))
            out.append({k: v for k, v in m.items() if k.startswith(("train/", "rollout/"))})
        assert not any("data_staleness" in k or "discarded" in k for k in out[-1])
        runs.append((out, w.model.flat.detach().cpu().clone()))
        runner.close()
    assert runs[0][0] == runs[1][0], "metrics with the keys absent and with their defaults written out"
    assert torch.equal(runs[0][1], runs[1][1])
