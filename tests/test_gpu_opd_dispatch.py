"""OPD through the dispatchers, on the device.

    calculate_adv_and_returns(task_type="embodied", adv_type="opd") and policy_loss(loss_type="opd") of this package, fed the
    reference learner's kwargs (embodied_fsdp_actor_worker.py compute_advantages_and_returns / train_micro_batch), against the
    reference's outputs recorded in tests/golden/opd.pt; the same reference dispatchers after rlinf_amd.ext.register() where
    the staged reference registry is present; and one micro-batch from stand-in action logits through
    DiscreteActionHead.logprobs_and_entropy -> OPD loss -> backward against a float64 torch chain."""

import os

import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = torch.load(os.path.join(GOLDEN_DIR, "opd.pt"))


def _dev(v):
    return v.to(DEV) if torch.is_tensor(v) else v


def _adv_kwargs(c):
    T, B, C = c["loss_mask"].shape
    return dict(task_type="embodied", adv_type="opd", rewards=torch.zeros(T, B, C, device=DEV),
                dones=torch.zeros(T + 1, B, C, dtype=torch.bool, device=DEV), values=None, prev_logprobs=_dev(c["prev"]),
                teacher_logprobs=_dev(c["teacher"]), num_action_chunks=c["num_action_chunks"], gamma=1, gae_lambda=1,
                group_size=8, reward_type="action_level", loss_mask=_dev(c["loss_mask"]), loss_mask_sum=_dev(c["loss_mask_sum"]),
                advantage_mode=None)


def _rel(got, want):
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-30)


def _loss_kwargs(c):
    kw = {k: _dev(v) for k, v in c["kwargs"].items()}
    x = kw["logprobs"].clone().requires_grad_(True)
    kw["logprobs"] = x
    return kw, x


@pytest.mark.parametrize("name", sorted(GOLD["adv"]))
def test_calculate_adv_and_returns_matches_the_recorded_reference(name):
    from rlinf_amd.algorithms import calculate_adv_and_returns
    c = GOLD["adv"][name]
    res = calculate_adv_and_returns(**_adv_kwargs(c))
    assert set(res) == {"advantages"}
    assert torch.equal(res["advantages"].cpu(), c["advantages"])


@pytest.mark.parametrize("name", sorted(GOLD["dispatch"]))
def test_policy_loss_matches_the_recorded_reference(name):
    from rlinf_amd.algorithms import policy_loss
    c = GOLD["dispatch"][name]
    kw, x = _loss_kwargs(c)
    loss, metrics = policy_loss(**kw)
    loss.backward()
    assert _rel(loss, c["loss"]) <= 1e-6
    assert set(metrics) == set(c["metrics"])
    for k, v in c["metrics"].items():
        assert _rel(metrics[k], v) <= 1e-6, k
    g, w = x.grad.double().cpu(), c["grad"].double()
    assert float((g - w).norm() / w.norm()) <= 1e-6


def test_reference_dispatchers_after_ext_register():
    """The reference's own registry.calculate_adv_and_returns / policy_loss (its preprocess_loss_inputs and .item() metrics) with
    the HIP callees that rlinf_amd.ext.register() installed, against the same recordings."""
    from oracle import reference_loader as RL
    if not RL.available():
        pytest.skip("neither /root/reference nor the staged oracle/_ref copy is present")
    ref = RL.load()
    mr = RL.load_models_registry()
    reg = ref.registry
    saved = dict(reg.ADV_REGISTRY), dict(reg.LOSS_REGISTRY), dict(mr.models._MODEL_REGISTRY)
    from rlinf_amd import ext
    ext.register()
    try:
        assert reg.ADV_REGISTRY["opd"] is not saved[0]["opd"] and reg.LOSS_REGISTRY["opd"] is not saved[1]["opd"]
        for c in GOLD["adv"].values():
            res = reg.calculate_adv_and_returns(**_adv_kwargs(c))
            assert res["advantages"].is_cuda and torch.equal(res["advantages"].cpu(), c["advantages"])
        for c in GOLD["dispatch"].values():
            kw, x = _loss_kwargs(c)
            loss, metrics = reg.policy_loss(**kw)
            loss.backward()
            assert _rel(loss, c["loss"]) <= 1e-6
            assert {k: type(v) for k, v in metrics.items()} == {k: float for k in c["metrics"]}
            for k, v in c["metrics"].items():
                assert _rel(metrics[k], v) <= 1e-6, k
            g, w = x.grad.double().cpu(), c["grad"].double()
            assert float((g - w).norm() / w.norm()) <= 1e-6
    finally:
        reg.ADV_REGISTRY.clear(), reg.ADV_REGISTRY.update(saved[0])
        reg.LOSS_REGISTRY.clear(), reg.LOSS_REGISTRY.update(saved[1])
        mr.models._MODEL_REGISTRY.clear(), mr.models._MODEL_REGISTRY.update(saved[2])


def test_action_logits_to_opd_loss_end_to_end():
    """Stand-in OpenVLA-OFT response logits -> DiscreteActionHead.logprobs_and_entropy (token_ops.hip) -> policy_loss(opd) on the
    learner's raw kwargs -> backward; d loss / d logits against the same chain in float64 torch."""
    from rlinf_amd.algorithms import policy_loss
    from rlinf_amd.models.embodiment.openvla_oft.discrete_action_head import DiscreteActionHead
    g = torch.Generator(device=DEV).manual_seed(17)
    bsz, C, A, V, bins, mes = 32, 8, 7, 400, 256, 240
    head = DiscreteActionHead(n_action_bins=bins, pad_to_multiple_of=64, action_dim=A, num_action_chunks=C)
    logits = torch.randn(bsz, C * A, V, device=DEV, generator=g) * 2
    tokens = torch.randint(0, bins, (bsz, C * A), device=DEV, generator=g)
    adv = torch.randn(bsz, C, A, device=DEV, generator=g) * 0.5
    mask = torch.rand(bsz, C, device=DEV, generator=g) < 0.8
    msum = torch.randint(1, mes + 1, (bsz, C), device=DEV, generator=g)
    x = logits.clone().requires_grad_(True)
    lp = head.logprobs_and_entropy(x, tokens)["logprobs"]
    assert lp.shape == (bsz, C * A) and lp.dtype == torch.float32
    loss, metrics = policy_loss(loss_type="opd", logprob_type="token_level", reward_type="action_level", single_action_dim=A,
                                logprobs=lp, old_logprobs=lp.detach(), advantages=adv, loss_mask=mask, loss_mask_sum=msum,
                                max_episode_steps=mes, task_type="embodied", clip_ratio_high=0.28, clip_ratio_low=0.2)
    loss.backward()
    # float64 chain: log_softmax over the bin window, gather, -(lp * adv) / ratio * mask, mean
    xd = logits.double().requires_grad_(True)
    hi = V - 64
    win = xd[..., hi - bins:hi]
    lpd = torch.log_softmax(win, dim=-1).gather(-1, tokens.unsqueeze(-1)).squeeze(-1).reshape(bsz, C, A)
    ratio = (msum.double() / mes).unsqueeze(-1)
    want = ((-lpd * adv.double()) / ratio * mask.double().unsqueeze(-1)).mean()
    want.backward()
    assert _rel(loss, want) <= 1e-5
    gx, gw = x.grad.double(), xd.grad
    assert float((gx - gw).norm() / gw.norm()) <= 1e-5
    assert set(metrics) == {"actor/policy_loss", "actor/opd_reward", "actor/opd_reverse_kl"}
