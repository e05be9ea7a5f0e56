"""Pin the oracle to the reference AT the boundary table of tests/helpers/loss_boundaries.py (CPU).

tests/test_gpu_loss_boundaries.py trusts the oracle's torch graph on ties and closed clamp edges; here the same inputs go through
the reference's own compute_ppo_actor_loss / compute_ppo_critic_loss / compute_decoupled_ppo_actor_critic_loss / kl_penalty, and
loss, metrics and autograd gradients must be EQUAL: both sides are the same torch expressions on the same host.  The forward
comparison takes plain inputs and replays from tests/golden/reference_calls where the reference tree is absent; differentiating
through the reference cannot be stored, so the gradient comparison runs where the tree is readable (as in
tests/test_oracle_vs_reference.py).
"""

import pytest
import torch

from helpers import loss_boundaries as LB
from oracle import ppo_oracle as O
from oracle import token_oracle as TO

pytestmark = pytest.mark.reference
CASES = LB.cases()
_ACTOR = ("logprobs", "old_logprobs", "advantages", "loss_mask", "loss_mask_sum")
_CRITIC = ("values", "returns", "prev_values", "loss_mask", "loss_mask_sum")


def _same(x, y, what):
    if torch.is_tensor(x) and torch.is_tensor(y):
        assert x.shape == y.shape and torch.equal(x.detach().float(), y.detach().float()), (what, x, y)
    else:
        assert float(x) == float(y), (what, x, y)


def _embodied(ref, case, inp, grad):
    """(loss, metrics, gradients) of the reference and of the oracle on one embodied case."""
    outs = []
    kw = LB.loss_kwargs(case)
    dec = case["family"] == "decoupled"
    for which in ("ref", "oracle"):
        lp = inp["logprobs"].clone().requires_grad_(grad)
        v = inp["values"].clone().requires_grad_(grad) if case["has_critic"] else None
        shaped, p2, v2 = LB.shaped_inputs(case, inp, lp=lp, v=v)
        more = dict(proximal_logprobs=p2, versions=v2, behave_weight_threshold=case["threshold"],
                    current_version=LB.CURRENT_VERSION if case["prox_mode"] == "versions" else None) if dec else {}
        actor_kw = {k: kw[k] for k in kw if k not in ("value_clip", "huber_delta")}
        critic_kw = {k: kw[k] for k in ("value_clip", "huber_delta", "max_episode_steps") if k in kw}
        if which == "oracle":
            if dec:
                loss, m = O.decoupled_actor_critic_loss(**more, **kw, **shaped)
            else:
                loss, m = O.ppo_actor_loss(**{k: shaped[k] for k in _ACTOR}, **actor_kw)
                if case["has_critic"]:
                    lc, mc = O.ppo_critic_loss(**{k: shaped[k] for k in _CRITIC}, **critic_kw)
                    loss, m = loss + lc, {**m, **mc}
        elif dec:
            loss, m = ref.losses.compute_decoupled_ppo_actor_critic_loss(**more, **kw, **shaped)
        else:
            loss, m = ref.losses.compute_ppo_actor_loss(**{k: shaped[k] for k in _ACTOR}, **actor_kw)
            if case["has_critic"]:
                lc, mc = ref.losses.compute_ppo_critic_loss(**{k: shaped[k] for k in _CRITIC}, **critic_kw)
                loss, m = loss + lc, {**m, **mc}
        grads = None
        if grad and loss.requires_grad:
            grads = torch.autograd.grad(loss, [lp] + ([v] if v is not None else []), allow_unused=True)
        outs.append((loss.detach(), m, grads))
    return outs


def _compare(outs, case):
    (l0, m0, g0), (l1, m1, g1) = outs
    _same(l0, l1, f"{case['id']} loss")
    actor = lambda m: {k for k in m if k.startswith("actor/")}  # noqa: E731
    assert actor(m0) == actor(m1), case["id"]
    for k in sorted(actor(m0)) + [k for k in ("critic/value_loss", "critic/value_clip_ratio") if k in m1]:
        _same(m0[k], m1[k], f"{case['id']} {k}")
    assert (g0 is None) == (g1 is None)
    for a, b in zip(g0 or (), g1 or ()):
        assert (a is None) == (b is None)
        if a is not None:
            _same(a, b, f"{case['id']} gradient")


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] != "token"], ids=lambda c: c["id"])
def test_embodied_forward_equals_the_reference(ref, case):
    _compare(_embodied(ref, case, LB.build(case), grad=False), case)


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] != "token"], ids=lambda c: c["id"])
def test_embodied_gradients_equal_the_reference(ref, case):
    _compare(_embodied(ref, case, LB.build(case), grad=True), case)


def _token_one(ref, case, inp, grad):
    """The reasoning loss as the learner composes it (fsdp_actor_worker.py:750-766): the actor loss, plus kl_beta times the
    aggregated kl_penalty.  ``ref`` None: the oracle's restatements; else every piece, the aggregation included, is the
    reference's.  (Without a mask the kernel takes every token; the reference's sequence aggregations need the mask spelled
    out, as LB.run_oracle does.)"""
    lp = inp["logprobs"].clone().requires_grad_(grad)
    mask = inp["loss_mask"] if inp["loss_mask"] is not None else torch.ones_like(lp, dtype=torch.bool)
    if ref is not None:
        fn, agg, pen = ref.losses.compute_ppo_actor_loss, ref.utils.get_loss_agg_func(case["agg"]), ref.algo_utils.kl_penalty
    else:
        fn, agg, pen = TO.token_actor_loss, TO.get_loss_agg_func(case["agg"]), TO.kl_penalty
    loss, m = fn(logprobs=lp, old_logprobs=inp["old_logprobs"], advantages=inp["advantages"], loss_mask=mask,
                 loss_agg_func=agg, fast_path_zero_loss_mask=True, **case["loss"])
    if case["kl"] is not None:
        kl_loss = agg(pen(inp["ref_logprobs"], lp, case["kl"]), mask)
        loss, m = loss + kl_loss * LB.KL_BETA, {**m, "actor/kl_loss": kl_loss.detach()}
    grads = torch.autograd.grad(loss, [lp]) if grad and loss.requires_grad else None
    return loss.detach(), m, grads


def _token(ref, case, inp, grad):
    return [_token_one(ref, case, inp, grad), _token_one(None, case, inp, grad)]


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] == "token"], ids=lambda c: c["id"])
def test_reasoning_oracle_entry_equals_the_pinned_composition(case):
    """tests/test_gpu_loss_boundaries.py takes its expectation from TO.reasoning_loss_from_logprobs (through LB.run_oracle); the
    tests below pin TO.token_actor_loss and TO.kl_penalty composed here.  The two are the same numbers, gradient included (the
    upstream 0.5 of run_oracle is a power of two: exact)."""
    inp = LB.build(case)
    loss, m, (g,) = _token_one(None, case, inp, grad=True)
    want = LB.run_oracle(case, inp)
    _same(want["loss"], loss, f"{case['id']} loss")
    _same(want["metrics"]["actor/final_loss"], loss, f"{case['id']} final_loss")
    for k in m:
        _same(want["metrics"][k], m[k], f"{case['id']} {k}")
    _same(want["d_logprobs"], g * LB.UPSTREAM, f"{case['id']} gradient")


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] == "token"], ids=lambda c: c["id"])
def test_reasoning_forward_equals_the_reference(ref, case):
    _compare(_token(ref, case, LB.build(case), grad=False), case)


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] == "token"], ids=lambda c: c["id"])
def test_reasoning_gradients_equal_the_reference(ref, case):
    _compare(_token(ref, case, LB.build(case), grad=True), case)
