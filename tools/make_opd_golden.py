"""Write tests/golden/opd.pt: the reference's on-policy distillation (OPD) advantage and loss on seeded inputs.

    python -m tools.make_opd_golden

Runs only where the reference tree is readable (oracle.reference_loader); the GPU tests read the stored file, never the tree.
Recorded, per case, the inputs and what the reference returned:
  adv/<case>       compute_opd_advantages (advantages.py:367-407) and the embodied dispatcher's OPD arm
                   (registry.calculate_adv_and_returns with the learner's kwargs)
  loss/<case>      compute_opd_actor_loss (losses.py:427-505) on shaped [bsz, C, A] tensors: loss, metrics, d loss / d logprobs
  dispatch/<case>  registry.policy_loss(task_type="embodied", loss_type="opd", ...) on the learner's RAW kwargs ([bsz, C*A]
                   log-probs, [bsz, C] mask and mask sum): loss, the .item()-ed metrics, d loss / d logprobs
"""

from __future__ import annotations

import os

import torch

from oracle import reference_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "opd.pt")


def _logprobs(g, *shape):
    return -(torch.rand(*shape, generator=g) * 6.0 + 0.01)


def adv_cases(ref, g):
    cases = {}
    for name, (t_in, t_mask, b, c, a, dtype) in {
        "T_f32": (6, 6, 5, 8, 7, torch.float32),
        "T1_f32": (7, 6, 5, 8, 7, torch.float32),
        "T1_bf16": (7, 6, 5, 8, 7, torch.bfloat16),
        "T_bf16_c2": (4, 4, 3, 2, 8, torch.bfloat16),
    }.items():
        prev = _logprobs(g, t_in, b, c * a).to(dtype)
        teacher = _logprobs(g, t_in, b, c * a).to(dtype)
        mask = torch.rand(t_mask, b, c, generator=g) < 0.8
        msum = mask.sum(dim=(0, 2), keepdim=True).expand_as(mask)
        direct, _ = ref.advantages.compute_opd_advantages(prev_logprobs=prev, teacher_logprobs=teacher, loss_mask=mask,
                                                         num_action_chunks=c)
        kw = dict(task_type="embodied", adv_type="opd", rewards=torch.zeros(t_mask, b, c), dones=torch.zeros(t_mask + 1, b, c,
                  dtype=torch.bool), values=None, prev_logprobs=prev, teacher_logprobs=teacher, num_action_chunks=c, gamma=1,
                  gae_lambda=1, group_size=8, reward_type="action_level", loss_mask=mask, loss_mask_sum=msum, advantage_mode=None)
        res = ref.registry.calculate_adv_and_returns(**kw)
        assert torch.equal(res["advantages"], direct) and "returns" not in res
        cases[name] = dict(prev=prev, teacher=teacher, loss_mask=mask, loss_mask_sum=msum.contiguous(), num_action_chunks=c,
                           advantages=direct)
    return cases


def _loss_inputs(g, bsz, c, a, p_on=0.75, max_steps=None, zero_sum_rows=0, all_false=False):
    lp = _logprobs(g, bsz, c, a)
    adv = torch.randn(bsz, c, a, generator=g) * 0.7
    mask = torch.rand(bsz, c, generator=g) < p_on
    if all_false:
        mask[:] = False
    msum = torch.randint(1, (max_steps or 64) + 1, (bsz, c), generator=g, dtype=torch.int64)
    if zero_sum_rows:
        msum[:zero_sum_rows] = 0
    return lp, adv, mask, msum


def loss_cases(ref, g):
    L = ref.losses
    cases = {}
    spec = {
        # name: (bsz, C, A, mask form, max_episode_steps, zero-sum rows, all-False)
        "mean_row_mask": (32, 8, 7, "row", None, 0, False),
        "mean_full_mask": (32, 8, 7, "full", None, 0, False),
        "ratio_row_mask": (32, 8, 7, "row", 240, 0, False),
        "ratio_full_mask": (32, 8, 7, "full", 240, 0, False),
        "mean_all_false": (16, 8, 7, "row", None, 0, True),
        "ratio_zero_sum": (16, 8, 7, "row", 240, 3, False),
        "mean_a4_c2": (24, 2, 4, "row", None, 0, False),
    }
    for name, (bsz, c, a, form, mes, zero_rows, all_false) in spec.items():
        lp, adv, mask, msum = _loss_inputs(g, bsz, c, a, max_steps=mes, zero_sum_rows=zero_rows, all_false=all_false)
        m = mask.unsqueeze(-1)
        s = msum.unsqueeze(-1)
        if form == "full":
            # per-token masks: a row's tokens are selected independently
            m = torch.rand(bsz, c, a, generator=g) < 0.75
            s = s.expand(bsz, c, a).contiguous()
        x = lp.clone().requires_grad_(True)
        loss, metrics = L.compute_opd_actor_loss(logprobs=x, advantages=adv, loss_mask=m, loss_mask_sum=s,
                                                 max_episode_steps=mes)
        loss.backward()
        cases[name] = dict(logprobs=lp, advantages=adv, loss_mask=m, loss_mask_sum=s, max_episode_steps=mes, loss=loss.detach(),
                           metrics={k: v.detach() for k, v in metrics.items()}, grad=x.grad.clone())
    return cases


def dispatch_cases(ref, g):
    cases = {}
    for name, (bsz, c, a, mes, zero_rows) in {"libero_like": (48, 8, 7, 240, 0), "mean_agg": (32, 8, 7, None, 0)}.items():
        lp, adv, mask, msum = _loss_inputs(g, bsz, c, a, max_steps=mes or 64, zero_sum_rows=zero_rows)
        raw = lp.reshape(bsz, c * a)
        x = raw.clone().requires_grad_(True)
        kw = dict(loss_type="opd", logprob_type="token_level", reward_type="action_level", single_action_dim=a, logprobs=x,
                  values=None, old_logprobs=raw.clone(), advantages=adv, returns=None, prev_values=None, clip_ratio_high=0.28,
                  clip_ratio_low=0.2, value_clip=None, huber_delta=None, loss_mask=mask, loss_mask_sum=msum,
                  max_episode_steps=mes, task_type="embodied", critic_warmup=False)
        loss, metrics = ref.registry.policy_loss(**kw)
        loss.backward()
        inputs = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
        cases[name] = dict(kwargs=inputs, loss=loss.detach(), metrics=dict(metrics), grad=x.grad.clone())
    return cases


def main():
    if not RL.available():
        raise SystemExit("the reference tree is not readable here: nothing to record")
    ref = RL.load()
    g = torch.Generator().manual_seed(20261015)
    data = {"adv": adv_cases(ref, g), "loss": loss_cases(ref, g), "dispatch": dispatch_cases(ref, g)}
    torch.save(data, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
