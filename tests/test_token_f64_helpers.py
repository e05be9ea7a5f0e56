"""The f64 restatements of oracle/token_f64.py (the yardstick of tests/test_gpu_token_shapes.py) agree with the f32 oracle
of oracle/token_oracle.py at a small shape, so that drift in the restatement shows up here, without a GPU.

Tolerances: the f32 oracle's own rounding -- log-prob / entropy / lse 2e-5 over 517 terms of |x| <= 10; d_logits 1e-6 absolute
+ 2e-5 relative; loss / metrics 1e-6 absolute + 1e-5 relative; GRPO advantages 1e-6 absolute + 1e-5 relative (the same bounds
the GPU tests use against the f32 oracle).
"""

import pytest
import torch

from oracle import token_f64 as T64
from oracle import token_oracle as TO
from oracle.make_golden import token_batch


def close(got, want, atol, rtol, what=""):
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.allclose(got, want, atol=atol, rtol=rtol, equal_nan=True), (what, float((got - want).abs().nan_to_num().max()))


def test_logprob_entropy_lse_and_grad_match_the_f32_oracle():
    b = token_batch(501, 4, 300, 517)
    x = b["logits"].reshape(-1, 517)
    labels = b["labels"].reshape(-1).clone()
    labels[7] = -100
    lp, ent, lse = T64.logprob_entropy_lse(x, labels, rows_per_chunk=128)
    assert lp.dtype == ent.dtype == lse.dtype == torch.float64
    close(lp, TO.logprobs_from_logits(x, labels), 2e-5, 0, "logprob")
    close(ent, TO.entropy_from_logits(x), 2e-5, 0, "entropy")
    close(lse, torch.logsumexp(x, -1), 2e-5, 0, "lse")
    assert float(lp[7]) == 0.0 and torch.signbit(lp[7])  # -cross_entropy at ignore_index: -0.0, as the kernel writes
    g = torch.Generator().manual_seed(2)
    dlp, dent = torch.randn(x.shape[0], generator=g), torch.randn(x.shape[0], generator=g)
    dlp[7] = dent[7] = 0.0
    leaf = (x / 1.3).requires_grad_(True)
    obj = (TO.logprobs_from_logits(leaf, labels) * dlp).sum() + (TO.entropy_from_logits(leaf) * dent).sum()
    want = torch.autograd.grad(obj, leaf)[0] / 1.3
    close(T64.logits_grad_rows(x / 1.3, labels, dlp, dent, 1.3), want, 1e-6, 2e-5, "d_logits")


@pytest.mark.parametrize("agg", ["token-mean", "seq-mean-token-sum", "seq-mean-token-mean"])
@pytest.mark.parametrize("kl", [None, "k3"])
def test_token_loss_matches_the_f32_oracle(agg, kl):
    b = token_batch(502, 4, 300, 5)
    g = torch.Generator().manual_seed(4)
    lp0 = b["old_logprobs"] + 0.4 * torch.randn(4, 300, generator=g)
    ent0 = torch.rand(4, 300, generator=g) * 3
    kw = dict(loss_agg=agg, clip_ratio_low=0.2, clip_ratio_high=0.28, clip_ratio_c=3.0, clip_log_ratio_max=0.6,
              fast_path_zero_loss_mask=True, entropy_bonus=0.01, kl_beta=0.1 if kl else 0.0, kl_penalty_type=kl)
    grads = []
    results = []
    for dt in (torch.float32, torch.float64):
        lp, ent = lp0.to(dt, copy=True).requires_grad_(True), ent0.to(dt, copy=True).requires_grad_(True)
        ref = b["ref_logprobs"].to(dt) if kl else None
        if dt == torch.float32:
            loss, m = TO.reasoning_loss_from_logprobs(lp, ent, b["old_logprobs"], b["advantages"], b["loss_mask"],
                                                      ref_logprobs=ref, kl_penalty_type=kl or "low_var_kl",
                                                      **{k: v for k, v in kw.items() if k not in ("fast_path_zero_loss_mask",
                                                                                                  "kl_penalty_type")})
            ent_loss, kl_loss = m["actor/entropy_loss"], m["actor/kl_loss"]
        else:
            loss, m, ent_loss, kl_loss = T64.token_loss(lp, b["old_logprobs"].double(), b["advantages"].double(), b["loss_mask"],
                                                        entropy=ent, ref_logprobs=ref, **kw)
        loss.backward()
        grads.append((lp.grad, ent.grad))
        results.append((loss, m, ent_loss, kl_loss))
    (l32, m32, e32, k32), (l64, m64, e64, k64) = results
    close(l64, l32, 1e-6, 1e-5, "loss")
    close(e64, e32, 1e-6, 1e-5, "entropy_loss")
    close(k64, k32, 1e-6, 1e-5, "kl_loss")
    for k in TO.ZERO_MASK_KEYS[1:]:
        if k in m32:
            close(m64[k], m32[k], 1e-6, 1e-5, k)
    close(grads[1][0], grads[0][0], 1e-9, 2e-5, "d_logprobs")
    close(grads[1][1], grads[0][1], 1e-9, 2e-5, "d_entropy")


@pytest.mark.parametrize("group", [1, 2, 8])
def test_grpo_advantages_match_the_f32_oracle(group):
    b = token_batch(503, 16, 300, 5)
    want = TO.grpo_reasoning_advantages(b["rewards"], b["loss_mask"], group)
    got = T64.grpo_advantages(b["rewards"], b["loss_mask"], group)
    assert got.dtype == torch.float64
    close(got, want, 1e-6, 1e-5, "advantages")
