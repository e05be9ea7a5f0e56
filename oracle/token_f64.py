"""Float64 restatements of the token path, for parity tests at GRPO-step shapes.  TEST INFRASTRUCTURE ONLY.

The same operations as ``token_oracle.py`` (which they reuse wherever a function is dtype-generic), evaluated in
float64 on whatever device the inputs live on, so that a [4096, 151936] batch can be checked on the GPU in a few
chunks.  They are the yardstick of ``tests/test_gpu_token_shapes.py`` and are pinned to the f32 oracle by
``tests/test_token_f64_helpers.py``.

Nothing under ``rlinf_amd/`` imports this file.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import token_oracle as TO


def logprob_entropy_lse(x: torch.Tensor, labels: torch.Tensor, rows_per_chunk: int = 256):
    """x [N, V] (any float dtype; the values are taken exactly), labels [N] -> (logprob, entropy, lse), f64 [N].
    logprob is ``-cross_entropy`` with torch's ignore_index (label -100 -> -0.0), entropy ``entropy_from_logits``."""
    n = x.shape[0]
    lp = torch.empty(n, dtype=torch.float64, device=x.device)
    ent, lse = torch.empty_like(lp), torch.empty_like(lp)
    for a in range(0, n, rows_per_chunk):
        x64 = x[a:a + rows_per_chunk].double()
        lp[a:a + rows_per_chunk] = -F.cross_entropy(x64, labels[a:a + rows_per_chunk], reduction="none")
        ent[a:a + rows_per_chunk] = TO.entropy_from_logits(x64)
        lse[a:a + rows_per_chunk] = torch.logsumexp(x64, -1)
    return lp, ent, lse


def logits_grad_rows(x: torch.Tensor, labels: torch.Tensor, d_logprob: torch.Tensor, d_entropy, temperature: float = 1.0):
    """d/dlogits of sum(d_logprob * logprob + d_entropy * entropy) for rows x [n, V] of the SCALED logits (what the
    softmax sees), returned w.r.t. the unscaled logits (the chain rule's 1 / temperature), f64 [n, V].  A row depends only
    on itself and its two upstream scalars, so callers bound memory by passing a chunk of rows at a time."""
    leaf = x.double().requires_grad_(True)
    obj = (-F.cross_entropy(leaf, labels, reduction="none") * d_logprob.double()).sum()
    if d_entropy is not None:
        obj = obj + (TO.entropy_from_logits(leaf) * d_entropy.double()).sum()
    (g,) = torch.autograd.grad(obj, leaf)
    return g / temperature


def token_loss(logprobs, old_logprobs, advantages, loss_mask, *, loss_agg: str, clip_ratio_low: float, clip_ratio_high: float,
               clip_ratio_c=None, clip_log_ratio_max=None, fast_path_zero_loss_mask=False, entropy=None, entropy_bonus=0.0,
               ref_logprobs=None, kl_beta=0.0, kl_penalty_type=None):
    """The reasoning learner's micro-batch loss (token_oracle.reasoning_loss_from_logprobs, fsdp_actor_worker.py:694-781) on f64
    leaves -> (loss, metrics dict, entropy_loss, kl_loss).  Inputs are used as given: pass f64 tensors (with requires_grad for the
    gradients)."""
    agg = TO.get_loss_agg_func(loss_agg)
    loss, metrics = TO.token_actor_loss(logprobs, old_logprobs, advantages, clip_ratio_low, clip_ratio_high, loss_mask=loss_mask,
                                        clip_ratio_c=clip_ratio_c, loss_agg_func=agg, clip_log_ratio_max=clip_log_ratio_max,
                                        fast_path_zero_loss_mask=fast_path_zero_loss_mask)
    dev, f64 = logprobs.device, torch.float64
    loss = loss.to(dev, f64)
    ent_loss = torch.zeros((), dtype=f64, device=dev)
    if entropy is not None:
        ent_loss = agg(entropy, mask=loss_mask)
        if entropy_bonus != 0.0:
            loss = loss - entropy_bonus * ent_loss
    kl_loss = torch.zeros((), dtype=f64, device=dev)
    if kl_beta > 0 and ref_logprobs is not None:
        kl_loss = agg(TO.kl_penalty(ref_logprobs, logprobs, kl_penalty_type), loss_mask)
        loss = loss + kl_loss * kl_beta
    return loss, {k: v.to(dev, f64) for k, v in metrics.items()}, ent_loss, kl_loss


def grpo_advantages(rewards: torch.Tensor, loss_mask: torch.Tensor, group_size: int, eps: float = 1e-6):
    """token_oracle.grpo_reasoning_advantages (advantages.py:89-121 with the reasoning pre/post shaping) in f64, on the inputs'
    device: rewards [bsz], loss_mask [bsz, seq] bool -> [bsz, seq] f64."""
    grouped = rewards.double().view(-1, group_size)
    mean = grouped.mean(dim=-1, keepdim=True).expand_as(grouped)
    std = grouped.std(dim=-1, keepdim=True).expand_as(grouped)
    adv = (grouped - mean) / (std + eps)
    mask = loss_mask.transpose(0, 1)
    out = (torch.zeros_like(mask, dtype=torch.float64) + adv.reshape(1, -1)) * mask
    return out.transpose(0, 1).contiguous()
