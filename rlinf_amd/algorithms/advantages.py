"""Built-in advantage estimators behind all seven registry names of the reference -- "gae", "grpo", "grpo_video",
"grpo_dynamic", "reinpp", "opd" and "raw" (mirror of rlinf/algorithms/advantages.py:24-438), served by gae_scan.hip /
grpo_adv.hip / adv_video_raw.hip / grpo_dynamic.hip / reinpp_adv.hip / opd.hip.

Two entry shapes exist for each name:
  * the reference's callee contract -- flattened ``[T, B]`` tensors, ``fn(**kwargs) -> (advantages,
    returns_or_None)`` -- so that a maintainer can re-register these functions inside the real RLinf
    (rlinf_amd/ext.py) and everything upstream keeps working;
  * a native ``[n_chunk, B, C]`` path used by ``calculate_adv_and_returns`` here, which skips the
    transpose/reshape copies entirely.
"""

from __future__ import annotations

from typing import Optional

import torch

from .. import ops, token_ops
from . import utils as _u
from .registry import _mark_native_adv, register_advantage


def _tb(t: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    return None if t is None else _u.stage(t, dev).contiguous().unsqueeze(-1)


@register_advantage("gae")
def compute_gae_advantages_and_returns(rewards: torch.Tensor, gamma: float = 1.0, gae_lambda: float = 1.0,
                                       values: Optional[torch.Tensor] = None, normalize_advantages: bool = True,
                                       normalize_returns: bool = False, loss_mask: Optional[torch.Tensor] = None,
                                       dones: Optional[torch.Tensor] = None, **kwargs):
    """rewards [T,B], values [T+1,B] (None = critic-free), dones [T+1,B] bool -> (advantages, returns) [T,B]."""
    dev = _u.compute_device(rewards, values, dones, loss_mask)
    adv, ret = ops.gae_scan(_tb(rewards.float(), dev), _tb(values, dev), _tb(dones, dev), _tb(loss_mask, dev),
                            gamma, gae_lambda, normalize_advantages, normalize_returns,
                            variant=int(kwargs.get("rlx_variant", 0)))
    return _u.unstage(adv[..., 0], rewards), _u.unstage(ret[..., 0], rewards)


@register_advantage("grpo")
def compute_grpo_advantages(rewards: torch.Tensor, loss_mask: torch.Tensor, group_size: int, **kwargs):
    """rewards = per-env scores (any shape with B elements, the reference passes [num_groups, group_size]);
    loss_mask [T,B] -> (advantages [T,B], None).  advantages.py:89-121."""
    dev = _u.compute_device(rewards, loss_mask)
    scores = _u.stage(rewards, dev).float().reshape(-1)
    mask = _u.stage(loss_mask, dev).contiguous().unsqueeze(-1)
    adv = ops.grpo_from_scores(scores, mask, int(group_size))
    return _u.unstage(adv[..., 0], loss_mask), None


# ---- native [n_chunk, B, C] paths -------------------------------------------------------------------------
def _chunk_level(rewards, dones, loss_mask, loss_mask_sum):
    rewards = rewards.sum(dim=-1, keepdim=True)
    dones = dones.max(dim=-1, keepdim=True)[0]
    if loss_mask is not None:
        loss_mask = loss_mask.max(dim=-1, keepdim=True)[0]
    if loss_mask_sum is not None:
        loss_mask_sum = loss_mask_sum.max(dim=-1, keepdim=True)[0]
    return rewards, dones, loss_mask, loss_mask_sum


def _native_gae(*, rewards, dones, values=None, loss_mask=None, loss_mask_sum=None, gamma=1.0, gae_lambda=1.0,
                reward_type="action_level", normalize_advantages=True, normalize_returns=False, **kwargs):
    dev = _u.compute_device(rewards, dones, values, loss_mask)
    r, d, m = _u.stage(rewards, dev), _u.stage(dones, dev), _u.stage(loss_mask, dev)
    if reward_type == "chunk_level":  # reductions over the chunk dim happen on device views (utils.py:80-89)
        r, d, m, _ = _chunk_level(r, d, m, None)
    v = _u.stage(values, dev)
    adv, ret = ops.gae_scan(r.float(), v, d, m, gamma, gae_lambda, normalize_advantages, normalize_returns,
                            variant=int(kwargs.get("rlx_variant", 0)))
    return {"advantages": _u.unstage(adv, rewards), "returns": _u.unstage(ret, rewards)}


def _native_grpo(*, rewards, dones, loss_mask=None, group_size=8, reward_type="action_level", **kwargs):
    if loss_mask is None:
        raise TypeError("compute_grpo_advantages() missing required argument: 'loss_mask'")
    dev = _u.compute_device(rewards, dones, loss_mask)
    r, d, m = _u.stage(rewards, dev), _u.stage(dones, dev), _u.stage(loss_mask, dev)
    if reward_type == "chunk_level":
        r, d, m, _ = _chunk_level(r, d, m, None)
    adv, _ = ops.grpo_group_adv(r.float(), d, m, int(group_size))
    return {"advantages": _u.unstage(adv, rewards)}


def _native_grpo_reasoning(*, rewards, loss_mask, group_size, **kwargs):
    """Reasoning GRPO: rewards [bsz], loss_mask [bsz, seq] -> (advantages [bsz, seq], None); replaces
    preprocess_reasoning_advantages_inputs + compute_grpo_advantages + postprocess (utils.py:177-277)."""
    if rewards.ndim != 1:
        raise AssertionError(f"Unsupported reward shape {rewards.shape}")
    dev = _u.compute_device(rewards, loss_mask)
    adv = token_ops.grpo_seq_adv(_u.stage(rewards, dev).float(), _u.stage(loss_mask, dev), int(group_size))
    return _u.unstage(adv, loss_mask), None


def _native_gae_reasoning(*, rewards, loss_mask, values=None, gamma=1.0, gae_lambda=1.0, normalize_advantages=True,
                          normalize_returns=False, **kwargs):
    """Reasoning GAE on [bsz, seq] tensors: (advantages, returns) -- the scan runs along the contiguous axis, nothing is
    transposed or padded (utils.py:177-277 + advantages.py:24-86)."""
    if rewards.ndim != 1:
        raise AssertionError(f"Unsupported reward shape {rewards.shape}")
    if values is None:  # critic-free GAE forces gamma = lambda = 1 and delta = r: the generic route handles it
        return None
    if values.ndim != 2:
        raise AssertionError(f"Unsupported values shape {values.shape}")
    dev = _u.compute_device(rewards, loss_mask, values)
    adv, ret = token_ops.gae_seq(_u.stage(values, dev).float(), _u.stage(rewards, dev).float(), gamma, gae_lambda)
    mask = _u.stage(loss_mask, dev)
    if normalize_advantages:
        ops.masked_standardize_(adv, mask)
    if normalize_returns:
        ops.masked_standardize_(ret, mask)
    return _u.unstage(adv, values), _u.unstage(ret, values)


def _native_reinpp_reasoning(*, rewards, loss_mask, group_size=None, use_reinpp_baseline=False, kl_beta=0.0, logprob=None,
                             ref_logprob=None, kl_penalty_type="", **kwargs):
    """Reinforce++ on [bsz, seq] tensors -> (advantages, None): replaces preprocess_reasoning_advantages_inputs +
    compute_reinpp_advantages (advantages.py:300-364) + postprocess, reward placement as the reference computes it."""
    if rewards.ndim != 1:
        raise AssertionError(f"Unsupported reward shape {rewards.shape}")
    if use_reinpp_baseline:
        # advantages.py:329-332,343: the group-centred rewards come back 1-D and scatter_ then rejects them against the
        # 2-D index -- the reference cannot run this option; fail the same way rather than guess what was meant
        raise IndexError("Dimension out of range (expected to be in range of [-1, 0], but got 1) -- use_reinpp_baseline "
                         "fails at the reward scatter in the reference (rlinf/algorithms/advantages.py:343)")
    dev = _u.compute_device(rewards, loss_mask, logprob, ref_logprob)
    kl = float(kl_beta) > 0
    adv = token_ops.reinpp_seq_adv(_u.stage(rewards, dev).float(), _u.stage(loss_mask, dev),
                                   _u.stage(logprob, dev).float() if kl else None,
                                   _u.stage(ref_logprob, dev).float() if kl else None, float(kl_beta), kl_penalty_type if kl else None)
    return _u.unstage(adv, loss_mask), None


@register_advantage("reinpp")
def compute_reinpp_advantages(rewards: torch.Tensor, loss_mask: torch.Tensor, group_size: int, use_reinpp_baseline: bool = False,
                              kl_beta: float = 0.0, logprob=None, ref_logprob=None, kl_penalty_type: str = "", **kwargs):
    """The reference's own signature (advantages.py:300-364): rewards [1, B], loss_mask / logprob / ref_logprob [L, B] ->
    (advantages [L, B], None).  The kernel works on sequence-major rows, so this entry transposes on the way in and out;
    ``calculate_adv_and_returns`` skips it and hands the [bsz, seq] tensors over untouched."""
    t = lambda x: None if x is None else x.transpose(0, 1)  # noqa: E731
    adv, _ = _native_reinpp_reasoning(rewards=rewards.reshape(-1), loss_mask=t(loss_mask), group_size=group_size,
                                      use_reinpp_baseline=use_reinpp_baseline, kl_beta=kl_beta, logprob=t(logprob),
                                      ref_logprob=t(ref_logprob), kl_penalty_type=kl_penalty_type)
    return adv.transpose(0, 1), None


@register_advantage("opd")
def compute_opd_advantages(prev_logprobs: torch.Tensor, teacher_logprobs: torch.Tensor,
                           loss_mask: Optional[torch.Tensor] = None, normalize_advantages: bool = False, **kwargs):
    """On-policy distillation (advantages.py:367-407): teacher - prev in f32, [T or T+1, B, C*A] -> [T, B, C, A] (trimmed to
    loss_mask's time length when a mask is given), (advantages, None).  The reference's checks run on the host first, with its
    messages; then ONE launch of opd.hip reads the kept time rows in place.  The dispatcher hands this function the raw kwargs
    (registry.py:106-111), so it is its own fast path."""
    assert teacher_logprobs is not None, "OPD advantage computation requires post-rollout teacher_logprobs."
    assert prev_logprobs is not None, "OPD advantage computation requires prev_logprobs from student rollout."
    assert teacher_logprobs.shape == prev_logprobs.shape, (
        f"teacher_logprobs shape {teacher_logprobs.shape} must match prev_logprobs shape {prev_logprobs.shape}.")
    assert not normalize_advantages, "VLA-OPD uses raw reverse-KL rewards; set normalize_advantages to False."
    num_action_chunks = kwargs.get("num_action_chunks", None)
    assert num_action_chunks is not None, "OPD advantage computation requires num_action_chunks."
    assert teacher_logprobs.shape[-1] % num_action_chunks == 0, (
        f"OPD token count {teacher_logprobs.shape[-1]} must be divisible by num_action_chunks {num_action_chunks}.")
    rows = None
    if loss_mask is not None:
        target_steps = loss_mask.shape[0]
        # dim 0 after the [..., C, A] reshape: the chunk axis itself for a 1-D input
        first = teacher_logprobs.shape[0] if teacher_logprobs.dim() > 1 else num_action_chunks
        assert first in {target_steps, target_steps + 1}, (
            f"OPD advantages time dimension {first} must match loss_mask time dimension {target_steps} or include one "
            "bootstrap step.")
        rows = target_steps
    dev = _u.compute_device(prev_logprobs, teacher_logprobs, loss_mask)
    adv = ops.opd_advantages(_u.stage(teacher_logprobs, dev), _u.stage(prev_logprobs, dev), int(num_action_chunks), rows)
    return _u.unstage(adv, prev_logprobs), None


def _grpo_dynamic_checks(num_rewards: int, group_size: int, idx_to_traj, advantage_mode: str) -> list:
    """The reference's host-side checks, in its order and with its messages (advantages.py:209-222,296-299), before any device
    work.  Returns idx_to_traj as a list of ints."""
    ids = token_ops.traj_ids(idx_to_traj)
    num_sequence = len(ids)
    assert num_rewards == num_sequence, f"Rewards size mismatch: {num_rewards} != {num_sequence}"
    num_trajectories = max(ids) + 1
    num_trajectories // group_size  # noqa: B018  (num_questions: a group_size of 0 raises here, as in the reference)
    assert num_trajectories % group_size == 0, (
        f"num_trajectories {num_trajectories} not divisible by group_size {group_size}")
    if advantage_mode not in ("trajectory", "turn"):
        raise ValueError(f"Invalid advantage_mode: {advantage_mode}. Must be 'trajectory' or 'turn'")
    return ids


def _grpo_dynamic_seq(rewards_flat, mask_rows, group_size, ids, advantage_mode):
    """[num_seq] rewards, [num_seq, seq] mask -> [num_seq, seq] advantages in the rewards' dtype (f16 / f64 rewards are computed
    in f32 and cast back)."""
    dev = _u.compute_device(rewards_flat, mask_rows)
    r = _u.stage(rewards_flat, dev)
    kernel_dtype = r.dtype if r.dtype in (torch.float32, torch.bfloat16) else torch.float32
    plan = token_ops.GrpoDynamicPlan(ids, int(group_size), dev)
    adv = token_ops.grpo_dynamic_adv(r.to(kernel_dtype), _u.stage(mask_rows, dev), plan, advantage_mode)
    return adv if adv.dtype == rewards_flat.dtype else adv.to(rewards_flat.dtype)


@register_advantage("grpo_dynamic")
def compute_grpo_dynamic_advantages(rewards: torch.Tensor, loss_mask: torch.Tensor, group_size: int, idx_to_traj,
                                    advantage_mode: str = "turn", **kwargs):
    """Multi-turn GRPO (advantages.py:167-299), the reference's callee contract: rewards [num_seq, 1], loss_mask [seq_len,
    num_seq] bool, idx_to_traj turn -> trajectory (a list of ints or a 1-D integer tensor, any order) -> (advantages [seq_len,
    num_seq], None).  advantage_mode "turn": mean / std over every turn of a question (trajectory // group_size);
    "trajectory": over the question's group_size trajectory rewards, each the mean of its turns.  One launch of grpo_dynamic.hip
    on the [num_seq, seq_len] layout; this entry transposes on the way in and out, ``calculate_adv_and_returns`` does not."""
    rewards_flat = rewards.squeeze(-1)
    ids = _grpo_dynamic_checks(rewards_flat.numel(), group_size, idx_to_traj, advantage_mode)
    adv = _grpo_dynamic_seq(rewards_flat.reshape(-1), loss_mask.transpose(0, 1), group_size, ids, advantage_mode)
    return _u.unstage(adv, loss_mask).transpose(0, 1), None


def _native_grpo_dynamic_reasoning(*, rewards, loss_mask, group_size, idx_to_traj, num_sequence=None, advantage_mode="turn",
                                   **kwargs):
    """Multi-turn GRPO on the learner's [num_seq, seq_len] tensors (ma_megatron_actor_worker.py:591-610) -> (advantages
    [num_seq, seq_len] contiguous, None): replaces preprocess_reasoning_advantages_inputs + compute_grpo_dynamic_advantages +
    postprocess (utils.py:207-215,265-277) without a transpose."""
    if loss_mask.dim() != 2:
        return None  # the generic route fails the way the reference does
    if rewards.ndim != 1:
        raise AssertionError(f"Unsupported reward shape {rewards.shape}")
    if num_sequence is None or rewards.numel() != num_sequence:
        return None  # the reference's reshape(-1, num_sequence) decides what happens
    ids = _grpo_dynamic_checks(rewards.numel(), group_size, idx_to_traj, advantage_mode)
    adv = _grpo_dynamic_seq(rewards, loss_mask, group_size, ids, advantage_mode)
    return _u.unstage(adv, loss_mask), None


def _grpo_video_mode(kwargs: dict) -> str:
    """advantages.py:153-162: anything but "frame" / "video" (None and a missing key included) is refused, before any launch."""
    mode = kwargs.get("advantage_mode")
    if mode not in ("frame", "video"):
        raise ValueError(f"Unsupported grpo_video advantage_mode: {mode}")
    return mode


@register_advantage("grpo_video")
def compute_grpo_video_advantages(rewards: torch.Tensor, loss_mask: torch.Tensor, group_size: int, **kwargs):
    """Frame / chunk-level GRPO for video rewards (advantages.py:124-164), the reference's callee contract: rewards [T, B],
    envs ordered as B / group_size prompts of group_size samples, loss_mask [T, B] -> (advantages [T, B], None).
    advantage_mode "frame": mean / unbiased std over the group_size samples of every (step, prompt); "video": over all
    T * group_size rewards of a prompt.  One launch of adv_video_raw.hip on the [T, B, 1] view."""
    mode = _grpo_video_mode(kwargs)
    dev = _u.compute_device(rewards, loss_mask)
    adv = ops.grpo_video_adv(_tb(rewards.float(), dev), _tb(loss_mask, dev), int(group_size), mode)
    return _u.unstage(adv[..., 0], rewards), None


@register_advantage("raw")
def compute_raw_advantages(rewards: torch.Tensor, loss_mask: torch.Tensor, normalize_advantages: bool = False, **kwargs):
    """Raw (optionally standardized) scores as advantages (advantages.py:410-438), the reference's callee contract: rewards =
    per-env scores ([B] or [num_groups, group_size]), loss_mask [T, B] -> (advantages [T, B], None).  adv = score[b] * mask;
    with normalize_advantages every element is standardized by the moments of the valid ones (safe_normalize's rule: one valid
    element gives NaN, none leaves the product).  adv_video_raw.hip on the [T, B, 1] view."""
    dev = _u.compute_device(rewards, loss_mask)
    scores = _u.stage(rewards, dev).float().reshape(-1)
    adv = ops.raw_adv(scores, _tb(loss_mask, dev), bool(normalize_advantages))
    return _u.unstage(adv[..., 0], loss_mask), None


def _native_grpo_video(*, rewards, dones=None, loss_mask=None, group_size=8, reward_type="action_level", **kwargs):
    """grpo_video on the [n_chunk, B, C] buffers: no score scan (registry.py:110), dones unused."""
    mode = _grpo_video_mode(kwargs)
    if loss_mask is None:
        raise TypeError("compute_grpo_video_advantages() missing required argument: 'loss_mask'")
    dev = _u.compute_device(rewards, loss_mask)
    r, m = _u.stage(rewards, dev), _u.stage(loss_mask, dev)
    if reward_type == "chunk_level":
        r, m = r.sum(dim=-1, keepdim=True), m.max(dim=-1, keepdim=True)[0]
    adv = ops.grpo_video_adv(r.float(), m, int(group_size), mode)
    return {"advantages": _u.unstage(adv, rewards)}


def _native_raw(*, rewards, dones, loss_mask=None, reward_type="action_level", normalize_advantages=False, **kwargs):
    """raw on the [n_chunk, B, C] buffers: the existing score scan (rlx_episode_scores), then score[b] * mask."""
    if loss_mask is None:
        raise TypeError("compute_raw_advantages() missing required argument: 'loss_mask'")
    dev = _u.compute_device(rewards, dones, loss_mask)
    r, d, m = _u.stage(rewards, dev), _u.stage(dones, dev), _u.stage(loss_mask, dev)
    if reward_type == "chunk_level":
        r, d, m, _ = _chunk_level(r, d, m, None)
    adv = ops.raw_adv(ops.episode_scores(r.float(), d), m, bool(normalize_advantages))
    return {"advantages": _u.unstage(adv, rewards)}


def _native_raw_reasoning(*, rewards, loss_mask, normalize_advantages=False, **kwargs):
    """Reasoning raw: rewards [bsz], loss_mask [bsz, seq] -> (advantages [bsz, seq] contiguous, None); replaces
    preprocess_reasoning_advantages_inputs + compute_raw_advantages + postprocess (utils.py:177-277) without a transpose."""
    if rewards.ndim != 1:
        raise AssertionError(f"Unsupported reward shape {rewards.shape}")
    if loss_mask.dim() != 2:
        return None  # the generic route fails the way the reference does
    dev = _u.compute_device(rewards, loss_mask)
    adv = ops.raw_adv(_u.stage(rewards, dev).float(), _u.stage(loss_mask, dev), bool(normalize_advantages))
    return _u.unstage(adv, loss_mask), None


_mark_native_adv("gae", _native_gae)
_mark_native_adv("grpo", _native_grpo)
_mark_native_adv("gae", _native_gae_reasoning, task_type="reasoning")
_mark_native_adv("grpo", _native_grpo_reasoning, task_type="reasoning")
_mark_native_adv("reinpp", _native_reinpp_reasoning, task_type="reasoning")
_mark_native_adv("grpo_dynamic", _native_grpo_dynamic_reasoning, task_type="reasoning")
_mark_native_adv("grpo_video", _native_grpo_video)  # embodied only: a reasoning batch fails in the generic route, as upstream
_mark_native_adv("raw", _native_raw)
_mark_native_adv("raw", _native_raw_reasoning, task_type="reasoning")
