"""Tensor-level launchers over the C ABI (include/rlx.h).  torch is plumbing only: device memory,
the current HIP stream and dtype/shape checks.  Every function requires HIP tensors and raises
otherwise -- there is no eager/CPU path.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import byref
from typing import Optional

import torch

from . import _lib
from ._lib import (AdamwGroup, AdamwParams, GaeParams, GatherField, IqlMlpLayout, MlpLayout, PpoLossParams, PpoStepArgs, RlxError,
                   RolloutStep, SacActorLayout, SacQLayout)


def _dev(*tensors) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RlxError("rlinf_amd ops need HIP (cuda) tensors; got a CPU tensor and there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RlxError(f"tensors on different devices: {dev} vs {t.device}")
    if dev is None:
        raise RlxError("no tensor argument")
    return dev


def _as_u8(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    if t.dtype == torch.uint8:
        return t.contiguous()
    raise RlxError(f"expected a bool/uint8 tensor, got {t.dtype}")


def _as_f32(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise RlxError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


def _nbc(t: torch.Tensor, name: str):
    if t.dim() != 3:
        raise RlxError(f"{name} must be [n_chunk, batch, chunk]; got {tuple(t.shape)}")
    return t.shape


def done_prefix_mask(dones: torch.Tensor):
    """dones bool [n+1, B, C] -> (loss_mask bool [n, B, C], mask_sum int64 [B]).  a9."""
    dev = _dev(dones)
    n1, B, C = _nbc(dones, "dones")
    if n1 < 1:
        raise RlxError("dones needs at least one row")
    d8 = _as_u8(dones)
    mask = torch.empty((n1 - 1, B, C), dtype=torch.bool, device=dev)
    cnt = torch.empty((B,), dtype=torch.int64, device=dev)
    _lib.launch("rlx_done_prefix_mask", dev, d8, mask, cnt, n1 - 1, B, C)
    return mask, cnt


def gae_scan(rewards: torch.Tensor, values: Optional[torch.Tensor], dones: torch.Tensor,
             loss_mask: Optional[torch.Tensor] = None, gamma: float = 1.0, gae_lambda: float = 1.0,
             normalize_advantages: bool = True, normalize_returns: bool = False, norm_eps: float = 1e-5,
             variant: int = 0, out: Optional[tuple] = None):
    """rewards [n,B,C] f32, values [n+1,B,C] f32|None, dones [n+1,B,C] bool -> (adv, ret) [n,B,C].  a10-a12."""
    lib = _lib.load()
    dev = _dev(rewards, values, dones, loss_mask)
    n, B, C = _nbc(rewards, "rewards")
    r = _as_f32(rewards, "rewards")
    v = _as_f32(values, "values")
    d8 = _as_u8(dones)
    m8 = _as_u8(loss_mask)
    if tuple(d8.shape) != (n + 1, B, C):
        raise RlxError(f"dones must be {(n + 1, B, C)}, got {tuple(d8.shape)}")
    if v is not None and tuple(v.shape) != (n + 1, B, C):
        raise RlxError(f"values must be {(n + 1, B, C)}, got {tuple(v.shape)}")
    if m8 is not None and tuple(m8.shape) != (n, B, C):
        raise RlxError(f"loss_mask must be {(n, B, C)}, got {tuple(m8.shape)}")
    if v is None:  # critic-free: the reference forces gamma = lambda = 1 (advantages.py:61-64)
        gamma, gae_lambda = 1.0, 1.0
    if out is not None:
        adv, ret = out
        if adv.shape != r.shape or ret.shape != r.shape or not (adv.is_contiguous() and ret.is_contiguous()):
            raise RlxError("gae_scan: out tensors must be contiguous and shaped like rewards")
    else:
        adv = torch.empty_like(r)
        ret = torch.empty_like(r)
    ws = _lib.workspace(dev, max(8, lib.rlx_gae_workspace_bytes(n, B, C)))
    p = GaeParams(float(gamma), float(float(gamma) * float(gae_lambda)), int(bool(normalize_advantages)),
                  int(bool(normalize_returns)), float(norm_eps), int(variant))
    _lib.launch("rlx_gae_scan", dev, r, v, d8, m8, adv, ret, ws, ws.numel(), n, B, C, p)
    return adv, ret


def masked_standardize_(x: torch.Tensor, mask: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    """In place x <- (x - mean(x[mask])) / (std(x[mask]) + eps).  a12."""
    lib = _lib.load()
    dev = _dev(x, mask)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RlxError("masked_standardize_ needs a contiguous float32 tensor")
    m8 = _as_u8(mask)
    if m8 is not None and m8.numel() != x.numel():
        raise RlxError("mask must have as many elements as x")
    ws = _lib.workspace(dev, lib.rlx_standardize_workspace_bytes(x.numel()))
    _lib.launch("rlx_masked_standardize", dev, x, m8, x.numel(), float(eps), ws, ws.numel())
    return x


def masked_stats(x: torch.Tensor, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    """(count, sum, sum of squares) of x[mask] as a device float64[3] (rlinf/utils/distributed.py:942-954);
    ``accumulate`` adds into ``out`` (several batches of one rank before the cross-rank sum)."""
    lib = _lib.load()
    dev = _dev(x, mask)
    xf = _as_f32(x, "x")
    m8 = _as_u8(mask)
    if m8 is not None and m8.numel() != xf.numel():
        raise AssertionError((tuple(mask.shape), tuple(x.shape)))
    if out is None:
        out = torch.zeros(3, dtype=torch.float64, device=dev)
    ws = _lib.workspace(dev, lib.rlx_masked_stats_workspace_bytes(xf.numel()))
    _lib.launch("rlx_masked_stats", dev, xf, m8, xf.numel(), out, int(bool(accumulate)), ws, ws.numel())
    return out


def normalize_from_stats(x: torch.Tensor, stats: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(x - mean) * rsqrt(var + 1e-5) from (count, sum, sumsq), f64 arithmetic -> f32 (rlinf/utils/distributed.py:957-965)."""
    dev = _dev(x, stats)
    xf = _as_f32(x, "x")
    if stats.dtype != torch.float64 or stats.numel() != 3:
        raise RlxError("stats must be float64[3]")
    if out is None:
        out = torch.empty_like(xf)
    st = stats.contiguous()
    _lib.launch("rlx_normalize_from_stats", dev, xf, st, out, xf.numel())
    return out.view(x.shape)


def masked_normalize(x: torch.Tensor, mask: Optional[torch.Tensor], stats: torch.Tensor, eps: float = 1e-5,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """masked_normalization's elementwise part (rlinf/utils/distributed.py:917-937) from (count, sum, sumsq):
    ((mask ? x : 0) - mean) / (sqrt(var_biased) + eps), f64 arithmetic -> f32."""
    dev = _dev(x, mask, stats)
    xf = _as_f32(x, "x")
    m8 = _as_u8(mask)
    if m8 is not None and m8.numel() != xf.numel():
        raise AssertionError((tuple(mask.shape), tuple(x.shape)))
    if stats.dtype != torch.float64 or stats.numel() != 3:
        raise RlxError("stats must be float64[3]")
    if out is None:
        out = torch.empty_like(xf)
    st = stats.contiguous()
    _lib.launch("rlx_masked_normalize", dev, xf, m8, st, float(eps), out, xf.numel())
    return out.view(x.shape)


def grpo_group_adv(rewards: torch.Tensor, dones: torch.Tensor, loss_mask: torch.Tensor, group_size: int,
                   eps: float = 1e-6):
    """rewards [n,B,C], dones [n+1,B,C], loss_mask [n,B,C] -> (advantages [n,B,C], scores [B]).  a13."""
    dev = _dev(rewards, dones, loss_mask)
    n, B, C = _nbc(rewards, "rewards")
    r = _as_f32(rewards, "rewards")
    d8 = _as_u8(dones)
    m8 = _as_u8(loss_mask)
    if tuple(d8.shape) != (n + 1, B, C) or tuple(m8.shape) != (n, B, C):
        raise RlxError("dones must be [n+1,B,C] and loss_mask [n,B,C]")
    if group_size < 1 or B % group_size != 0:
        raise RlxError(f"batch {B} not divisible by group_size {group_size}")
    adv = torch.empty_like(r)
    scores = torch.empty((B,), dtype=torch.float32, device=dev)
    _lib.launch("rlx_grpo_group_adv", dev, r, d8, m8, scores, adv, n, B, C, int(group_size), float(eps))
    return adv, scores


def grpo_from_scores(scores: torch.Tensor, loss_mask: torch.Tensor, group_size: int, eps: float = 1e-6) -> torch.Tensor:
    """scores [B] f32, loss_mask [n,B,C] -> advantages [n,B,C] (advantages.py:107-121)."""
    dev = _dev(scores, loss_mask)
    n, B, C = _nbc(loss_mask, "loss_mask")
    sc = _as_f32(scores.reshape(-1), "scores")
    if sc.numel() != B or group_size < 1 or B % group_size != 0:
        raise RlxError(f"scores must have {B} elements and batch must divide by group_size={group_size}")
    m8 = _as_u8(loss_mask)
    adv = torch.empty((n, B, C), dtype=torch.float32, device=dev)
    _lib.launch("rlx_grpo_from_scores", dev, sc, m8, adv, n, B, C, int(group_size), float(eps))
    return adv


def gaussian_entropy_bonus_(params: torch.Tensor, layout: MlpLayout, grads_slab0: torch.Tensor, out_row: torch.Tensor,
                            entropy_bonus: float, grad_scale: float, has_mask: bool, elem_scale: float = 1.0,
                            actor_scale: Optional[torch.Tensor] = None):
    """a22 for the Gaussian MLP policy: fold -entropy_bonus * masked_mean(entropy) into the loss row and the logstd
    gradient (see include/rlx.h).  ``grads_slab0`` is the first gradient slab [n_params].  ``actor_scale`` (one device float):
    the slab is in sum form behind a decoupled ppo_step and will be multiplied by it later -- the bonus is pre-divided."""
    dev = _dev(params, grads_slab0, out_row)
    off, A = int(layout.off_logstd), int(layout.act_dim)
    logstd = params[off:off + A]
    g = grads_slab0[off:off + A]
    argv = (logstd, A, g, out_row, float(entropy_bonus), float(grad_scale), int(bool(has_mask)), float(elem_scale))
    if actor_scale is not None:
        _lib.launch("rlx_gaussian_entropy_bonus_deferred", dev, *argv, actor_scale)
    else:
        _lib.launch("rlx_gaussian_entropy_bonus", dev, *argv)


def rollout_metrics(arrays: list, loss_mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a15: masked (sum, count, -min, max) of up to three f32 arrays in one pass -> f64 [len(arrays), 4] on the device
    (compute_rollout_metrics, metric_utils.py:422-506).  ``loss_mask`` broadcasts over trailing dimensions like the reference's
    ``v[mask.expand_as(v)]``: every array's element count must be a multiple of the mask's."""
    lib = _lib.load()
    dev = _dev(*arrays, loss_mask)
    xs = [_as_f32(a, "metric array") for a in arrays]
    k = len(xs)
    m8 = _as_u8(loss_mask)
    ptrs = (ctypes.c_void_p * k)(*[x.data_ptr() for x in xs])
    sizes = (ctypes.c_int64 * k)(*[x.numel() for x in xs])
    out = torch.empty((k, 4), dtype=torch.float64, device=dev) if out is None else out
    wsb = lib.rlx_rollout_metrics_workspace_bytes()
    ws = workspace if workspace is not None and workspace.numel() >= wsb else _lib.workspace(dev, wsb)
    _lib.launch("rlx_rollout_metrics", dev, ptrs, sizes, k, m8, 0 if m8 is None else m8.numel(), out, ws, ws.numel())
    return out


def reward_filter_mask(rewards: torch.Tensor, loss_mask: Optional[torch.Tensor], group_size: int, lower: float,
                       upper: float) -> torch.Tensor:
    """rewards [n, B, C] f32 (+ loss_mask [n, B, C] bool) -> the filtered loss mask (bool): [n, B, C] with a mask,
    [n, B, 1] without (embodied_fsdp_actor_worker.py:235-281)."""
    dev = _dev(rewards, loss_mask)
    n, B, C = _nbc(rewards, "rewards")
    r = _as_f32(rewards, "rewards")
    m = _as_u8(loss_mask)
    if m is not None and m.shape != r.shape:
        raise RlxError("loss_mask must have the shape of rewards")
    if group_size < 1 or B % group_size != 0:
        raise AssertionError(f"batch {B} not divisible by group_size {group_size}")
    out = torch.empty((n, B, C if m is not None else 1), dtype=torch.uint8, device=dev)
    _lib.launch("rlx_reward_filter_mask", dev, r, m, out, n, B, C, int(group_size), float(lower), float(upper))
    return out.view(torch.bool)


def episode_scores(rewards: torch.Tensor, dones: torch.Tensor) -> torch.Tensor:
    """rewards [n,B,C], dones [n+1,B,C] -> per-env first-episode return [B] (utils.py:134-152)."""
    dev = _dev(rewards, dones)
    n, B, C = _nbc(rewards, "rewards")
    r = _as_f32(rewards, "rewards")
    d8 = _as_u8(dones)
    if tuple(d8.shape) != (n + 1, B, C):
        raise RlxError("dones must be [n+1,B,C]")
    scores = torch.empty((B,), dtype=torch.float32, device=dev)
    _lib.launch("rlx_episode_scores", dev, r, d8, scores, n, B, C)
    return scores


def grpo_video_adv(rewards: torch.Tensor, loss_mask: torch.Tensor, group_size: int, mode: str, eps: float = 1e-6) -> torch.Tensor:
    """rewards [n,B,C] f32, loss_mask [n,B,C] bool -> advantages [n,B,C] f32 (advantages.py:124-164): per (step, prompt)
    moments for mode "frame", per prompt for "video".  a13b."""
    if mode not in _lib.GRPO_VIDEO_MODES:
        raise ValueError(f"Unsupported grpo_video advantage_mode: {mode}")
    dev = _dev(rewards, loss_mask)
    n, B, C = _nbc(rewards, "rewards")
    r = _as_f32(rewards, "rewards")
    m8 = _as_u8(loss_mask)
    if tuple(m8.shape) != (n, B, C):
        raise RlxError(f"loss_mask must be {(n, B, C)}, got {tuple(m8.shape)}")
    if group_size < 1 or B % group_size != 0:
        raise RlxError(f"batch {B} not divisible by group_size {group_size}")
    adv = torch.empty_like(r)
    _lib.launch("rlx_grpo_video_adv", dev, r, m8, adv, n, B, C, int(group_size), _lib.GRPO_VIDEO_MODES[mode], float(eps))
    return adv


def raw_adv(scores: torch.Tensor, loss_mask: torch.Tensor, normalize: bool = False, eps: float = 1e-5) -> torch.Tensor:
    """scores [B] f32 (any shape with B elements), loss_mask [n,B,C] or [bsz,seq] bool -> scores[b] * mask in the mask's shape,
    f32; ``normalize`` standardizes EVERY element with the moments of the valid ones (advantages.py:410-438).  a13c."""
    lib = _lib.load()
    dev = _dev(scores, loss_mask)
    if loss_mask.dim() == 3:
        outer, batch, inner = loss_mask.shape
    elif loss_mask.dim() == 2:
        outer, (batch, inner) = 1, loss_mask.shape
    else:
        raise RlxError(f"loss_mask must be [n_chunk, batch, chunk] or [bsz, seq]; got {tuple(loss_mask.shape)}")
    sc = _as_f32(scores.reshape(-1), "scores")
    if sc.numel() != batch:
        raise RlxError(f"scores must have {batch} elements, got {sc.numel()}")
    m8 = _as_u8(loss_mask)
    adv = torch.empty(tuple(loss_mask.shape), dtype=torch.float32, device=dev)
    ws = _lib.workspace(dev, lib.rlx_raw_adv_workspace_bytes(outer, batch, inner)) if normalize else None
    _lib.launch("rlx_raw_adv", dev, sc, m8, adv, outer, batch, inner, int(bool(normalize)), float(eps), ws,
                ws.numel() if normalize else 0)
    return adv


# --------------------------------------------------------------------------------------------
# a18-a21  fused PPO loss (forward + backward) as an autograd node
# --------------------------------------------------------------------------------------------
_LEVELS = ("action_level", "token_level", "chunk_level")


def _adv_geometry(logprob_type: str, action_dim: int, chunks: int, reward_type: Optional[str] = None):
    """(raw_per_adv, sub_per_adv, metric_unbroadcast): raw log-probs and ratios under one advantage element
    (algorithms/utils.py:325-356).  With reward_type='chunk_level' the advantage / mask / value tensors are per env-step ([bsz],
    utils.py:296-308) while token-level log-probs keep one loss element per action dimension of every chunk."""
    if reward_type == "chunk_level" and logprob_type == "token_level":  # one advantage per env step, a ratio per raw log-prob
        return action_dim * chunks, action_dim * chunks, 0
    if reward_type == "chunk_level" and logprob_type == "action_level" and chunks > 1:
        # ratio [bsz, C] against [bsz, 1] advantages / mask: one advantage element per env step, C ratios under it, each the
        # sum of action_dim raw log-probs; the ratio metrics keep the un-broadcast mask count (PpoLossParams.metric_unbroadcast)
        return action_dim * chunks, chunks, 1
    if logprob_type == "action_level":
        return action_dim, 1, 0
    if logprob_type == "token_level":
        return action_dim, action_dim, 0
    if logprob_type == "chunk_level":
        return action_dim * chunks, 1, 0
    raise RlxError(f"logprob_type must be one of {_LEVELS}")


def _loss_geometry(logprobs: torch.Tensor, logprob_type: str, action_dim: int, reward_type: Optional[str] = None):
    """(n_adv, chunks) for a [bsz, C*A] log-prob tensor: the advantage elements it spans and its action chunks per row."""
    per_row = logprobs.numel() // max(logprobs.shape[0], 1)
    if logprob_type not in _LEVELS:
        raise RlxError(f"logprob_type must be one of {_LEVELS}, got {logprob_type!r}")
    if per_row % action_dim != 0:
        raise RlxError(f"logprobs row of {per_row} elements is not a multiple of action_dim={action_dim}")
    chunks = per_row // action_dim
    return logprobs.shape[0] * per_row // _adv_geometry(logprob_type, action_dim, chunks, reward_type)[0], chunks


def _loss_forward(ctx, logprobs, values, params: PpoLossParams, n_adv: int, workspace_bytes, launch):
    """The forward both loss nodes share: per-element gradient factors, the metric row and the workspace are allocated here,
    ``launch(lp, g_lp, g_v, out, ws)`` issues the node's own forward, ``ctx`` keeps what rlx_ppo_loss_bwd needs."""
    dev = logprobs.device
    g_lp = torch.empty((n_adv * params.sub_per_adv,), dtype=torch.float32, device=dev)
    g_v = torch.empty((n_adv,), dtype=torch.float32, device=dev) if params.has_critic else None
    out = torch.empty((_lib.PPO_OUT_FLOATS,), dtype=torch.float32, device=dev)
    launch(logprobs.contiguous(), g_lp, g_v, out, _lib.workspace(dev, workspace_bytes(n_adv)))
    ctx.save_for_backward(g_lp, g_v if g_v is not None else out, out)
    ctx.has_critic = bool(params.has_critic)
    ctx.geom = (n_adv, params.raw_per_adv, params.sub_per_adv)
    ctx.lp_shape = logprobs.shape
    ctx.v_shape = None if values is None else values.shape
    ctx.mark_non_differentiable(out)
    return out[0].clone(), out


class _PpoLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logprobs, values, old_logprobs, advantages, prev_values, returns, loss_mask, loss_mask_sum,
                params: PpoLossParams, n_adv: int):
        lib = _lib.load()

        def launch(lp, g_lp, g_v, out, ws):
            _lib.launch("rlx_ppo_loss_fwd", lp.device, lp, old_logprobs, advantages, values, prev_values, returns, loss_mask,
                        loss_mask_sum, n_adv, params, g_lp, g_v, out, ws, ws.numel())

        return _loss_forward(ctx, logprobs, values, params, n_adv, lib.rlx_ppo_loss_workspace_bytes, launch)

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        g_lp, g_v, out = ctx.saved_tensors
        n_adv, raw, sub = ctx.geom
        dev = g_lp.device
        go = grad_loss.to(dtype=torch.float32).contiguous()
        d_lp = torch.empty((n_adv * raw,), dtype=torch.float32, device=dev)
        d_v = torch.empty((n_adv,), dtype=torch.float32, device=dev) if ctx.has_critic else None
        _lib.launch("rlx_ppo_loss_bwd", dev, g_lp, g_v if ctx.has_critic else None, out, go, d_lp, d_v, n_adv, raw, sub)
        return (d_lp.view(ctx.lp_shape), None if d_v is None else d_v.view(ctx.v_shape), None, None, None, None, None,
                None, None, None)


def ppo_loss(logprobs: torch.Tensor, old_logprobs: torch.Tensor, advantages: torch.Tensor, *,
             logprob_type: str = "action_level", action_dim: int = 8, clip_ratio_low: float, clip_ratio_high: float,
             values: Optional[torch.Tensor] = None, prev_values: Optional[torch.Tensor] = None,
             returns: Optional[torch.Tensor] = None, value_clip: Optional[float] = None,
             huber_delta: Optional[float] = None, loss_mask: Optional[torch.Tensor] = None,
             loss_mask_sum: Optional[torch.Tensor] = None, max_episode_steps: Optional[int] = None,
             clip_ratio_c: Optional[float] = None, clip_log_ratio_min: Optional[float] = None,
             clip_log_ratio_max: Optional[float] = None, critic_warmup: bool = False, has_critic: bool = True,
             decoupled: Optional[dict] = None, reward_type: Optional[str] = None):
    """Fused actor(+critic) PPO loss.  Inputs are the RAW per-dimension tensors the reference hands to
    policy_loss (before preprocess_loss_inputs); returns (loss 0-dim tensor with grad, out f32[20] on device,
    see _lib.PPO_OUT_NAMES).  losses.py asserts float32 inputs (:232-240); so do we."""
    dev = _dev(logprobs, old_logprobs, advantages, values, prev_values, returns, loss_mask, loss_mask_sum)
    for name, t in (("logprobs", logprobs), ("old_logprobs", old_logprobs), ("advantages", advantages)):
        if t.dtype != torch.float32:
            raise RlxError(f"{name} must be float32 to keep numerical stability")
    n_adv, chunks = _loss_geometry(logprobs, logprob_type, action_dim, reward_type)
    if old_logprobs.numel() != logprobs.numel():
        raise RlxError("old_logprobs must have the shape of logprobs")
    if advantages.numel() != n_adv:
        raise RlxError(f"advantages has {advantages.numel()} elements, expected {n_adv} for {logprob_type}")
    if has_critic:
        if values is None or prev_values is None or returns is None or value_clip is None or huber_delta is None:
            raise RlxError("actor_critic loss needs values, prev_values, returns, value_clip and huber_delta")
        for name, t in (("values", values), ("prev_values", prev_values), ("returns", returns)):
            if t.numel() != n_adv:
                raise RlxError(f"{name} has {t.numel()} elements, expected {n_adv}")
            if t.dtype != torch.float32:
                raise RlxError(f"{name} must be float32")
    m8 = _as_u8(loss_mask)
    if m8 is not None and m8.numel() != n_adv:
        raise RlxError(f"loss_mask has {m8.numel()} elements, expected {n_adv}")
    msum = None
    if loss_mask_sum is not None:
        if loss_mask_sum.numel() != n_adv:
            msum = loss_mask_sum.expand(advantages.shape if loss_mask_sum.dim() == advantages.dim() else loss_mask_sum.shape)
        else:
            msum = loss_mask_sum
        msum = msum.to(torch.int64).contiguous()
        if msum.numel() != n_adv:
            raise RlxError(f"loss_mask_sum has {msum.numel()} elements, expected {n_adv}")
    if clip_ratio_c is not None and not clip_ratio_c > 1.0:
        raise AssertionError("clip_ratio_c must be greater than 1.0")
    p = make_ppo_params(logprob_type=logprob_type, action_dim=action_dim, chunks=chunks, clip_ratio_low=clip_ratio_low,
                        clip_ratio_high=clip_ratio_high, value_clip=value_clip, huber_delta=huber_delta,
                        max_episode_steps=max_episode_steps, clip_ratio_c=clip_ratio_c, clip_log_ratio_min=clip_log_ratio_min,
                        clip_log_ratio_max=clip_log_ratio_max, critic_warmup=critic_warmup, has_critic=has_critic,
                        reward_type=reward_type)
    v = values.contiguous() if has_critic else None
    if decoupled is not None:
        dp, prox, versions = _decoupled_params(p, logprobs, **decoupled)
        return _DecoupledLossFn.apply(logprobs, v, old_logprobs.contiguous(), advantages.contiguous(),
                                      prev_values.contiguous() if has_critic else None,
                                      returns.contiguous() if has_critic else None, m8, msum, prox, versions, dp, n_adv)
    return _PpoLossFn.apply(logprobs, v, old_logprobs.contiguous(), advantages.contiguous(),
                            prev_values.contiguous() if has_critic else None,
                            returns.contiguous() if has_critic else None, m8, msum, p, n_adv)


def _decoupled_params(p: PpoLossParams, logprobs, proximal_logprobs=None, versions=None, current_version=None,
                      behave_weight_threshold=None):
    """rlx_decoupled_loss_params + the two optional raw tensors (losses.py:68-89: which proximal policy applies)."""
    dp = _lib.DecoupledLossParams()
    dp.ppo = p
    for name, t in (("proximal_logprobs", proximal_logprobs), ("versions", versions)):
        if t is not None and t.numel() != logprobs.numel():
            raise RlxError(f"{name} must have the shape of logprobs")
    if proximal_logprobs is not None:
        if proximal_logprobs.dtype != torch.float32:
            raise AssertionError("proximal_logprobs must be float32 to keep numerical stability")
        dp.proximal_mode = _lib.PROX_GIVEN
    elif versions is None or current_version is None:
        dp.proximal_mode = _lib.PROX_IS_OLD
    else:
        dp.proximal_mode = _lib.PROX_FROM_VERSIONS
    dp.current_version = float(current_version) if current_version is not None else 0.0
    dp.use_behave_threshold = int(behave_weight_threshold is not None)
    dp.behave_weight_threshold = float(behave_weight_threshold) if behave_weight_threshold is not None else 0.0
    prox = proximal_logprobs.contiguous() if proximal_logprobs is not None else None
    ver = versions.float().contiguous() if (versions is not None and current_version is not None) else None
    return dp, prox, ver


class _DecoupledLossFn(torch.autograd.Function):
    """rlx_decoupled_loss_fwd + the shared rlx_ppo_loss_bwd."""

    @staticmethod
    def forward(ctx, logprobs, values, old_logprobs, advantages, prev_values, returns, loss_mask, loss_mask_sum,
                proximal_logprobs, versions, dp, n_adv: int):
        lib = _lib.load()

        def launch(lp, g_lp, g_v, out, ws):
            _lib.launch("rlx_decoupled_loss_fwd", lp.device, lp, old_logprobs, proximal_logprobs, versions, advantages, values,
                        prev_values, returns, loss_mask, loss_mask_sum, n_adv, dp, g_lp, g_v, out, ws, ws.numel())

        return _loss_forward(ctx, logprobs, values, dp.ppo, n_adv, lib.rlx_decoupled_loss_workspace_bytes, launch)

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        d_lp, d_v = _PpoLossFn.backward(ctx, grad_loss, _grad_out)[:2]
        return (d_lp, d_v) + (None,) * 10


def make_ppo_params(*, logprob_type="action_level", action_dim=8, chunks=1, clip_ratio_low, clip_ratio_high,
                    value_clip=None, huber_delta=None, max_episode_steps=None, clip_ratio_c=None,
                    clip_log_ratio_min=None, clip_log_ratio_max=None, critic_warmup=False, has_critic=True,
                    reward_type=None) -> PpoLossParams:
    p = PpoLossParams()
    p.ratio_lo, p.ratio_hi = float(1.0 - clip_ratio_low), float(1.0 + clip_ratio_high)
    p.clip_ratio_c = float(clip_ratio_c) if clip_ratio_c is not None else 0.0
    p.use_dual_clip = int(clip_ratio_c is not None)
    p.clip_log_ratio_min = float(clip_log_ratio_min) if clip_log_ratio_min is not None else 0.0
    p.clip_log_ratio_max = float(clip_log_ratio_max) if clip_log_ratio_max is not None else 0.0
    p.use_clip_log_ratio_min, p.use_clip_log_ratio_max = int(clip_log_ratio_min is not None), int(clip_log_ratio_max is not None)
    p.value_clip = float(value_clip) if has_critic else 0.0
    p.huber_delta = float(huber_delta) if has_critic else 0.0
    p.has_critic, p.critic_warmup = int(has_critic), int(bool(critic_warmup))
    p.max_episode_steps = int(max_episode_steps) if max_episode_steps else 0
    p.raw_per_adv, p.sub_per_adv, p.metric_unbroadcast = _adv_geometry(logprob_type, action_dim, chunks, reward_type)
    return p


def ppo_loss_fwd_raw(params: PpoLossParams, n_adv: int, logprobs, old_logprobs, advantages, values, prev_values, returns,
                     loss_mask, loss_mask_sum, g_logp, g_value, out, workspace):
    """Allocation-free launcher (all tensors caller-owned) used by the learner's fused/graph-captured step."""
    _lib.launch("rlx_ppo_loss_fwd", logprobs.device, logprobs, old_logprobs, advantages, values, prev_values, returns, loss_mask,
                loss_mask_sum, n_adv, params, g_logp, g_value, out, workspace, workspace.numel())


def ppo_loss_bwd_raw(params: PpoLossParams, n_adv: int, g_logp, g_value, out, grad_out, d_logprobs, d_values):
    _lib.launch("rlx_ppo_loss_bwd", g_logp.device, g_logp, g_value, out, grad_out, d_logprobs, d_values, n_adv, params.raw_per_adv,
                params.sub_per_adv)


# --------------------------------------------------------------------------------------------
# a19c  on-policy distillation (OPD): advantage and loss
# --------------------------------------------------------------------------------------------
_OPD_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def _opd_rows(t: torch.Tensor, num_action_chunks: int) -> torch.Tensor:
    """[T, ..., C*A] -> a [T, ..., C, A] view whose rows (dim 0) hold contiguous elements; only a tensor whose rows are not
    contiguous is copied.  Dtypes other than f32 / bf16 / f16 are converted to f32 first, as ``.float()`` would."""
    if t.dtype not in _OPD_DTYPES:
        t = t.float()
    v = t.reshape(*t.shape[:-1], num_action_chunks, -1)
    if v.shape[0] > 0 and not v[0].is_contiguous():
        v = v.contiguous()
    return v


def opd_advantages(teacher_logprobs: torch.Tensor, prev_logprobs: torch.Tensor, num_action_chunks: int,
                   rows: Optional[int] = None) -> torch.Tensor:
    """(teacher.float() - prev.float()) reshaped to [..., C, A], first ``rows`` entries of dim 0 (all when None): ONE launch of
    rlx_opd_advantages, f32 out.  The caller has checked shapes (algorithms/advantages.py holds the reference's asserts)."""
    dev = _dev(teacher_logprobs, prev_logprobs)
    t = _opd_rows(teacher_logprobs, int(num_action_chunks))
    p = _opd_rows(prev_logprobs, int(num_action_chunks))
    if t.shape != p.shape:
        raise RlxError(f"teacher_logprobs {tuple(teacher_logprobs.shape)} and prev_logprobs {tuple(prev_logprobs.shape)} differ")
    n_rows = t.shape[0] if rows is None else int(rows)
    if not 0 <= n_rows <= t.shape[0]:
        raise RlxError(f"rows={n_rows} outside [0, {t.shape[0]}]")
    out = torch.empty((n_rows,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
    inner = out[0].numel() if n_rows > 0 else 0
    _lib.launch("rlx_opd_advantages", dev, t, _OPD_DTYPES[t.dtype], t.stride(0) if t.dim() else 1, p, _OPD_DTYPES[p.dtype],
                p.stride(0) if p.dim() else 1, n_rows, inner, out)
    return out


def _opd_div(t: Optional[torch.Tensor], n: int, action_dim: int, name: str) -> int:
    """1 when ``t`` holds one entry per loss element, ``action_dim`` when it holds one per row of action_dim elements."""
    if t is None:
        return 1
    if t.numel() == n:
        return 1
    if action_dim >= 1 and t.numel() * action_dim == n:
        return action_dim
    raise RlxError(f"{name} has {t.numel()} elements; expected {n} or {n // max(action_dim, 1)}")


class _OpdLossFn(torch.autograd.Function):
    """rlx_opd_loss_fwd / rlx_opd_loss_bwd.  The advantages are a stop-gradient input (``advantages.detach()``)."""

    @staticmethod
    def forward(ctx, logprobs, advantages, loss_mask, mask_div, loss_mask_sum, msum_div, max_episode_steps: int):
        lib = _lib.load()
        dev = logprobs.device
        lp = logprobs.contiguous()
        n = lp.numel()
        i64 = int(loss_mask_sum is not None and loss_mask_sum.dtype == torch.int64)
        out = torch.empty((_lib.OPD_OUT_FLOATS,), dtype=torch.float32, device=dev)
        ws = _lib.workspace(dev, lib.rlx_opd_loss_workspace_bytes(n))
        _lib.launch("rlx_opd_loss_fwd", dev, lp, advantages, loss_mask, mask_div, loss_mask_sum, msum_div, i64, n, max_episode_steps,
                    out, ws, ws.numel())
        ctx.save_for_backward(advantages, loss_mask, loss_mask_sum if loss_mask_sum is not None else out, out)
        ctx.geom = (mask_div, msum_div, i64, n, max_episode_steps, loss_mask_sum is not None)
        ctx.lp_shape = logprobs.shape
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        adv, mask, msum, out = ctx.saved_tensors
        mask_div, msum_div, i64, n, mes, has_msum = ctx.geom
        dev = adv.device
        go = grad_loss.to(dtype=torch.float32).contiguous()
        d_lp = torch.empty((n,), dtype=torch.float32, device=dev)
        _lib.launch("rlx_opd_loss_bwd", dev, adv, mask, mask_div, msum if has_msum else None, msum_div, i64, n, mes, out, go, d_lp)
        return d_lp.view(ctx.lp_shape), None, None, None, None, None, None


def opd_loss(logprobs: torch.Tensor, advantages: torch.Tensor, loss_mask: torch.Tensor, *, action_dim: int,
             loss_mask_sum: Optional[torch.Tensor] = None, max_episode_steps: Optional[int] = None):
    """OPD actor loss agg(-logprobs * advantages.detach(), loss_mask) and its metrics in ONE forward launch pair (stream pass +
    finalize) and ONE backward launch.  ``logprobs`` f32 with a last dimension of ``action_dim`` elements per row (any leading
    shape); ``advantages`` f32 of the same element count; ``loss_mask`` / ``loss_mask_sum`` with one entry per element or one
    per row (the reference's broadcast of a last dimension of 1).  ``max_episode_steps`` selects masked_mean_ratio with
    ratio = loss_mask_sum / max_episode_steps, else masked_mean.  Returns (loss 0-dim with grad, out f32[8] on device, see
    _lib.OPD_OUT_NAMES)."""
    _dev(logprobs, advantages, loss_mask, loss_mask_sum)
    for name, t in (("logprobs", logprobs), ("advantages", advantages)):
        if t.dtype != torch.float32:
            raise RlxError(f"{name} must be float32 to keep numerical stability")
    n = logprobs.numel()
    if advantages.numel() != n:
        raise RlxError(f"advantages has {advantages.numel()} elements, expected {n}")
    if loss_mask is None:
        raise RlxError("opd_loss needs loss_mask")
    mes = 0
    if max_episode_steps is not None:
        if int(max_episode_steps) != max_episode_steps or int(max_episode_steps) <= 0:
            raise RlxError(f"max_episode_steps must be a positive integer, got {max_episode_steps!r}")
        if loss_mask_sum is None:
            raise RlxError("max_episode_steps needs loss_mask_sum")
        mes = int(max_episode_steps)
    m8 = _as_u8(loss_mask)
    mdiv = _opd_div(m8, n, int(action_dim), "loss_mask")
    msum, sdiv = None, 1
    if loss_mask_sum is not None and mes > 0:
        msum = loss_mask_sum if loss_mask_sum.dtype in (torch.int64, torch.float32) else loss_mask_sum.float()
        msum = msum.contiguous()
        sdiv = _opd_div(msum, n, int(action_dim), "loss_mask_sum")
    return _OpdLossFn.apply(logprobs, advantages.detach().contiguous(), m8, mdiv, msum, sdiv, mes)


# --------------------------------------------------------------------------------------------
# a16  shuffle gather
# --------------------------------------------------------------------------------------------
def gather_rows(fields: list, index: torch.Tensor, outs: Optional[list] = None) -> list:
    """fields: list of [N, ...] contiguous HIP tensors; returns [t[index] for t in fields] (one launch per 16)."""
    if not fields:
        return []
    dev = _dev(index, *fields)
    if index.dtype != torch.int64:
        raise RlxError("index must be int64")
    idx = index.contiguous()
    n = idx.numel()
    for t in fields:
        if not t.is_contiguous():
            raise RlxError("gather_rows needs contiguous fields")
    if outs is None:
        outs = [torch.empty((n, *t.shape[1:]), dtype=t.dtype, device=dev) for t in fields]
    for lo in range(0, len(fields), _lib.GATHER_MAX_FIELDS):
        chunk = list(zip(fields, outs))[lo:lo + _lib.GATHER_MAX_FIELDS]
        arr = (GatherField * len(chunk))()
        k = 0
        for src, dst in chunk:
            row_bytes = src.element_size() * (src.numel() // max(src.shape[0], 1))
            if row_bytes == 0:
                continue
            arr[k].src, arr[k].dst, arr[k].row_bytes = src.data_ptr(), dst.data_ptr(), row_bytes
            k += 1
        if k and n:
            _lib.launch("rlx_gather_rows", dev, arr, k, idx, n)
    return outs


# --------------------------------------------------------------------------------------------
# s1 / s2  the async-PPO rollout store: version statistics, segmented gather
# --------------------------------------------------------------------------------------------
def version_stats_workspace(device) -> tuple:
    """(device struct, workspace) for version_stats: allocate once, reuse for every added trajectory."""
    lib = _lib.load()
    out = torch.zeros(ctypes.sizeof(_lib.VersionStats) // 8, dtype=torch.int64, device=device)
    ws = torch.empty(lib.rlx_version_stats_workspace_bytes(0) // 8, dtype=torch.int64, device=device)
    return out, ws


def version_stats(versions: torch.Tensor, base: int, n_bins: int = _lib.VERSION_STATS_MAX_BINS, workspace: Optional[tuple] = None
                  ) -> _lib.VersionStats:
    """One pass over a trajectory's contiguous f32 ``versions`` -> the host copy of rlx_version_stats_out (min, n, the exact sum
    of the rounded versions, count[k] of round(v) - base == k, below / above the bin range).  One read-back."""
    dev = _dev(versions)
    if versions.dtype != torch.float32 or not versions.is_contiguous():
        raise RlxError("version_stats needs a contiguous float32 tensor")
    out, ws = workspace if workspace is not None else version_stats_workspace(dev)
    _lib.launch("rlx_version_stats", dev, versions, versions.numel(), int(base), int(n_bins), out, ws, ws.numel() * 8)
    host = out.cpu()  # the one read-back per added trajectory
    return _lib.VersionStats.from_buffer_copy(host.numpy().tobytes())


def gather_rows_segmented(slot_fields: list, index: Optional[torch.Tensor], outs: Optional[list] = None) -> list:
    """``slot_fields``: per field the list of its S per-slot tensors, each a contiguous ``[t_rows, B_s, ...]`` block (B_s the same
    for every field of a slot; t_rows may differ between fields).  -> per field ``cat(slots, dim=1).flatten(0, 1)[index]``, or with
    ``index=None`` the concatenation itself ``[t_rows, sum B, ...]`` -- one launch per 16 fields, no concatenated intermediate."""
    if not slot_fields:
        return []
    S = len(slot_fields[0])
    if not 1 <= S <= _lib.STORE_MAX_SLOTS:
        raise RlxError(f"gather_rows_segmented takes 1..{_lib.STORE_MAX_SLOTS} slots, got {S}")
    dev = _dev(index, *[t for f in slot_fields for t in f])
    envs = [int(t.shape[1]) for t in slot_fields[0]]
    sum_b = sum(envs)
    for f in slot_fields:
        if len(f) != S or [int(t.shape[1]) for t in f] != envs:
            raise RlxError("gather_rows_segmented: every field needs the same per-slot env counts")
        for t in f:
            if not t.is_contiguous() or t.shape[0] != f[0].shape[0] or t.shape[2:] != f[0].shape[2:] or t.dtype != f[0].dtype:
                raise RlxError("gather_rows_segmented needs contiguous [t_rows, B_s, ...] slots of one row shape and dtype per field")
    if index is not None:
        if index.dtype != torch.int64:
            raise RlxError("index must be int64")
        index = index.contiguous()
        n = index.numel()
    else:
        n = 0
    if outs is None:
        outs = [torch.empty((n, *f[0].shape[2:]) if index is not None else (f[0].shape[0], sum_b, *f[0].shape[2:]),
                            dtype=f[0].dtype, device=dev) for f in slot_fields]
    env_table = (ctypes.c_int64 * S)(*envs)
    for lo in range(0, len(slot_fields), _lib.GATHER_MAX_FIELDS):
        chunk = list(zip(slot_fields, outs))[lo:lo + _lib.GATHER_MAX_FIELDS]
        arr, tables, k = (_lib.SegField * len(chunk))(), [], 0
        for f, dst in chunk:
            row_bytes = f[0].element_size() * (f[0][0, 0].numel() if f[0].dim() > 2 else 1)
            if row_bytes == 0 or f[0].shape[0] == 0:
                continue
            if not dst.is_contiguous():
                raise RlxError("gather_rows_segmented needs contiguous destinations")
            tables.append((ctypes.c_void_p * S)(*[t.data_ptr() for t in f]))
            arr[k].srcs, arr[k].dst, arr[k].row_bytes, arr[k].t_rows = tables[-1], dst.data_ptr(), row_bytes, f[0].shape[0]
            k += 1
        if k and (index is None or n):
            _lib.launch("rlx_gather_rows_segmented", dev, arr, k, S, env_table, index, n)
    return outs


# --------------------------------------------------------------------------------------------
# a23  clip + AdamW on flat buffers
# --------------------------------------------------------------------------------------------
def actor_param_ranges(layout: MlpLayout) -> list:
    """Element ranges of the flat buffer that belong to the ACTOR network (actor_logstd; backbone.* + actor_mean.*): the
    gradients a decoupled ppo_step leaves in sum form."""
    A = int(layout.act_dim)
    lo = int(layout.off_w[1][0])
    hi = max(int(layout.off_w[1][3]) + A * int(layout.hidden), (int(layout.off_b[1][3]) + A) if int(layout.off_b[1][3]) >= 0 else 0)
    return [(int(layout.off_logstd), int(layout.off_logstd) + A), (lo, hi)]


def deferred_actor_scale(layout: MlpLayout, rows: torch.Tensor, groups: int) -> dict:
    """``deferred`` argument of the AdamW wrappers behind decoupled ppo_steps: ``rows`` = the [groups, PPO_OUT_FLOATS] metric rows
    of the optimizer step's micro-batches (contiguous); their out[RLX_PPO_ACTOR_GRAD_SCALE] scale the actor ranges."""
    assert rows.dim() == 2 and rows.shape[0] == groups and rows.stride(1) == 1
    return dict(scale=rows[0, _lib.PPO_ACTOR_GRAD_SCALE:], stride=int(rows.stride(0)), groups=int(groups),
                ranges=actor_param_ranges(layout), keep=rows)


def adamw_sync_words(n: int, device) -> Optional[torch.Tensor]:
    """Zeroed ``rlx_adamw_params.sync_words`` buffer for a set of ``n`` parameters: with it the optimizer step is ONE launch
    (slab sum, norm, clip and AdamW around a device-side exchange of the norm partials) where the plan allows it.  One buffer per
    parameter set, reused by every step on it.  ``RLX_ADAMW_ONE_LAUNCH=0`` -> None (the two-launch form)."""
    if os.environ.get("RLX_ADAMW_ONE_LAUNCH", "1") == "0":
        return None
    return torch.zeros((int(_lib.load().rlx_adamw_sync_words(int(n))),), dtype=torch.int64, device=device)


def check_adamw_sync(sync: Optional[torch.Tensor], grad_norm: float) -> bool:
    """Call with a step's gradient norm once it is on the host.  A NON-FINITE norm is either a real one (the step was skipped, like
    the reference's) or the one-launch optimizer step reporting that one of its workgroups never became resident within its 2 s
    bound (word 1 of the sync buffer, sticky) -- another process or stream holds part of the GPU.  Steps since then were skipped
    as a whole (the kernel reads the word first thing), so the parameters are those of the last complete step.  Returns True in
    that case, after a warning: the caller drops ``sync`` (and whatever captured its pointer) and continues on two launches."""
    import math
    if sync is None or math.isfinite(grad_norm):
        return False
    if int(sync[1].item()) == 0:
        return False
    import warnings
    warnings.warn("the one-launch optimizer step timed out waiting for its own workgroups (another process or stream holds part of "
                  "this GPU); the optimizer steps since then were skipped. Continuing with the two-launch form "
                  "(RLX_ADAMW_ONE_LAUNCH=0 selects it from the start).", RuntimeWarning, stacklevel=2)
    return True


def _set_deferred(p: AdamwParams, deferred: Optional[dict]):
    if deferred is None:
        return
    p.deferred_scale = deferred["scale"].data_ptr()
    p.deferred_stride, p.deferred_groups = int(deferred["stride"]), int(deferred["groups"])
    for k, (b, e) in enumerate(deferred["ranges"]):
        p.deferred_range[k][0], p.deferred_range[k][1] = int(b), int(e)


def _adamw_params(groups: list, slabs: int, step: int, *, betas, eps, weight_decay, max_grad_norm, grad_scale, tile_layout, tiles,
                  deferred, sync) -> AdamwParams:
    """rlx_adamw_params for ``groups`` = [(begin, end, lr), ...] over ``slabs`` gradient slabs."""
    if len(groups) > _lib.ADAMW_MAX_GROUPS:
        raise RlxError("too many parameter groups")
    p = AdamwParams()
    p.beta1, p.beta2, p.eps, p.weight_decay = float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    p.max_grad_norm = float(max_grad_norm) if max_grad_norm else 0.0
    p.step, p.n_groups, p.grad_partials, p.grad_scale = int(step), len(groups), int(slabs), float(grad_scale)
    for k, (b, e, lr) in enumerate(groups):
        p.groups[k] = AdamwGroup(int(b), int(e), float(lr))
    if tile_layout is not None and tiles is not None:  # keep the fragment-tile weight image in step with the parameters
        p.tile_layout, p.tiles = ctypes.pointer(tile_layout), tiles.data_ptr()
        p.tiles_bf16 = int(tiles.dtype == torch.bfloat16)
    _set_deferred(p, deferred)
    if sync is not None:
        p.sync_words = sync.data_ptr()
    return p


def clip_adamw_step_(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor,
                     groups: list, step: int, *, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
                     max_grad_norm: float = 0.5, grad_scale: float = 1.0, stats: Optional[torch.Tensor] = None,
                     step_state: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                     tile_layout: Optional[MlpLayout] = None, tiles: Optional[torch.Tensor] = None,
                     deferred: Optional[dict] = None, sync: Optional[torch.Tensor] = None):
    """In-place clip_grad_norm_ + AdamW over flat f32 buffers.  groups = [(begin, end, lr), ...].
    sync: ``adamw_sync_words(n, device)`` -> the one-launch form.
    grads may be [n] or [slabs, n] (split-K slabs, summed first).  Returns stats f32[2] = (norm, applied).
    step_state: device int32[2] keeping the step count on the device (then ``step`` is ignored).
    deferred: see ``deferred_actor_scale`` (scales read on the device while the slabs are summed)."""
    lib = _lib.load()
    dev = _dev(params, grads, exp_avg, exp_avg_sq)
    n = params.numel()
    for t in (params, grads, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RlxError("clip_adamw_step_ needs contiguous float32 buffers")
    if grads.numel() % max(n, 1) != 0 or grads.numel() < n or exp_avg.numel() != n or exp_avg_sq.numel() != n:
        raise RlxError("buffer sizes do not match")
    if stats is None:
        stats = torch.empty((2,), dtype=torch.float32, device=dev)
    if n == 0:  # nothing to update and nothing to launch (the library returns before it writes stats, too)
        return stats
    p = _adamw_params(groups, grads.numel() // n, step, betas=betas, eps=eps, weight_decay=weight_decay,
                      max_grad_norm=max_grad_norm, grad_scale=grad_scale, tile_layout=tile_layout, tiles=tiles, deferred=deferred,
                      sync=sync)
    ws_bytes = lib.rlx_adamw_workspace_bytes(n)
    ws = workspace if workspace is not None and workspace.numel() >= ws_bytes else _lib.workspace(dev, ws_bytes)
    if step_state is not None and (step_state.dtype != torch.int32 or step_state.numel() < 2):
        raise RlxError("step_state must be int32[2]")
    _lib.launch("rlx_clip_adamw_step", dev, params, grads, exp_avg, exp_avg_sq, n, p, stats, step_state, ws, ws.numel())
    return stats


def bootstrap_rewards_(rewards: torch.Tensor, flags: torch.Tensor, bootstrap_values: torch.Tensor, gamma: float):
    """rewards [B,C] f32 in place: r[:, -1] += gamma * V[:, 0] where flags[:, -1]  (env_worker.py:744-758)."""
    dev = _dev(rewards, flags, bootstrap_values)
    if rewards.dim() != 2 or not rewards.is_contiguous() or rewards.dtype != torch.float32:
        raise RlxError("rewards must be a contiguous float32 [B, C] tensor")
    f8 = _as_u8(flags)
    v = _as_f32(bootstrap_values, "bootstrap_values")
    B, C = rewards.shape
    if tuple(f8.shape) != (B, C) or v.shape[0] != B:
        raise RlxError("flags must be [B,C] and bootstrap_values [B, >=1]")
    _lib.launch("rlx_bootstrap_rewards", dev, rewards, f8, v, B, C, v.numel() // max(B, 1), float(gamma))
    return rewards


def store_env_rows_(rewards, terminations, truncations, reward_row, done_row, termination_row, truncation_row):
    """One env step's [B, C] outputs -> buffer rows; dones = terminations | truncations.  One launch."""
    dev = _dev(rewards, terminations, truncations, reward_row, done_row, termination_row, truncation_row)
    r = _as_f32(rewards, "rewards")
    te, tr = _as_u8(terminations), _as_u8(truncations)
    n = r.numel()
    for t in (te, tr, reward_row, done_row, termination_row, truncation_row):
        if t.numel() != n or not t.is_contiguous():
            raise RlxError("store_env_rows_: all tensors must be contiguous with rewards' number of elements")
    _lib.launch("rlx_store_env_rows", dev, r, te, tr, reward_row, done_row, termination_row, truncation_row, n)


# --------------------------------------------------------------------------------------------
# a1-a5, a17  MLP policy kernels (flat parameter buffer + layout descriptor)
# --------------------------------------------------------------------------------------------
def mlp_pack(params: torch.Tensor, layout: MlpLayout, packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    dev = _dev(params)
    nbytes = lib.rlx_mlp_packed_bytes(byref(layout))
    if packed is None:
        packed = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    _lib.launch("rlx_mlp_pack", dev, params, layout, packed)
    return packed


def _rollout_outputs(out: Optional[tuple], M: int, layout: MlpLayout, dev, who: str) -> tuple:
    """(action [M,act], logprob [M,act], value [M,val]): the caller's rows checked (e.g. the trajectory buffer's), or new ones."""
    if out is None:
        action = torch.empty((M, layout.act_dim), dtype=torch.float32, device=dev)
        return action, torch.empty_like(action), torch.empty((M, layout.val_dim), dtype=torch.float32, device=dev)
    for t, w in zip(out, (layout.act_dim, layout.act_dim, layout.val_dim)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != M * w:
            raise RlxError(f"{who}: out tensors must be contiguous float32 of the right size")
    return tuple(out)


def mlp_rollout(params: torch.Tensor, packed: torch.Tensor, layout: MlpLayout, states: torch.Tensor,
                eps: Optional[torch.Tensor], out: Optional[tuple] = None):
    """states [M,D], eps [M,act]|None -> (action [M,act], logprob [M,act], value [M,val])."""
    dev = _dev(params, packed, states, eps)
    st = _as_f32(states, "states")
    M = st.shape[0]
    if st.dim() != 2 or st.shape[1] != layout.obs_dim:
        raise RlxError(f"states must be [M, {layout.obs_dim}], got {tuple(st.shape)}")
    e = _as_f32(eps, "eps")
    if e is not None and tuple(e.shape) != (M, layout.act_dim):
        raise RlxError(f"eps must be [{M}, {layout.act_dim}]")
    action, logprob, value = _rollout_outputs(out, M, layout, dev, "mlp_rollout")
    _lib.launch("rlx_mlp_rollout", dev, params, packed, layout, st, e, M, action, logprob, value)
    return action, logprob, value


def mlp_value(params, packed, layout: MlpLayout, states, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Value head only: states [M,D] -> value [M,val]."""
    dev = _dev(params, packed, states)
    st = _as_f32(states, "states")
    M = st.shape[0]
    value = out if out is not None else torch.empty((M, layout.val_dim), dtype=torch.float32, device=dev)
    _lib.launch("rlx_mlp_value", dev, params, packed, layout, st, M, value)
    return value


def sum_slabs(grads: torch.Tensor, out: Optional[torch.Tensor] = None, deferred: Optional[dict] = None) -> torch.Tensor:
    """[slabs, n] -> [n].  ``deferred`` (deferred_actor_scale): the slabs are micro-batch groups behind decoupled ppo_steps."""
    dev = _dev(grads)
    slabs, n = grads.shape
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=dev)
    if deferred is not None:
        p = AdamwParams()
        _set_deferred(p, deferred)
        _lib.launch("rlx_sum_slabs_deferred", dev, grads, n, slabs, out, p)
    else:
        _lib.launch("rlx_sum_slabs", dev, grads, n, slabs, out)
    return out


def mlp_train_fwd(params, packed, layout: MlpLayout, states, action, acts: Optional[torch.Tensor] = None,
                  out: Optional[tuple] = None):
    """-> (logprob, entropy [M,act], value [M,val], mean [M,act], acts [2,3,M,256])."""
    dev = _dev(params, packed, states, action)
    st, ac = _as_f32(states, "states"), _as_f32(action, "action")
    M = st.shape[0]
    if tuple(ac.shape) != (M, layout.act_dim):
        raise RlxError(f"action must be [{M}, {layout.act_dim}], got {tuple(ac.shape)}")
    if out is not None:
        logprob, entropy, value, mean = out
    else:
        logprob = torch.empty((M, layout.act_dim), dtype=torch.float32, device=dev)
        entropy = torch.empty_like(logprob)
        mean = torch.empty_like(logprob)
        value = torch.empty((M, layout.val_dim), dtype=torch.float32, device=dev)
    if acts is None or acts.numel() != 6 * M * 256:
        acts = torch.empty((2, 3, M, 256), dtype=torch.float32, device=dev)
    _lib.launch("rlx_mlp_train_fwd", dev, params, packed, layout, st, ac, M, logprob, entropy, value, mean, acts)
    return logprob, entropy, value, mean, acts


def mlp_bwd_slabs(m: int) -> int:
    return _lib.load().rlx_mlp_bwd_slabs(int(m))


def mlp_train_bwd(params, packed, layout: MlpLayout, states, action, mean, acts, d_logprob, d_entropy, d_value,
                  grads: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """-> grads [slabs, n_params] (split-K slabs; every element written)."""
    lib = _lib.load()
    dev = _dev(params, packed, states, action, mean, acts, d_logprob, d_entropy, d_value)
    M = states.shape[0]
    slabs = lib.rlx_mlp_bwd_slabs(M) if grads is None else grads.shape[0]
    if grads is None:
        grads = torch.empty((slabs, layout.n_params), dtype=torch.float32, device=dev)
    ws_bytes = lib.rlx_mlp_bwd_workspace_bytes(byref(layout), M)
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = _lib.workspace(dev, ws_bytes)
    dl, dv = _as_f32(d_logprob, "d_logprob"), _as_f32(d_value, "d_value")
    de = _as_f32(d_entropy, "d_entropy")
    _lib.launch("rlx_mlp_train_bwd", dev, params, packed, layout, states, action, mean, acts, dl, de, dv, M, grads, slabs, workspace,
                workspace.numel())
    return grads


# --------------------------------------------------------------------------------------------
# SAC (Q-head) MLP policy: the model calls (sac_mlp.hip)
# --------------------------------------------------------------------------------------------
def sac_actor_fwd(params, layout: SacActorLayout, states, eps: Optional[torch.Tensor], action_scale: float, action_bias: float,
                  train: bool):
    """-> (action, logprob [M, A'], acts [3,M,256] | None, aux [2,M,A'] | None); ``train`` keeps what backward needs."""
    dev = _dev(params, states, eps)
    st, ep = _as_f32(states, "states"), _as_f32(eps, "eps")
    M, A = st.shape[0], layout.act_dim
    if st.dim() != 2 or st.shape[1] != layout.obs_dim:
        raise RlxError(f"states must be [M, {layout.obs_dim}], got {tuple(st.shape)}")
    if ep is not None and tuple(ep.shape) != (M, A):
        raise RlxError(f"eps must be [{M}, {A}], got {tuple(ep.shape)}")
    action = torch.empty((M, A), dtype=torch.float32, device=dev)
    logprob = torch.empty_like(action)
    acts = torch.empty((3, M, 256), dtype=torch.float32, device=dev) if train else None
    aux = torch.empty((2, M, A), dtype=torch.float32, device=dev) if train else None
    _lib.launch("rlx_sac_actor_fwd", dev, params, layout, st, ep, M, action_scale, action_bias, action, logprob, acts, aux)
    return action, logprob, acts, aux


def sac_actor_bwd(params, layout: SacActorLayout, states, eps, acts, aux, d_action, d_logprob, action_scale: float):
    """-> grads [slabs, n_params] (split-K slabs; every element written)."""
    lib = _lib.load()
    dev = _dev(params, states, eps, acts, aux, d_action, d_logprob)
    M = states.shape[0]
    slabs = lib.rlx_sac_actor_bwd_slabs(M)
    grads = torch.empty((slabs, layout.n_params), dtype=torch.float32, device=dev)
    workspace = _lib.workspace(dev, lib.rlx_sac_actor_bwd_workspace_bytes(byref(layout), M))
    _lib.launch("rlx_sac_actor_bwd", dev, params, layout, states, eps, acts, aux, _as_f32(d_action, "d_action"),
                _as_f32(d_logprob, "d_logprob"), M, action_scale, grads, slabs, workspace, workspace.numel())
    return grads


def sac_q_fwd(params, layout: SacQLayout, states, actions, train: bool):
    """-> (q [M, 2*out], acts [2,3,2,M,256] | None, rstd [2,3,M] | None)."""
    dev = _dev(params, states, actions)
    st, ac = _as_f32(states, "states"), _as_f32(actions, "actions")
    M = st.shape[0]
    if st.dim() != 2 or st.shape[1] != layout.obs_dim:
        raise RlxError(f"states must be [M, {layout.obs_dim}], got {tuple(st.shape)}")
    if tuple(ac.shape) != (M, layout.act_dim):
        raise RlxError(f"actions must be [{M}, {layout.act_dim}], got {tuple(ac.shape)}")
    q = torch.empty((M, 2 * layout.out_dim), dtype=torch.float32, device=dev)
    acts = torch.empty((2, 3, 2, M, 256), dtype=torch.float32, device=dev) if train else None
    rstd = torch.empty((2, 3, M), dtype=torch.float32, device=dev) if train else None
    _lib.launch("rlx_sac_q_fwd", dev, params, layout, st, ac, M, q, acts, rstd)
    return q, acts, rstd


def sac_q_bwd(params, layout: SacQLayout, states, actions, acts, rstd, d_q, want_params: bool, want_actions: bool):
    """-> (grads [slabs, n_params] | None, d_actions [M, A'] | None): only what is asked for is computed."""
    lib = _lib.load()
    dev = _dev(params, states, actions, acts, rstd, d_q)
    M = states.shape[0]
    slabs = lib.rlx_sac_q_bwd_slabs(M)
    grads = torch.empty((slabs, layout.n_params), dtype=torch.float32, device=dev) if want_params else None
    d_actions = torch.empty((M, layout.act_dim), dtype=torch.float32, device=dev) if want_actions else None
    workspace = _lib.workspace(dev, lib.rlx_sac_q_bwd_workspace_bytes(byref(layout), M))
    _lib.launch("rlx_sac_q_bwd", dev, params, layout, states, actions, acts, rstd, _as_f32(d_q, "d_q"), M, grads, slabs, d_actions,
                workspace, workspace.numel())
    return grads, d_actions


# --------------------------------------------------------------------------------------------
# offline IQL for the MLP policy: networks, loss legs, target update (iql_mlp.hip)
# --------------------------------------------------------------------------------------------
def _rows(t, width: int, name: str):
    t = _as_f32(t, name)
    if t.dim() != 2 or t.shape[1] != width:
        raise RlxError(f"{name} must be [M, {width}], got {tuple(t.shape)}")
    return t


def _f32_vec(t, n: int, name: str):
    t = _as_f32(t, name)
    if t.numel() != n:
        raise RlxError(f"{name} must hold {n} elements, got {tuple(t.shape)}")
    return t


def iql_mlp_fwd(params, layout: IqlMlpLayout, xa, xb=None, xa2=None, train: bool = False, actions=None):
    """-> (out [n_nets, M, out_dim], acts [n_nets, n_hidden, M, 256] | None, logprob [M] | None).  ``xa2``: further rows behind
    ``xa``'s in the same launch; ``actions`` [M, out_dim]: the actor's log-prob of them; ``train`` keeps what backward needs."""
    dev = _dev(params, xa, xb, xa2, actions)
    a1 = _rows(xa, layout.in_a, "xa")
    a2 = _rows(xa2, layout.in_a, "xa2") if xa2 is not None else None
    M = a1.shape[0] + (a2.shape[0] if a2 is not None else 0)
    b = _rows(xb, layout.in_b, "xb") if xb is not None else None
    ac = _rows(actions, layout.out_dim, "actions") if actions is not None else None
    for t, name in ((b, "xb"), (ac, "actions")):
        if t is not None and t.shape[0] != M:
            raise RlxError(f"{name} must have {M} rows, got {t.shape[0]}")
    out = torch.empty((layout.n_nets, M, layout.out_dim), dtype=torch.float32, device=dev)
    acts = torch.empty((layout.n_nets, layout.n_hidden, M, 256), dtype=torch.float32, device=dev) if train else None
    logprob = torch.empty((M,), dtype=torch.float32, device=dev) if ac is not None else None
    _lib.launch("rlx_iql_mlp_fwd", dev, _as_f32(params, "params"), layout, a1, a1.shape[0], a2, b, M, out, acts, ac, logprob)
    return out, acts, logprob


def iql_mlp_bwd(params, layout: IqlMlpLayout, xa, xb, acts, d_out, d_logstd=None, grads=None, workspace=None):
    """-> grads [slabs, n_params] (split-K slabs; every element written)."""
    lib = _lib.load()
    dev = _dev(params, xa, xb, acts, d_out, d_logstd)
    a1 = _rows(xa, layout.in_a, "xa")
    M = a1.shape[0]
    b = _rows(xb, layout.in_b, "xb") if xb is not None else None
    do = _f32_vec(d_out, layout.n_nets * M * layout.out_dim, "d_out")
    ac = _f32_vec(acts, layout.n_nets * layout.n_hidden * M * 256, "acts")
    dl = _f32_vec(d_logstd, layout.out_dim, "d_logstd") if d_logstd is not None else None
    slabs = lib.rlx_iql_mlp_bwd_slabs(M) if grads is None else grads.shape[0]
    if grads is None:
        grads = torch.empty((slabs, layout.n_params), dtype=torch.float32, device=dev)
    ws_bytes = lib.rlx_iql_mlp_bwd_workspace_bytes(byref(layout), M)
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = _lib.workspace(dev, ws_bytes)
    _lib.launch("rlx_iql_mlp_bwd", dev, _as_f32(params, "params"), layout, a1, b, ac, do, dl, M, grads, slabs, workspace,
                workspace.numel())
    return grads


def iql_value_loss(q_target, v, expectile: float, metrics):
    """q_target [2, M] (the target twin's out), v [M] -> (d_v [M], q_min [M]); metrics[value_loss, v] written."""
    dev = _dev(q_target, v, metrics)
    M = v.numel()
    qt, vv, mt = _f32_vec(q_target, 2 * M, "q_target"), _as_f32(v, "v"), _f32_vec(metrics, 8, "metrics")
    d_v, q_min = torch.empty((M,), dtype=torch.float32, device=dev), torch.empty((M,), dtype=torch.float32, device=dev)
    _lib.launch("rlx_iql_value_loss", dev, qt, vv, M, float(expectile), d_v, q_min, mt)
    return d_v, q_min


def iql_actor_loss(params, layout: IqlMlpLayout, q_min, new_v, logprob, mean, actions, temperature: float, metrics):
    """-> (d_mean [M, A], d_logstd [A], d_lp [M]); metrics[actor_loss, adv_mean, adv_std] written."""
    dev = _dev(params, q_min, new_v, logprob, mean, actions, metrics)
    M, A = logprob.numel(), layout.out_dim
    qm, nv, lp = _f32_vec(q_min, M, "q_min"), _f32_vec(new_v, M, "new_v"), _as_f32(logprob, "logprob")
    mu, ac, mt = _f32_vec(mean, M * A, "mean"), _f32_vec(actions, M * A, "actions"), _f32_vec(metrics, 8, "metrics")
    d_lp = torch.empty((M,), dtype=torch.float32, device=dev)
    d_mean = torch.empty((M, A), dtype=torch.float32, device=dev)
    d_logstd = torch.empty((A,), dtype=torch.float32, device=dev)
    _lib.launch("rlx_iql_actor_loss", dev, _as_f32(params, "params"), layout, qm, nv, lp, mu, ac, M, float(temperature), d_lp, d_mean,
                d_logstd, mt)
    return d_mean, d_logstd, d_lp


def iql_logprob_bwd(params, layout: IqlMlpLayout, mean, actions, d_lp):
    """The actor's log-prob backward alone, from a given d_lp [M] -> (d_mean [M, A], d_logstd [A])."""
    dev = _dev(params, mean, actions, d_lp)
    M, A = d_lp.numel(), layout.out_dim
    mu, ac, dl = _f32_vec(mean, M * A, "mean"), _f32_vec(actions, M * A, "actions"), _as_f32(d_lp, "d_lp")
    d_mean = torch.empty((M, A), dtype=torch.float32, device=dev)
    d_logstd = torch.empty((A,), dtype=torch.float32, device=dev)
    _lib.launch("rlx_iql_actor_loss", dev, _as_f32(params, "params"), layout, None, None, None, mu, ac, M, 1.0, dl, d_mean, d_logstd,
                None)
    return d_mean, d_logstd


def iql_critic_loss(q, next_v, rewards, masks, gamma: float, metrics):
    """q [2, M] -> d_q [2, M]; metrics[critic_loss, q1, q2] written."""
    dev = _dev(q, next_v, rewards, masks, metrics)
    M = next_v.numel()
    qq, nv, mt = _f32_vec(q, 2 * M, "q"), _as_f32(next_v, "next_v"), _f32_vec(metrics, 8, "metrics")
    r, mk = _f32_vec(rewards, M, "rewards"), _f32_vec(masks, M, "masks")
    d_q = torch.empty((2, M), dtype=torch.float32, device=dev)
    _lib.launch("rlx_iql_critic_loss", dev, qq, nv, r, mk, M, float(gamma), d_q, mt)
    return d_q


def soft_update_(target, online, tau: float):
    """target <- target * (1 - tau); target <- target + tau * online, over flat f32 buffers, in place."""
    dev = _dev(target, online)
    for t in (target, online):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RlxError("soft_update_ needs contiguous float32 buffers")
    if target.numel() != online.numel():
        raise RlxError("buffer sizes do not match")
    _lib.launch("rlx_soft_update", dev, target, online, target.numel(), float(tau))
    return target


# --------------------------------------------------------------------------------------------
# fused hot launches (ppo_step.hip)
# --------------------------------------------------------------------------------------------
def mlp_pack_tiles(params: torch.Tensor, layout: MlpLayout, tiles: Optional[torch.Tensor] = None, bf16: bool = False) -> torch.Tensor:
    """Fragment-tile weight image the fused launches stream (rebuild after every change of ``params``); f32 or bf16."""
    lib = _lib.load()
    dev = _dev(params)
    dt = torch.bfloat16 if bf16 else torch.float32
    n = lib.rlx_mlp_tiles_bytes_for(byref(layout), 1 if bf16 else 0) // (2 if bf16 else 4)  # the f32 image is opaque (include/rlx.h)
    if tiles is None or tiles.dtype != dt or tiles.numel() != n:
        tiles = torch.empty((n,), dtype=dt, device=dev)
    _lib.launch("rlx_mlp_pack_tiles_bf16" if bf16 else "rlx_mlp_pack_tiles", dev, params, layout, tiles)
    return tiles


def mlp_rollout_step(params: torch.Tensor, tiles: torch.Tensor, layout: MlpLayout, states: Optional[torch.Tensor],
                     eps: Optional[torch.Tensor], out: Optional[tuple] = None, states_copy: Optional[torch.Tensor] = None,
                     value_jobs: tuple = ()):
    """ONE launch: policy job on ``states`` (-> action, logprob, value rows in ``out``) plus up to two value-only jobs
    ``dict(states=[m,D], values=[m,val]|None, rewards=[m,C]|None, flags=[m,C] bool, gamma=float)``: values <- V(states),
    rewards[:, -1] += gamma * V(states)[:, 0] where flags[:, -1].  With ``env=(rewards, terminations, truncations)`` and
    ``rows=(done_row, termination_row, truncation_row)`` the job also stores the env step's outputs into the buffer rows
    (``rewards`` is then the destination row; the flag is done, or truncation with ``flag_is_truncation``)."""
    dev = _dev(params, states, eps, *[j["states"] for j in value_jobs])
    st = RolloutStep()
    st.params, st.tiles, st.layout = params.data_ptr(), tiles.data_ptr(), ctypes_pointer(layout)
    st.bf16 = int(tiles.dtype == torch.bfloat16)  # the tile image's element type selects the MFMA operand precision
    action = logprob = value = None
    if states is not None:
        s_ = _as_f32(states, "states")
        M = s_.shape[0]
        if s_.dim() != 2 or s_.shape[1] != layout.obs_dim:
            raise RlxError(f"states must be [M, {layout.obs_dim}], got {tuple(s_.shape)}")
        e = _as_f32(eps, "eps")
        if e is not None and tuple(e.shape) != (M, layout.act_dim):
            raise RlxError(f"eps must be [{M}, {layout.act_dim}]")
        action, logprob, value = _rollout_outputs(out, M, layout, dev, "mlp_rollout_step")
        if states_copy is not None and (states_copy.dtype != torch.float32 or not states_copy.is_contiguous()
                                        or states_copy.numel() != s_.numel()):
            raise RlxError("mlp_rollout_step: states_copy must be a contiguous float32 tensor shaped like states")
        st.states, st.eps, st.m = s_.data_ptr(), None if e is None else e.data_ptr(), M
        st.action, st.logprob, st.value = action.data_ptr(), logprob.data_ptr(), value.data_ptr()
        st.states_copy = None if states_copy is None else states_copy.data_ptr()
    if len(value_jobs) > 2:
        raise RlxError("at most two value jobs per launch")
    keep = []
    for k, j in enumerate(value_jobs):
        js = _as_f32(j["states"], "value job states")
        m = js.shape[0]
        vals, rew, flags = j.get("values"), j.get("rewards"), j.get("flags")
        if vals is not None and (vals.dtype != torch.float32 or not vals.is_contiguous() or vals.numel() != m * layout.val_dim):
            raise RlxError("value job: values must be contiguous float32 [m, val_dim]")
        chunk = 1
        env = j.get("env")
        if rew is not None:
            if rew.dim() != 2 or rew.dtype != torch.float32 or not rew.is_contiguous() or rew.shape[0] != m:
                raise RlxError("value job: rewards must be a contiguous float32 [m, C] tensor")
            chunk = rew.shape[1]
            if env is None:
                flags = _as_u8(flags)
                if flags is None or tuple(flags.shape) != tuple(rew.shape):
                    raise RlxError("value job: flags must be a bool tensor shaped like rewards")
        keep += [js, flags]
        vj = st.value_jobs[k]
        vj.states, vj.m = js.data_ptr(), m
        vj.values, vj.rewards, vj.flags = (None if t is None else t.data_ptr() for t in (vals, rew, flags))
        vj.chunk, vj.gamma = chunk, float(j.get("gamma", 1.0))
        if env is not None:
            if rew is None:
                raise RlxError("value job: env rows need the destination reward row")
            er, ete, etr = _as_f32(env[0], "env rewards"), _as_u8(env[1]), _as_u8(env[2])
            rows = [t if t.dtype == torch.uint8 else t.view(torch.uint8) for t in j["rows"]]
            for t in (er, ete, etr, *rows):
                if t.numel() != rew.numel() or not t.is_contiguous():
                    raise RlxError("value job: env tensors and rows must be contiguous with the reward row's number of elements")
            keep += [er, ete, etr, *rows]
            vj.env_rewards, vj.env_terminations, vj.env_truncations = er.data_ptr(), ete.data_ptr(), etr.data_ptr()
            vj.done_row, vj.termination_row, vj.truncation_row = (t.data_ptr() for t in rows)
            vj.flag_is_truncation = int(bool(j.get("flag_is_truncation", False)))
    st.n_value_jobs = len(value_jobs)
    _lib.launch("rlx_mlp_rollout_step", dev, st)
    return action, logprob, value


def ctypes_pointer(layout: MlpLayout):
    return ctypes.pointer(layout)


def ppo_step_slabs(layout: MlpLayout, m: int, bf16: bool = False) -> int:
    """Split-K slabs `grads` must hold for a minibatch of m rows at the given operand precision."""
    return _lib.load().rlx_ppo_step_slabs_for(byref(layout), int(m), 1 if bf16 else 0)


def ppo_step_workspace_bytes(layout: MlpLayout, m: int) -> int:
    return _lib.load().rlx_ppo_step_workspace_bytes(byref(layout), int(m))


def _ppo_step_args(params, layout, loss, mbatch, grads, out_row, workspace, grad_out, tiles, bf16, decoupled) -> PpoStepArgs:
    a = PpoStepArgs()
    a.params, a.layout, a.loss = params.data_ptr(), ctypes_pointer(layout), ctypes_pointer(loss)
    st = mbatch["states"]
    a.states, a.action = st.data_ptr(), mbatch["action"].data_ptr()
    a.old_logprobs, a.advantages = mbatch["prev_logprobs"].data_ptr(), mbatch["advantages"].data_ptr()
    has_critic = bool(loss.has_critic)
    a.prev_values = mbatch["prev_values"].data_ptr() if has_critic else None
    a.returns = mbatch["returns"].data_ptr() if has_critic else None
    lm, lms = mbatch.get("loss_mask"), mbatch.get("loss_mask_sum")
    a.loss_mask = None if lm is None else lm.data_ptr()
    a.loss_mask_sum = None if lms is None else lms.data_ptr()
    a.m, a.grad_out = st.shape[0], float(grad_out)
    a.grads, a.slabs, a.out = grads.data_ptr(), grads.shape[0], out_row.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    a.tiles, a.bf16 = None if tiles is None else tiles.data_ptr(), int(bool(bf16))
    if tiles is not None and (tiles.dtype == torch.bfloat16) != bool(bf16):
        raise RlxError("ppo_step: the tile image's dtype does not match the requested precision")
    if decoupled is not None:  # dict(params=DecoupledLossParams, proximal_logprobs, versions, current_version_dev): see decoupled_step_args
        a.decoupled = ctypes.addressof(decoupled["params"])
        for name in ("proximal_logprobs", "versions", "current_version_dev"):
            if decoupled.get(name) is not None:
                setattr(a, name, decoupled[name].data_ptr())
    return a


def decoupled_step_args(loss: PpoLossParams, mbatch: dict, *, current_version, behave_weight_threshold,
                        current_version_dev: Optional[torch.Tensor] = None) -> dict:
    """``decoupled`` argument of ppo_step / PreparedPpoStep: which proximal policy applies (losses.py:68-89) from what the
    micro-batch carries -- ``proximal_logprobs`` (given), else ``versions`` (+ a current version: interpolated), else the
    behaviour policy itself.  ``current_version_dev`` (one device float) is read when the launch executes."""
    dp, prox, ver = _decoupled_params(loss, mbatch["prev_logprobs"], mbatch.get("proximal_logprobs"), mbatch.get("versions"),
                                      current_version, behave_weight_threshold)
    for name, t, src in (("proximal_logprobs", prox, mbatch.get("proximal_logprobs")), ("versions", ver, mbatch.get("versions"))):
        if t is not None and t.data_ptr() != src.data_ptr():
            raise RlxError(f"decoupled ppo_step needs contiguous float32 {name}")
    return dict(params=dp, proximal_logprobs=prox, versions=ver, current_version_dev=current_version_dev)


def ppo_step(params: torch.Tensor, layout: MlpLayout, loss: PpoLossParams, mbatch: dict, grads: torch.Tensor,
             out_row: torch.Tensor, workspace: torch.Tensor, grad_out: float = 1.0, tiles: Optional[torch.Tensor] = None,
             bf16: bool = False, decoupled: Optional[dict] = None):
    """forward + loss + backward of one micro-batch (two launches).  ``mbatch``: states, action, prev_logprobs,
    advantages [, prev_values, returns, loss_mask, loss_mask_sum] as flattened minibatch views; ``grads`` [slabs, n].
    ``decoupled`` (decoupled_step_args): the asynchronous-PPO actor loss; the actor network's gradients then leave in sum
    form (include/rlx.h) -- pass ``deferred_actor_scale`` of the row(s) to the AdamW step."""
    dev = params.device
    a = _ppo_step_args(params, layout, loss, mbatch, grads, out_row, workspace, grad_out, tiles, bf16, decoupled)
    _lib.launch("rlx_ppo_step", dev, a)


# --------------------------------------------------------------------------------------------
# prepared launches: marshal once, replay with one ctypes call (the update loop issues ~500 launches per iteration;
# building the argument structs in Python every time costs more host time than the kernels take on the GPU)
# --------------------------------------------------------------------------------------------
class PreparedPpoStep:
    """rlx_ppo_step with every pointer fixed (persistent minibatch views and workspaces)."""

    def __init__(self, params, layout, loss, mbatch, grads, out_row, workspace, grad_out=1.0, tiles=None, bf16=False,
                 decoupled=None):
        self._lib = _lib.load()
        self._keep = (params, layout, loss, dict(mbatch), grads, out_row, workspace, tiles, decoupled)
        self._args = _ppo_step_args(params, layout, loss, mbatch, grads, out_row, workspace, grad_out, tiles, bf16, decoupled)
        self._ref = byref(self._args)

    def __call__(self, stream: int):
        rc = self._lib.rlx_ppo_step(self._ref, stream)
        if rc:
            _lib.check(rc, "rlx_ppo_step")


class PreparedAdamw:
    """rlx_clip_adamw_step with every pointer fixed; ``stats`` is this step's (norm, applied) row."""

    def __init__(self, params, grads, exp_avg, exp_avg_sq, groups, *, betas, eps, weight_decay, max_grad_norm, grad_scale,
                 stats, step_state, workspace, tile_layout=None, tiles=None, xgmi=None, grad_flat=None, deferred=None,
                 deferred_in_caller=False, sync=None):
        """``xgmi`` (scheduler.xgmi.XgmiAllReduce) + ``grad_flat`` [n]: rlx_xgmi_clip_adamw_step instead -- ``grads`` are this
        rank's slabs, the reduced gradient (scaled by grad_scale = 1 / world_size) lands in grad_flat, then clip + AdamW."""
        self._lib = _lib.load()
        n = params.numel()
        # one GPU: slab sum + norm + clip + AdamW as one launch.  Over xGMI: the exchange INSIDE that launch, when the communicator's
        # start-up validation has passed it (XgmiAllReduce.one_launch); otherwise the exchange's launch chain with its hand-shakes
        p = _adamw_params(groups, grads.numel() // n, 0, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                          grad_scale=grad_scale, tile_layout=tile_layout, tiles=tiles, deferred=deferred,
                          sync=sync if (xgmi is None or getattr(xgmi, "one_launch", False)) else None)
        self.deferred = deferred  # (a data-parallel caller that collapses the slabs itself -- RCCL path -- applies it there)
        if deferred is not None and deferred_in_caller:
            p.deferred_scale = None  # the caller sums (and scales: sum_slabs(deferred=...)) the slabs in front of its all-reduce
        self._keep = (params, grads, exp_avg, exp_avg_sq, stats, step_state, workspace, tile_layout, tiles, p, xgmi, grad_flat, deferred, sync)
        if xgmi is not None:
            self._fn, self._name = self._lib.rlx_xgmi_clip_adamw_step, "rlx_xgmi_clip_adamw_step"
            self._argv = (xgmi.handle, params.data_ptr(), grads.data_ptr(), grad_flat.data_ptr(), exp_avg.data_ptr(),
                          exp_avg_sq.data_ptr(), n, byref(p), stats.data_ptr(), step_state.data_ptr(), workspace.data_ptr(),
                          workspace.numel())
        else:
            self._fn, self._name = self._lib.rlx_clip_adamw_step, "rlx_clip_adamw_step"
            self._argv = (params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n, byref(p),
                          stats.data_ptr(), step_state.data_ptr(), workspace.data_ptr(), workspace.numel())

    def __call__(self, stream: int):
        rc = self._fn(*self._argv, stream)
        if rc:
            _lib.check(rc, self._name)
