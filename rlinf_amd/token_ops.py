"""Tensor-level launchers of the token tier (include/rlx.h t1-t5): per-token log-prob / entropy over
vocabulary logits, the reasoning learner's micro-batch loss, GRPO / multi-turn GRPO advantages in the [bsz, seq] layout and
the dynamic-batch loss scales.

Same rules as ``ops.py``: HIP tensors only, no eager path; torch supplies memory, the stream and autograd
plumbing.
"""

from __future__ import annotations

import os

from typing import Optional

import torch

from . import _lib
from ._lib import RlxError, TokenLossParams, TokenRows
from .ops import _as_f32, _as_u8, _dev, make_ppo_params

_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16}


def _rows_of(logits: torch.Tensor, temperature: float, round_outputs: bool):
    """Describe ``logits[..., V]`` to the kernels without copying when it is a [bsz, rows, V] slice of a larger
    buffer (the reference's ``logits[:, -resp-1:-1, :]``); anything else is made contiguous."""
    if logits.dtype not in _DTYPES:
        raise RlxError(f"logits must be float32 or bfloat16 (got {logits.dtype})")
    if logits.dim() < 2:
        raise RlxError("logits must be [..., vocab]")
    vocab = logits.shape[-1]
    n = logits.numel() // max(vocab, 1)
    rows = TokenRows()
    rows.vocab, rows.dtype = vocab, _DTYPES[logits.dtype]
    rows.n_tokens, rows.temperature, rows.round_outputs = n, float(temperature), int(bool(round_outputs))
    if logits.dim() == 3 and logits.stride(-1) == 1 and logits.stride(1) >= vocab and not logits.is_contiguous():
        rows.rows_per_seq, rows.seq_stride, rows.row_stride = logits.shape[1], logits.stride(0), logits.stride(1)
        return logits, rows
    logits = logits.contiguous()
    rows.rows_per_seq, rows.seq_stride, rows.row_stride = max(n, 1), 0, vocab
    return logits, rows


def token_logprob_fwd(logits: torch.Tensor, labels: torch.Tensor, temperature: float = 1.0, with_entropy: bool = False,
                      round_outputs: bool = False):
    """-> (logprob, entropy or None, lse), each f32 of shape ``logits.shape[:-1]``."""
    dev = _dev(logits, labels)
    if labels.dtype != torch.int64:
        raise RlxError(f"labels must be int64 (got {labels.dtype})")
    if labels.numel() != logits.numel() // max(logits.shape[-1], 1):
        raise RlxError("labels must have one entry per logits row")
    if not temperature > 0:
        raise RlxError("temperature must be positive")
    lead = logits.shape[:-1]
    x, rows = _rows_of(logits, temperature, round_outputs)
    lab = labels.contiguous()
    logprob = torch.empty(lead, dtype=torch.float32, device=dev)
    lse = torch.empty(lead, dtype=torch.float32, device=dev)
    entropy = torch.empty(lead, dtype=torch.float32, device=dev) if with_entropy else None
    _lib.launch("rlx_token_logprob_fwd", dev, x, lab, rows, logprob, entropy, lse)
    return logprob, entropy, lse


def token_logprob_bwd(logits: torch.Tensor, labels: torch.Tensor, lse: torch.Tensor, entropy: Optional[torch.Tensor],
                      d_logprob: torch.Tensor, d_entropy: Optional[torch.Tensor], temperature: float = 1.0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient w.r.t. the UNSCALED logits, in their dtype.  ``out`` may be ``logits`` itself (in-place)."""
    dev = _dev(logits, labels, lse, d_logprob)
    x, rows = _rows_of(logits, temperature, False)
    if out is None:
        out = torch.empty(logits.shape, dtype=logits.dtype, device=dev)
    if out.shape != logits.shape or out.dtype != logits.dtype:
        raise RlxError("d_logits must match logits in shape and dtype")
    if rows.seq_stride == 0:  # flat contiguous logits: rows are addressed as i * vocab
        if not out.is_contiguous():
            raise RlxError("a strided d_logits needs logits of the same [bsz, rows, V] slicing")
        dss, drs = 0, rows.vocab
    elif out.dim() == 3 and out.stride(-1) == 1 and out.stride(1) >= rows.vocab:
        dss, drs = out.stride(0), out.stride(1)  # dense [bsz, rows, V] or a slice like the logits
    else:
        raise RlxError("d_logits must be contiguous or a [bsz, rows, V] slice like logits")
    lab, lse_f, ent = labels.contiguous(), _as_f32(lse, "lse"), _as_f32(entropy, "entropy")
    d_lp, d_ent = _as_f32(d_logprob, "d_logprob"), _as_f32(d_entropy, "d_entropy")
    _lib.launch("rlx_token_logprob_bwd", dev, x, lab, rows, lse_f, ent, d_lp, d_ent, out, dss, drs)
    return out


class _TokenLogprobFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, temperature, with_entropy, round_outputs, inplace_grad, window):
        # ``window`` = (start, stop) along dim 1 of a [bsz, S, V] tensor: the kernels address that slice in place and the backward
        # hands autograd a gradient for the WHOLE tensor (zeros outside the window, written by two fills of the outside rows) --
        # what SliceBackward would build as zeros(logits.shape) + a strided copy of the window gradient: 2 x [bsz, S, V] of
        # traffic and one more allocation per micro-batch.
        view = logits if window is None else logits[:, window[0]:window[1], :]
        logprob, entropy, lse = token_logprob_fwd(view, labels, temperature, with_entropy, round_outputs)
        ctx.save_for_backward(logits, labels, lse, entropy if with_entropy else lse)
        ctx.cfg = (float(temperature), bool(with_entropy), bool(inplace_grad), window)
        ctx.mark_non_differentiable(lse)
        if with_entropy:
            return logprob, entropy, lse
        return logprob, lse.new_empty(0), lse

    @staticmethod
    def backward(ctx, d_logprob, d_entropy, _d_lse):
        logits, labels, lse, entropy = ctx.saved_tensors
        temperature, with_entropy, inplace, window = ctx.cfg
        if d_logprob is None:
            d_logprob = torch.zeros_like(lse)
        use_ent = with_entropy and d_entropy is not None
        if window is None:
            dx = token_logprob_bwd(logits, labels, lse, entropy if use_ent else None, d_logprob.contiguous(),
                                   d_entropy.contiguous() if use_ent else None, temperature, out=logits if inplace else None)
            return dx, None, None, None, None, None, None
        full = logits if inplace else torch.empty_like(logits)
        token_logprob_bwd(logits[:, window[0]:window[1], :], labels, lse, entropy if use_ent else None, d_logprob.contiguous(),
                          d_entropy.contiguous() if use_ent else None, temperature, out=full[:, window[0]:window[1], :])
        full[:, :window[0], :].zero_()
        full[:, window[1]:, :].zero_()
        return full, None, None, None, None, None, None


class _PackedLogprobFn(torch.autograd.Function):
    """Packed-stream scoring with the unpack fused into the stores (include/rlx.h, rlx_token_logprob_fwd_packed)."""

    @staticmethod
    def forward(ctx, logits, labels, lp_dst, ent_dst, bsz, response_len, temperature, with_entropy, round_outputs, inplace_grad):
        dev = _dev(logits, labels, lp_dst)
        x, rows = _rows_of(logits, temperature, round_outputs)
        n = rows.n_tokens
        if labels.dtype != torch.int64 or labels.numel() != n or lp_dst.numel() != n or lp_dst.dtype != torch.int32:
            raise RlxError("packed scoring needs int64 labels and int32 destination maps with one entry per packed row")
        lab = labels.contiguous().reshape(-1)
        logprob = torch.zeros((bsz, response_len), dtype=torch.float32, device=dev)   # pad_val 0 of unpack_sequences
        entropy = torch.zeros((bsz, response_len), dtype=torch.float32, device=dev) if with_entropy else None
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.launch("rlx_token_logprob_fwd_packed", dev, x, lab, rows, lp_dst, ent_dst if with_entropy else None, logprob, entropy, lse)
        ctx.save_for_backward(logits, lab, lse, lp_dst, ent_dst, entropy if with_entropy else lse)
        ctx.cfg = (float(temperature), bool(with_entropy), bool(inplace_grad))
        ctx.out_shape = (int(bsz), int(response_len))
        return (logprob, entropy) if with_entropy else (logprob, lse.new_empty(0))

    @staticmethod
    def backward(ctx, d_logprob, d_entropy):
        logits, lab, lse, lp_dst, ent_dst, entropy = ctx.saved_tensors
        temperature, with_entropy, inplace = ctx.cfg
        dev = logits.device
        # the upstream gradients stay in their unpacked [bsz, response_len] shape: the kernel follows the forward's maps (a packed row
        # that fed nothing is written as zeros without being read)
        use_ent = with_entropy and d_entropy is not None
        if d_logprob is None:
            d_logprob = torch.zeros(ctx.out_shape, dtype=torch.float32, device=dev)
        x, rows = _rows_of(logits, temperature, False)
        out = logits if inplace else torch.empty(logits.shape, dtype=logits.dtype, device=dev)
        if rows.seq_stride == 0:
            if not out.is_contiguous():  # (a transposed lm_head output with inplace_grad: the forward scored a contiguous copy,
                #                          so there is no buffer of the logits' own layout to overwrite -- a fresh gradient instead)
                out = torch.empty(logits.shape, dtype=logits.dtype, device=dev)
            dss, drs = 0, rows.vocab
        else:
            dss, drs = out.stride(0), out.stride(1)
        d_lp, d_ent = _as_f32(d_logprob, "d_logprob"), _as_f32(d_entropy, "d_entropy") if use_ent else None
        _lib.launch("rlx_token_logprob_bwd_packed", dev, x, lab, rows, lse, entropy if use_ent else None, lp_dst,
                    ent_dst if use_ent else None, d_lp, d_ent, out, dss, drs)
        return out, None, None, None, None, None, None, None, None, None


def packed_token_logprobs(logits: torch.Tensor, packed_input_ids: torch.Tensor, idx_starts, idx_ends, *, max_seq_len_unpack: int,
                          response_len: int, eos_token_id: int, temperature: float = 1.0, with_entropy: bool = False,
                          round_outputs: bool = False, inplace_grad: bool = False):
    """``unpack_fsdp_logprobs`` + ``unpack_sequences`` of the entropy + the ``[:, -response_len:]`` slices in one scoring launch
    (rlinf/hybrid_engines/fsdp/utils.py:980-1022, rlinf/workers/actor/fsdp_actor_worker.py:482-503): ``logits`` [1, L, V] (or [L, V])
    of a packed stream, ``packed_input_ids`` [1, L] -> differentiable (logprobs [bsz, response_len], entropy or None), zeros where
    the reference pads."""
    from .hybrid_engines.fsdp.utils import unpack_index_maps
    ids = packed_input_ids.reshape(-1)
    L = ids.numel()
    if logits.numel() // max(logits.shape[-1], 1) != L:
        raise RlxError("packed logits and input_ids disagree on the stream length")
    labels = torch.cat([ids[1:], ids.new_full((1,), int(eos_token_id))]).to(torch.int64)  # token t + 1, eos behind the last (:1000-1009)
    lp_dst, ent_dst = unpack_index_maps(idx_starts, idx_ends, L, int(max_seq_len_unpack), int(response_len), logits.device)
    out = _PackedLogprobFn.apply(logits, labels, lp_dst, ent_dst, len(idx_starts), int(response_len), float(temperature),
                                 bool(with_entropy), bool(round_outputs), bool(inplace_grad))
    return (out[0], out[1]) if with_entropy else (out[0], None)


def token_logprobs(logits: torch.Tensor, labels: torch.Tensor, *, temperature: float = 1.0, with_entropy: bool = False,
                   round_outputs: bool = False, inplace_grad: bool = False, window: Optional[tuple] = None):
    """Differentiable (logprob, entropy or None).  ``inplace_grad`` lets the backward pass overwrite the logits
    buffer with its gradient (saves one [tokens, vocab] allocation; only valid when nothing else reads the logits
    afterwards, which holds for an lm_head output feeding only this op).  ``window`` = (start, stop): ``logits`` is the model's
    whole [bsz, S, V] output and only rows start..stop-1 of every sequence are scored (``labels`` [bsz, stop - start]); the
    gradient comes back for the whole tensor, zero outside the window."""
    if window is not None:
        if logits.dim() != 3 or not (0 <= window[0] < window[1] <= logits.shape[1]):
            raise RlxError(f"window {window} does not fit logits of shape {tuple(logits.shape)}")
        window = (int(window[0]), int(window[1]))
    logprob, entropy, _ = _TokenLogprobFn.apply(logits, labels, float(temperature), bool(with_entropy),
                                                bool(round_outputs), bool(inplace_grad), window)
    return logprob, (entropy if with_entropy else None)


# ---------------------------------------------------------------------------------------------------------
def make_token_loss_params(*, loss_agg: str, clip_ratio_low: float, clip_ratio_high: float, clip_ratio_c=None,
                           clip_log_ratio_min=None, clip_log_ratio_max=None, critic_warmup=False,
                           fast_path_zero_loss_mask=False, kl_penalty_type: Optional[str] = None, kl_beta: float = 0.0,
                           use_entropy: bool = False, entropy_bonus: float = 0.0) -> TokenLossParams:
    if loss_agg not in _lib.LOSS_AGG:
        raise ValueError(f"Unsupported loss aggregation method: {loss_agg}")
    if kl_penalty_type not in _lib.KL_TYPE:
        raise NotImplementedError(f"kl_penalty type {kl_penalty_type!r}")
    if clip_ratio_c is not None and not clip_ratio_c > 1.0:
        raise AssertionError("clip_ratio_c must be greater than 1.0")
    p = TokenLossParams()
    p.ppo = make_ppo_params(clip_ratio_low=clip_ratio_low, clip_ratio_high=clip_ratio_high, clip_ratio_c=clip_ratio_c,
                            clip_log_ratio_min=clip_log_ratio_min, clip_log_ratio_max=clip_log_ratio_max,
                            critic_warmup=critic_warmup, has_critic=False, action_dim=1)
    p.loss_agg = _lib.LOSS_AGG[loss_agg]
    p.fast_path_zero_loss_mask = int(bool(fast_path_zero_loss_mask))
    p.kl_type = _lib.KL_TYPE[kl_penalty_type] if kl_beta > 0 else 0
    p.kl_beta = float(kl_beta)
    p.use_entropy, p.entropy_bonus = int(bool(use_entropy)), float(entropy_bonus)
    return p


class _TokenLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logprobs, entropy, old_logprobs, advantages, ref_logprobs, loss_mask, params: TokenLossParams):
        lib = _lib.load()
        dev = logprobs.device
        bsz, seq = logprobs.shape
        g_lp = torch.empty((bsz, seq), dtype=torch.float32, device=dev)
        needs_gent = bool(params.use_entropy) and entropy is not None and params.entropy_bonus != 0.0
        g_ent = torch.empty((bsz, seq), dtype=torch.float32, device=dev) if needs_gent else None
        row_w = torch.empty((bsz,), dtype=torch.float32, device=dev)
        out = torch.empty((_lib.TOK_OUT_FLOATS,), dtype=torch.float32, device=dev)
        ws = _lib.workspace(dev, lib.rlx_token_loss_workspace_bytes(bsz, seq))
        _lib.launch("rlx_token_loss_fwd", dev, logprobs, old_logprobs, advantages, ref_logprobs, entropy, loss_mask, bsz, seq, params,
                    g_lp, g_ent, row_w, out, ws, ws.numel())
        ctx.save_for_backward(g_lp, g_ent if needs_gent else row_w, row_w)
        ctx.needs_gent = needs_gent
        ctx.ent_given = entropy is not None
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_loss, _grad_out):
        g_lp, g_ent, row_w = ctx.saved_tensors
        dev = g_lp.device
        bsz, seq = g_lp.shape
        go = grad_loss.to(dtype=torch.float32).contiguous()
        d_lp = torch.empty_like(g_lp)
        d_ent = torch.empty_like(g_lp) if ctx.needs_gent else None
        _lib.launch("rlx_token_loss_bwd", dev, g_lp, g_ent if ctx.needs_gent else None, row_w, go, d_lp, d_ent, bsz, seq)
        return d_lp, d_ent, None, None, None, None, None


def token_loss(logprobs: torch.Tensor, old_logprobs: torch.Tensor, advantages: torch.Tensor,
               loss_mask: Optional[torch.Tensor], params: TokenLossParams, *, entropy: Optional[torch.Tensor] = None,
               ref_logprobs: Optional[torch.Tensor] = None):
    """-> (loss scalar with grad into logprobs/entropy, out f32[16] in rlx_tok_out order)."""
    dev = _dev(logprobs, old_logprobs, advantages, loss_mask, entropy, ref_logprobs)
    if logprobs.dim() != 2:
        raise RlxError(f"logprobs must be [bsz, seq]; got {tuple(logprobs.shape)}")
    for name, t in (("logprobs", logprobs), ("old_logprobs", old_logprobs), ("advantages", advantages)):
        if t.dtype != torch.float32:
            raise AssertionError(f"{name} must be float32 to keep numerical stability")
        if t.shape != logprobs.shape:
            raise RlxError(f"{name} shape {tuple(t.shape)} != logprobs shape {tuple(logprobs.shape)}")
    del dev
    mask = _as_u8(loss_mask)
    if mask is not None and mask.shape != logprobs.shape:
        raise RlxError("loss_mask must be [bsz, seq]")
    return _TokenLossFn.apply(logprobs.contiguous(), _as_f32(entropy, "entropy"), old_logprobs.contiguous(),
                              advantages.contiguous(), _as_f32(ref_logprobs, "ref_logprobs"), mask, params)


def grpo_seq_adv(rewards: torch.Tensor, loss_mask: torch.Tensor, group_size: int, eps: float = 1e-6) -> torch.Tensor:
    """rewards [bsz] f32, loss_mask [bsz, seq] bool -> advantages [bsz, seq] f32."""
    dev = _dev(rewards, loss_mask)
    if loss_mask.dim() != 2 or rewards.numel() != loss_mask.shape[0]:
        raise RlxError("grpo_seq_adv: rewards [bsz], loss_mask [bsz, seq]")
    bsz, seq = loss_mask.shape
    if group_size < 1 or bsz % group_size != 0:
        raise RlxError(f"bsz {bsz} is not a multiple of group_size {group_size}")
    r = _as_f32(rewards.reshape(-1), "rewards")
    m = _as_u8(loss_mask)
    adv = torch.empty((bsz, seq), dtype=torch.float32, device=dev)
    _lib.launch("rlx_grpo_seq_adv", dev, r, m, adv, bsz, seq, int(group_size), float(eps))
    return adv


def reinpp_seq_adv(rewards: torch.Tensor, loss_mask: torch.Tensor, logprob: Optional[torch.Tensor] = None,
                   ref_logprob: Optional[torch.Tensor] = None, kl_beta: float = 0.0, kl_penalty_type: Optional[str] = None
                   ) -> torch.Tensor:
    """Reinforce++ (no group baseline): rewards [bsz] f32, loss_mask [bsz, seq] bool, logprob / ref_logprob [bsz, seq] f32
    (only with kl_beta > 0) -> normalised advantages [bsz, seq] f32 (advantages.py:300-364 incl. the pre / post shaping)."""
    dev = _dev(rewards, loss_mask, logprob, ref_logprob)
    if loss_mask.dim() != 2 or rewards.numel() != loss_mask.shape[0]:
        raise RlxError("reinpp_seq_adv: rewards [bsz], loss_mask [bsz, seq]")
    bsz, seq = loss_mask.shape
    r = _as_f32(rewards.reshape(-1), "rewards")
    m = _as_u8(loss_mask)
    lp = rp = None
    kind = 0
    if kl_beta > 0:
        if logprob is None or ref_logprob is None:
            raise RlxError("reinpp_seq_adv: kl_beta > 0 needs logprob and ref_logprob")
        if kl_penalty_type not in _lib.KL_TYPE or kl_penalty_type is None:
            raise NotImplementedError(kl_penalty_type)  # kl_penalty raises the same for "full" / unknown (utils.py:58-64)
        kind = _lib.KL_TYPE[kl_penalty_type]
        lp, rp = _as_f32(logprob, "logprob"), _as_f32(ref_logprob, "ref_logprob")
        if tuple(lp.shape) != (bsz, seq) or tuple(rp.shape) != (bsz, seq):
            raise RlxError("reinpp_seq_adv: logprob / ref_logprob must be [bsz, seq]")
    adv = torch.empty((bsz, seq), dtype=torch.float32, device=dev)
    ws = _lib.workspace(dev, _lib.load().rlx_reinpp_workspace_bytes(bsz))
    _lib.launch("rlx_reinpp_seq_adv", dev, r, m, lp, rp, kind, float(kl_beta), adv, bsz, seq, ws, ws.numel())
    return adv


def reference_softmax_lanes() -> int:
    """f32 lanes of the vector kernels torch's CPU softmax runs with on THIS host: 16 (AVX-512 builds) or 8 (AVX2).  The order of
    the additions in the reference's row sum -- and with it the last bit of softmax(x), and with that a sampled index on a near
    tie -- depends on it; ``categorical_sample`` replays that order (include/rlx.h, rlx_categorical_sample).  Builds whose vector
    width this package has not pinned (NEON, SVE, DEFAULT ...) get 16 with a warning."""
    try:
        cap = torch.backends.cpu.get_cpu_capability().upper()
    except Exception:  # noqa: BLE001
        cap = "?"
    if cap == "AVX2":
        return 8
    if cap != "AVX512":
        import warnings
        warnings.warn(f"torch CPU capability {cap!r}: its softmax summation order is not one this package replays; using 16 lanes")
    return 16


def default_softmax_lanes() -> int:
    """What ``categorical_sample`` uses when the caller names no lane count: a FIXED 16 (the C ABI's own default, the golden
    fixtures' order), so that the same seed samples the same tokens on every node of a job whatever CPUs the hosts have.
    ``RLX_SOFTMAX_LANES=host`` (or 8 / 16) opts in to matching THIS host's torch CPU softmax instead -- for side-by-side parity
    runs against a CPU reference on the same machine."""
    v = os.environ.get("RLX_SOFTMAX_LANES", "16").strip().lower()
    if v == "host":
        return reference_softmax_lanes()
    if v not in ("8", "16"):
        raise RlxError(f"RLX_SOFTMAX_LANES must be 8, 16 or host (got {v!r})")
    return int(v)


def categorical_sample(logits: torch.Tensor, noise: Optional[torch.Tensor] = None, *, temperature: float = 1.0,
                       top_k: int = -1, bin_centers: Optional[torch.Tensor] = None, with_logprob: bool = True,
                       round_outputs: bool = True, softmax_lanes: Optional[int] = None):
    """logits [..., K<=1024] (a view into the model's logits is fine) -> (tokens i64, logprobs f32 or None,
    actions f32 or None), each of shape ``logits.shape[:-1]``.  ``noise``: Exp(1) draws of the logits' dtype and
    shape (what torch.multinomial draws internally); None = argmax.  The sampled indices are bit-exact against the reference's
    CPU path on a host with ``softmax_lanes`` f32 SIMD lanes (None: default_softmax_lanes() -- 16 unless RLX_SOFTMAX_LANES says
    otherwise; ``reference_softmax_lanes()`` is this host's)."""
    dev = _dev(logits, noise, bin_centers)
    lead = logits.shape[:-1]
    x, rows = _rows_of(logits, temperature if noise is not None else 1.0, round_outputs)
    if rows.vocab > 1024:
        raise RlxError(f"categorical_sample handles up to 1024 categories per row (got {rows.vocab})")
    if noise is not None:
        if noise.dtype != logits.dtype or noise.shape != logits.shape:
            raise RlxError("noise must match the logits in dtype and shape")
        noise = noise.contiguous()
    centers = _as_f32(bin_centers, "bin_centers")
    tokens = torch.empty(lead, dtype=torch.int64, device=dev)
    logprob = torch.empty(lead, dtype=torch.float32, device=dev) if with_logprob else None
    actions = torch.empty(lead, dtype=torch.float32, device=dev) if centers is not None else None
    lanes = int(softmax_lanes if softmax_lanes is not None else default_softmax_lanes())
    _lib.launch("rlx_categorical_sample", dev, x, rows, noise, int(top_k), lanes, centers, 0 if centers is None else centers.numel(),
                tokens, logprob, actions)
    return tokens, logprob, actions


def gae_seq(values: torch.Tensor, rewards: torch.Tensor, gamma: float = 1.0, gae_lambda: float = 1.0, out=None, workspace=None):
    """Reasoning GAE in the [bsz, seq] layout: values [bsz, seq] f32, rewards [bsz] -> (advantages, returns), un-normalised.
    ``out`` = (advantages, returns) and ``workspace`` (rlx_gae_seq_workspace_bytes) make the call allocation-free."""
    dev = _dev(values, rewards)
    if values.dim() != 2 or rewards.numel() != values.shape[0]:
        raise RlxError("gae_seq: values [bsz, seq], rewards [bsz]")
    v = _as_f32(values, "values")
    r = _as_f32(rewards.reshape(-1), "rewards")
    bsz, seq = v.shape
    adv, ret = (torch.empty_like(v), torch.empty_like(v)) if out is None else out
    wsb = _lib.load().rlx_gae_seq_workspace_bytes(bsz, seq)
    ws = workspace if workspace is not None and workspace.numel() >= wsb else _lib.workspace(dev, wsb)
    _lib.launch("rlx_gae_seq", dev, v, r, adv, ret, bsz, seq, float(gamma), float(gamma * gae_lambda), ws, ws.numel())
    return adv, ret


# ---- multi-turn GRPO (grpo_dynamic) and the dynamic-batch loss scales (include/rlx.h t3c / t3d) ------------------------------
def traj_ids(idx_to_traj) -> list:
    """idx_to_traj as the reference iterates it: a list of Python ints (a 1-D integer tensor is accepted too)."""
    if isinstance(idx_to_traj, torch.Tensor):
        if idx_to_traj.dim() != 1 or idx_to_traj.is_floating_point() or idx_to_traj.is_complex():
            raise RlxError(f"idx_to_traj must be a 1-D integer tensor or a list of ints (got {idx_to_traj.dtype}, "
                           f"shape {tuple(idx_to_traj.shape)})")
        return idx_to_traj.tolist()
    return list(idx_to_traj)


def grpo_dynamic_csr(idx_to_traj, num_traj: Optional[int] = None):
    """Host CSR of idx_to_traj: (order, traj_offsets) as int64 numpy arrays -- the turn rows sorted stably by trajectory (turn
    order kept inside a trajectory) and offsets[num_traj + 1].  Trajectories with no turns get an empty range."""
    import numpy as np

    ids = np.asarray(traj_ids(idx_to_traj), dtype=np.int64).reshape(-1)
    if ids.size and ids.min() < 0:
        raise RlxError("idx_to_traj holds a negative trajectory id")
    n_traj = int(ids.max()) + 1 if ids.size else 0
    if num_traj is not None:
        if num_traj < n_traj:
            raise RlxError(f"num_traj {num_traj} < max(idx_to_traj) + 1 = {n_traj}")
        n_traj = int(num_traj)
    order = np.argsort(ids, kind="stable")
    offsets = np.zeros(n_traj + 1, dtype=np.int64)
    np.cumsum(np.bincount(ids, minlength=n_traj), out=offsets[1:])
    return order.astype(np.int64), offsets


def _to_device_i32(*parts, device) -> torch.Tensor:
    import numpy as np

    host = torch.from_numpy(np.concatenate([np.asarray(p, dtype=np.int32) for p in parts]))
    if host.numel() > 0x7fffffff:
        raise RlxError("plan too large")
    return host.pin_memory().to(device, non_blocking=True)


class GrpoDynamicPlan:
    """Device plan of rlx_grpo_dynamic_adv: int32 traj_of_row | order | traj_offsets, built on the host in O(num_seq) and copied
    to the device once.  Build it outside a graph capture; the launch itself is capturable."""

    def __init__(self, idx_to_traj, group_size: int, device):
        ids = traj_ids(idx_to_traj)
        order, offsets = grpo_dynamic_csr(ids)
        self.num_seq, self.num_traj, self.group_size = len(ids), len(offsets) - 1, int(group_size)
        if self.group_size < 1 or self.num_traj % self.group_size != 0:
            raise RlxError(f"num_trajectories {self.num_traj} not divisible by group_size {self.group_size}")
        if self.num_seq >= 2 ** 31:
            raise RlxError("grpo_dynamic: more than 2^31 - 1 turns")
        self.plan = _to_device_i32(ids, order, offsets, device=torch.device(device))


def grpo_dynamic_adv(rewards: torch.Tensor, loss_mask: torch.Tensor, plan: GrpoDynamicPlan, mode: str = "turn",
                     eps: float = 1e-6) -> torch.Tensor:
    """rewards [num_seq] f32 / bf16, loss_mask [num_seq, seq] bool / u8 -> advantages [num_seq, seq] in the rewards' dtype:
    the turn's multi-turn GRPO advantage times the mask (advantages.py:167-299), ONE launch, no host sync."""
    dev = _dev(rewards, loss_mask, plan.plan)
    if mode not in _lib.GRPO_DYN_MODES:
        raise RlxError(f"grpo_dynamic_adv: mode {mode!r} is not 'trajectory' or 'turn'")
    if rewards.dtype not in _DTYPES:
        raise RlxError(f"grpo_dynamic_adv: rewards must be float32 or bfloat16 (got {rewards.dtype})")
    if loss_mask.dim() != 2 or rewards.numel() != plan.num_seq or loss_mask.shape[0] != plan.num_seq:
        raise RlxError(f"grpo_dynamic_adv: rewards [num_seq], loss_mask [num_seq, seq] with num_seq = {plan.num_seq} "
                       f"(got {tuple(rewards.shape)}, {tuple(loss_mask.shape)})")
    r = rewards.reshape(-1).contiguous()
    m = _as_u8(loss_mask)
    if m.data_ptr() % 4:
        m = m.clone()
    num_seq, seq = loss_mask.shape
    adv = torch.empty((num_seq, seq), dtype=rewards.dtype, device=dev)
    _lib.launch("rlx_grpo_dynamic_adv", dev, r, _DTYPES[r.dtype], plan.plan, m, adv, num_seq, plan.num_traj, seq, plan.group_size,
                _lib.GRPO_DYN_MODES[mode], float(eps))
    return adv


def loss_scale_groups(idx_to_traj, idx_to_sub_traj):
    """Host grouping of the loss scales (loss_scales.py): turn rows grouped by (trajectory, sub-trajectory).  Returns int64
    numpy arrays (order, group_offsets, agents) -- rows of a group contiguous in `order` (turn order kept), offsets[num_groups
    + 1], and per group A_i, the number of distinct sub-trajectories of its trajectory."""
    import numpy as np

    traj = np.asarray(traj_ids(idx_to_traj), dtype=np.int64).reshape(-1)
    sub = np.asarray(list(idx_to_sub_traj), dtype=np.int64).reshape(-1)
    if sub.size != traj.size:
        raise RlxError(f"idx_to_sub_traj has {sub.size} entries, idx_to_traj {traj.size}")
    if traj.size == 0:
        return np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    order = np.lexsort((sub, traj))  # stable: equal (traj, sub) keys keep their turn order
    t, s = traj[order], sub[order]
    new = np.ones(traj.size, dtype=bool)
    new[1:] = (t[1:] != t[:-1]) | (s[1:] != s[:-1])
    starts = np.flatnonzero(new)
    offsets = np.append(starts, traj.size).astype(np.int64)
    gtraj = t[starts]
    tstart = np.ones(gtraj.size, dtype=bool)
    tstart[1:] = gtraj[1:] != gtraj[:-1]
    run = np.cumsum(tstart) - 1  # trajectory run of each group
    agents = np.bincount(run)[run]
    return order.astype(np.int64), offsets, agents.astype(np.int64)


def agent_level_factors(order, offsets, agents):
    """Per-row f32 factor of agent_level: (1 / A_i) / T_ia in f64, as the reference's Python floats, rounded to f32 once."""
    import numpy as np

    turns = np.diff(offsets)
    f = (1.0 / agents.astype(np.float64)) / turns.astype(np.float64)
    out = np.empty(order.size, dtype=np.float32)
    out[order] = np.repeat(f, turns).astype(np.float32)
    return out


def _scaled_dtype(x: torch.Tensor, who: str) -> int:
    if x.dtype not in _DTYPES:
        raise RlxError(f"{who}: float32 or bfloat16 tensor expected (got {x.dtype})")
    if not x.is_contiguous():
        raise RlxError(f"{who}: the tensor scaled in place must be contiguous")
    if x.data_ptr() % (16 if x.dtype == torch.float32 else 8):
        raise RlxError(f"{who}: the tensor scaled in place is misaligned")
    return _DTYPES[x.dtype]


def scale_rows_(x: torch.Tensor, factor: float = 1.0, row_factors: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x *= factor (row_factors None) or x[row] *= row_factors[row] (f32 [rows]), in place, one launch: the f32 product of each
    element with the factor rounded to f32 -- torch's `t *= python_float` (loss_scales.py group_scale / agent_scale)."""
    dev = _dev(x, row_factors)
    dt = _scaled_dtype(x, "scale_rows_")
    if row_factors is None:
        rows, cols = 1, x.numel()
    else:
        if x.dim() < 1 or row_factors.dtype != torch.float32 or row_factors.numel() != x.shape[0]:
            raise RlxError("scale_rows_: row_factors must be f32 [x.shape[0]]")
        rows, cols = x.shape[0], (x.numel() // x.shape[0] if x.shape[0] else 0)
        row_factors = row_factors.contiguous()
    _lib.launch("rlx_loss_scale_rows", dev, x, dt, row_factors, float(factor), rows, cols)
    return x


class TurnScalePlan:
    """Device plan of rlx_loss_scale_turn: int32 order | group_offsets | zero flag (0)."""

    def __init__(self, order, offsets, device):
        self.num_seq, self.num_groups = int(order.size), int(offsets.size - 1)
        self.plan = _to_device_i32(order, offsets, [0], device=torch.device(device))
        self.zero_flag = self.plan[-1:]


def turn_level_scale_(loss_scales: torch.Tensor, response_mask: torch.Tensor, plan: TurnScalePlan) -> torch.Tensor:
    """loss_scales[t] *= f32(T * |o_t| / sum_t |o_t|) per (trajectory, sub-trajectory) group, in place, one launch.  Returns the
    plan's device zero flag (1: some group's mask total is 0 and was left unscaled) without reading it."""
    dev = _dev(loss_scales, response_mask, plan.plan)
    dt = _scaled_dtype(loss_scales, "turn_level_scale_")
    if response_mask.dim() != 2 or loss_scales.dim() != 2 or tuple(loss_scales.shape) != tuple(response_mask.shape) \
            or loss_scales.shape[0] != plan.num_seq:
        raise RlxError(f"turn_level_scale_: loss_scales and response_mask must both be [num_seq = {plan.num_seq}, seq] "
                       f"(got {tuple(loss_scales.shape)}, {tuple(response_mask.shape)})")
    m = _as_u8(response_mask)
    if m.data_ptr() % 4:
        m = m.clone()
    _lib.launch("rlx_loss_scale_turn", dev, loss_scales, dt, m, plan.plan, plan.num_seq, plan.num_groups, loss_scales.shape[1],
                plan.zero_flag)
    return plan.zero_flag
