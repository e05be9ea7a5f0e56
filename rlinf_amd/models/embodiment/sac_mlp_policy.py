"""The SAC (Q-head) variant of the MLP policy as the module a REAL RLinf install gets from its own model registry.

The reference's SAC learner (rlinf/workers/actor/fsdp_sac_policy_worker.py:346-549) drives its ``MLPPolicy(add_q_head=True)``
(rlinf/models/embodiment/mlp_policy/mlp_policy.py) through ``model(forward_type=ForwardType.SAC | SAC_Q, ...)``.  With this module
those calls are HIP launches with HIP backwards (csrc/sac_mlp.hip):

* ``sac_forward``: backbone, the two heads, the rsample, the tanh squash and the log-prob in ONE launch; under autograd it is one
  node over the named actor parameters whose backward differentiates through the rsample (``rlx_sac_actor_bwd``).
* ``sac_q_forward``: both Q heads (Linear -> LayerNorm -> tanh, three times, then Linear) over ``cat(states, actions)`` in ONE
  launch; one autograd node over the named Q parameters AND ``actions`` (the actor loss back-propagates through Q into the action).

The parameters are ordinary ``nn.Parameter``s under the reference's names, shapes, ``named_parameters()`` order and initial values
(same RNG draws in the same order), so ``build_optimizers`` (critic group = names containing ``q_head``), ``clip_grad_norm_``, torch
optimizers, checkpoints and the target network's ``deepcopy`` work unchanged.

Stale weights cannot happen: the reference's soft update writes ``target_param.data.mul_().add_()``, which bumps no version
counter, so NO cache key is kept here -- every call gathers the parameters it reads into the kernels' flat f32 buffer with one
multi-tensor copy.  A forward that will be back-propagated gathers into a buffer of its own, which its backward then reads: the
backward sees the weights of its forward whatever ran in between.
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from ... import ops
from ..._lib import SacActorLayout, SacQLayout

HIDDEN = 256
MAX_OBS_DIM, MAX_ACT_DIM = 64, 16
LOGSTD_RANGE = (-5, 2)


def _linear_norm_tanh_stack(in_dim: int, out_dim: int) -> nn.Sequential:
    """modules/utils.py:38-50 with use_layer_norm=True, last_act=False: indices 0,3,6,9 are Linear, 1,4,7 LayerNorm."""
    mods, c_in = [], in_dim
    for _ in range(3):
        mods += [nn.Linear(c_in, HIDDEN), nn.LayerNorm(HIDDEN), nn.Tanh()]
        c_in = HIDDEN
    mods.append(nn.Linear(c_in, out_dim))
    return nn.Sequential(*mods)


class _QHead(nn.Module):  # parameter holder under the reference's names (modules/q_head.py:22-96)
    def __init__(self, in_dim: int, out_dim: int):
        super().__init__()
        self.net = _linear_norm_tanh_stack(in_dim, out_dim)
        gain = nn.init.calculate_gain("tanh")
        for m in self.net:
            if isinstance(m, nn.Linear):
                if m is self.net[-1]:
                    nn.init.normal_(m.weight, mean=0.0, std=0.02)
                else:
                    nn.init.xavier_uniform_(m.weight, gain=gain)
                nn.init.zeros_(m.bias)


class _MultiQHead(nn.Module):  # modules/q_head.py:117-160
    def __init__(self, in_dim: int, out_dim: int, num_q_heads: int = 2):
        super().__init__()
        self.num_q_heads = num_q_heads
        self.qs = nn.ModuleList([_QHead(in_dim, out_dim) for _ in range(num_q_heads)])


def _orthogonal(layer: nn.Linear, std: float) -> nn.Linear:  # modules/utils.py:20-23
    nn.init.orthogonal_(layer.weight, std)
    nn.init.constant_(layer.bias, 0.0)
    return layer


def check_sac_shapes(obs_dim, action_dim, num_action_chunks, critic_obs_dim=None, compute_dtype=torch.float32):
    act = int(action_dim) * int(num_action_chunks)
    if not 1 <= int(obs_dim) <= MAX_OBS_DIM:
        raise NotImplementedError(f"the HIP SAC MLP policy serves 1 <= obs_dim <= {MAX_OBS_DIM} (got obs_dim={obs_dim})")
    if not 1 <= act <= MAX_ACT_DIM:
        raise NotImplementedError(f"the HIP SAC MLP policy serves 1 <= action_dim * num_action_chunks <= {MAX_ACT_DIM} (got {act})")
    if critic_obs_dim is not None and int(critic_obs_dim) != int(obs_dim):
        raise NotImplementedError(f"critic_obs_dim must be None or obs_dim={obs_dim} (got {critic_obs_dim}): sac_q_forward feeds the "
                                  "Q heads the actor's states")
    if compute_dtype != torch.float32:
        raise NotImplementedError(f"the HIP SAC MLP policy computes in float32 only (got compute_dtype={compute_dtype})")


class _ActorFn(torch.autograd.Function):
    """sac_forward as ONE autograd node over the named actor parameters."""

    @staticmethod
    def forward(ctx, module, states, eps, *params):
        flat = module._gather(module._actor_params(), params, fresh=True)
        action, logprob, acts, aux = ops.sac_actor_fwd(flat, module._actor_layout, states, eps, module._scale, module._bias, True)
        ctx.module, ctx.flat, ctx.eps = module, flat, eps
        ctx.save_for_backward(states, acts, aux)
        return action, logprob

    @staticmethod
    def backward(ctx, d_action, d_logprob):
        states, acts, aux = ctx.saved_tensors
        module = ctx.module
        cont = lambda t: None if t is None else t.contiguous()  # noqa: E731
        slabs = ops.sac_actor_bwd(ctx.flat, module._actor_layout, states, ctx.eps, acts, aux, cont(d_action), cont(d_logprob),
                                  module._scale)
        flat_grad = ops.sum_slabs(slabs)
        return (None, None, None, *module._split(flat_grad, module._actor_params(), ctx.needs_input_grad[3:]))


class _QFn(torch.autograd.Function):
    """sac_q_forward as ONE autograd node over ``actions`` and the named Q parameters."""

    @staticmethod
    def forward(ctx, module, states, actions, *params):
        flat = module._gather(module._q_params(), params, fresh=True)
        q, acts, rstd = ops.sac_q_fwd(flat, module._q_layout, states, actions, True)
        ctx.module, ctx.flat = module, flat
        ctx.save_for_backward(states, actions, acts, rstd)
        return q

    @staticmethod
    def backward(ctx, d_q):
        states, actions, acts, rstd = ctx.saved_tensors
        module = ctx.module
        want_params, want_actions = any(ctx.needs_input_grad[3:]), ctx.needs_input_grad[2]
        slabs, d_actions = ops.sac_q_bwd(ctx.flat, module._q_layout, states, actions, acts, rstd, d_q.contiguous(), want_params,
                                         want_actions)
        grads = [None] * len(ctx.needs_input_grad[3:])
        if want_params:
            grads = module._split(ops.sum_slabs(slabs), module._q_params(), ctx.needs_input_grad[3:])
        return (None, None, d_actions, *grads)


class SacMLPPolicy(nn.Module):
    """Constructor arguments, parameter names, initialisation (same RNG stream), method names and return structures of the
    reference's ``MLPPolicy(add_q_head=True, q_head_type="default")``."""

    def __init__(self, obs_dim, action_dim, num_action_chunks, add_value_head=False, add_q_head=True, q_head_type="default",
                 value_granularity="action_level", critic_obs_dim=None, compute_dtype=torch.float32):
        super().__init__()
        if add_value_head or not add_q_head or q_head_type != "default":
            raise NotImplementedError("SacMLPPolicy is the add_q_head=True, q_head_type='default' variant without a value head "
                                      f"(got add_value_head={add_value_head}, add_q_head={add_q_head}, q_head_type={q_head_type!r})")
        check_sac_shapes(obs_dim, action_dim, num_action_chunks, critic_obs_dim, compute_dtype)
        self.obs_dim, self.action_dim, self.num_action_chunks = int(obs_dim), int(action_dim), int(num_action_chunks)
        self.critic_obs_dim = self.obs_dim
        self.value_granularity, self.compute_dtype = value_granularity, compute_dtype
        self.independent_std, self.final_tanh, self.logstd_range = False, True, LOGSTD_RANGE
        self.torch_compile_enabled, self.cuda_graph_manager = False, None
        act = self.action_dim * self.num_action_chunks
        self.q_out_dim = 1 if value_granularity == "chunk_level" else self.num_action_chunks
        # the reference's construction order, which is its order of RNG draws and of named_parameters() (mlp_policy.py:66-116)
        self.q_head = _MultiQHead(self.obs_dim + act, self.q_out_dim)
        self.backbone = nn.Sequential(_orthogonal(nn.Linear(self.obs_dim, HIDDEN), math.sqrt(2)), nn.Tanh(),
                                      _orthogonal(nn.Linear(HIDDEN, HIDDEN), math.sqrt(2)), nn.Tanh(),
                                      _orthogonal(nn.Linear(HIDDEN, HIDDEN), math.sqrt(2)), nn.Tanh())
        self.actor_mean = _orthogonal(nn.Linear(HIDDEN, act), 0.01 * math.sqrt(2))
        self.actor_logstd = nn.Linear(HIDDEN, act)
        self.register_buffer("action_scale", torch.tensor(1.0, dtype=torch.float32))  # action range (-1, 1)
        self.register_buffer("action_bias", torch.tensor(0.0, dtype=torch.float32))
        self._scale, self._bias = 1.0, 0.0  # the kernels take them as scalars; read again after load_state_dict
        self._actor_layout, self._q_layout = self._layouts()
        self._flat = {}

    # ---- the kernels' view of the parameters ----------------------------------------------------------------------
    def _actor_params(self):
        """(name, parameter) in the order of the actor's flat buffer: the head's two weights, then its two biases, lie together."""
        b = self.backbone
        return [("w0", b[0].weight), ("b0", b[0].bias), ("w1", b[2].weight), ("b1", b[2].bias), ("w2", b[4].weight),
                ("b2", b[4].bias), ("wh", self.actor_mean.weight), ("wh2", self.actor_logstd.weight),
                ("bh", self.actor_mean.bias), ("bh2", self.actor_logstd.bias)]

    def _q_params(self):
        """Order of the Q flat buffer: per head the layers' (weight, bias, norm weight, norm bias), the last layer's weight; the two
        odd-sized last biases go to the end so that every 256-wide weight starts at a multiple of 4."""
        out, tail = [], []
        for y, qh in enumerate(self.q_head.qs):
            for l in range(3):
                lin, ln = qh.net[3 * l], qh.net[3 * l + 1]
                out += [(f"w{y}{l}", lin.weight), (f"b{y}{l}", lin.bias), (f"g{y}{l}", ln.weight), (f"beta{y}{l}", ln.bias)]
            out.append((f"w{y}3", qh.net[9].weight))
            tail.append((f"b{y}3", qh.net[9].bias))
        return out + tail

    @staticmethod
    def _offsets(named):
        offs, at = {}, 0
        for name, p in named:
            offs[name] = at
            at += p.numel()
        return offs, at

    def _layouts(self):
        act = self.action_dim * self.num_action_chunks
        o, n = self._offsets(self._actor_params())
        al = SacActorLayout(obs_dim=self.obs_dim, act_dim=act, hidden=HIDDEN, n_params=n, off_wh=o["wh"], off_bh=o["bh"],
                            logstd_lo=LOGSTD_RANGE[0], logstd_hi=LOGSTD_RANGE[1])
        for l in range(3):
            al.off_w[l], al.off_b[l] = o[f"w{l}"], o[f"b{l}"]
        o, n = self._offsets(self._q_params())
        ql = SacQLayout(obs_dim=self.obs_dim, act_dim=act, out_dim=self.q_out_dim, hidden=HIDDEN, n_params=n)
        for y in range(2):
            for l in range(4):
                ql.off_w[y][l], ql.off_b[y][l] = o[f"w{y}{l}"], o[f"b{y}{l}"]
            for l in range(3):
                ql.off_g[y][l], ql.off_beta[y][l] = o[f"g{y}{l}"], o[f"beta{y}{l}"]
        return al, ql

    @staticmethod
    def _local(p: torch.Tensor) -> torch.Tensor:
        t = p.detach()
        if hasattr(t, "full_tensor"):  # FSDP2 hands out DTensors; the kernels need this rank's whole copy
            t = t.full_tensor()
        return t.to(torch.float32)

    def _gather(self, named, params=None, fresh=False) -> torch.Tensor:
        """The parameters AS THEY ARE NOW, in the kernels' flat buffer: one multi-tensor copy, on every call (no cache key: writes
        through ``.data`` bump no version counter).  ``fresh``: a buffer of the caller's own (kept for its backward)."""
        src = [self._local(p) for p in (params if params is not None else [p for _, p in named])]
        n, dev = sum(t.numel() for t in src), src[0].device
        which = named[0][0]  # "w0": the actor's buffer, "w00": the Q ensemble's
        flat = None if fresh else self._flat.get(which)
        if flat is None or flat.device != dev:
            flat = torch.empty((n,), dtype=torch.float32, device=dev)
            if not fresh:
                self._flat[which] = flat
        views, at = [], 0
        for t in src:
            views.append(flat[at:at + t.numel()].view(t.shape))
            at += t.numel()
        torch._foreach_copy_(views, src)
        return flat

    @staticmethod
    def _split(flat_grad, named, needs):
        grads, at = [], 0
        for (_, p), need in zip(named, needs):
            grads.append(flat_grad[at:at + p.numel()].view(p.shape) if need else None)
            at += p.numel()
        return grads

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._scale, self._bias = float(self.action_scale), float(self.action_bias)
        return out

    def __deepcopy__(self, memo):  # the target network: the layouts (ctypes) are rebuilt, the scratch buffers not shared
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k in ("_actor_layout", "_q_layout", "_flat"):
                continue
            new.__dict__[k] = copy.deepcopy(v, memo)
        new._actor_layout, new._q_layout = new._layouts()
        new._flat = {}
        return new

    def set_global_step(self, global_step):
        self.global_step = global_step

    # ---- reference API ----------------------------------------------------------------------------------------------
    def preprocess_env_obs(self, env_obs):
        return {"states": env_obs["states"].to(self.actor_mean.weight.device)}  # mlp_policy.py:122-124

    def forward(self, forward_type="default", **kwargs):
        for key in ("obs", "next_obs"):  # mlp_policy.py:139-147
            if kwargs.get(key) is not None:
                kwargs[key] = self.preprocess_env_obs(kwargs[key])
        kind = getattr(forward_type, "value", forward_type)
        if kind == "sac":
            return self.sac_forward(**kwargs)
        if kind == "sac_q":
            return self.sac_q_forward(**kwargs)
        raise NotImplementedError(f"forward_type={kind!r}: the HIP SAC MLP policy serves 'sac' and 'sac_q'")

    def _states(self, obs) -> torch.Tensor:
        states = obs["states"].to(self.actor_mean.weight.device, torch.float32).contiguous()
        if states.dim() != 2 or states.shape[1] != self.obs_dim:
            raise ValueError(f"states must be [batch, {self.obs_dim}], got {tuple(states.shape)}")
        return states

    def _noise(self, states, eps, generator):
        act = self.action_dim * self.num_action_chunks
        if eps is None:
            return torch.randn((states.shape[0], act), dtype=torch.float32, device=states.device, generator=generator)
        return eps.to(states.device, torch.float32).reshape(states.shape[0], act).contiguous()

    def sac_forward(self, obs, eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, **kwargs):
        """-> (action, logprob [M, A'], None): an rsample through the tanh squash (mlp_policy.py:179-200).  ``eps``: the N(0,1)
        draws to use; otherwise ``torch.randn`` on the device (``generator``)."""
        states = self._states(obs)
        eps = self._noise(states, eps, generator)
        named = self._actor_params()
        if torch.is_grad_enabled() and any(p.requires_grad for _, p in named):
            action, logprob = _ActorFn.apply(self, states, eps, *[p for _, p in named])
        else:
            action, logprob, _, _ = ops.sac_actor_fwd(self._gather(named), self._actor_layout, states, eps, self._scale, self._bias,
                                                       False)
        return action, logprob, None

    def sac_q_forward(self, obs, actions, shared_feature=None, detach_encoder=False, **kwargs):
        """-> q [M, 2 * out]: both heads on cat(states, actions) (mlp_policy.py:322-323)."""
        states = self._states(obs)
        actions = actions.to(states.device, torch.float32).reshape(states.shape[0], -1).contiguous()
        named = self._q_params()
        if torch.is_grad_enabled() and (actions.requires_grad or any(p.requires_grad for _, p in named)):
            return _QFn.apply(self, states, actions, *[p for _, p in named])
        return ops.sac_q_fwd(self._gather(named), self._q_layout, states, actions, False)[0]

    def default_forward(self, **kwargs):
        raise NotImplementedError("the SAC variant is trained through forward_type='sac' / 'sac_q'")

    @torch.no_grad()
    def predict_action_batch(self, env_obs, calculate_logprobs=True, calculate_values=True, return_obs=True, mode="train",
                             eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None, **kwargs):
        """mlp_policy.py:295-320 with final_tanh: train samples, eval acts with tanh(mean); there is no value head: zeros."""
        if mode not in ("train", "eval"):
            raise NotImplementedError(f"{mode=}")
        obs = self.preprocess_env_obs(env_obs)
        states = self._states(obs)
        noise = self._noise(states, eps, generator) if mode == "train" else None
        action, logprob, _, _ = ops.sac_actor_fwd(self._gather(self._actor_params()), self._actor_layout, states, noise, self._scale,
                                                   self._bias, False)
        forward_inputs = {"action": action, "model_action": action}
        if return_obs:
            forward_inputs["states"] = obs["states"]
        result = {"prev_logprobs": logprob, "prev_values": torch.zeros_like(logprob[..., :1]), "forward_inputs": forward_inputs}
        return action.reshape(-1, self.num_action_chunks, self.action_dim), result

    # A model call is ONE hand-written launch already: nothing for a tracing compiler or a graph capture to remove.
    def enable_torch_compile(self, mode: str = "max-autotune-no-cudagraphs"):
        self.torch_compile_enabled = True

    def capture_cuda_graph(self, train_batch_size: int, eval_batch_size: int):
        return None

    def release_cuda_graph(self):
        return None

    def is_cuda_graph_enabled(self) -> bool:
        return False
