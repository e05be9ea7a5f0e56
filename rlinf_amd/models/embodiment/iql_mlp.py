"""The networks of offline IQL for the MLP policy as flat float32 buffers over the HIP kernels of csrc/iql_mlp.hip.

Replaces ``IQLMLPPolicy`` / ``IQLTwinCritic`` (rlinf/models/embodiment/mlp_policy/iql_mlp_policy.py) on the learner's path: one flat
buffer per module (actor, twin critic, target twin critic, value) with views under the reference's LIVE parameter names

    actor   backbone.{0,2,4}.{weight,bias}, actor_mean.{weight,bias}, actor_logstd
    value   net.{0,2,4}.{weight,bias}
    critic  q1.net.{0,2,4}.{weight,bias}, q2.net.{0,2,4}.{weight,bias}

Initialisation is draw-for-draw the reference's: after the same ``torch.manual_seed`` the live parameters are bit-equal to
``IQLMLPPolicy(obs, act, 1, add_value_head=(type == "actor"), False)`` + ``configure_iql(...)`` built in the reference worker's
order (actor, q1, q2, value, the target's q1 and q2, then ``target.load_state_dict(critic)``).  The parent class builds modules
that ``configure_iql`` replaces or never uses (its orthogonal backbone / actor_mean and, for the actor, a value head); their
draws come first and are reproduced here.  Rollout and evaluation are not on this path.
"""

from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn as nn

from ... import ops
from ..._lib import IqlMlpLayout

HIDDEN = 256
MAX_OBS_DIM, MAX_ACTION_DIM = 64, 32
KINDS = ("actor", "critic", "value")


def check_dims(obs_dim: int, action_dim: int, num_action_chunks: int = 1, hidden_dims=(HIDDEN, HIDDEN), dtype=torch.float32) -> None:
    """The limits of the HIP kernels, refused by name."""
    if list(hidden_dims) != [HIDDEN, HIDDEN]:
        raise ValueError(f"hidden_dims={list(hidden_dims)} is not supported: the HIP IQL networks are [256, 256] (hidden width 256)")
    if not 1 <= int(obs_dim) <= MAX_OBS_DIM:
        raise ValueError(f"obs_dim={obs_dim} out of range [1, {MAX_OBS_DIM}]")
    if not 1 <= int(action_dim) <= MAX_ACTION_DIM:
        raise ValueError(f"action_dim={action_dim} out of range [1, {MAX_ACTION_DIM}]")
    if int(num_action_chunks) != 1:
        raise ValueError(f"num_action_chunks={num_action_chunks} is not supported: offline IQL on HIP needs num_action_chunks == 1")
    if dtype != torch.float32:
        raise ValueError(f"dtype={dtype} is not supported: the HIP IQL networks are float32")


def iql_layout(kind: str, obs_dim: int, action_dim: int, log_std_min: float = -5.0, log_std_max: float = 2.0):
    """-> (rlx_iql_mlp_layout, OrderedDict name -> (offset, shape)).  Per network the hidden layers and the head weight, then the
    head biases of all networks, then actor_logstd: every 256-wide weight starts at a multiple of 4 elements without padding."""
    check_dims(obs_dim, action_dim)
    if kind not in KINDS:
        raise ValueError(f"Unsupported iql_type: {kind}")
    D, A = int(obs_dim), int(action_dim)
    lay = IqlMlpLayout()
    lay.n_nets = 2 if kind == "critic" else 1
    lay.in_a, lay.in_b = D, A if kind == "critic" else 0
    lay.n_hidden = 3 if kind == "actor" else 2
    lay.out_dim, lay.hidden = A if kind == "actor" else 1, HIDDEN
    lay.logstd_lo, lay.logstd_hi = float(log_std_min), float(log_std_max)
    nh, K = lay.n_hidden, lay.in_a + lay.in_b
    if kind == "actor":
        names = [["backbone.0", "backbone.2", "backbone.4", "actor_mean"]]
    else:
        prefixes = ("q1.", "q2.") if kind == "critic" else ("",)
        names = [[p + "net.0", p + "net.2", p + "net.4"] for p in prefixes]
    views, off = OrderedDict(), 0
    for y, net in enumerate(names):
        for l in range(nh + 1):
            rows, cols = (lay.out_dim if l == nh else HIDDEN), (K if l == 0 else HIDDEN)
            lay.off_w[y][l] = off
            views[net[l] + ".weight"] = (off, (rows, cols))
            off += rows * cols
            if l < nh:
                lay.off_b[y][l] = off
                views[net[l] + ".bias"] = (off, (rows,))
                off += rows
    for y, net in enumerate(names):
        lay.off_b[y][nh] = off
        views[net[nh] + ".bias"] = (off, (lay.out_dim,))
        off += lay.out_dim
    lay.off_logstd = -1
    if kind == "actor":
        lay.off_logstd = off
        views["actor_logstd"] = (off, (1, A))
        off += A
    lay.n_params = off
    return lay, views


def _orthogonal(layer: nn.Linear, std: float) -> nn.Linear:
    nn.init.orthogonal_(layer.weight, std)
    nn.init.constant_(layer.bias, 0.0)
    return layer


def _parent_draws(obs_dim: int, action_dim: int, value_head: bool) -> "OrderedDict[str, torch.Tensor]":
    """The modules the parent class (MLPPolicy.__init__) builds before ``configure_iql``: they take their draws from the global
    generator.  -> the value head's state (``value_head.mlp.*``: it stays in the actor's state dict, unused)."""
    dead = OrderedDict()
    if value_head:
        dims = [obs_dim, HIDDEN, HIDDEN, HIDDEN]
        layers = [nn.Linear(dims[i], dims[i + 1]) for i in range(3)] + [nn.Linear(HIDDEN, 1, bias=False)]
        for lin in layers[:-1]:
            nn.init.kaiming_normal_(lin.weight, mode="fan_out", nonlinearity="tanh")
            nn.init.zeros_(lin.bias)
        nn.init.normal_(layers[-1].weight, mean=0.0, std=0.02)
        for i, lin in enumerate(layers):
            dead[f"value_head.mlp.{2 * i}.weight"] = lin.weight.detach().clone()
            if lin.bias is not None:
                dead[f"value_head.mlp.{2 * i}.bias"] = lin.bias.detach().clone()
    for c_in in (obs_dim, HIDDEN, HIDDEN):
        _orthogonal(nn.Linear(c_in, HIDDEN), math.sqrt(2))
    _orthogonal(nn.Linear(HIDDEN, action_dim), 0.01 * math.sqrt(2))
    return dead


def _live_draws(kind: str, obs_dim: int, action_dim: int) -> "OrderedDict[str, torch.Tensor]":
    """``_init_iql``: plain nn.Linear modules in their default initialisation, in the reference's order."""
    out = OrderedDict()
    if kind == "actor":
        for name, c_in in (("backbone.0", obs_dim), ("backbone.2", HIDDEN), ("backbone.4", HIDDEN)):
            lin = nn.Linear(c_in, HIDDEN)
            out[name + ".weight"], out[name + ".bias"] = lin.weight.detach(), lin.bias.detach()
        lin = nn.Linear(HIDDEN, action_dim)
        out["actor_mean.weight"], out["actor_mean.bias"] = lin.weight.detach(), lin.bias.detach()
        out["actor_logstd"] = torch.zeros(1, action_dim)
        return out
    c_in = obs_dim + (action_dim if kind == "critic" else 0)
    for name, (i, o) in (("net.0", (c_in, HIDDEN)), ("net.2", (HIDDEN, HIDDEN)), ("net.4", (HIDDEN, 1))):
        lin = nn.Linear(i, o)
        out[name + ".weight"], out[name + ".bias"] = lin.weight.detach(), lin.bias.detach()
    return out


def _module_draws(kind: str, obs_dim: int, action_dim: int):
    """One ``IQLMLPPolicy(...)`` + ``configure_iql``: -> (live parameters by name, dead value-head entries)."""
    dead = _parent_draws(obs_dim, action_dim, value_head=(kind == "actor"))
    return _live_draws(kind, obs_dim, action_dim), dead


class IqlFlatNet:
    """One module of the learner (actor / twin critic / value) as ONE flat float32 buffer with named views."""

    def __init__(self, kind: str, obs_dim: int, action_dim: int, device, values: dict, log_std_min=-5.0, log_std_max=2.0):
        self.kind = kind
        self.layout, self._views = iql_layout(kind, obs_dim, action_dim, log_std_min, log_std_max)
        self.flat = torch.zeros(self.layout.n_params, dtype=torch.float32, device=device)
        self.views = OrderedDict((n, self.flat[o:o + math.prod(shape)].view(shape)) for n, (o, shape) in self._views.items())
        assert sorted(values) == sorted(self.views), (sorted(values), sorted(self.views))
        for n, v in values.items():
            self.views[n].copy_(v)

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict(self.views)

    def load_state_dict(self, state: dict) -> None:
        missing = [n for n in self.views if n not in state]
        if missing:
            raise KeyError(f"missing keys: {missing}")
        for n, v in self.views.items():
            v.copy_(state[n])

    # ---- the model calls --------------------------------------------------------------------------------------------------
    def forward(self, obs, actions=None, obs2=None, train: bool = False, logprob_of=None):
        """critic: ``actions`` beside ``obs``; value: ``obs2`` = further rows in the same launch; actor: ``logprob_of`` = the actions
        whose log-prob is wanted.  -> (out [n_nets, M, out_dim], acts | None, logprob | None)"""
        return ops.iql_mlp_fwd(self.flat, self.layout, obs, xb=actions, xa2=obs2, train=train, actions=logprob_of)

    def backward(self, obs, actions, acts, d_out, d_logstd=None, grads=None, workspace=None):
        return ops.iql_mlp_bwd(self.flat, self.layout, obs, actions, acts, d_out, d_logstd, grads=grads, workspace=workspace)


class IqlNetworks:
    """actor, critic (twin), target (twin), value -- built in the reference worker's order from the global torch generator."""

    def __init__(self, obs_dim: int, action_dim: int, device, num_action_chunks: int = 1, hidden_dims=(HIDDEN, HIDDEN),
                 log_std_min: float = -5.0, log_std_max: float = 2.0, dtype=torch.float32):
        check_dims(obs_dim, action_dim, num_action_chunks, hidden_dims, dtype)
        self.obs_dim, self.action_dim = int(obs_dim), int(action_dim)
        D, A = self.obs_dim, self.action_dim

        def twin():
            vals = OrderedDict()
            for p in ("q1.", "q2."):
                live, _ = _module_draws("critic", D, A)
                vals.update((p + n, v) for n, v in live.items())
            return vals

        actor_vals, self._dead_value_head = _module_draws("actor", D, A)
        critic_vals = twin()
        value_vals, _ = _module_draws("value", D, A)
        twin()  # the target's own draws; target.load_state_dict(critic) then overwrites them
        self.actor = IqlFlatNet("actor", D, A, device, actor_vals, log_std_min, log_std_max)
        self.critic = IqlFlatNet("critic", D, A, device, critic_vals)
        self.value = IqlFlatNet("value", D, A, device, value_vals)
        self.target = IqlFlatNet("critic", D, A, device, critic_vals)

    def get_policy_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """What a reference ``IQLMLPPolicy`` of type actor loads with ``strict=True``: the live entries plus the parent's unused
        ``value_head.mlp.*`` at their initial values (the last of them has no bias)."""
        dev = self.actor.flat.device
        sd = OrderedDict((n, v.to(dev)) for n, v in self._dead_value_head.items())
        sd.update(self.actor.state_dict())
        return sd
