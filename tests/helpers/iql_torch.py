"""Offline IQL for the MLP policy restated in plain torch, written from the arithmetic: the three module kinds under the
reference's parameter names, their construction (the same draws from the global generator in the same order), the three losses,
torch.optim.Adam, CosineAnnealingLR and the soft update.  Runs in any dtype.

tests/test_iql_restatement_vs_reference.py pins this file to the real reference where the reference exists; the GPU tests compare
the HIP kernels with it, since the reference's IQL files are not on the GPU machine.
"""

import math

import torch
import torch.nn as nn

HIDDEN = 256
METRICS = ("critic_loss", "q1", "q2", "value_loss", "v", "actor_loss", "adv_mean", "adv_std")


def _relu_mlp(dims, final_relu):
    layers = []
    for i in range(len(dims) - 2):
        layers += [nn.Linear(dims[i], dims[i + 1]), nn.ReLU()]
    layers.append(nn.Linear(dims[-2], dims[-1]))
    if final_relu:
        layers.append(nn.ReLU())
    return nn.Sequential(*layers)


def _ortho(lin, std):
    nn.init.orthogonal_(lin.weight, std)
    nn.init.constant_(lin.bias, 0.0)
    return lin


class _ParentValueHead(nn.Module):
    """The generic policy's value head (tanh, three hidden layers, no bias on the last): never used by IQL, but it is in the
    actor's state dict and takes its draws first."""

    def __init__(self, obs_dim):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(obs_dim, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, HIDDEN), nn.Tanh(), nn.Linear(HIDDEN, HIDDEN),
                                 nn.Tanh(), nn.Linear(HIDDEN, 1, bias=False))
        for m in list(self.mlp)[:-1]:
            if isinstance(m, nn.Linear):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="tanh")
                nn.init.zeros_(m.bias)
        nn.init.normal_(self.mlp[-1].weight, mean=0.0, std=0.02)


class IqlModule(nn.Module):
    """kind 'actor' | 'critic' | 'value'.  ``live_only``: without the parent's unused modules in the state dict (their draws are
    still taken)."""

    def __init__(self, kind, obs_dim, action_dim, log_std_min=-5.0, log_std_max=2.0, live_only=True):
        super().__init__()
        self.kind, self.logstd_range = kind, (float(log_std_min), float(log_std_max))
        value_head = _ParentValueHead(obs_dim) if kind == "actor" else None
        parent_backbone = nn.Sequential(_ortho(nn.Linear(obs_dim, HIDDEN), math.sqrt(2)), nn.Tanh(),
                                        _ortho(nn.Linear(HIDDEN, HIDDEN), math.sqrt(2)), nn.Tanh(),
                                        _ortho(nn.Linear(HIDDEN, HIDDEN), math.sqrt(2)), nn.Tanh())
        parent_mean = _ortho(nn.Linear(HIDDEN, action_dim), 0.01 * math.sqrt(2))
        if kind == "actor":
            if not live_only:
                self.value_head = value_head
            self.backbone = _relu_mlp([obs_dim, HIDDEN, HIDDEN, HIDDEN], final_relu=True)
            self.actor_mean = nn.Linear(HIDDEN, action_dim)
            self.actor_logstd = nn.Parameter(torch.zeros(1, action_dim))
        else:
            if not live_only:
                self.backbone, self.actor_mean = parent_backbone, parent_mean
                self.actor_logstd = nn.Parameter(torch.ones(1, action_dim) * -0.5)
            self.net = _relu_mlp([obs_dim + (action_dim if kind == "critic" else 0), HIDDEN, HIDDEN, 1], final_relu=False)

    def actor_mean_of(self, obs):
        return self.actor_mean(self.backbone(obs))

    def log_prob(self, obs, actions):
        mean = self.actor_mean_of(obs)
        logstd = torch.clamp(self.actor_logstd, self.logstd_range[0], self.logstd_range[1])
        raw = torch.atanh(actions.clamp(-1 + 1e-6, 1 - 1e-6))
        mean, std = torch.broadcast_tensors(mean, torch.exp(logstd))  # one gradient per element of std, summed over the rows once
        normal = -((raw - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))
        lp = normal.sum(-1)
        lp = lp - (2 * (math.log(2) - raw - nn.functional.softplus(-2 * raw))).sum(-1)
        return lp

    def q(self, obs, actions):
        return self.net(torch.cat([obs, actions], dim=-1)).squeeze(-1)

    def v(self, obs):
        return self.net(obs).squeeze(-1)


class IqlTwin(nn.Module):
    def __init__(self, obs_dim, action_dim, live_only=True):
        super().__init__()
        self.q1 = IqlModule("critic", obs_dim, action_dim, live_only=live_only)
        self.q2 = IqlModule("critic", obs_dim, action_dim, live_only=live_only)

    def forward(self, obs, actions):
        return self.q1.q(obs, actions), self.q2.q(obs, actions)


class IqlLearner:
    """The four modules in the reference worker's construction order, three Adams, the actor's cosine schedule."""

    def __init__(self, obs_dim, action_dim, dtype=torch.float32, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_steps=1, gamma=0.99,
                 tau=0.005, expectile=0.7, temperature=3.0, live_only=True):
        self.actor = IqlModule("actor", obs_dim, action_dim, live_only=live_only)
        self.critic = IqlTwin(obs_dim, action_dim, live_only=live_only)
        self.value = IqlModule("value", obs_dim, action_dim, live_only=live_only)
        self.target = IqlTwin(obs_dim, action_dim, live_only=live_only)
        self.target.load_state_dict(self.critic.state_dict())
        for m in (self.actor, self.critic, self.value, self.target):
            m.to(dtype)
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.gamma, self.tau, self.expectile, self.temperature = float(gamma), float(tau), float(expectile), float(temperature)
        self.build_optimizers(lr, betas, eps, max_steps)
        # deliberate mistakes for the negative controls of tests/test_iql_host.py
        self.mistake = None

    def build_optimizers(self, lr, betas, eps, max_steps):
        mk = lambda m: torch.optim.Adam(m.parameters(), lr=float(lr), betas=tuple(betas), eps=float(eps))  # noqa: E731
        self.opt_actor, self.opt_value, self.opt_critic = mk(self.actor), mk(self.value), mk(self.critic)
        self.sched = torch.optim.lr_scheduler.CosineAnnealingLR(self.opt_actor, T_max=max(1, int(max_steps)), eta_min=0.0)

    def modules(self):
        return {"actor": self.actor, "critic": self.critic, "value": self.value, "target": self.target}

    def soft_update(self):
        with torch.no_grad():
            tp, cp = list(self.target.parameters()), list(self.critic.parameters())
            torch._foreach_mul_(tp, 1.0 - self.tau)
            torch._foreach_add_(tp, cp, alpha=self.tau)


def expectile_loss(diff, expectile):
    weight = torch.abs(float(expectile) - (diff < 0).to(diff.dtype))
    return weight * diff.square()


def iql_update_step(L, obs, actions, rewards, masks, next_obs):
    """One update in the reference's order: value, actor (then the schedule), critic, soft update.  -> the eight metrics (a tensor
    in METRICS order) and lr_actor after the scheduler step."""
    # value
    with torch.no_grad():
        q_t = torch.min(*L.target(obs, actions))
    old_v_for_mistake = L.value.v(obs).detach() if L.mistake == "stale_new_v" else None
    v = L.value.v(obs)
    value_loss = expectile_loss(q_t - v, L.expectile).mean()
    L.opt_value.zero_grad(set_to_none=True)
    value_loss.backward()
    L.opt_value.step()
    # actor
    with torch.no_grad():
        new_v = L.value.v(obs) if old_v_for_mistake is None else old_v_for_mistake
        q_t = torch.min(*L.target(obs, actions))
        adv = q_t - new_v
        exp_a = torch.exp(adv * L.temperature).clamp(max=100.0)
    actor_loss = -(exp_a * L.actor.log_prob(obs, actions)).mean()
    L.opt_actor.zero_grad(set_to_none=True)
    actor_loss.backward()
    L.opt_actor.step()
    if L.mistake != "constant_lr":
        L.sched.step()
    # critic
    with torch.no_grad():
        target_q = rewards + L.gamma * masks * L.value.v(next_obs)
    q1, q2 = L.critic(obs, actions)
    critic_loss = ((q1 - target_q) ** 2 + (q2 - target_q) ** 2).mean()
    L.opt_critic.zero_grad(set_to_none=True)
    critic_loss.backward()
    L.opt_critic.step()
    if L.mistake != "no_soft_update":
        L.soft_update()
    metrics = torch.stack([critic_loss.detach(), q1.detach().mean(), q2.detach().mean(), value_loss.detach(), v.detach().mean(),
                           actor_loss.detach(), adv.mean(), adv.std()])
    return metrics, float(L.opt_actor.param_groups[0]["lr"])


# ---- shared inputs of the tests -------------------------------------------------------------------------------------------
SHAPES = ((17, 6), (1, 1), (64, 32), (11, 3))
BATCHES = (1, 32, 67)
LOOP = dict(lr=1e-3, max_steps=8, gamma=0.8, tau=0.05, expectile=0.8, temperature=3.0)


def make_batch(shape, m, seed=0, clamp_actions=None):
    """float64 on the CPU.  Actions are tanh(randn); for m >= 32 two planted rows hold an exact +1 and an exact -1."""
    D, A = shape
    g = torch.Generator().manual_seed(1000 * D + 10 * A + m + 7919 * seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    b = {"obs": r(m, D), "actions": torch.tanh(r(m, A)), "rewards": r(m), "next_obs": r(m, D),
         "masks": (torch.rand(m, generator=g) > 0.3).to(torch.float64)}
    if m >= 32 and clamp_actions is None:
        b["actions"][3, 0], b["actions"][m - 2, A - 1] = 1.0, -1.0
        b["masks"][0], b["masks"][1] = 0.0, 1.0
    if clamp_actions is not None:
        b["actions"] = b["actions"].clamp(-clamp_actions, clamp_actions)
    # float32-representable inputs, so that the float32 and float64 runs see the same numbers
    return {k: v.float().double() for k, v in b.items()}


def make_learner(shape, dtype, weights="init", seed=5, **kw):
    torch.manual_seed(seed)
    L = IqlLearner(shape[0], shape[1], dtype=torch.float32, **kw)
    if weights == "perturbed":
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for m in (L.actor, L.critic, L.value):
                for p in m.parameters():
                    p.add_(0.05 * torch.randn(p.shape, generator=g))
            L.target.load_state_dict(L.critic.state_dict())
            for p in L.target.parameters():
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    for m in L.modules().values():
        m.to(dtype)
    opts = dict(lr=kw.get("lr", 3e-4), betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8), max_steps=kw.get("max_steps", 1))
    L.build_optimizers(**opts)  # over the converted parameters
    return L


def cast(batch, dtype, device="cpu"):
    return {k: v.to(dtype).to(device) for k, v in batch.items()}
