"""The REAL reference's offline IQL on the CPU, where the reference tree exists: ``iql_mlp_policy.py`` executed by path behind
``oracle.reference_loader.load()``, and the worker's update methods compiled on their own over a stand-in ``self`` (the worker's
module needs Ray, omegaconf and FSDP).  Used by tests/test_iql_restatement_vs_reference.py and tools/make_iql_golden.py."""

import importlib.util
import os
import sys

import torch

from oracle import reference_loader as RL

POLICY = "rlinf/models/embodiment/mlp_policy/iql_mlp_policy.py"
WORKER = "rlinf/workers/actor/fsdp_iql_policy_worker.py"
METHODS = ("forward_value", "forward_actor", "forward_critic", "update_step_forward", "soft_update_target_model")


def available():
    return RL.available() and os.path.isfile(os.path.join(RL.REFERENCE_ROOT, POLICY)) and os.path.isfile(os.path.join(RL.REFERENCE_ROOT, WORKER))


_policy = None


def policy_module():
    global _policy
    if _policy is None:
        RL.load()
        name = "rlinf.models.embodiment.mlp_policy.iql_mlp_policy"
        spec = importlib.util.spec_from_file_location(name, os.path.join(RL.REFERENCE_ROOT, POLICY))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        _policy = mod
    return _policy


def build_module(kind, obs_dim, action_dim):
    pm = policy_module()
    m = pm.IQLMLPPolicy(obs_dim, action_dim, 1, kind == "actor", False)
    m.configure_iql({"type": kind, "hidden_dims": (256, 256), "dropout_rate": None, "state_dependent_std": False, "log_std_min": -5.0,
                     "log_std_max": 2.0})
    return m


class ReferenceLearner:
    """The reference worker's construction order and its own update methods."""

    def __init__(self, obs_dim, action_dim, dtype=torch.float32, lr=3e-4, max_steps=1, gamma=0.99, tau=0.005, expectile=0.7,
                 temperature=3.0):
        pm = policy_module()
        ft = RL.load().mlp_policy.ForwardType
        twin = lambda: pm.IQLTwinCritic(build_module("critic", obs_dim, action_dim), build_module("critic", obs_dim, action_dim))  # noqa: E731
        self.model = build_module("actor", obs_dim, action_dim)
        self.critic_model = twin()
        self.value_model = build_module("value", obs_dim, action_dim)
        self.target_model = twin()
        self.target_model.load_state_dict(self.critic_model.state_dict(), strict=True)
        for m in (self.model, self.critic_model, self.value_model, self.target_model):
            m.to(dtype)
        for p in self.target_model.parameters():
            p.requires_grad_(False)
        self.target_model_initialized, self._use_fsdp_wrap = True, False
        self._critic_params, self._target_params = list(self.critic_model.parameters()), list(self.target_model.parameters())
        self.discount, self.tau, self.expectile, self.temperature = float(gamma), float(tau), float(expectile), float(temperature)
        mk = lambda m: torch.optim.Adam(m.parameters(), lr=float(lr), betas=(0.9, 0.999), eps=1e-8)  # noqa: E731
        self.optimizer, self.vf_optimizer, self.qf_optimizer = mk(self.model), mk(self.value_model), mk(self.critic_model)
        self.lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=max(1, int(max_steps)), eta_min=0.0)
        self.ForwardType = ft

    def modules(self):
        return {"actor": self.model, "critic": self.critic_model, "value": self.value_model, "target": self.target_model}


def _bind():
    ft = RL.load().mlp_policy.ForwardType
    loss = RL.load_function(WORKER, "iql_expectile_loss", torch=torch)
    globs = dict(torch=torch, ForwardType=ft, iql_expectile_loss=loss)
    for name in METHODS:
        setattr(ReferenceLearner, name, RL.load_function(WORKER, "EmbodiedIQLFSDPPolicy." + name, **globs))
    ReferenceLearner.forward_critic_module = staticmethod(RL.load_function(WORKER, "EmbodiedIQLFSDPPolicy.forward_critic_module", **globs))
    ReferenceLearner.iql_expectile_loss = staticmethod(loss)


_bound = False


def make_learner(shape, dtype, seed=5, **kw):
    global _bound
    if not _bound:
        _bind()
        _bound = True
    torch.manual_seed(seed)
    return ReferenceLearner(shape[0], shape[1], dtype=dtype, **kw)


def run_loop(m, dtype, batches, cast, loop_kw):
    """-> metrics [steps, 8], lr_actor [steps] and the live parameters, named as the restatement names them."""
    L = make_learner((17, 6), dtype, **loop_kw)
    metrics, lrs = [], []
    for b in batches:
        b = cast(b, dtype)
        flat = L.update_step_forward(b["obs"], b["actions"], b["rewards"], b["masks"], b["next_obs"])
        metrics.append(flat.detach().double()), lrs.append(float(L.optimizer.param_groups[0]["lr"]))
    out = {"metrics": torch.stack(metrics), "lr_actor": torch.tensor(lrs, dtype=torch.float64)}
    return out, L
