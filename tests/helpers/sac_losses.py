"""What the reference's SAC learner computes from the model calls, restated in a few lines each: ``forward_critic``,
``forward_actor`` and ``forward_alpha`` of rlinf/workers/actor/fsdp_sac_policy_worker.py:346-549 for the default Q head (no CrossQ,
no DSRL, no critic subsampling).  The worker file itself is not staged for the GPU machine; tests/test_sac_policy_host.py shows,
where the reference tree is readable, that these give bit-equal losses and gradients to the worker's own methods.

``ft`` is the reference's ``ForwardType`` enum.  ``eps``: N(0,1) draws to inject into the policy's rsample (both the HIP module,
through its ``eps=`` argument, and the reference's torch module, through ``injected_noise``); None = the model draws its own."""

from contextlib import contextmanager

import torch
import torch.nn.functional as F


@contextmanager
def injected_noise(eps):
    """Make torch's Normal.rsample / .sample use ``eps`` as their standard-normal draws (the reference's torch module)."""
    if eps is None:
        yield
        return
    import torch.distributions.normal as N

    saved = N._standard_normal, torch.normal
    N._standard_normal = lambda shape, dtype, device: eps.to(device=device, dtype=dtype).reshape(shape)
    torch.normal = lambda mean, std, **kw: mean + eps.to(device=mean.device, dtype=mean.dtype).reshape(mean.shape) * std
    try:
        yield
    finally:
        N._standard_normal, torch.normal = saved


def policy(model, ft, obs, eps=None):
    """-> (action, log_pi summed over the action dimension [M, 1])"""
    with injected_noise(eps):
        action, log_pi, _ = model(forward_type=ft.SAC, obs=obs, **({} if eps is None else {"eps": eps}))
    if log_pi.ndim == 1:
        log_pi = log_pi.unsqueeze(-1)
    return action, log_pi.sum(dim=-1, keepdim=True)


def _aggregate(q, agg_q):
    return torch.min(q, dim=1, keepdim=True)[0] if agg_q == "min" else torch.mean(q, dim=1, keepdim=True)


def critic_loss(model, target_model, ft, batch, alpha, *, gamma, agg_q="min", bootstrap_type="standard", backup_entropy=True,
                eps=None, dtype=None):
    dtype = dtype or next(model.parameters()).dtype
    rewards = batch["rewards"].sum(dim=-1, keepdim=True).to(dtype)
    terminations = batch["terminations"].to(dtype)
    with torch.no_grad():
        next_actions, next_log_pi = policy(model, ft, batch["next_obs"], eps)
        q_next = _aggregate(target_model(forward_type=ft.SAC_Q, obs=batch["next_obs"], actions=next_actions, shared_feature=None),
                            agg_q)
        if backup_entropy:
            q_next = (q_next - alpha * next_log_pi).to(dtype=dtype)
        if bootstrap_type == "always":
            target_q = rewards + gamma * q_next
        elif bootstrap_type == "standard":
            target_q = rewards + (~(terminations.any(dim=-1, keepdim=True))) * gamma * q_next
        else:
            raise NotImplementedError(f"{bootstrap_type=} is not supported!")
    q_data = model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=batch["actions"])
    return F.mse_loss(q_data, target_q.to(dtype=q_data.dtype).expand_as(q_data))


def actor_loss(model, ft, batch, alpha, *, agg_q="min", eps=None, keep=None):
    """``keep``: a dict that receives ``pi`` (with its gradient retained: d loss / d pi is what sac_q_forward's backward returns)."""
    pi, log_pi = policy(model, ft, batch["curr_obs"], eps)
    if keep is not None:
        pi.retain_grad()
        keep["pi"] = pi
    q_pi = _aggregate(model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=pi, shared_feature=None, detach_encoder=True), agg_q)
    return ((alpha * log_pi) - q_pi).mean(), -log_pi.mean()


def alpha_loss(model, ft, batch, alpha_tensor, target_entropy, *, eps=None):
    with torch.no_grad():
        _, log_pi = policy(model, ft, batch["curr_obs"], eps)
    return -alpha_tensor * (log_pi.mean() + target_entropy)
