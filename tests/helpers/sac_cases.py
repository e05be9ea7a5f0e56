"""The cases of tests/test_gpu_sac_policy.py, run by ONE piece of code on any implementation of the SAC MLP policy: the HIP module
on the GPU in float32 (tests/helpers/sac_gpu_child.py) and the reference's torch module on the CPU in float64 and float32 (the
test itself).  Everything a case needs (weights, batch, noise) is drawn on the CPU from fixed seeds, so both sides see the same
numbers; every result comes back as a CPU tensor under a name."""

import copy

import torch

from helpers import sac_losses as SL

SHAPES = [(42, 4, 1), (9, 7, 2), (64, 8, 2), (1, 1, 1)]   # (obs_dim, action_dim, num_action_chunks)
BATCHES = [1, 32, 67]                                      # one row; one exact tile; two tiles and a three-row tail
WEIGHTS = ["init", "perturbed"]
GAMMA, TAU, ALPHA0, LR = 0.8, 0.005, 0.2, 3e-4
LOOP_SHAPE, LOOP_M, LOOP_STEPS = (42, 4, 1), 32, 5


def case_id(shape, m, weights):
    return f"D{shape[0]}A{shape[1]}C{shape[2]}-M{m}-{weights}"


def all_cases():
    return [(s, m, w) for s in SHAPES for m in BATCHES for w in WEIGHTS]


def make_model(cls, shape, weights, granularity="action_level", seed=5):
    """``cls(obs_dim, action_dim, chunks, add_value_head=False, add_q_head=True)`` after the same manual_seed (the two classes draw the
    same initial values: tests/test_sac_policy_host.py); "perturbed" adds 0.05 * randn to every parameter."""
    torch.manual_seed(seed)
    model = cls(shape[0], shape[1], shape[2], False, True, value_granularity=granularity)
    if weights == "perturbed":
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    return model


def make_batch(shape, m, seed=3):
    D, A, C = shape
    g = torch.Generator().manual_seed(seed + 1000 * m + D)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(curr_obs={"states": r(m, D)}, next_obs={"states": r(m, D)}, actions=torch.tanh(r(m, A * C)),
                rewards=torch.rand(m, C, generator=g), terminations=torch.rand(m, C, generator=g) < 0.3,
                eps_curr=r(m, A * C), eps_next=r(m, A * C))


def _to(batch, device, dtype):
    out = {}
    for k, v in batch.items():
        if isinstance(v, dict):
            out[k] = {kk: vv.to(device, dtype) for kk, vv in v.items()}
        else:
            out[k] = v.to(device) if v.dtype == torch.bool else v.to(device, dtype)
    return out


def _cpu(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _grads(model, prefix, out):
    for name, p in model.named_parameters():
        g = p.grad
        out[f"{prefix}/{name}"] = _cpu(torch.zeros_like(p) if g is None else g)  # None and zero are the same statement
        out[f"{prefix}.none/{name}"] = torch.tensor(float(g is None))
        p.grad = None


def run_case(cls, ft, device, dtype, shape, m, weights):
    """Forwards and the three losses' backwards of one case -> {name: CPU float64 tensor}."""
    out = {}
    batch = _to(make_batch(shape, m), device, dtype)
    model = make_model(cls, shape, weights).to(device=device, dtype=dtype)
    target = copy.deepcopy(model)
    with torch.no_grad():  # the target differs from the online network, as after soft updates
        g = torch.Generator().manual_seed(17)
        for p in target.parameters():
            p.add_((0.01 * torch.randn(p.shape, generator=g)).to(device, dtype))
    # ---- forwards -------------------------------------------------------------------------------------------------
    with SL.injected_noise(batch["eps_curr"]):
        action, logprob, _ = model(forward_type=ft.SAC, obs=batch["curr_obs"], eps=batch["eps_curr"])
        with torch.no_grad():
            action_ng, logprob_ng, _ = model(forward_type=ft.SAC, obs=batch["curr_obs"], eps=batch["eps_curr"])
    out["action"], out["logprob"], out["action.nograd"], out["logprob.nograd"] = map(_cpu, (action, logprob, action_ng, logprob_ng))
    out["q/action_level"] = _cpu(model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=batch["actions"]))
    with torch.no_grad():
        out["q.nograd/action_level"] = _cpu(model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=batch["actions"]))
        chunk_model = make_model(cls, shape, weights, "chunk_level").to(device=device, dtype=dtype)
        out["q/chunk_level"] = _cpu(chunk_model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=batch["actions"]))
    # ---- the three losses' backwards ----------------------------------------------------------------------------------
    for agg_q, bootstrap, backup in (("min", "standard", True), ("mean", "always", False)):
        tag = f"critic[{agg_q},{bootstrap}]"
        loss = SL.critic_loss(model, target, ft, batch, ALPHA0, gamma=GAMMA, agg_q=agg_q, bootstrap_type=bootstrap,
                              backup_entropy=backup, eps=batch["eps_next"])
        loss.backward()
        out[f"{tag}/loss"] = _cpu(loss)
        _grads(model, tag, out)
    for agg_q in ("min", "mean"):
        tag, keep = f"actor[{agg_q}]", {}
        loss, entropy = SL.actor_loss(model, ft, batch, ALPHA0, agg_q=agg_q, eps=batch["eps_curr"], keep=keep)
        loss.backward()
        out[f"{tag}/loss"], out[f"{tag}/entropy"], out[f"{tag}/d_actions"] = _cpu(loss), _cpu(entropy), _cpu(keep["pi"].grad)
        _grads(model, tag, out)
    base_alpha = torch.tensor(0.3, device=device, dtype=dtype, requires_grad=True)
    loss = SL.alpha_loss(model, ft, batch, torch.nn.functional.softplus(base_alpha), -float(shape[1] * shape[2]), eps=batch["eps_curr"])
    loss.backward()
    out["alpha/loss"], out["alpha/base_alpha.grad"] = _cpu(loss), _cpu(base_alpha.grad)
    _grads(model, "alpha", out)
    return out


def _soft_update(model, target, tau):  # the reference's soft_update_target_model, verbatim: writes through .data
    for param, target_param in zip(model.parameters(), target.parameters()):
        target_param.data.mul_(1.0 - tau)
        target_param.data.add_(param.data * tau)


def run_stale(cls, ft, device, dtype):
    """A forward, the reference's soft update (through ``.data``: no version counter moves) and an in-place optimizer step, the
    same forwards again: the second results must come from the NEW weights."""
    shape, m, out = (9, 7, 2), 32, {}
    batch = _to(make_batch(shape, m), device, dtype)
    model = make_model(cls, shape, "perturbed").to(device=device, dtype=dtype)
    target = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)

    def forwards(tag):
        with torch.no_grad(), SL.injected_noise(batch["eps_curr"]):
            out[f"{tag}/q_target"] = _cpu(target(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=batch["actions"]))
            out[f"{tag}/q_online"] = _cpu(model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=batch["actions"]))
            a, lp, _ = model(forward_type=ft.SAC, obs=batch["curr_obs"], eps=batch["eps_curr"])
            out[f"{tag}/action"], out[f"{tag}/logprob"] = _cpu(a), _cpu(lp)

    forwards("before")
    SL.critic_loss(model, target, ft, batch, ALPHA0, gamma=GAMMA, eps=batch["eps_next"]).backward()
    SL.actor_loss(model, ft, batch, ALPHA0, eps=batch["eps_curr"])[0].backward()
    opt.step()
    _soft_update(model, target, 0.5)
    forwards("after")
    return out


def run_predict(cls, ft, device, dtype):
    shape, m, out = (9, 7, 2), 67, {}
    batch = _to(make_batch(shape, m), device, dtype)
    model = make_model(cls, shape, "perturbed").to(device=device, dtype=dtype)
    for mode in ("train", "eval"):
        with SL.injected_noise(batch["eps_curr"]):
            chunk_actions, result = model.predict_action_batch(env_obs={"states": batch["curr_obs"]["states"]}, mode=mode,
                                                               eps=batch["eps_curr"])
        out[f"{mode}/chunk_actions"], out[f"{mode}/prev_logprobs"] = _cpu(chunk_actions), _cpu(result["prev_logprobs"])
        out[f"{mode}/prev_values"] = _cpu(result["prev_values"])
        out[f"{mode}/action"], out[f"{mode}/model_action"] = (_cpu(result["forward_inputs"][k]) for k in ("action", "model_action"))
        out[f"{mode}/states"] = _cpu(result["forward_inputs"]["states"])
        out[f"{mode}/keys"] = sorted(result) + sorted(result["forward_inputs"])
    return out


def run_loop(cls, ft, device, dtype):
    """Five consecutive SAC updates (critic step, actor step, soft update) with torch Adam and injected noise."""
    shape, m, out = LOOP_SHAPE, LOOP_M, {}
    model = make_model(cls, shape, "init").to(device=device, dtype=dtype)
    target = copy.deepcopy(model)
    critic = [p for n, p in model.named_parameters() if "q_head" in n]
    actor = [p for n, p in model.named_parameters() if "q_head" not in n]
    opt_q, opt_pi = torch.optim.Adam(critic, lr=LR), torch.optim.Adam(actor, lr=LR)
    critic_losses, actor_losses = [], []
    for step in range(LOOP_STEPS):
        batch = _to(make_batch(shape, m, seed=100 + step), device, dtype)
        opt_q.zero_grad(set_to_none=True)
        loss = SL.critic_loss(model, target, ft, batch, ALPHA0, gamma=GAMMA, eps=batch["eps_next"])
        loss.backward()
        opt_q.step()
        critic_losses.append(_cpu(loss))
        opt_pi.zero_grad(set_to_none=True)
        loss, _ = SL.actor_loss(model, ft, batch, ALPHA0, eps=batch["eps_curr"])
        loss.backward()
        opt_pi.step()
        actor_losses.append(_cpu(loss))
        _soft_update(model, target, TAU)
    out["critic_losses"], out["actor_losses"] = torch.stack(critic_losses), torch.stack(actor_losses)
    for name, p in model.named_parameters():
        out[f"param/{name}"] = _cpu(p)
    for name, p in target.named_parameters():
        out[f"target/{name}"] = _cpu(p)
    return out
