"""The cases of tests/test_gpu_iql.py, each written twice over the same inputs: ``ref_*`` on the restatement (helpers/iql_torch.py,
CPU, any dtype) and ``hip_*`` on the HIP kernels (run in the child process).  Both return dicts of named CPU float64 tensors."""

import math

import torch

from helpers import iql_torch as T

WEIGHTS = ("init", "perturbed")


def all_cases():
    cases = [(s, m, w) for s in T.SHAPES for m in T.BATCHES for w in WEIGHTS]
    cases.append(((17, 6), 256, "perturbed"))
    cases.append(((17, 6), 32, "logstd"))  # actor_logstd entries at 2.5, -5.5 and exactly 2.0
    return cases


def case_id(shape, m, weights):
    return f"D{shape[0]}A{shape[1]}-m{m}-{weights}"


def learner_for(shape, weights, dtype, **kw):
    L = T.make_learner(shape, dtype, "perturbed" if weights == "logstd" else weights, **kw)
    if weights == "logstd":
        with torch.no_grad():
            L.actor.actor_logstd[0, 0], L.actor.actor_logstd[0, 1], L.actor.actor_logstd[0, 2] = 2.5, -5.5, 2.0
    return L


def aux(shape, m):
    """Seeded upstream gradients and loss-leg inputs (float64, float32-representable)."""
    D, A = shape
    g = torch.Generator().manual_seed(31 * D + 7 * A + m)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    a = {"d_lp": r(m) / m, "d_v": r(m) / m, "d_q": r(2, m) / m, "q_target": r(2, m), "v": r(m), "q_min": r(m), "new_v": r(m),
         "q": r(2, m), "next_v": r(m)}
    a["new_v"][0] = a["q_min"][0] - 5.0  # adv = 5: exp(5 * 3) > 100, the clamp is active
    if m >= 2:
        a["v"][0], a["v"][1] = a["q_target"].min(0)[0][0] - 0.5, a["q_target"].min(0)[0][1] + 0.5  # diff of both signs
    return {k: t.float().double() for k, t in a.items()}


def _named_grads(module, prefix):
    return {f"{prefix}/{n}": p.grad.detach().double().clone() for n, p in module.named_parameters()}


# ---- restatement ------------------------------------------------------------------------------------------------------------
def ref_case(shape, m, weights, dtype):
    L = learner_for(shape, weights, dtype)
    b, bg, a = T.cast(T.make_batch(shape, m), dtype), T.cast(T.make_batch(shape, m, clamp_actions=0.999), dtype), T.cast(aux(shape, m), dtype)
    out = {}
    with torch.no_grad():
        out["fwd/actor_mean"] = L.actor.actor_mean_of(b["obs"])
        out["fwd/value"] = L.value.v(b["obs"])
        out["fwd/value_next"] = L.value.v(b["next_obs"])
        out["fwd/critic"] = torch.stack(L.critic(b["obs"], b["actions"]))
        out["fwd/logprob"] = L.actor.log_prob(b["obs"], b["actions"])
    # backwards from seeded upstream gradients
    for mod in (L.actor, L.value, L.critic):
        mod.zero_grad(set_to_none=True)
    (L.actor.log_prob(bg["obs"], bg["actions"]) * a["d_lp"]).sum().backward()
    (L.value.v(bg["obs"]) * a["d_v"]).sum().backward()
    (torch.stack(L.critic(bg["obs"], bg["actions"])) * a["d_q"]).sum().backward()
    out.update(_named_grads(L.actor, "grad/actor")), out.update(_named_grads(L.value, "grad/value")), out.update(_named_grads(L.critic, "grad/critic"))
    # loss legs
    v = a["v"].clone().requires_grad_(True)
    q_min = torch.min(a["q_target"][0], a["q_target"][1])
    loss = T.expectile_loss(q_min - v, 0.8).mean()
    loss.backward()
    out["loss/value/d_v"], out["loss/value/q_min"] = v.grad, q_min
    out["loss/value/metrics"] = torch.stack([loss.detach(), a["v"].mean()])
    adv = a["q_min"] - a["new_v"]
    exp_a = torch.exp(adv * 3.0).clamp(max=100.0)
    with torch.no_grad():
        lp = L.actor.log_prob(bg["obs"], bg["actions"])
    out["loss/actor/d_lp"] = -exp_a / m
    out["loss/actor/metrics"] = torch.stack([-(exp_a * lp).mean(), adv.mean()])
    out["loss/actor/adv_std"] = adv.std().reshape(1)
    q = a["q"].clone().requires_grad_(True)
    target = b["rewards"] + 0.8 * b["masks"] * a["next_v"]
    closs = ((q[0] - target) ** 2 + (q[1] - target) ** 2).mean()
    closs.backward()
    out["loss/critic/d_q"] = q.grad
    out["loss/critic/metrics"] = torch.stack([closs.detach(), a["q"][0].mean(), a["q"][1].mean()])
    return {k: t.detach().double().cpu() for k, t in out.items()}


def ref_optim(dtype, n=1037, slabs=3, steps=3):
    g = torch.Generator().manual_seed(77)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    p0, grads, t0, c0 = r(n), [r(slabs, n) for _ in range(steps)], r(n), r(n)
    p = p0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for s in range(steps):
        p.grad = grads[s].to(dtype).sum(0)
        opt.step()
    t = [t0.to(dtype).clone()]
    torch._foreach_mul_(t, 1.0 - 0.05)
    torch._foreach_add_(t, [c0.to(dtype)], alpha=0.05)
    st = opt.state[p]
    return {"adam/params": p.detach().double(), "adam/exp_avg": st["exp_avg"].double(), "adam/exp_avg_sq": st["exp_avg_sq"].double(),
            "soft/target": t[0].double()}, (p0, grads, t0, c0)


def loop_batches(m, steps=5):
    return [T.make_batch((17, 6), m, seed=s + 1) for s in range(steps)]


def ref_loop(m, dtype, mistake=None):
    L = T.make_learner((17, 6), dtype, "init", **T.LOOP)
    L.mistake = mistake
    metrics, lrs = [], []
    for b in loop_batches(m):
        b = T.cast(b, dtype)
        mt, lr = T.iql_update_step(L, b["obs"], b["actions"], b["rewards"], b["masks"], b["next_obs"])
        metrics.append(mt.double()), lrs.append(lr)
    out = {"metrics": torch.stack(metrics), "lr_actor": torch.tensor(lrs, dtype=torch.float64)}
    for name, mod in L.modules().items():
        out.update({f"{name}/{n}": p.detach().double().clone() for n, p in mod.named_parameters()})
    return out


# ---- HIP (child process) ----------------------------------------------------------------------------------------------------
def _load_nets(L, shape, dev):
    from rlinf_amd.models.embodiment.iql_mlp import IqlNetworks

    nets = IqlNetworks(shape[0], shape[1], dev)
    for name, mod in L.modules().items():
        getattr(nets, name).load_state_dict({k: v.detach().float() for k, v in mod.state_dict().items()})
    return nets


def _views_of_grads(net, grads):
    """Slab sum on the host in float64, then the named views."""
    flat = grads.double().sum(0).cpu()
    return {n: flat[o:o + math.prod(shape)].view(shape).clone() for n, (o, shape) in net._views.items()}


def hip_case(shape, m, weights, dev):
    from rlinf_amd import ops

    f32 = torch.float32
    L = learner_for(shape, weights, f32)
    nets = _load_nets(L, shape, dev)
    b, bg, a = T.cast(T.make_batch(shape, m), f32, dev), T.cast(T.make_batch(shape, m, clamp_actions=0.999), f32, dev), T.cast(aux(shape, m), f32, dev)
    out = {}
    for train in (False, True):
        sfx = ".saved" if train else ""
        mean, _, lp = nets.actor.forward(b["obs"], train=train, logprob_of=b["actions"])
        out["fwd/actor_mean" + sfx], out["fwd/logprob" + sfx] = mean[0], lp
        out["fwd/value" + sfx] = nets.value.forward(b["obs"], train=train)[0].view(-1)
        out["fwd/critic" + sfx] = nets.critic.forward(b["obs"], actions=b["actions"], train=train)[0].view(2, m)
    out["fwd/actor_mean.nolp"] = nets.actor.forward(b["obs"])[0][0]
    out["fwd/value_next"] = nets.value.forward(b["next_obs"])[0].view(-1)
    out["fwd/value_cat"] = nets.value.forward(b["obs"], obs2=b["next_obs"])[0].view(-1)
    # backwards
    mean, acts, _ = nets.actor.forward(bg["obs"], train=True, logprob_of=bg["actions"])
    d_mean, d_logstd = ops.iql_logprob_bwd(nets.actor.flat, nets.actor.layout, mean, bg["actions"], a["d_lp"])
    g = nets.actor.backward(bg["obs"], None, acts, d_mean, d_logstd)
    out.update({f"grad/actor/{n}": t for n, t in _views_of_grads(nets.actor, g).items()})
    _, acts, _ = nets.value.forward(bg["obs"], train=True)
    g = nets.value.backward(bg["obs"], None, acts, a["d_v"])
    out.update({f"grad/value/{n}": t for n, t in _views_of_grads(nets.value, g).items()})
    _, acts, _ = nets.critic.forward(bg["obs"], actions=bg["actions"], train=True)
    g = nets.critic.backward(bg["obs"], bg["actions"], acts, a["d_q"])
    out.update({f"grad/critic/{n}": t for n, t in _views_of_grads(nets.critic, g).items()})
    # loss legs
    mt = torch.full((8,), float("nan"), dtype=f32, device=dev)
    d_v, q_min = ops.iql_value_loss(a["q_target"], a["v"], 0.8, mt)
    out["loss/value/d_v"], out["loss/value/q_min"] = d_v, q_min
    mean, _, lp = nets.actor.forward(bg["obs"], logprob_of=bg["actions"])
    _, _, d_lp = ops.iql_actor_loss(nets.actor.flat, nets.actor.layout, a["q_min"], a["new_v"], lp, mean, bg["actions"], 3.0, mt)
    out["loss/actor/d_lp"] = d_lp
    out["loss/critic/d_q"] = ops.iql_critic_loss(a["q"], a["next_v"], b["rewards"], b["masks"], 0.8, mt)
    torch.cuda.synchronize()
    mt = mt.cpu()
    out["loss/value/metrics"], out["loss/actor/metrics"], out["loss/actor/adv_std"] = mt[3:5], mt[5:7], mt[7:8]
    out["loss/critic/metrics"] = mt[0:3]
    return {k: t.detach().double().cpu() for k, t in out.items()}


def hip_optim(dev, inputs, steps=3):
    from rlinf_amd import ops

    p0, grads, t0, c0 = inputs
    f = lambda t: t.float().to(dev).contiguous()  # noqa: E731
    p, m, v = f(p0), torch.zeros(p0.numel(), device=dev), torch.zeros(p0.numel(), device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    for s in range(steps):
        ops.clip_adamw_step_(p, f(grads[s]), m, v, [(0, p.numel(), 1e-3)], 0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                             max_grad_norm=0.0, step_state=state)
    t = ops.soft_update_(f(t0), f(c0), 0.05)
    assert state.cpu().sum().item() == steps  # {steps folded in, one pending}
    return {"adam/params": p.double().cpu(), "adam/exp_avg": m.double().cpu(), "adam/exp_avg_sq": v.double().cpu(),
            "soft/target": t.double().cpu()}


def loop_cfg(m, local_update_steps=4, max_steps=8):
    from rlinf_amd.config import DictConfig

    optim = dict(lr=T.LOOP["lr"], adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8)
    return DictConfig({
        "runner": {"task_type": "offline", "only_eval": False, "max_steps": max_steps, "local_update_steps": local_update_steps},
        "algorithm": {"hidden_dims": [256, 256], "gamma": T.LOOP["gamma"], "tau": T.LOOP["tau"], "expectile": T.LOOP["expectile"],
                      "temperature": T.LOOP["temperature"], "dropout_rate": None},
        "data": {"dataset_type": "synthetic", "seed": 42, "shuffle": True, "size": 300},
        "actor": {"seed": 5, "micro_batch_size": m, "global_batch_size": m, "optim": dict(optim), "critic_optim": dict(optim),
                  "value_optim": dict(optim),
                  "model": {"num_action_chunks": 1, "obs_dim": 17, "action_dim": 6,
                            "iql_config": {"type": "actor", "hidden_dims": [256, 256], "dropout_rate": None, "state_dependent_std": False,
                                           "log_std_min": -5.0, "log_std_max": 2.0}}},
    })


def hip_loop(m, dev):
    from rlinf_amd.config import validate_cfg
    from rlinf_amd.workers.actor.fsdp_iql_policy_worker import EmbodiedIQLFSDPPolicy

    w = EmbodiedIQLFSDPPolicy(validate_cfg(loop_cfg(m)), device=dev)
    w.init_worker()
    L = T.make_learner((17, 6), torch.float32, "init", **T.LOOP)
    for name, mod in L.modules().items():  # the same start as the restatement's (init parity has its own test)
        getattr(w.nets, name).load_state_dict({k: v.detach().float() for k, v in mod.state_dict().items()})
    metrics, lrs = [], []
    for b in loop_batches(m):
        b = T.cast(b, torch.float32, dev)
        info = w.update_one_epoch((b["obs"], b["actions"], b["rewards"], b["masks"], b["next_obs"]))
        metrics.append(torch.stack([info[k] for k in T.METRICS]).double().cpu()), lrs.append(info["lr_actor"])
    out = {"metrics": torch.stack(metrics), "lr_actor": torch.tensor(lrs, dtype=torch.float64)}
    for name in ("actor", "critic", "value", "target"):
        out.update({f"{name}/{n}": v.double().cpu().clone() for n, v in getattr(w.nets, name).views.items()})
    return out


def hip_run_training(dev, tmpdir):
    """3 calls x 4 steps, checkpoint, reload into a new learner, one more call -- and the same 16 steps uninterrupted."""
    from rlinf_amd.config import validate_cfg
    from rlinf_amd.workers.actor.fsdp_iql_policy_worker import EmbodiedIQLFSDPPolicy

    def fresh():
        w = EmbodiedIQLFSDPPolicy(validate_cfg(loop_cfg(67, max_steps=100)), device=dev)
        w.init_worker()
        return w

    a = fresh()
    res_a = [a.run_training() for _ in range(4)]
    b = fresh()
    res_b = [b.run_training() for _ in range(3)]
    b.save_checkpoint(tmpdir, 12)
    c = fresh()
    c.load_checkpoint(tmpdir)
    res_b.append(c.run_training())
    out = {"a/results": res_a, "b/results": res_b}
    for tag, w in (("a", a), ("b", c)):
        for name in ("actor", "critic", "value", "target"):
            out[f"{tag}/{name}"] = getattr(w.nets, name).flat.cpu().clone()
        for name, ad in w._adam.items():
            out[f"{tag}/{name}/exp_avg"], out[f"{tag}/{name}/exp_avg_sq"] = ad.exp_avg.cpu().clone(), ad.exp_avg_sq.cpu().clone()
            out[f"{tag}/{name}/steps"] = ad.step_state.cpu().clone()
    return out


def probe(t, name):
    """A parameter tensor's 2-norm and its dot products with 8 seeded Gaussian vectors (what tests/golden/iql_step.pt records)."""
    import zlib

    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    flat = t.double().reshape(-1)
    return torch.cat([flat.norm().reshape(1), torch.randn(8, flat.numel(), generator=g, dtype=torch.float64) @ flat])
