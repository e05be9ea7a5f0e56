"""Times the eight model calls of ONE SAC update of the MLP policy (fsdp_sac_policy_worker.py:346-549) on the GPU: the HIP module
(rlinf_amd/models/embodiment/sac_mlp_policy.py) against the same reference-named parameters driven through eager torch.

    python tools/sac_model_calls_probe.py [--m 1024] [--runs 10] [--warmup 3] [--out profiles/sac_mlp_model_calls.txt]

The calls, in the learner's order:  1 actor forward on next_obs (no grad)   2 target-Q forward (no grad)   3 data-Q forward
4 critic backward   5 actor forward on curr_obs   6 policy-Q forward (actions = pi)   7 actor backward (through Q into the actor)
8 actor forward for the alpha loss (no grad).  Each call is timed with device events around it (median of --runs after --warmup);
the two implementations alternate within one process.  Launch counts come from torch's profiler in a pass of its own.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


class EagerTorch:
    """The reference's arithmetic (mlp_policy.py:179-200,322-323; q_head.py) in eager torch over a SacMLPPolicy's own parameters."""

    def __init__(self, module):
        self.m = module

    def sac(self, states, eps):
        m = self.m
        feat = m.backbone(states)
        mean, logstd = m.actor_mean(feat), torch.tanh(m.actor_logstd(feat))
        logstd = m.logstd_range[0] + 0.5 * (m.logstd_range[1] - m.logstd_range[0]) * (logstd + 1)
        std = torch.exp(logstd)
        raw = mean + std * eps
        a_n = torch.tanh(raw)
        logprob = -((raw - mean) ** 2) / (2 * std ** 2) - torch.log(std) - 0.9189385332046727
        return a_n * m.action_scale + m.action_bias, logprob - torch.log(m.action_scale * (1 - a_n.pow(2)) + 1e-6)

    def q(self, states, actions):
        x = torch.cat([states, actions], dim=-1)
        return torch.cat([qh.net(x) for qh in self.m.q_head.qs], dim=-1)


class Hip:
    def __init__(self, module):
        self.m = module

    def sac(self, states, eps):
        return self.m.sac_forward({"states": states}, eps=eps)[:2]

    def q(self, states, actions):
        return self.m.sac_q_forward({"states": states}, actions)


def one_update(impl, target_impl, batch, record):
    """record(name, fn) runs fn and returns its result; the learner's arithmetic between the calls is not timed."""
    model = impl.m
    with torch.no_grad():
        a2, lp2 = record("1 actor fwd next_obs (no grad)", lambda: impl.sac(batch["next"], batch["eps_next"]))
        qn = record("2 target-Q fwd (no grad)", lambda: target_impl.q(batch["next"], a2))
        target_q = batch["rewards"] + 0.8 * (qn.min(1, keepdim=True)[0] - 0.2 * lp2.sum(-1, keepdim=True))
    q = record("3 data-Q fwd", lambda: impl.q(batch["curr"], batch["actions"]))
    loss = F.mse_loss(q, target_q.expand_as(q))
    record("4 critic bwd", loss.backward)
    model.zero_grad(set_to_none=True)
    pi, lp = record("5 actor fwd curr_obs", lambda: impl.sac(batch["curr"], batch["eps_curr"]))
    qpi = record("6 policy-Q fwd", lambda: impl.q(batch["curr"], pi))
    loss = (0.2 * lp.sum(-1, keepdim=True) - qpi.min(1, keepdim=True)[0]).mean()
    record("7 actor bwd", loss.backward)
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        record("8 actor fwd alpha (no grad)", lambda: impl.sac(batch["curr"], batch["eps_curr"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this probe measures on the GPU and has no fallback")
    import copy

    from rlinf_amd.models.embodiment.sac_mlp_policy import SacMLPPolicy

    dev, (D, A, C) = torch.device("cuda"), (42, 4, 1)
    torch.manual_seed(0)
    model = SacMLPPolicy(D, A, C, False, True).to(dev)
    target = copy.deepcopy(model)
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    batch = dict(curr=r(a.m, D), next=r(a.m, D), actions=torch.tanh(r(a.m, A)), rewards=r(a.m, 1), eps_curr=r(a.m, A), eps_next=r(a.m, A))
    impls = {"hip": (Hip(model), Hip(target)), "torch": (EagerTorch(model), EagerTorch(target))}
    times = {k: {} for k in impls}

    def timed(store):
        def record(name, fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            t1.synchronize()
            if store is not None:
                store.setdefault(name, []).append(t0.elapsed_time(t1) * 1e3)
            return out
        return record

    for it in range(a.warmup + a.runs):
        for k, (impl, timpl) in impls.items():  # alternate the two within the process
            one_update(impl, timpl, batch, timed(times[k] if it >= a.warmup else None))

    with torch.no_grad():  # faster and different is not faster: the two must agree at the size that is timed
        (ah, lh_), (at, lt_) = impls["hip"][0].sac(batch["curr"], batch["eps_curr"]), impls["torch"][0].sac(batch["curr"], batch["eps_curr"])
        qh, qt = impls["hip"][0].q(batch["curr"], batch["actions"]), impls["torch"][0].q(batch["curr"], batch["actions"])
        agree = f"max |hip - torch|: action {(ah - at).abs().max().item():.2e}  logprob {(lh_ - lt_).abs().max().item():.2e}  q {(qh - qt).abs().max().item():.2e}"
    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile

        for k, (impl, timpl) in impls.items():
            counts = {}

            def record(name, fn):
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    out = fn()
                    torch.cuda.synchronize()
                counts[name] = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower())
                return out
            one_update(impl, timpl, batch, record)
            launches[k] = counts
    except Exception as e:  # the profiler is optional: the timings stand without it
        launches = {"error": repr(e)}

    lines = [f"SAC model calls, MLP policy (obs {D}, action {A}, chunks {C}), M = {a.m}, float32; device {torch.cuda.get_device_name(0)}",
             f"median of {a.runs} runs after {a.warmup} warm-ups, device events around each call, microseconds; launches = device kernels"
             " and memsets per call (torch profiler)", "",
             f"{'call':34s} {'hip us':>10s} {'torch us':>10s} {'torch/hip':>10s} {'hip launches':>13s} {'torch launches':>15s}"]
    tot = {"hip": 0.0, "torch": 0.0}
    for name in times["hip"]:
        h, t = statistics.median(times["hip"][name]), statistics.median(times["torch"][name])
        tot["hip"] += h
        tot["torch"] += t
        lh = launches.get("hip", {}).get(name, "n/a") if "error" not in launches else "n/a"
        lt = launches.get("torch", {}).get(name, "n/a") if "error" not in launches else "n/a"
        lines.append(f"{name:34s} {h:10.1f} {t:10.1f} {t / h:10.2f} {str(lh):>13s} {str(lt):>15s}")
    lines.append(f"{'sum of the eight calls':34s} {tot['hip']:10.1f} {tot['torch']:10.1f} {tot['torch'] / tot['hip']:10.2f}")
    lines.append(agree)
    if "error" in launches:
        lines.append(f"launch counts not measured: {launches['error']}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
