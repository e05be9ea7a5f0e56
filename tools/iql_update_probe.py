"""Times ONE offline-IQL update of the MLP policy on the GPU: the HIP learner (rlinf_amd/workers/actor/fsdp_iql_policy_worker.py)
against the same update in eager torch (autograd, three torch.optim.Adam, _foreach soft update: tests/helpers/iql_torch.py).

    python tools/iql_update_probe.py [--m 256] [--blocks 10] [--updates 100] [--warmup 20] [--out profiles/iql_update_step.txt]

Microseconds per update = the median over --blocks blocks of --updates updates, device events around each block, after --warmup
updates; the two implementations alternate block by block within one process.  Launch counts (device kernels and memsets of one
update) come from torch's profiler in a pass of its own.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: this probe measures on the GPU and has no fallback")
    from helpers import iql_cases as C
    from helpers import iql_torch as T
    from rlinf_amd.config import validate_cfg
    from rlinf_amd.workers.actor.fsdp_iql_policy_worker import EmbodiedIQLFSDPPolicy

    dev, shape = torch.device("cuda"), (17, 6)
    total = a.warmup + a.blocks * a.updates
    hip = EmbodiedIQLFSDPPolicy(validate_cfg(C.loop_cfg(a.m, local_update_steps=a.updates, max_steps=2 * total)), device=dev)
    hip.init_worker()
    eager = T.make_learner(shape, torch.float32, "init", **dict(T.LOOP, max_steps=2 * total))
    for mod in eager.modules().values():
        mod.to(dev)
    eager.build_optimizers(T.LOOP["lr"], (0.9, 0.999), 1e-8, 2 * total)
    b = T.cast(T.make_batch(shape, a.m, seed=3), torch.float32, dev)
    batch = (b["obs"], b["actions"], b["rewards"], b["masks"], b["next_obs"])
    steps = {"hip": lambda: hip.update_one_epoch(batch), "torch": lambda: T.iql_update_step(eager, *batch)}

    for fn in steps.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(a.blocks):
        for k, fn in steps.items():  # alternate the two within the process
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.updates):
                fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1e3 / a.updates)

    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile

        for k, fn in steps.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            launches[k] = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower())
    except Exception as e:  # the profiler is optional: the timings stand without it
        launches = {"error": repr(e)}

    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"offline IQL update, MLP policy (obs {shape[0]}, action {shape[1]}), M = {a.m}, float32; device {torch.cuda.get_device_name(0)}",
             f"microseconds per update: median of {a.blocks} blocks of {a.updates} updates after {a.warmup} warm-ups, device events around "
             "each block; the two alternate block by block", "",
             f"{'':8s} {'median us':>10s} {'min us':>10s} {'max us':>10s} {'launches':>10s}"]
    for k in steps:
        n = launches.get(k, "n/a") if "error" not in launches else "n/a"
        lines.append(f"{k:8s} {med[k]:10.1f} {min(times[k]):10.1f} {max(times[k]):10.1f} {str(n):>10s}")
    lines.append(f"torch / hip: {med['torch'] / med['hip']:.2f}")
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
