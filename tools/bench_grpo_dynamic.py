#!/usr/bin/env python
"""Time multi-turn GRPO (grpo_dynamic) and the turn-level loss scale on one GPU against the same arithmetic as vectorized torch.

    python tools/bench_grpo_dynamic.py [--shape searchr1|rank] [--windows 9] [--calls 10]

Shapes: searchr1 = 512 prompts x group 4 = 2048 trajectories of 1-7 turns (about 8 k turn rows, unsorted), seq_len 7096;
rank = the 1024-row share of one rank (256 trajectories of 1-7 turns, group 4, seq_len 7096).  Timed, each as `calls`
back-to-back calls captured in one hipGraph (plans built outside), a window = one replay between two device events, the median
of `windows` windows divided by `calls`:
  adv_turn_hip / adv_traj_hip      token_ops.grpo_dynamic_adv, one launch
  adv_turn_torch / adv_traj_torch  the same arithmetic with index_add_ / gather in f32 (counts formed outside), masked broadcast
  turn_hip                         token_ops.turn_level_scale_ (one launch; the caller's flag read is not timed)
  turn_torch                       mask.sum(1), index_add_ of the group totals, the f64 factors, one f32 multiply
End to end (host clock around a synchronised call, median of `windows`): the public entries calculate_adv_and_returns and the
turn_level process, plan building and the flag read included.
Bytes are the algorithm's: advantages 1 B mask read + 4 B written per element; turn_level 1 B mask + 4 B read + 4 B written per
element.  Prints one JSON line."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BYTES_PER_US = 8.0e6  # 8 TB/s


def graph_time_us(fn, calls: int, windows: int) -> float:
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0 / calls)
    return statistics.median(times)


def wall_us(fn, windows: int) -> float:
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("searchr1", "rank"), default="searchr1")
    ap.add_argument("--seq", type=int, default=7096)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grpo_dynamic needs a GPU")
    if a.windows < 7:
        raise SystemExit("--windows must be at least 7")
    from rlinf_amd import token_ops
    from rlinf_amd.algorithms import calculate_adv_and_returns
    from rlinf_amd.algorithms import loss_scales as ls

    dev = torch.device("cuda", 0)
    G, seq = 4, a.seq
    num_traj = 2048 if a.shape == "searchr1" else 256
    g = torch.Generator().manual_seed(0)
    turns = torch.randint(1, 8, (num_traj,), generator=g)
    ids_cpu = torch.repeat_interleave(torch.arange(num_traj), turns)
    ids_cpu = ids_cpu[torch.randperm(ids_cpu.numel(), generator=g)]
    n = ids_cpu.numel()
    ids_list = ids_cpu.tolist()
    ids = ids_cpu.to(dev)
    r = (torch.rand(n, generator=g) < 0.5).float().to(dev)  # exact-match rewards
    mask = (torch.rand(n, seq, generator=g) < 0.85).to(dev)
    sub = torch.zeros(n, dtype=torch.long)
    plan = token_ops.GrpoDynamicPlan(ids_list, G, dev)
    order, offsets, _ = token_ops.loss_scale_groups(ids_list, sub.tolist())
    tplan = token_ops.TurnScalePlan(order, offsets, dev)
    scales = torch.rand(n, seq, device=dev)

    # torch restatement (vectorized, f32): what the reference's loops compute
    n_traj, nq = num_traj, num_traj // G
    q = ids // G
    # counts depend on idx_to_traj only: formed outside the timed region, like the HIP path's plan (bincount syncs)
    cnt_traj = torch.bincount(ids, minlength=n_traj).clamp(min=1)
    cnt_q = torch.bincount(q, minlength=nq)

    def adv_torch(mode):
        if mode == "trajectory":
            s = torch.zeros(n_traj, device=dev).index_add_(0, ids, r)
            tr = (s / cnt_traj).view(nq, G)
            adv = ((tr - tr.mean(1, keepdim=True)) / (tr.std(1, keepdim=True) + 1e-6)).view(-1)[ids]
        else:
            mean = torch.zeros(nq, device=dev).index_add_(0, q, r) / cnt_q
            var = torch.zeros(nq, device=dev).index_add_(0, q, (r - mean[q]) ** 2) / (cnt_q - 1)
            adv = (r - mean[q]) / (var.sqrt()[q] + 1e-6)
        return adv[:, None] * mask

    inv = torch.as_tensor(order, device=dev)  # rows of a group are contiguous in `order`
    grp = torch.empty(n, dtype=torch.long, device=dev)
    grp[inv] = torch.repeat_interleave(torch.arange(len(offsets) - 1, device=dev),
                                       torch.as_tensor(offsets[1:] - offsets[:-1], device=dev))
    t_cnt = torch.bincount(grp)[grp]

    def turn_torch():
        c = mask.sum(1)
        total = torch.zeros(len(offsets) - 1, dtype=torch.int64, device=dev).index_add_(0, grp, c)
        f = ((t_cnt * c).double() / total[grp].double()).float()
        scales.mul_(f[:, None])

    def turn_hip():
        token_ops.turn_level_scale_(scales, mask, tplan)

    # same answers before timing anything
    for mode in ("turn", "trajectory"):
        got, want = token_ops.grpo_dynamic_adv(r, mask, plan, mode), adv_torch(mode)
        assert float((got - want).abs().max()) < 1e-4, mode
    s0 = scales.clone()
    turn_hip()
    s1 = scales.clone()
    scales.copy_(s0)
    turn_torch()
    assert torch.equal(s1, scales)

    res = {}
    for name, fn in (("adv_turn_hip", lambda: token_ops.grpo_dynamic_adv(r, mask, plan, "turn")),
                     ("adv_turn_torch", lambda: adv_torch("turn")),
                     ("adv_traj_hip", lambda: token_ops.grpo_dynamic_adv(r, mask, plan, "trajectory")),
                     ("adv_traj_torch", lambda: adv_torch("trajectory")),
                     ("turn_hip", turn_hip), ("turn_torch", turn_torch)):
        res[name + "_us"] = round(graph_time_us(fn, a.calls, a.windows), 3)

    def e2e_adv():
        return calculate_adv_and_returns(task_type="reasoning", adv_type="grpo_dynamic", advantage_mode="turn", rewards=r,
                                         loss_mask=mask, num_sequence=n, group_size=G, idx_to_traj=ids_list)

    def e2e_turn():
        ls.turn_scale({"folding_scale": ["group_level", "agent_level"]},
                      {"idx_to_traj": ids_list, "extra:idx_to_sub_traj": sub, "response_mask": mask, "loss_scales": scales})

    res["e2e_adv_turn_us"] = round(wall_us(e2e_adv, a.windows), 1)
    res["e2e_turn_level_us"] = round(wall_us(e2e_turn, a.windows), 1)
    elems = n * seq
    adv_bytes, turn_bytes = elems * (1 + 4), elems * (1 + 4 + 4)
    res.update(shape=dict(name=a.shape, trajectories=num_traj, group_size=G, rows=n, seq_len=seq, elements=elems),
               windows=a.windows, calls_per_window=a.calls, adv_bytes=adv_bytes, turn_bytes=turn_bytes)
    for name, nbytes in (("adv_turn_hip", adv_bytes), ("adv_traj_hip", adv_bytes), ("turn_hip", turn_bytes)):
        bpu = nbytes / res[name + "_us"]
        res[name + "_share_of_8TBps"] = round(bpu / PEAK_BYTES_PER_US, 4)
    for base in ("adv_turn", "adv_traj", "turn"):
        res[base + "_speedup_vs_torch"] = round(res[base + "_torch_us"] / res[base + "_hip_us"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
