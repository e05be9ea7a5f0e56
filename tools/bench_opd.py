#!/usr/bin/env python
"""Time the OPD launches at the LIBERO OPD shape against the same arithmetic as eager torch expressions, on one GPU.

    python tools/bench_opd.py [--steps 30] [--envs 512] [--chunks 8] [--action-dim 7] [--max-episode-steps 240]
                              [--windows 9] [--calls 20] [--dtype f32|bf16]

Shape: rollout_epoch 8 x 64 envs = 512 envs, max_steps_per_rollout_epoch 240 / 8 chunks = 30 chunk steps, 8 chunks x 7 action
dims = 56 tokens per env step.  Timed, each as `calls` back-to-back calls captured in one hipGraph, a window = one replay between
two device events, the median of `windows` windows divided by `calls`:
  adv_hip          ops.opd_advantages on the [T+1, B, C*A] buffers (one launch)
  adv_torch        (teacher.float() - prev.float()).reshape(..., C, A)[:T]
  loss_hip         ops.opd_loss forward + backward (three launches: stream pass, finalize, backward)
  loss_torch       loss = ((-lp * adv) / ratio * mask).mean() with ratio = mask_sum * 1.0 / max_episode_steps, the two masked-mean
                   metrics and the backward, as torch expressions (the all-False branch of masked_mean becomes a torch.where so that
                   the expression can be captured)
Bytes are the algorithm's: every input read once, every output written once; bytes_per_us is over the median time and is compared
with the 8 TB/s HBM peak.  Prints one JSON line."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--action-dim", type=int, default=7)
    ap.add_argument("--max-episode-steps", type=int, default=240)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_opd needs a GPU")
    if a.windows < 7:
        raise SystemExit("--windows must be at least 7")
    from rlinf_amd import ops

    dev = torch.device("cuda", 0)
    T, B, C, A, mes = a.steps, a.envs, a.chunks, a.action_dim, a.max_episode_steps
    K = C * A
    g = torch.Generator(device=dev).manual_seed(0)
    in_dtype = torch.float32 if a.dtype == "f32" else torch.bfloat16
    teacher = (-torch.rand(T + 1, B, K, device=dev, generator=g) * 5).to(in_dtype)
    prev = (-torch.rand(T + 1, B, K, device=dev, generator=g) * 5).to(in_dtype)
    n_rows = T * B
    lp = -torch.rand(n_rows, C, A, device=dev, generator=g) * 6
    adv = torch.randn(n_rows, C, A, device=dev, generator=g) * 0.5
    mask = torch.rand(n_rows, C, 1, device=dev, generator=g) < 0.85
    msum = torch.randint(1, mes + 1, (n_rows, C, 1), device=dev, generator=g)

    def adv_hip():
        return ops.opd_advantages(teacher, prev, C, T)

    def adv_torch():
        return (teacher.float() - prev.float()).reshape(T + 1, B, C, A)[:T]

    def loss_hip():
        x = lp.detach().requires_grad_(True)
        loss, out = ops.opd_loss(x, adv, mask, action_dim=A, loss_mask_sum=msum, max_episode_steps=mes)
        return torch.autograd.grad(loss, x)[0], out

    def loss_torch():
        x = lp.detach().requires_grad_(True)
        m = mask.expand_as(x)
        ratio = (msum.expand_as(x) * 1.0) / mes
        loss = ((-x * adv) / ratio * m).mean()
        cnt = m.sum()
        s = (adv * m).sum()
        reward = torch.where(cnt > 0, s / cnt, s)
        s_neg = (-adv * m).sum()
        reverse_kl = torch.where(cnt > 0, s_neg / cnt, s_neg)
        return torch.autograd.grad(loss, x)[0], loss.detach(), reward, reverse_kl

    # same answers before timing anything
    assert torch.equal(adv_hip(), adv_torch())
    gh, gt = loss_hip()[0], loss_torch()[0]
    assert float((gh - gt).norm() / gt.norm()) < 1e-5

    res = {}
    for name, fn in (("adv_hip", adv_hip), ("adv_torch", adv_torch), ("loss_hip", loss_hip), ("loss_torch", loss_torch)):
        res[name + "_us"] = round(graph_time_us(fn, a.calls, a.windows), 3)
    n = n_rows * K
    isz = torch.tensor([], dtype=in_dtype).element_size()
    adv_bytes = 2 * n * isz + n * 4                    # two inputs read (T of the T+1 rows), f32 written
    rows_bytes = (n // A) * (1 + 8)                    # mask (u8) and mask_sum (i64), one per row of A
    loss_bytes = (2 * n * 4 + rows_bytes) + (n * 4 + rows_bytes + n * 4)  # fwd: lp, adv; bwd: adv read, d_lp written
    res.update(shape=dict(T=T, B=B, C=C, A=A, elements=n, max_episode_steps=mes, input_dtype=a.dtype),
               windows=a.windows, calls_per_window=a.calls, adv_bytes=adv_bytes, loss_fwd_bwd_bytes=loss_bytes)
    for name, nbytes in (("adv_hip", adv_bytes), ("loss_hip", loss_bytes)):
        bpu = nbytes / res[name + "_us"]
        res[name + "_bytes_per_us"] = round(bpu, 1)
        res[name + "_share_of_8TBps"] = round(bpu / PEAK_BYTES_PER_US, 4)
    res["adv_speedup_vs_torch"] = round(res["adv_torch_us"] / res["adv_hip_us"], 2)
    res["loss_speedup_vs_torch"] = round(res["loss_torch_us"] / res["loss_hip_us"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
