#!/usr/bin/env python
"""Time the "grpo_video" (frame, video) and "raw" (plain, normalised) advantages on one GPU against the same arithmetic composed
from what the tree had before adv_video_raw.hip: torch tensor ops on the device, and ops.masked_standardize_ for raw's
normalisation.

    python tools/bench_adv_video_raw.py [--windows 9] [--calls 10] [--shapes contract,diffusion,large,reasoning]

Shapes (n_chunk, B, C, G): contract (128, 1024, 1, 8), diffusion (16, 64, 16, 8), large (128, 65536, 1, 8); reasoning raw on a
(4096, 8192) mask.  Each entry is timed as `calls` back-to-back calls captured in one hipGraph; a window is one replay between
two device events, divided by `calls`; the median, minimum and maximum of `windows` windows are printed.  Both sides run in this
process, by this method, on the same buffers.  Timed:
  frame_hip / video_hip        ops.grpo_video_adv, one launch each
  frame_torch / video_torch    ((g - g.mean) / (g.std + 1e-6)).view_as(r) * mask on the [n, P, G, C] view, f32
  raw_hip / raw_norm_hip       ops.raw_adv from given scores: one launch / two launches
  raw_torch / raw_norm_torch   scores[None, :, None] * mask (one fused elementwise kernel) / the same, then
                               ops.masked_standardize_ on the product
Algorithmic bytes per element: 9 (frame, video: 4 + 1 read, 4 written), 5 (raw), 6 (raw normalised: the mask twice).  A shape
is `faster` when the new entry's slowest window is below the baseline's fastest.  The two small shapes are latency-bound: read
their microseconds, not a ratio.  Prints one JSON line."""

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
SHAPES = {"contract": (128, 1024, 1, 8), "diffusion": (16, 64, 16, 8), "large": (128, 65536, 1, 8)}
REASONING = (4096, 8192)
LAUNCHES = {"frame": 1, "video": 1, "raw": 1, "raw_norm": 2}
BYTES = {"frame": 9, "video": 9, "raw": 5, "raw_norm": 6}


def graph_times_us(fn, calls: int, windows: int) -> dict:
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
    del graph
    return dict(median=round(statistics.median(times), 3), min=round(min(times), 3), max=round(max(times), 3))


def video_torch(r, mask, G, mode):
    n, B, C = r.shape
    g = r.view(n, B // G, G, C)
    dims = (2,) if mode == "frame" else (0, 2, 3)
    return ((g - g.mean(dim=dims, keepdim=True)) / (g.std(dim=dims, keepdim=True) + 1e-6)).view(n, B, C) * mask


def entries(ops, r, scores, mask, G):
    """name -> (hip fn, torch fn); r None for a reasoning shape."""
    s_b = scores[None, :, None] if mask.dim() == 3 else scores[:, None]

    def raw_norm_torch():
        return ops.masked_standardize_(s_b * mask, mask)

    out = {"raw": (lambda: ops.raw_adv(scores, mask), lambda: s_b * mask),
           "raw_norm": (lambda: ops.raw_adv(scores, mask, normalize=True), raw_norm_torch)}
    if r is not None:
        out["frame"] = (lambda: ops.grpo_video_adv(r, mask, G, "frame"), lambda: video_torch(r, mask, G, "frame"))
        out["video"] = (lambda: ops.grpo_video_adv(r, mask, G, "video"), lambda: video_torch(r, mask, G, "video"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shapes", default="contract,diffusion,large,reasoning")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adv_video_raw needs a GPU")
    if a.windows < 7:
        raise SystemExit("--windows must be at least 7")
    from rlinf_amd import ops

    dev = torch.device("cuda", 0)
    res = dict(windows=a.windows, calls_per_window=a.calls, launches=LAUNCHES, bytes_per_element=BYTES, shapes={})
    for name in a.shapes.split(","):
        g = torch.Generator().manual_seed(0)
        if name == "reasoning":
            bsz, seq = REASONING
            r, G, elems = None, 1, bsz * seq
            scores = (torch.rand(bsz, generator=g) < 0.3).float().to(dev)
            mask = (torch.rand(bsz, seq, generator=g) < 0.8).to(dev)
            shape = dict(bsz=bsz, seq=seq)
        else:
            n, B, C, G = SHAPES[name]
            elems = n * B * C
            r = torch.rand(n, B, C, generator=g).to(dev)
            scores = torch.rand(B, generator=g).to(dev)
            mask = (torch.rand(n, B, C, generator=g) < 0.8).to(dev)
            shape = dict(n_chunk=n, batch=B, chunk=C, group_size=G)
        out = dict(shape=shape, elements=elems)
        for key, (hip, ref) in entries(ops, r, scores, mask, G).items():
            got, want = hip(), ref()  # same answers before timing anything
            assert float((got - want).abs().max()) < (1e-2 if key == "raw_norm" else 1e-3), (name, key)
            th, tt = graph_times_us(hip, a.calls, a.windows), graph_times_us(ref, a.calls, a.windows)
            out[key] = dict(hip_us=th, torch_us=tt, speedup=round(tt["median"] / th["median"], 2),
                            faster=bool(th["max"] < tt["min"]),
                            share_of_8TBps=round(elems * BYTES[key] / th["median"] / PEAK_BYTES_PER_US, 4))
        res["shapes"][name] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
