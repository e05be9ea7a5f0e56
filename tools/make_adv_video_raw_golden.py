"""Write tests/golden/adv_video_raw.pt: the reference's "grpo_video" and "raw" advantages on seeded inputs.

    python -m tools.make_adv_video_raw_golden

Runs only where the reference tree is readable (oracle.reference_loader); the GPU tests read the stored file, never the tree.
Recorded, per case, the inputs and what the reference returned:
  video/<case>      registry.calculate_adv_and_returns(task_type="embodied", adv_type="grpo_video", ...) on [n_chunk, B, C]
                    buffers; the tool checks that compute_grpo_video_advantages (advantages.py:124-164) on the [T, B] views
                    gives the same tensor, so a test can derive the callee's inputs and outputs by the same transposes
  raw/<case>        the same entry with adv_type="raw", plus `scores`, what calculate_scores (utils.py:134-152) handed the
                    callee, and `from_scores` = compute_raw_advantages (advantages.py:410-438) on them
  reasoning/<case>  registry.calculate_adv_and_returns(task_type="reasoning", adv_type="raw", ...) on [bsz] rewards and a
                    [bsz, seq] mask
  errors            the exception types and messages of an unsupported advantage_mode and of grpo_video on a reasoning batch
"""

from __future__ import annotations

import os

import torch

from oracle import reference_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "adv_video_raw.pt")


def _mask(g, shape, form):
    if form == "none":
        return torch.zeros(shape, dtype=torch.bool)
    if form == "full":
        return torch.ones(shape, dtype=torch.bool)
    if form == "one":
        m = torch.zeros(shape, dtype=torch.bool)
        m.view(-1)[int(torch.randint(0, m.numel(), (1,), generator=g))] = True
        return m
    return torch.rand(shape, generator=g) < 0.8


def _rewards(g, shape, kind, group_size):
    if kind == "binary":
        return (torch.rand(shape, generator=g) < 0.3).float()
    if kind == "same":  # every group holds one value: std == 0
        n, b, c = shape
        return (torch.rand(n, b // group_size, 1, c, generator=g) * 4 - 2).expand(n, b // group_size, group_size, c).reshape(shape).clone()
    if kind == "const":  # one value everywhere: std == 0 in video mode too
        return torch.full(shape, 0.7)
    return torch.rand(shape, generator=g) * 6 - 2


def _embodied_kwargs(g, adv_type, n, b, c, group, reward_type, kind, form, **extra):
    rewards = _rewards(g, (n, b, c), kind, group)
    dones = torch.rand(n + 1, b, c, generator=g) < 0.06
    mask = _mask(g, (n, b, c), form)
    return dict(task_type="embodied", adv_type=adv_type, rewards=rewards, dones=dones, values=None, gamma=1, gae_lambda=1,
                group_size=group, reward_type=reward_type, loss_mask=mask, loss_mask_sum=None, **extra)


VIDEO = {  # name: (n_chunk, B, C, G, reward_type, rewards, mask)
    "g8_c1": (12, 32, 1, 8, "action_level", "uniform", "rand"),
    "g8_c1_binary": (12, 32, 1, 8, "action_level", "binary", "rand"),
    "g16_c2": (5, 32, 2, 16, "action_level", "uniform", "rand"),
    "g3_c5": (4, 12, 5, 3, "action_level", "uniform", "rand"),
    "g2_c16_binary": (3, 8, 16, 2, "action_level", "binary", "rand"),
    "g1_c2": (3, 4, 2, 1, "action_level", "uniform", "rand"),
    "g4_c1": (7, 16, 1, 4, "action_level", "uniform", "full"),
    "g8_c16_chunk_level": (6, 16, 16, 8, "chunk_level", "binary", "rand"),
    "g3_c5_chunk_level": (4, 9, 5, 3, "chunk_level", "uniform", "rand"),
    "g8_c1_mask_none": (4, 16, 1, 8, "action_level", "uniform", "none"),
    "g8_c2_mask_one": (4, 16, 2, 8, "action_level", "uniform", "one"),
    "g8_c1_same": (6, 24, 1, 8, "action_level", "same", "rand"),
    "g2_c2_const": (3, 8, 2, 2, "action_level", "const", "rand"),
    "g1_t1": (1, 3, 1, 1, "action_level", "uniform", "full"),
}


def video_cases(ref, g):
    pre = ref.algo_utils.preprocess_embodied_advantages_inputs
    cases = {}
    for name, (n, b, c, group, rtype, kind, form) in VIDEO.items():
        for mode in ("frame", "video"):
            kw = _embodied_kwargs(g, "grpo_video", n, b, c, group, rtype, kind, form, advantage_mode=mode)
            res = ref.registry.calculate_adv_and_returns(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()})
            assert set(res) == {"advantages"}
            flat = pre(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()})
            direct, ret = ref.advantages.compute_grpo_video_advantages(rewards=flat["rewards"], loss_mask=flat["loss_mask"],
                                                                       group_size=group, advantage_mode=mode)
            assert ret is None
            back = direct.reshape(flat["num_chunk"], flat["chunk_size"], -1).transpose(1, 2)
            assert torch.equal(torch.isnan(back), torch.isnan(res["advantages"]))
            assert torch.equal(torch.nan_to_num(back), torch.nan_to_num(res["advantages"]))
            cases[f"{name}_{mode}"] = dict(kwargs=kw, advantages=res["advantages"].contiguous())
    return cases


RAW = {  # name: (n_chunk, B, C, G, reward_type, rewards, mask)
    "g8_c1": (12, 32, 1, 8, "action_level", "uniform", "rand"),
    "g8_c1_binary": (12, 32, 1, 8, "action_level", "binary", "rand"),
    "g16_c2": (5, 32, 2, 16, "action_level", "uniform", "rand"),
    "g3_c5": (4, 12, 5, 3, "action_level", "uniform", "rand"),
    "g1_c16": (3, 5, 16, 1, "action_level", "binary", "rand"),
    "g2_c5_chunk_level": (4, 8, 5, 2, "chunk_level", "uniform", "rand"),
    "g8_c1_mask_none": (4, 16, 1, 8, "action_level", "uniform", "none"),
    "g8_c2_mask_one": (4, 16, 2, 8, "action_level", "uniform", "one"),
    "g4_c1_mask_full": (7, 16, 1, 4, "action_level", "uniform", "full"),
    "g2_c2_const": (3, 8, 2, 2, "action_level", "const", "rand"),
}


def raw_cases(ref, g):
    cases = {}
    for name, (n, b, c, group, rtype, kind, form) in RAW.items():
        for norm in (False, True, None):  # None: the key is absent, the callee's default (False) applies
            extra = {} if norm is None else {"normalize_advantages": norm}
            kw = _embodied_kwargs(g, "raw", n, b, c, group, rtype, kind, form, advantage_mode=None, **extra)
            if kind == "const":  # no episode ends: every env's score is the same sum, std == 0
                kw["dones"] = torch.zeros_like(kw["dones"])
            copy = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}
            res = ref.registry.calculate_adv_and_returns(**copy)
            assert set(res) == {"advantages"}
            flat = ref.algo_utils.calculate_scores(**ref.algo_utils.preprocess_embodied_advantages_inputs(
                **{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}))
            from_scores, _ = ref.advantages.compute_raw_advantages(rewards=flat["rewards"], loss_mask=flat["loss_mask"], **extra)
            tag = {False: "plain", True: "norm", None: "default"}[norm]
            cases[f"{name}_{tag}"] = dict(kwargs=kw, advantages=res["advantages"].contiguous(), scores=flat["rewards"].clone(),
                                          from_scores=from_scores.contiguous())
    return cases


def reasoning_cases(ref, g):
    cases = {}
    for name, (bsz, seq, kind, form) in {
        "b16_s33": (16, 33, "uniform", "rand"),
        "b8_s64_binary": (8, 64, "binary", "rand"),
        "b5_s1": (5, 1, "uniform", "rand"),
        "b6_s17_mask_none": (6, 17, "uniform", "none"),
        "b6_s17_mask_one": (6, 17, "uniform", "one"),
        "b4_s16_mask_full": (4, 16, "uniform", "full"),
        "b7_s9_const": (7, 9, "const", "rand"),
    }.items():
        for norm in (False, True):
            rewards = _rewards(g, (1, bsz, 1), kind, 1).reshape(bsz) * (1.0 if kind != "uniform" else 5.0)
            mask = _mask(g, (bsz, seq), form)
            kw = dict(task_type="reasoning", adv_type="raw", rewards=rewards, loss_mask=mask, normalize_advantages=norm)
            adv, ret = ref.registry.calculate_adv_and_returns(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()})
            assert ret is None and adv.is_contiguous() and tuple(adv.shape) == (bsz, seq)
            cases[f"{name}_{'norm' if norm else 'plain'}"] = dict(kwargs=kw, advantages=adv)
    return cases


def error_cases(ref, g):
    out = {}
    kw = _embodied_kwargs(g, "grpo_video", 2, 4, 1, 2, "action_level", "uniform", "rand")
    for tag, extra in {"mode_none": {"advantage_mode": None}, "mode_missing": {}, "mode_clip": {"advantage_mode": "clip"}}.items():
        try:
            ref.registry.calculate_adv_and_returns(**kw, **extra)
            raise SystemExit(f"{tag}: the reference did not raise")
        except ValueError as e:
            out[tag] = dict(type=type(e).__name__, message=str(e))
    try:
        ref.registry.calculate_adv_and_returns(task_type="reasoning", adv_type="grpo_video", rewards=torch.rand(4),
                                               loss_mask=torch.ones(4, 3, dtype=torch.bool), group_size=2, advantage_mode="frame")
        raise SystemExit("reasoning grpo_video: the reference did not raise")
    except AssertionError as e:
        out["reasoning_grpo_video"] = dict(type=type(e).__name__, message=str(e))
    try:
        ref.registry.calculate_adv_and_returns(task_type="reasoning", adv_type="raw", rewards=torch.rand(4, 1),
                                               loss_mask=torch.ones(4, 3, dtype=torch.bool))
        raise SystemExit("reasoning raw with 2-D rewards: the reference did not raise")
    except AssertionError as e:
        out["reasoning_raw_2d"] = dict(type=type(e).__name__, message=str(e))
    return out


def main():
    if not RL.available():
        raise SystemExit("the reference tree is not readable here: nothing to record")
    ref = RL.load()
    g = torch.Generator().manual_seed(20261016)
    data = {"video": video_cases(ref, g), "raw": raw_cases(ref, g), "reasoning": reasoning_cases(ref, g),
            "errors": error_cases(ref, g)}
    torch.save(data, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
