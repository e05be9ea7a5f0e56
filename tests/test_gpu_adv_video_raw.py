"""The "grpo_video" and "raw" advantages on the device (csrc/adv_video_raw.hip), reached through this package's registry.

    expected   tests/golden/adv_video_raw.pt (the reference's callees and its calculate_adv_and_returns, recorded by
               tools/make_adv_video_raw_golden.py), and float64 restatements of advantages.py:124-164,410-438 below
    got        the HIP callees, the embodied / reasoning dispatchers and the learner on device tensors

Against the fixtures a value may differ from the reference's f32 result by `2 * k` units, where a unit is one ulp (2^-23) of the
case's reward scale divided by (std + eps) of the element's group, and k is what the reference's own f32 output needs against
the float64 restatement of the same case -- computed here from those two, once for the reference and the same again for the
kernel.  NaN positions and signs must be identical.  Against the restatement at step shapes the bounds are
    grpo_video       |got - a64| <= 4e-6 / (std + 1e-6) + 1e-6 |a64|
    raw, normalised  |got - a64| <= 4 * 2^-23 * max|score| / (std + 1e-5) + 1e-6 |a64|
(a few f32 roundings of O(scale) values divided by the std, plus a few ulp of the result); every element is compared."""

import math
import os

import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = torch.load(os.path.join(GOLDEN_DIR, "adv_video_raw.pt"), weights_only=False)
RTOL, ATOL = 1e-5, 5e-6  # tests/test_gpu_advantages.py: the score scan's bound


@pytest.fixture(autouse=True)
def builtins_installed():
    """Another test of the suite registers and pops its own "raw": install the two names as the package does at import time,
    restore the registries afterwards."""
    from rlinf_amd.algorithms import advantages as A
    from rlinf_amd.algorithms import registry as R
    saved = dict(R.ADV_REGISTRY), dict(R._NATIVE_ADV), dict(R._NATIVE_ADV_REASONING)
    R.ADV_REGISTRY["grpo_video"], R.ADV_REGISTRY["raw"] = A.compute_grpo_video_advantages, A.compute_raw_advantages
    R._NATIVE_ADV["grpo_video"], R._NATIVE_ADV["raw"] = A._native_grpo_video, A._native_raw
    R._NATIVE_ADV_REASONING.pop("grpo_video", None)
    R._NATIVE_ADV_REASONING["raw"] = A._native_raw_reasoning
    try:
        yield R
    finally:
        for live, old in zip((R.ADV_REGISTRY, R._NATIVE_ADV, R._NATIVE_ADV_REASONING), saved):
            live.clear()
            live.update(old)


def _dev(v):
    return v.to(DEV) if isinstance(v, torch.Tensor) else v


def _tb(x):
    """[n, B, C] -> the reference's [T, B] view (utils.py:107)."""
    n, b, c = x.shape
    return x.transpose(1, 2).reshape(n * c, b)


def _nbc(x, n, c):
    """[T, B] -> [n, B, C] (utils.py:164)."""
    return x.reshape(n, c, -1).transpose(1, 2)


def _reduced(kw):
    """The dispatcher's chunk_level reduction (utils.py:80-89) of rewards / dones / mask, on whatever device they are."""
    r, d, m = kw["rewards"], kw["dones"], kw["loss_mask"]
    if kw["reward_type"] == "chunk_level":
        r, d, m = r.sum(-1, keepdim=True), d.max(-1, keepdim=True)[0], m.max(-1, keepdim=True)[0]
    return r, d, m


# ---- float64 restatements ---------------------------------------------------------------------------------------------------
def f64_video(r, mask, G, mode):
    """advantages.py:124-164 in float64 on [n, B, C]: (advantages, the std each element was divided by)."""
    n, B, C = r.shape
    g = r.double().reshape(n, B // G, G, C)
    dims = (2,) if mode == "frame" else (0, 2, 3)
    mean, std = g.mean(dim=dims, keepdim=True), g.std(dim=dims, keepdim=True)
    a = ((g - mean) / (std + 1e-6)).reshape(n, B, C) * mask
    return a, std.expand_as(g).reshape(n, B, C)


def f64_raw(scores, mask, normalize):
    """advantages.py:410-438 in float64; mask [n, B, C] or [bsz, seq]: (advantages, std of the valid ones or None)."""
    s = scores.double().reshape(-1)
    a = (s[None, :, None] if mask.dim() == 3 else s[:, None]) * mask
    if not normalize:
        return a, None
    valid = a[mask]
    if valid.numel() == 0:
        return a, None
    std = valid.std()
    return (a - valid.mean()) / (std + 1e-5), std


def _same_nan_and_sign(got, want, a64=None):
    """NaN positions identical; signs identical (-0.0 where a negative value is masked).  With a restatement `a64` of the same
    case, an element where the reference's own sign contradicts the float64 result is left out of the SIGN comparison (its value
    is still compared): that happens only where the exact value is 0 -- a group of identical rewards, std == 0 -- and the
    reference's f32 mean leaves rounding noise of either sign, 1e-7 / eps large, which no other summation order reproduces."""
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN positions differ"
    ok = ~torch.isnan(want)
    sure = ok if a64 is None else ok & (torch.signbit(want) == torch.signbit(a64))
    assert torch.equal(torch.signbit(got[sure]), torch.signbit(want[sure])), "signs differ (-0.0 where a negative value is masked)"
    if a64 is not None:
        noise = ok & ~sure
        assert bool((a64[noise] == 0).all()), "the reference's sign contradicts a non-zero float64 value"
    return ok


def _assert_within_reference_units(got, want, a64, unit, what):
    """got, want f32; a64 the restatement; unit f64 per element.  k = what `want` needs against a64, allowed: 2 k units."""
    got, want, a64, unit = got.cpu(), want.cpu(), a64.cpu(), unit.cpu()
    assert torch.equal(torch.isnan(a64), torch.isnan(want)), "the restatement's NaN positions differ from the reference's"
    ok = _same_nan_and_sign(got, want, a64)
    if not bool(ok.any()):
        return
    ref_units = ((want[ok].double() - a64[ok]).abs() / unit[ok]).max().item()
    k = math.ceil(ref_units)
    err = (got[ok].double() - want[ok].double()).abs()
    worst = (err / unit[ok]).max().item()
    print(f"{what}: reference needs {ref_units:.3f} units (k = {k}), kernel is {worst:.3f} units from the reference")
    assert bool((err <= 2 * k * unit[ok]).all()), f"{what}: {worst:.3f} units > 2 * {k}"


def _bit_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    nan = torch.isnan(a)
    assert torch.equal(nan, torch.isnan(b))
    assert torch.equal(a[~nan], b[~nan]) and torch.equal(torch.signbit(a[~nan]), torch.signbit(b[~nan]))


# ---- 5 / 6: fixtures, callee and dispatcher ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(GOLD["video"]))
def test_grpo_video_matches_reference_golden(case, builtins_installed):
    R = builtins_installed
    c = GOLD["video"][case]
    kw = {k: _dev(v) for k, v in c["kwargs"].items()}
    want = c["advantages"]
    res = R.calculate_adv_and_returns(**kw)
    assert set(res) == {"advantages"}
    adv = res["advantages"]
    assert adv.device.type == "cuda" and tuple(adv.shape) == tuple(want.shape)
    r, _, m = _reduced(c["kwargs"])
    a64, std = f64_video(r, m, kw["group_size"], kw["advantage_mode"])
    scale = float(r.abs().max()) or 1.0
    unit = 2.0 ** -23 * scale / (std + 1e-6)
    _assert_within_reference_units(adv, want, a64, unit, case)
    # the callee on the reference's [T, B] views gives the same bits
    rd, _, md = _reduced(kw)
    direct, ret = R.get_adv_and_returns("grpo_video")(rewards=_tb(rd), loss_mask=_tb(md), group_size=kw["group_size"],
                                                      advantage_mode=kw["advantage_mode"])
    assert ret is None and direct.device.type == "cuda"
    _bit_equal(_nbc(direct, rd.shape[0], rd.shape[2]), adv)


@pytest.mark.parametrize("case", sorted(GOLD["raw"]))
def test_raw_matches_reference_golden(case, builtins_installed):
    R = builtins_installed
    c = GOLD["raw"][case]
    kw = {k: _dev(v) for k, v in c["kwargs"].items()}
    norm = bool(kw.get("normalize_advantages", False))
    r, _, m = _reduced(c["kwargs"])
    rd, _, md = _reduced(kw)
    n, _, C = r.shape
    callee = R.get_adv_and_returns("raw")
    extra = {k: kw[k] for k in ("normalize_advantages",) if k in kw}
    # the callee from the reference's own scores
    direct, ret = callee(rewards=_dev(c["scores"]), loss_mask=_tb(md), **extra)
    assert ret is None and direct.device.type == "cuda"
    if not norm:
        _bit_equal(direct.cpu(), c["from_scores"])
    else:
        a64, std = f64_raw(c["scores"], _tb(m).unsqueeze(-1), True)
        scale = float(c["scores"].abs().max()) or 1.0
        unit = torch.full_like(a64, 2.0 ** -23 * scale / (float(std) + 1e-5)) if std is not None and std == std \
            else torch.ones_like(a64)
        _assert_within_reference_units(direct.unsqueeze(-1), c["from_scores"].unsqueeze(-1), a64, unit, case + " (callee)")
    # the embodied dispatcher (its scores come from the device scan)
    res = R.calculate_adv_and_returns(**kw)
    assert set(res) == {"advantages"}
    adv, want = res["advantages"], c["advantages"]
    assert adv.device.type == "cuda" and tuple(adv.shape) == tuple(want.shape)
    if not norm:
        _same_nan_and_sign(adv.cpu(), want)
        torch.testing.assert_close(adv.cpu(), want, rtol=RTOL, atol=ATOL, equal_nan=True)
    else:
        a64, std = f64_raw(c["scores"], m, True)
        scale = float(c["scores"].abs().max()) or 1.0
        if std is None or std != std:
            unit = torch.ones_like(a64)
        else:  # the scan's own bound on a score, carried through the division, on top of the kernel's units
            unit = torch.full_like(a64, (2.0 ** -23 * scale + RTOL * scale + ATOL) / (float(std) + 1e-5))
        _assert_within_reference_units(adv, want, a64, unit, case + " (dispatcher)")
    # dispatcher == callee on transposed views, from the device scan's scores
    from rlinf_amd import ops
    scores = ops.episode_scores(rd.float().contiguous(), _reduced(kw)[1].contiguous())
    again, _ = callee(rewards=scores.reshape(-1, kw["group_size"]), loss_mask=_tb(md), **extra)
    _bit_equal(_nbc(again, n, rd.shape[2]), adv)


@pytest.mark.parametrize("case", sorted(GOLD["reasoning"]))
def test_reasoning_raw_matches_reference_golden(case, builtins_installed):
    R = builtins_installed
    c = GOLD["reasoning"][case]
    kw = {k: _dev(v) for k, v in c["kwargs"].items()}
    adv, ret = R.calculate_adv_and_returns(**kw)
    want = c["advantages"]
    assert ret is None and adv.is_contiguous() and adv.device.type == "cuda" and tuple(adv.shape) == tuple(want.shape)
    if not kw["normalize_advantages"]:
        _bit_equal(adv.cpu(), want)
    else:
        a64, std = f64_raw(c["kwargs"]["rewards"], c["kwargs"]["loss_mask"], True)
        scale = float(c["kwargs"]["rewards"].abs().max()) or 1.0
        unit = torch.full_like(a64, 2.0 ** -23 * scale / (float(std) + 1e-5)) if std is not None and std == std \
            else torch.ones_like(a64)
        _assert_within_reference_units(adv, want, a64, unit, case)
    # the callee on the transposed views ([seq, bsz] mask) gives the same bits
    direct, _ = R.get_adv_and_returns("raw")(rewards=kw["rewards"], loss_mask=kw["loss_mask"].transpose(0, 1),
                                             normalize_advantages=kw["normalize_advantages"])
    _bit_equal(direct.transpose(0, 1), adv)


# ---- 7: float64 restatement at step shapes ----------------------------------------------------------------------------------
SHAPES = [(128, 1024, 1, 8), (80, 256, 1, 8), (16, 64, 16, 8), (12, 24, 2, 4), (5, 6, 1, 3), (128, 65536, 1, 8)]


def _step_inputs(shape, kind):
    n, B, C, G = shape
    g = torch.Generator().manual_seed(n * 131 + B * 7 + C * 3 + G)
    r = torch.rand(n, B, C, generator=g) if kind == "uniform" else (torch.rand(n, B, C, generator=g) < 0.3).float()
    mask = torch.rand(n, B, C, generator=g) < 0.8
    mask[:, B // 3] = False  # one env fully masked
    dones = torch.rand(n + 1, B, C, generator=g) < 0.02
    return r.to(DEV), mask.to(DEV), dones.to(DEV)


@pytest.mark.parametrize("kind", ["uniform", "bernoulli"])
@pytest.mark.parametrize("mode", ["frame", "video"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grpo_video_matches_float64_restatement_at_step_shapes(shape, mode, kind, builtins_installed):
    n, B, C, G = shape
    r, mask, dones = _step_inputs(shape, kind)
    kw = dict(task_type="embodied", adv_type="grpo_video", rewards=r, dones=dones, values=None, group_size=G,
              reward_type="action_level", loss_mask=mask, loss_mask_sum=None, advantage_mode=mode)
    adv = builtins_installed.calculate_adv_and_returns(**kw)["advantages"]
    assert adv.dtype == torch.float32 and tuple(adv.shape) == (n, B, C)
    a64, std = f64_video(r, mask, G, mode)
    assert not bool(torch.isnan(a64).any()) and not bool(torch.isnan(adv).any())
    tol = 4e-6 / (std + 1e-6) + 1e-6 * a64.abs()
    err = (adv.double() - a64).abs()
    print(f"{shape} {mode} {kind}: worst err / bound = {(err / tol).max().item():.4f}")
    bad = err > tol
    assert not bool(bad.any()), f"{int(bad.sum())} elements off, max err {err.max().item():.3g}"
    assert torch.equal(torch.signbit(adv), torch.signbit(a64))  # -0.0 where a negative value is masked
    assert bool((adv[~mask] == 0).all())
    again = builtins_installed.calculate_adv_and_returns(**kw)["advantages"]
    assert torch.equal(adv, again) and torch.equal(torch.signbit(adv), torch.signbit(again))  # repeatable bits


def _assert_raw_close(adv, a64, std, scores, what):
    tol = 4 * 2.0 ** -23 * float(scores.abs().max()) / (float(std) + 1e-5) + 1e-6 * a64.abs()
    err = (adv.double() - a64).abs()
    print(f"{what}: worst err / bound = {(err / tol).max().item():.4f}")
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, max err {err.max().item():.3g}"


@pytest.mark.parametrize("kind", ["uniform", "bernoulli"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_embodied_raw_matches_float64_restatement_at_step_shapes(shape, kind, builtins_installed):
    from rlinf_amd import ops
    n, B, C, G = shape
    r, mask, dones = _step_inputs(shape, kind)
    kw = dict(task_type="embodied", adv_type="raw", rewards=r, dones=dones, values=None, group_size=G,
              reward_type="action_level", loss_mask=mask, loss_mask_sum=None, advantage_mode=None)
    scores = ops.episode_scores(r, dones)  # the existing scan, held to its own bound elsewhere
    plain = builtins_installed.calculate_adv_and_returns(**kw)["advantages"]
    _bit_equal(plain, scores[None, :, None] * mask)  # the product is exact
    adv = builtins_installed.calculate_adv_and_returns(**kw, normalize_advantages=True)["advantages"]
    a64, std = f64_raw(scores, mask, True)
    _assert_raw_close(adv, a64, std, scores, f"{shape} {kind}")
    again = builtins_installed.calculate_adv_and_returns(**kw, normalize_advantages=True)["advantages"]
    assert torch.equal(adv, again)


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("bsz,seq", [(16, 8192), (1024, 7096), (4096, 8192)])
def test_reasoning_raw_matches_float64_restatement_at_step_shapes(bsz, seq, scale, builtins_installed):
    g = torch.Generator().manual_seed(bsz + seq)
    rewards = ((torch.rand(bsz, generator=g) if scale > 1 else (torch.rand(bsz, generator=g) < 0.3).float()) * scale).to(DEV)
    mask = (torch.rand(bsz, seq, generator=g) < 0.8).to(DEV)
    mask[bsz // 3] = False
    kw = dict(task_type="reasoning", adv_type="raw", rewards=rewards, loss_mask=mask)
    plain, ret = builtins_installed.calculate_adv_and_returns(**kw)
    assert ret is None and plain.is_contiguous()
    _bit_equal(plain, rewards[:, None] * mask)
    adv, _ = builtins_installed.calculate_adv_and_returns(**kw, normalize_advantages=True)
    a64, std = f64_raw(rewards, mask, True)
    _assert_raw_close(adv, a64, std, rewards, f"({bsz}, {seq}) x{scale}")
    again, _ = builtins_installed.calculate_adv_and_returns(**kw, normalize_advantages=True)
    assert torch.equal(adv, again)


# ---- 8: plumbing ------------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager():
    from rlinf_amd import ops
    g = torch.Generator().manual_seed(11)
    n, B, C, G = 9, 48, 2, 8
    r = torch.rand(n, B, C, generator=g).to(DEV)
    scores = torch.rand(B, generator=g).to(DEV)
    mask = (torch.rand(n, B, C, generator=g) < 0.8).to(DEV)

    def run():
        return [ops.grpo_video_adv(r, mask, G, "frame"), ops.grpo_video_adv(r, mask, G, "video"), ops.raw_adv(scores, mask),
                ops.raw_adv(scores, mask, normalize=True)]

    eager = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
    r.copy_(torch.rand(n, B, C, generator=g).to(DEV))  # new data, same buffers
    scores.copy_(torch.rand(B, generator=g).to(DEV))
    mask.copy_((torch.rand(n, B, C, generator=g) < 0.6).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, run()):
        assert torch.equal(a, b)


def test_cpu_inputs_come_back_on_the_cpu_and_views_are_not_misread(builtins_installed):
    R = builtins_installed
    c = GOLD["video"]["g3_c5_frame"]
    res = R.calculate_adv_and_returns(**c["kwargs"])  # CPU tensors in
    assert res["advantages"].device.type == "cpu"
    on_dev = R.calculate_adv_and_returns(**{k: _dev(v) for k, v in c["kwargs"].items()})["advantages"]
    assert torch.equal(res["advantages"], on_dev.cpu())
    c = GOLD["reasoning"]["b16_s33_norm"]
    adv, _ = R.calculate_adv_and_returns(**c["kwargs"])
    assert adv.device.type == "cpu"
    # a non-contiguous mask view (every second column of a wider mask) and an offset, unaligned one
    g = torch.Generator().manual_seed(3)
    wide = (torch.rand(16, 66, generator=g) < 0.7).to(DEV)
    rewards = torch.rand(16, generator=g).to(DEV)
    for view in (wide[:, ::2], wide[:, 1:34]):
        assert not view.is_contiguous()
        for norm in (False, True):
            a, _ = R.calculate_adv_and_returns(task_type="reasoning", adv_type="raw", rewards=rewards, loss_mask=view,
                                               normalize_advantages=norm)
            b, _ = R.calculate_adv_and_returns(task_type="reasoning", adv_type="raw", rewards=rewards,
                                               loss_mask=view.contiguous(), normalize_advantages=norm)
            assert torch.equal(a, b)
    r3 = torch.rand(6, 16, 4, generator=g).to(DEV)
    m3 = (torch.rand(6, 16, 8, generator=g) < 0.7).to(DEV)[:, :, ::2]
    for mode in ("frame", "video"):
        kw = dict(task_type="embodied", adv_type="grpo_video", rewards=r3, dones=None, group_size=4, reward_type="action_level",
                  advantage_mode=mode)
        assert torch.equal(R.calculate_adv_and_returns(**kw, loss_mask=m3)["advantages"],
                           R.calculate_adv_and_returns(**kw, loss_mask=m3.contiguous())["advantages"])


def test_bad_arguments_return_einval_with_a_message():
    from rlinf_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, device=DEV)
    m = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert lib.rlx_grpo_video_adv(x.data_ptr(), m.data_ptr(), x.data_ptr(), 2, 8, 1, 3, 0, 1e-6, None) == -22
    assert b"group_size" in lib.rlx_last_error()
    assert lib.rlx_grpo_video_adv(x.data_ptr(), m.data_ptr(), x.data_ptr(), 2, 8, 1, 4, 2, 1e-6, None) == -22
    assert b"mode" in lib.rlx_last_error()
    assert lib.rlx_grpo_video_adv(None, m.data_ptr(), x.data_ptr(), 2, 8, 1, 4, 0, 1e-6, None) == -22
    assert lib.rlx_raw_adv(x.data_ptr(), m.data_ptr(), x.data_ptr(), -1, 8, 1, 0, 1e-5, None, 0, None) == -22
    assert lib.rlx_raw_adv(x.data_ptr(), None, x.data_ptr(), 2, 8, 1, 0, 1e-5, None, 0, None) == -22
    assert lib.rlx_raw_adv(x.data_ptr(), m.data_ptr(), x.data_ptr(), 2, 8, 1, 1, 1e-5, None, 0, None) == -22  # no workspace
    assert b"workspace" in lib.rlx_last_error()


# ---- 9: the learner ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adv_type,mode", [("grpo_video", "frame"), ("grpo_video", "video"), ("raw", None)])
def test_learner_iteration(adv_type, mode, builtins_installed):
    """One iteration of this package's learner on the synthetic env (set-up of tests/test_end_to_end.py::
    test_embodied_grpo_iteration): the batch's advantages are the dispatcher's on the same buffers, and the loss is finite."""
    from oracle import ppo_loop as L
    from oracle import ppo_oracle as O
    from test_end_to_end import _build, make_cfg
    cfg = make_cfg(total_envs=32, steps=10, global_batch=160, auto_reset=False)
    cfg.algorithm.adv_type, cfg.algorithm.loss_type, cfg.algorithm.group_size = adv_type, "actor", 4
    if mode is not None:
        cfg.algorithm.advantage_mode = mode
    cfg.env.train.group_size = 4
    env = L.synthetic_env_tensors(3, 10, 32, 42, mode="bernoulli", p_done=0.06)
    torch.manual_seed(5)
    sd = O.OracleMLPPolicy(42, 8, 1).state_dict()
    runner = _build(cfg, env, sd)
    model = runner.actor.worker.model
    before = model.flat.detach().clone()
    m = runner.run_step(torch.randn(10, 32, 8).cuda())
    rb = runner.actor.worker.rollout_batch
    want = builtins_installed.calculate_adv_and_returns(
        task_type="embodied", adv_type=adv_type, rewards=rb["rewards"], dones=rb["dones"], values=None, group_size=4,
        reward_type="action_level", loss_mask=rb.get("loss_mask"), loss_mask_sum=rb.get("loss_mask_sum"), advantage_mode=mode)
    assert torch.equal(rb["advantages"], want["advantages"])
    assert float((model.flat.detach() - before).abs().max()) > 0
    losses = {k: v for k, v in m.items() if isinstance(v, float) and "loss" in k}
    assert losses and all(math.isfinite(v) for v in losses.values()), m
