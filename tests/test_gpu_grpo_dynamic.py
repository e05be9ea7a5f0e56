"""Multi-turn GRPO ("grpo_dynamic") and the loss-scale processes on the device (csrc/grpo_dynamic.hip), reached through this
package's registries.

    expected   tests/golden/grpo_dynamic.pt (the reference's compute_grpo_dynamic_advantages, its reasoning dispatcher and its
               loss_scales.py chains, recorded by tools/make_grpo_dynamic_golden.py), and restatements below: the advantage in
               float64 (index_add_ / bincount over the same inputs, on the device), the loss scales as vectorized torch with the
               reference's factors rounded to f32 once
    got        the HIP callees on device tensors"""

import os

import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = torch.load(os.path.join(GOLDEN_DIR, "grpo_dynamic.pt"), weights_only=False)


def _adv_fn():
    from rlinf_amd.algorithms import get_adv_and_returns
    return get_adv_and_returns("grpo_dynamic")


def _dev(v):
    return v.to(DEV) if isinstance(v, torch.Tensor) else v


def _ulp(x: torch.Tensor) -> torch.Tensor:
    """Unit in the last place of |x| in x's dtype (as f64)."""
    x = x.abs()
    nxt = torch.nextafter(x, torch.full_like(x, float("inf")))
    return (nxt.double() - x.double()).clamp_min(torch.finfo(x.dtype).tiny)


def _assert_adv_close(got, want, ulps):
    """NaN positions and signs (-0.0 where a negative advantage is masked) identical; values within `ulps` units in the last
    place of the want value -- for f32 of at least 1.0, the scale of the rewards: a trajectory reward is a turn mean (a sum
    divided by 3, 5, 7, ... turns is inexact), and the reference's f32 group mean over such values rounds in its own reduction
    order, which moves (r - mean) by up to an ulp of the reward scale."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN positions differ"
    ok = ~torch.isnan(want)
    assert torch.equal(torch.signbit(got[ok]), torch.signbit(want[ok])), "signs differ (-0.0 at masked negatives)"
    err = (got[ok].double() - want[ok].double()).abs()
    unit = _ulp(want[ok])
    if want.dtype == torch.float32:
        unit = unit.clamp_min(2.0 ** -23)
    assert bool((err <= ulps * unit).all()), f"max err {err.max().item():.3g}"


@pytest.mark.parametrize("case", sorted(GOLD["adv"]))
def test_callee_matches_reference_golden(case):
    c = GOLD["adv"][case]
    kw = {k: _dev(v) for k, v in c.items() if k != "advantages"}
    adv, ret = _adv_fn()(**kw)
    assert ret is None and adv.device.type == "cuda"
    _assert_adv_close(adv, c["advantages"], 1 if c["advantages"].dtype == torch.bfloat16 else 4)


@pytest.mark.parametrize("case", sorted(GOLD["dispatch"]))
def test_reasoning_dispatcher_matches_reference_golden_and_the_callee(case):
    from rlinf_amd.algorithms import calculate_adv_and_returns
    c = GOLD["dispatch"][case]
    kw = {k: _dev(v) for k, v in c.items() if k != "advantages"}
    adv, ret = calculate_adv_and_returns(**kw)
    assert ret is None and adv.is_contiguous() and tuple(adv.shape) == tuple(c["advantages"].shape)
    _assert_adv_close(adv, c["advantages"], 4)
    direct, _ = _adv_fn()(rewards=kw["rewards"].reshape(-1, 1), loss_mask=kw["loss_mask"].transpose(0, 1),
                          group_size=kw["group_size"], idx_to_traj=kw["idx_to_traj"], advantage_mode=kw["advantage_mode"])
    assert torch.equal(adv, direct.transpose(0, 1))
    # idx_to_traj as a device tensor gives the same bits
    adv_t, _ = calculate_adv_and_returns(**dict(kw, idx_to_traj=torch.tensor(kw["idx_to_traj"], device=DEV)))
    assert torch.equal(adv_t, adv)


def _bit_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


@pytest.mark.parametrize("case", sorted(GOLD["scale"]))
def test_loss_scale_chains_are_bit_identical_to_reference_golden(case):
    from rlinf_amd.algorithms import get_loss_scales
    c = GOLD["scale"][case]
    batch = {k: _dev(v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in c["inputs"].items()}
    context = dict(c["context"], folding_scale=[], enable_scale_of_group=False)
    for fn in get_loss_scales(c["chain"]):
        batch = fn(context, batch)
    assert context["folding_scale"] == c["folding_scale"]
    _bit_equal(batch["advantages"].cpu(), c["advantages"])
    _bit_equal(batch["loss_scales"].cpu(), c["loss_scales"])
    # CPU tensors are staged and written back in place
    cpu = {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in c["inputs"].items()}
    ls_obj, adv_obj = cpu["loss_scales"], cpu["advantages"]
    context = dict(c["context"], folding_scale=[])
    for fn in get_loss_scales(c["chain"]):
        cpu = fn(context, cpu)
    assert cpu["loss_scales"] is ls_obj and cpu["advantages"] is adv_obj
    _bit_equal(ls_obj, c["loss_scales"])
    _bit_equal(adv_obj, c["advantages"])


def test_turn_level_zero_total_raises_like_the_reference():
    from rlinf_amd.algorithms import loss_scales as ls
    want = GOLD["errors"]["turn_zero_total"]
    batch = {"idx_to_traj": [0, 0, 1, 1, 1], "extra:idx_to_sub_traj": torch.tensor([0, 0, 0, 0, 0]),
             "response_mask": torch.ones(5, 9, dtype=torch.bool, device=DEV), "loss_scales": torch.ones(5, 9, device=DEV)}
    batch["response_mask"][:2] = False
    with pytest.raises(ZeroDivisionError) as ei:
        ls.turn_scale({"folding_scale": ["group_level", "agent_level"]}, batch)
    assert (type(ei.value).__name__, str(ei.value)) == (want["type"], want["message"])


# ---- float64 restatement at GRPO-step shapes ----------------------------------------------------------------------------
def _ids(g, num_traj, lo=1, hi=7):
    turns = torch.randint(lo, hi + 1, (num_traj,), generator=g)
    ids = torch.repeat_interleave(torch.arange(num_traj), turns)
    return ids[torch.randperm(ids.numel(), generator=g)]  # unsorted: merged batches interleave trajectories


def f64_adv(r, ids, G, mode):
    """advantages.py:167-299 in float64 on the device; returns (per-row advantage, per-row std of its question)."""
    r64, n_traj = r.double(), int(ids.max()) + 1
    if mode == "trajectory":
        s = torch.zeros(n_traj, dtype=torch.float64, device=r.device).index_add_(0, ids, r64)
        tr = s / torch.bincount(ids, minlength=n_traj).clamp(min=1)
        grp = tr.view(-1, G)
        mean, std = grp.mean(1, keepdim=True), grp.std(1, keepdim=True)
        a = ((grp - mean) / (std + 1e-6)).view(-1)[ids]
        return a, std.expand_as(grp).reshape(-1)[ids]
    q, nq = ids // G, n_traj // G
    cnt = torch.bincount(q, minlength=nq)
    mean = torch.zeros(nq, dtype=torch.float64, device=r.device).index_add_(0, q, r64) / cnt
    var = torch.zeros(nq, dtype=torch.float64, device=r.device).index_add_(0, q, (r64 - mean[q]) ** 2) / (cnt - 1)
    std = var.sqrt()
    return (r64 - mean[q]) / (std[q] + 1e-6), std[q]


SHAPES = [  # (num_traj, group_size, seq_len, turns lo..hi)
    (2048, 4, 7096, 1, 7),   # searchr1-like: 512 prompts x 4, ~8 k turn rows
    (256, 4, 7097, 1, 7),    # odd row length: every row start alignment
    (64, 2, 1, 1, 7),
    (64, 8, 7, 1, 7),
    (128, 16, 4100, 1, 7),
    (16384, 4, 5, 4, 4),     # 65 536 rows
]


@pytest.mark.parametrize("mode", ["turn", "trajectory"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_matches_float64_restatement_at_step_shapes(shape, mode):
    from rlinf_amd.algorithms import calculate_adv_and_returns
    num_traj, G, seq, lo, hi = shape
    g = torch.Generator().manual_seed(num_traj * 31 + G * 7 + seq)
    ids = _ids(g, num_traj, lo, hi)
    n = ids.numel()
    r = torch.rand(n, generator=g).to(DEV)
    mask = torch.rand(n, seq, generator=torch.Generator().manual_seed(seq)).lt(0.85).to(DEV)
    mask[n // 3] = False
    ids_d = ids.to(DEV)
    adv, _ = calculate_adv_and_returns(task_type="reasoning", adv_type="grpo_dynamic", advantage_mode=mode, rewards=r,
                                       loss_mask=mask, num_sequence=n, group_size=G, idx_to_traj=ids.tolist())
    assert adv.dtype == torch.float32 and adv.is_contiguous() and tuple(adv.shape) == (n, seq)
    a64, std = f64_adv(r, ids_d, G, mode)
    # f32 error bound: a few roundings of O(1) rewards (and of a trajectory's <= 7-term sum) over std, plus a few ulp of |a|
    tol = 4e-6 / (std + 1e-6) + 1e-6 * a64.abs()
    err = (adv.double() - a64[:, None] * mask).abs()
    bad = err > tol[:, None]
    assert not bool(bad.any()), f"{int(bad.sum())} elements off, max err {err.max().item():.3g}"
    assert torch.equal(adv == 0, ~mask | (a64 == 0)[:, None])  # masked positions are exactly zero
    again, _ = calculate_adv_and_returns(task_type="reasoning", adv_type="grpo_dynamic", advantage_mode=mode, rewards=r,
                                         loss_mask=mask, num_sequence=n, group_size=G, idx_to_traj=ids.tolist())
    assert torch.equal(adv, again) and torch.equal(torch.signbit(adv), torch.signbit(again))  # repeatable bits


def _restated_scales(ids, sub, mask, ls, chain_turn):
    """agent_level (and turn_level) as vectorized torch: the reference's f64 factors, rounded to f32 once, one f32 multiply."""
    pairs, inv, t_cnt = torch.unique(torch.stack([ids, sub], 1), dim=0, return_inverse=True, return_counts=True)
    agents = torch.bincount(pairs[:, 0])[pairs[:, 0]]
    f = ((1.0 / agents.double()) / t_cnt.double()).float()[inv]
    out = ls * f[:, None]
    if chain_turn:
        c = mask.sum(1)
        total = torch.zeros(len(pairs), dtype=torch.int64, device=ls.device).index_add_(0, inv, c)
        f2 = ((t_cnt[inv] * c).double() / total[inv].double()).float()
        out = out * f2[:, None]
    return out


@pytest.mark.parametrize("num_traj,seq,agents_max", [(2048, 7096, 1), (512, 4100, 3), (97 * 4, 7, 5), (300, 1, 2)])
def test_loss_scales_bit_identical_to_vectorized_restatement(num_traj, seq, agents_max):
    from rlinf_amd.algorithms import get_loss_scales
    g = torch.Generator().manual_seed(num_traj + seq)
    ids = _ids(g, num_traj)
    n = ids.numel()
    sub = torch.randint(0, agents_max, (n,), generator=g)
    mask = torch.rand(n, seq, generator=g).lt(0.7).to(DEV)
    mask[:, 0] = True  # no (trajectory, agent) group without a token
    adv = torch.randn(n, seq, device=DEV) * mask
    ls0 = torch.ones_like(adv).masked_fill(~mask, 0)
    batch = {"idx_to_traj": ids.tolist(), "extra:idx_to_sub_traj": sub, "response_mask": mask, "advantages": adv.clone(),
             "loss_scales": ls0.clone()}
    agbs, dp = 512 * 4 / 3, 2
    context = {"folding_scale": [], "actor_global_batch_size": agbs, "data_parallel_world_size": dp}
    for fn in get_loss_scales(["group_level", "agent_level", "turn_level"]):
        batch = fn(context, batch)
    _bit_equal(batch["advantages"], adv * (n * dp / agbs))
    _bit_equal(batch["loss_scales"], _restated_scales(ids.to(DEV), sub.to(DEV), mask, ls0, True))


def test_bf16_rows_scale_like_torch():
    from rlinf_amd import token_ops
    x = torch.randn(37, 29, device=DEV).to(torch.bfloat16)
    f = torch.rand(37, device=DEV) * 3
    want = (x.float() * f[:, None]).to(torch.bfloat16)
    _bit_equal(token_ops.scale_rows_(x.clone(), row_factors=f), want)
    y = x.clone()
    y *= 0.3
    _bit_equal(token_ops.scale_rows_(x.clone(), 0.3), y)


def test_graph_replay_matches_eager():
    from rlinf_amd import token_ops
    g = torch.Generator().manual_seed(5)
    ids = _ids(g, 64)
    n, seq = ids.numel(), 1031
    r = torch.rand(n, generator=g).to(DEV)
    mask = torch.rand(n, seq, generator=g).lt(0.8).to(DEV)
    plan = token_ops.GrpoDynamicPlan(ids.tolist(), 4, DEV)  # built outside the capture
    eager = {m: token_ops.grpo_dynamic_adv(r, mask, plan, m) for m in ("turn", "trajectory")}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        token_ops.grpo_dynamic_adv(r, mask, plan, "turn")
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = {m: token_ops.grpo_dynamic_adv(r, mask, plan, m) for m in ("turn", "trajectory")}
    graph.replay()
    torch.cuda.synchronize()
    for m in outs:
        assert torch.equal(outs[m], eager[m])
    r.copy_(torch.rand(n, generator=g).to(DEV))  # new rewards, same plan
    graph.replay()
    torch.cuda.synchronize()
    for m in outs:
        assert torch.equal(outs[m], token_ops.grpo_dynamic_adv(r, mask, plan, m))
