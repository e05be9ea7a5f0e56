"""The MLP policy kernels at every kind of obs / action shape config.validate_mlp_kernel_shapes admits, against float64.

The rest of the suite builds the policy with obs_dim = 42 (the bench shape).  The shapes below reach what 42 never does: a first
layer whose padded k extent (round_up(D, 32)) is 32 while its GEMM takes Tiles::K1P / 32 = 2 k-steps, flat buffers whose size is
no multiple of four (the scalar paths of the optimizer, the norm reduction and the weight-gradient stores), alignment gaps behind
actor_logstd, 2-, 9-, 15- and 16-wide heads, 3 and 4 value columns, and the value-free (phantom value net) policy.

References are float64 restatements evaluated on the same f32 inputs the kernels read.  Bars are derived, not tuned:
  * f32 (the three-plane split path): no farther from float64 than F32_MULT x the CPU float32 oracle's own distance, plus a floor
    of F32_FLOOR of the tensor's magnitude (the two differ only in summation order and the hardware tanh);
  * bf16: the bars of test_*_pinned_to_the_operand_rounded_restatement (tests/test_gpu_fused_step.py) against
    oracle/bf16_operand_model.py, with the same keep-away from the PPO clip edges.
"""

import copy
import ctypes
import math
import os
import subprocess
import tempfile

import pytest
import torch

from oracle import bf16_operand_model as BM
from oracle import ppo_oracle as O

pytestmark = pytest.mark.gpu

# (D, A, C, value head): reference configurations (examples/embodiment/config/) and the validator's edges
SHAPES = [
    (42, 8, 1, True),    # maniskill_ppo_mlp: the bench shape, the control
    (6, 2, 1, True),     # embodichain cart-pole: k extent 32, n_params % 4 == 2, 2-wide head
    (10, 8, 1, True),    # frankasim: k extent 32, vector optimizer path
    (16, 9, 1, True),    # genesis cube-pick: k extent 32, n_params % 4 == 1, 16-wide head at C = 1
    (8, 7, 1, False),    # LIBERO GRPO: phantom value net, value-free loss
    (1, 1, 1, True),     # validator minimum
    (32, 4, 4, True),    # D == KPAD, 16 outputs, 4 value columns
    (33, 5, 3, True),    # first D with a second k-block, 15 outputs, 3 value columns
    (64, 16, 1, True),   # validator maximum, no k padding
]
SHAPE_IDS = [f"D{d}-A{a}-C{c}-{'v' if v else 'novalue'}" for d, a, c, v in SHAPES]
PRECISIONS = ["f32", "bf16"]

F32_MULT = 4.0        # x the CPU float32 oracle's distance from float64
F32_FLOOR = 2.0 ** -16  # x the reference tensor's magnitude: f32 summation-order noise of a 256-term (or M-row) sum, with room


def _policies(shape, bf16, seed=7, jitter=0.02):
    from rlinf_amd.models.embodiment.mlp_policy import MLPPolicy
    D, A, C, vh = shape
    torch.manual_seed(seed)
    ora = O.OracleMLPPolicy(D, A, C, add_value_head=vh)
    with torch.no_grad():
        for p in ora.parameters():
            p.add_(torch.randn_like(p) * jitter)
    pol = MLPPolicy(D, A, C, vh, False, compute_dtype=torch.bfloat16 if bf16 else torch.float32)
    pol.load_reference_state_dict(ora.state_dict())
    return ora, pol.to("cuda")


def _owned(pol) -> torch.Tensor:
    """True at every flat-buffer element some exposed tensor owns; False at alignment gaps and the phantom value net."""
    m = torch.zeros(pol.n_params, dtype=torch.bool)
    for name in pol.shapes:
        o = pol.offsets[name]
        m[o:o + math.prod(pol.shapes[name])] = True
    return m


def _check_f32(name, got, want64, cpu32):
    """got (kernel) vs want64 (float64) against the CPU float32 oracle's own distance from float64."""
    got, want64, cpu32 = got.double().cpu(), want64.double().cpu(), cpu32.double().cpu()
    assert got.shape == want64.shape, (name, tuple(got.shape), tuple(want64.shape))
    assert torch.isfinite(got).all(), name
    err = float((got - want64).abs().max()) if got.numel() else 0.0
    own = float((cpu32 - want64).abs().max()) if got.numel() else 0.0
    bar = F32_MULT * own + F32_FLOOR * float(want64.abs().max()) + 1e-30
    assert err <= bar, f"{name}: |kernel - f64| {err:.3e} > {bar:.3e} (CPU f32 oracle: {own:.3e})"


def _check_bf16_rows(name, got, want, pool):
    """Rollout outputs vs the operand-rounding model: the bar of test_rollout_step_bf16_pinned_to_the_operand_rounded_restatement
    -- every element within 5e-3 here; the share within 2e-6 (at least 85 %) is a statistic over rows (one flipped activation
    moves a whole row), so it is taken over all batch sizes of the shape together (``pool``), not over one row at M = 1."""
    d = (got.cpu().double() - want.double()).abs().reshape(-1)
    assert float(d.max()) <= 5e-3, (name, float(d.max()))
    pool.setdefault(name.split(" M=")[0], []).append(d)


def _f64(ora):
    return copy.deepcopy(ora).double()


# ---- rollout launch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_rollout_step_shapes(shape, prec):
    """rlx_mlp_rollout_step: the policy job (actions, log-probs, values, states_copy), both value-job kinds (bootstrap fold into
    the rewards, plain values) and eval mode, at 1, a row tile + 1 and a large ragged batch."""
    from rlinf_amd import ops
    D, A, C, vh = shape
    bf16 = prec == "bf16"
    ora, pol = _policies(shape, bf16)
    o64 = _f64(ora)
    act, val = pol.layout.act_dim, pol.layout.val_dim
    pool = {}
    for M in (1, 33, 1029):
        g = torch.Generator().manual_seed(3 + M)
        states, eps = torch.randn(M, D, generator=g), torch.randn(M, act, generator=g)
        fin, last = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
        rewards = torch.rand(M, C, generator=g)
        flags = torch.rand(M, C, generator=g) < 0.4
        copy_ = torch.full((M, D), float("nan"), device="cuda")
        r_dev, last_v = rewards.cuda(), torch.full((M, val), float("nan"), device="cuda")
        a, lp, v = ops.mlp_rollout_step(pol.flat.data, pol.tiles(), pol.layout, states.cuda(), eps.cuda(), states_copy=copy_,
                                        value_jobs=(dict(states=fin.cuda(), rewards=r_dev, flags=flags.cuda(), gamma=0.8),
                                                    dict(states=last.cuda(), values=last_v)))
        a_eval, lp_eval, v_eval = ops.mlp_rollout_step(pol.flat.data, pol.tiles(), pol.layout, states.cuda(), None)
        assert torch.equal(copy_.cpu(), states)
        if not vh:  # the phantom value net: tanh(0) = 0 through every layer, exactly
            for t in (v, last_v, v_eval):
                assert not t.any()
            assert torch.equal(r_dev.cpu(), rewards)
        want_boot = o64.value_head.mlp(fin.double())[:, :1] if vh else torch.zeros(M, 1, dtype=torch.float64)
        if bf16:
            w_a, w_lp, w_v = BM.act(ora, states, eps)
            _check_bf16_rows(f"action M={M}", a, w_a, pool)
            torch.testing.assert_close(lp.cpu(), w_lp, rtol=1e-4, atol=1e-4)
            we_a = BM.act(ora, states, torch.zeros_like(eps))[0]
            _check_bf16_rows(f"eval action M={M}", a_eval, we_a, pool)
            if vh:
                _check_bf16_rows(f"value M={M}", v, w_v, pool)
                _check_bf16_rows(f"last value M={M}", last_v, BM.act(ora, last, eps)[2], pool)
                w_boot = BM.act(ora, fin, eps)[2][:, :1].double()
                w_r = rewards.double().clone()
                w_r[:, -1] += torch.where(flags[:, -1], 0.8 * w_boot[:, 0], torch.zeros(M, dtype=torch.float64))
                _check_bf16_rows(f"bootstrapped rewards M={M}", r_dev, w_r, pool)
            continue
        with torch.no_grad():
            w_a, w_lp, w_v = o64.act(states.double(), eps=eps.double(), mode="train")
            c_a, c_lp, c_v = ora.act(states, eps=eps, mode="train")
            _check_f32(f"action M={M}", a, w_a, c_a)
            _check_f32(f"logprob M={M}", lp, w_lp, c_lp)
            we = o64.act(states.double(), mode="eval")
            ce = ora.act(states, mode="eval")
            _check_f32(f"eval action M={M}", a_eval, we[0], ce[0])
            _check_f32(f"eval logprob M={M}", lp_eval, we[1], ce[1])
            if vh:
                _check_f32(f"value M={M}", v, w_v, c_v)
                _check_f32(f"last value M={M}", last_v, o64.value_head.mlp(last.double()), ora.value_head.mlp(last))
                c_boot = ora.value_head.mlp(fin)[:, :1]
                w_r, c_r = rewards.double().clone(), rewards.clone()
                w_r[:, -1] += torch.where(flags[:, -1], 0.8 * want_boot[:, 0], torch.zeros(M, dtype=torch.float64))
                c_r[:, -1] += torch.where(flags[:, -1], 0.8 * c_boot[:, 0], torch.zeros(M))
                _check_f32(f"bootstrapped rewards M={M}", r_dev, w_r, c_r)
                assert torch.equal(r_dev.cpu()[:, :-1], rewards[:, :-1]) and torch.equal(r_dev.cpu()[~flags[:, -1], -1],
                                                                                          rewards[~flags[:, -1], -1])
    for name, ds in pool.items():  # (D = 1: one input per first-layer unit, the smallest pre-activations and the most flips)
        exact = float((torch.cat(ds) <= 2e-6).double().mean())
        assert exact >= (0.75 if D == 1 else 0.85), (name, exact)


# ---- unfused learner / worker entries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_train_fwd_bwd_and_value_shapes(shape):
    """mlp_train_fwd / mlp_train_bwd (+ sum_slabs) and mlp_value (the learner's autograd forward, the async worker's values):
    log-prob, entropy, value and every parameter gradient of sum(lp * dlp + ent * dent + v * dv) against float64 autograd.
    Slabs start NaN at owned elements and 0 elsewhere: every owned element is written, nothing else is."""
    from rlinf_amd import ops
    D, A, C, vh = shape
    ora, pol = _policies(shape, False, seed=9)
    o64 = _f64(ora)
    lay = pol.layout
    owned = _owned(pol)
    for M in (1, 31, 4101):
        g = torch.Generator().manual_seed(17 + M)
        states, action = torch.randn(M, D, generator=g), torch.randn(M, lay.act_dim, generator=g) * 0.6
        d_lp, d_ent = torch.randn(M, lay.act_dim, generator=g), torch.randn(M, lay.act_dim, generator=g)
        d_v = torch.randn(M, lay.val_dim, generator=g)
        lp, ent, v, mean, acts = ops.mlp_train_fwd(pol.flat.data, pol.packed(), lay, states.cuda(), action.cuda())
        slabs = ops.mlp_bwd_slabs(M)
        grads = torch.where(owned, float("nan"), 0.0).repeat(slabs, 1).cuda()
        ops.mlp_train_bwd(pol.flat.data, pol.packed(), lay, states.cuda(), action.cuda(), mean, acts, d_lp.cuda(), d_ent.cuda(),
                          d_v.cuda(), grads=grads)
        got = ops.sum_slabs(grads).cpu()
        v_only = ops.mlp_value(pol.flat.data, pol.packed(), lay, states.cuda())
        assert torch.isfinite(got[owned]).all(), "an owned gradient element was never written"
        assert not got[~owned].any(), "a gap / phantom element was written"
        outs = {}
        for tag, model, st, ac, dl, de, dv in (("f64", o64, states.double(), action.double(), d_lp.double(), d_ent.double(), d_v.double()),
                                                ("f32", ora, states, action, d_lp, d_ent, d_v)):
            model.zero_grad()
            out = model.evaluate(st, ac)
            obj = (out["logprobs"] * dl).sum() + (out["entropy"] * de).sum()
            if vh:
                obj = obj + (out["values"] * dv).sum()
            obj.backward()
            outs[tag] = (out, {n: p.grad.detach().clone() for n, p in model.named_parameters()})
        (o_w, g_w), (o_c, g_c) = outs["f64"], outs["f32"]
        _check_f32(f"logprob M={M}", lp, o_w["logprobs"].detach(), o_c["logprobs"].detach())
        _check_f32(f"entropy M={M}", ent, o_w["entropy"].detach(), o_c["entropy"].detach())
        if vh:
            _check_f32(f"value M={M}", v, o_w["values"].detach(), o_c["values"].detach())
            _check_f32(f"mlp_value M={M}", v_only, o_w["values"].detach(), o_c["values"].detach())
        else:
            assert not v.any() and not v_only.any()
        for name, w in g_w.items():
            o = pol.offsets[name]
            _check_f32(f"grad {name} M={M}", got[o:o + w.numel()], w.reshape(-1), g_c[name].reshape(-1))


# ---- fused optimizer step ------------------------------------------------------------------------------------------------------
def _step_case(shape, M, g, with_mask, policy_eval):
    """A minibatch whose PPO ratios sit 0.04 away from both clip edges and whose values sit 0.02 away from the value clip, in
    the model's own outputs (``policy_eval`` -> dict(logprobs, values)): f64, f32 and bf16 arithmetic take the same branches."""
    D, A, C, vh = shape
    act = A * C
    mb = dict(states=torch.randn(M, D, generator=g), action=torch.randn(M, act, generator=g) * 0.6)
    if vh:  # action-level actor-critic: [M, C] ratios, advantages, values
        mb.update(advantages=torch.randn(M, C, generator=g), prev_values=torch.randn(M, C, generator=g),
                  returns=torch.randn(M, C, generator=g))
        nm, groups = C, C
    else:   # value-free GRPO: one chunk-level ratio per row
        mb.update(advantages=torch.randn(M, 1, generator=g))
        nm, groups = 1, 1
    if with_mask:
        mb["loss_mask"] = torch.rand(M, nm, generator=g) < 0.7
    cur = policy_eval(mb["states"], mb["action"])
    delta = (torch.randn(M, act, generator=g) * 0.08).view(M, groups, act // groups)
    for edge in (math.log(0.8), math.log(1.2)):  # a ratio's log is -sum(delta) over its group
        near = (-delta.sum(-1) - edge).abs() < 0.04
        delta[:, :, 0] = torch.where(near, delta[:, :, 0] + 0.1, delta[:, :, 0])
    mb["prev_logprobs"] = (cur["logprobs"].float() + delta.reshape(M, act)).contiguous()
    if vh:
        gap = (cur["values"].float() - mb["prev_values"]).abs()
        mb["prev_values"] = torch.where((gap - 1.0).abs() < 0.02, mb["prev_values"] + 0.05, mb["prev_values"])
    return mb


def _oracle_loss(shape, out, mb):
    D, A, C, vh = shape
    if vh:
        sh = O.shape_loss_inputs(out["logprobs"], mb["prev_logprobs"].to(out["logprobs"].dtype), mb["advantages"].to(out["logprobs"].dtype),
                                 "action_level", A, loss_mask=mb.get("loss_mask"), values=out["values"],
                                 prev_values=mb["prev_values"].to(out["values"].dtype), returns=mb["returns"].to(out["values"].dtype),
                                 reward_type="action_level")
        return O.ppo_actor_critic_loss(clip_ratio_low=0.2, clip_ratio_high=0.2, value_clip=1.0, huber_delta=10.0, **sh)
    sh = O.shape_loss_inputs(out["logprobs"], mb["prev_logprobs"].to(out["logprobs"].dtype), mb["advantages"].to(out["logprobs"].dtype),
                             "chunk_level", A, loss_mask=mb.get("loss_mask"), reward_type="chunk_level")
    return O.ppo_actor_loss(sh["logprobs"], sh["old_logprobs"], sh["advantages"], 0.2, 0.2, loss_mask=sh["loss_mask"])


def _run_step(pol, shape, mb, bf16, grads=None):
    from rlinf_amd import ops
    from rlinf_amd._lib import PPO_OUT_FLOATS
    D, A, C, vh = shape
    lay, M = pol.layout, mb["states"].shape[0]
    if vh:
        lp = ops.make_ppo_params(logprob_type="action_level", action_dim=A, chunks=C, clip_ratio_low=0.2, clip_ratio_high=0.2,
                                 value_clip=1.0, huber_delta=10.0, max_episode_steps=50, has_critic=True, reward_type="action_level")
    else:
        lp = ops.make_ppo_params(logprob_type="chunk_level", action_dim=A, chunks=C, clip_ratio_low=0.2, clip_ratio_high=0.2,
                                 max_episode_steps=50, has_critic=False, reward_type="chunk_level")
    if grads is None:
        grads = torch.where(_owned(pol), float("nan"), 0.0).repeat(ops.ppo_step_slabs(lay, M, bf16=bf16), 1).cuda()
    ws = torch.empty(ops.ppo_step_workspace_bytes(lay, M), dtype=torch.uint8, device="cuda")
    row = torch.zeros(PPO_OUT_FLOATS, device="cuda")
    dev_mb = {k: v.cuda().contiguous() for k, v in mb.items()}
    if "loss_mask" in dev_mb:
        dev_mb["loss_mask"] = dev_mb["loss_mask"].view(torch.uint8)
    ops.ppo_step(pol.flat.data, lay, lp, dev_mb, grads, row, ws, grad_out=1.0, bf16=bf16)
    return grads, row


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_ppo_step_shapes(shape, prec):
    """rlx_ppo_step (forward + loss + backward) with and without a loss mask: gradients tensor by tensor and the metric row.
    Slabs start NaN at every owned element and 0 at every gap / phantom element: afterwards every owned element is finite (it
    was written) and every other one is still exactly 0."""
    from rlinf_amd._lib import PPO_OUT_NAMES
    D, A, C, vh = shape
    bf16 = prec == "bf16"
    ora, pol = _policies(shape, bf16, seed=11)
    o64 = _f64(ora)
    owned = _owned(pol)
    keys = ("actor/ratio", "actor/clipped_ratio", "actor/approx_kl", "actor/policy_loss") + (("critic/value_loss",) if vh else ())
    for M, with_mask in ((1, False), (31, True), (33, False), (4101, True)):
        g = torch.Generator().manual_seed(5 + M)
        if bf16:
            mb = _step_case(shape, M, g, with_mask, lambda s, a: {k: v.detach() for k, v in BM.evaluate(ora, s, a).items()})
        else:
            mb = _step_case(shape, M, g, with_mask, lambda s, a: {k: v.detach().float() for k, v in o64.evaluate(s.double(), a.double()).items()})
        grads, row = _run_step(pol, shape, mb, bf16)
        slab = grads.cpu()
        assert torch.isfinite(slab[:, owned]).all(), "an owned gradient element was never written"
        assert not slab[:, ~owned].any(), "a gap / phantom gradient element was written"
        got = slab.sum(0)
        host = row.cpu()
        if bf16:
            ora.zero_grad()
            loss, metrics = _oracle_loss(shape, BM.evaluate(ora, mb["states"], mb["action"]), mb)
            loss.backward()
            want = {n: p.grad.clone() for n, p in ora.named_parameters()}
            cat = torch.cat([want[n].reshape(-1) for n in want])
            flat = torch.cat([got[pol.offsets[n]:pol.offsets[n] + want[n].numel()] for n in want])
            rel = float((flat - cat).norm() / cat.norm())
            worst = max((float((got[pol.offsets[n]:pol.offsets[n] + w.numel()] - w.reshape(-1)).norm() / (w.norm() + 1e-12)), n)
                        for n, w in want.items() if w.numel() >= 64)
            # The pinned test's bars, with two absolute floors it does not need at D = 42: a flipped bf16 rounding moves a row's
            # outputs by up to ~1e-3 in a few per cent of the rows, so a loss / metric near 0 moves by up to ~5e-5 absolute, and at
            # D <= 16 the first layers' pre-activations are small (few inputs), their bf16 ulp with them, and flips several times as
            # frequent: one tensor's relative error may reach 5e-3 (a dropped column or output is 1e-1 and more).  The whole-gradient
            # bar and the small-batch bars are the pinned test's own.  At D = 1 (one input per first-layer unit) backbone.0.weight is
            # a single 256-vector of dZ . x sums, and its flips do not average out: 1e-2 there.
            small = M <= 8
            assert rel <= (2e-6 if small else 1e-3), (M, rel)
            assert worst[0] <= (1e-5 if small else 1e-2 if D == 1 else 5e-3), (M, worst)
            assert float(host[PPO_OUT_NAMES["loss"]]) == pytest.approx(float(loss), rel=1e-4, abs=1e-6 if small else 5e-5)
            assert float(host[PPO_OUT_NAMES["actor/clip_fraction"]]) == float(metrics["actor/clip_fraction"])
            for key in keys:
                assert float(host[PPO_OUT_NAMES[key]]) == pytest.approx(float(metrics[key]), rel=5e-4, abs=2e-5 if small else 5e-5), key
            continue
        res = {}
        for tag, model, cast in (("f64", o64, torch.float64), ("f32", ora, torch.float32)):
            model.zero_grad()
            mb_t = {k: (v.to(cast) if v.is_floating_point() else v) for k, v in mb.items()}
            loss, metrics = _oracle_loss(shape, model.evaluate(mb_t["states"], mb_t["action"]), mb_t)
            loss.backward()
            res[tag] = (float(loss.detach()), {k: float(v) for k, v in metrics.items()},
                        {n: p.grad.detach().clone() for n, p in model.named_parameters()})
        (l64, m64, g64), (l32, m32, g32) = res["f64"], res["f32"]
        for name, w in g64.items():
            o = pol.offsets[name]
            _check_f32(f"grad {name} M={M}", got[o:o + w.numel()], w.reshape(-1), g32[name].reshape(-1))
        assert float(host[PPO_OUT_NAMES["actor/clip_fraction"]]) == m64["actor/clip_fraction"]  # same branches, row by row
        for key, k64, k32 in (("loss", l64, l32),) + tuple((k, m64[k], m32[k]) for k in keys):
            err, own = abs(float(host[PPO_OUT_NAMES[key]]) - k64), abs(k32 - k64)
            assert err <= F32_MULT * own + F32_FLOOR * abs(k64) + 1e-9, (key, M, err, own)


# ---- clip + AdamW with the weight image ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_clip_adamw_shapes(shape, prec):
    """rlx_clip_adamw_step over several steps on split-K slabs with the policy's own groups and the tile image: parameters and
    both moments against torch.optim.AdamW in float64 on the same clipped gradients, a non-finite gradient that skips the whole
    step, gaps that stay 0, and an image bit-identical to rlx_mlp_pack_tiles of the final parameters.  Where the parameter count
    allows it (n % 4 == 0) the one-launch form runs the same sequence."""
    from rlinf_amd import ops
    D, A, C, vh = shape
    bf16 = prec == "bf16"
    lr, vlr, wd, max_norm, betas, eps_ = 3e-3, 1e-3, 0.01, 0.5, (0.9, 0.999), 1e-8
    _, pol = _policies(shape, bf16, seed=5)
    lay = pol.layout
    n = lay.n_params
    owned = _owned(pol)
    groups = pol.group_ranges(lr, vlr, train_value_head=vh)
    covered = torch.zeros(n, dtype=torch.bool)
    for b, e, _ in groups:
        covered[b:e] = True
    assert torch.equal(covered & owned, owned)  # every owned element is trained; the ranges may span gaps (zeros)
    last = int(owned.nonzero().max())
    w1 = pol.offsets["backbone.0.weight"]
    g = torch.Generator().manual_seed(13)
    steps = []
    for k in range(5):
        # every summed gradient at least 1e-2 (before the clip) from 0: AdamW's g / (|g| + eps) is then insensitive to the f32
        # rounding of the slab sum, and the comparison is of the optimizer's arithmetic, not of a sign flip of a ~0 gradient
        s = (torch.rand(n, generator=g) + 0.5) * torch.where(torch.rand(n, generator=g) < 0.5, -1e-2, 1e-2)
        s = s.repeat(3, 1) * (torch.rand(3, n, generator=g) * 0.5 + 0.75)
        s[:, last] = 0.2 * (k + 1)      # the last owned element carries the norm: a reduction that drops it clips differently
        s[:, w1 + D - 1] += 0.05        # ... and the first layer's last input column a visible update
        s[:, ~owned] = 0.0
        if k == 2:
            s[1, w1 + min(3, D - 1)] = float("inf")  # this step is skipped as a whole
        steps.append(s)
    forms = [None]
    sync = ops.adamw_sync_words(n, "cuda") if n % 4 == 0 else None
    if sync is not None:
        forms.append(sync)
    init = pol.flat.data.clone()
    for sync in forms:
        params = init.clone()
        tiles = ops.mlp_pack_tiles(params, lay, bf16=bf16)
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        ref = params.cpu().double()
        pref = [torch.nn.Parameter(ref[b:e].clone()) for b, e, _ in groups]
        opt = torch.optim.AdamW([{"params": [p], "lr": r} for p, (_, _, r) in zip(pref, groups)], betas=betas, eps=eps_,
                                weight_decay=wd)
        t = 0
        for k, s in enumerate(steps):
            stats = ops.clip_adamw_step_(params, s.cuda(), m, v, groups, t + 1, betas=betas, eps=eps_, weight_decay=wd,
                                         max_grad_norm=max_norm, tile_layout=lay, tiles=tiles, sync=sync)
            st = stats.cpu()
            gsum = s.double().sum(0)
            norm = float(gsum.norm())
            if not math.isfinite(norm):
                assert not math.isfinite(float(st[0])) and float(st[1]) == 0.0, st
            else:
                assert float(st[0]) == pytest.approx(norm, rel=1e-5), (k, float(st[0]), norm)
                coef = min(1.0, max_norm / (norm + 1e-6))
                for p, (b, e, _) in zip(pref, groups):
                    p.grad = gsum[b:e] * coef
                opt.step()
                t += 1
            host = params.cpu()
            want = torch.zeros(n, dtype=torch.float64)
            want_m, want_v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
            want[:] = init.cpu().double()
            for p, (b, e, _) in zip(pref, groups):
                want[b:e] = p.detach()
                if opt.state.get(p):
                    want_m[b:e], want_v[b:e] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
            lr_of = torch.zeros(n, dtype=torch.float64)
            for b, e, r in groups:
                lr_of[b:e] = r
            perr = (host.double() - want).abs()
            pbar = t * (2.0 ** -21 * want.abs() + 2.0 ** -14 * lr_of) + 1e-30
            assert bool((perr <= pbar).all()), (sync is not None, k, float((perr - pbar).max()), int((perr > pbar).nonzero()[0]))
            for nm_, got_, w_ in (("exp_avg", m.cpu(), want_m), ("exp_avg_sq", v.cpu(), want_v)):
                err = (got_.double() - w_).abs()
                assert bool((err <= 2.0 ** -17 * w_.abs() + 1e-30 + 2.0 ** -18 * float(w_.abs().max())).all()), (nm_, k, float(err.max()))
            assert not host[~owned].any(), "an alignment gap / phantom element moved"
            fresh = ops.mlp_pack_tiles(params, lay, bf16=bf16)
            bits = (lambda x: x.view(torch.int16)) if bf16 else (lambda x: x.view(torch.int32))
            assert torch.equal(bits(tiles), bits(fresh)), f"weight image out of step after step {k} (one launch: {sync is not None})"


# ---- LDS independence ----------------------------------------------------------------------------------------------------------
_LDS_LIB = None


def _lds_fill_lib():
    """tests/helpers/lds_fill.hip, compiled on first use with the package's own hipcc flags into a temporary directory."""
    global _LDS_LIB
    if _LDS_LIB is None:
        from rlinf_amd.csrc import build as B
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "lds_fill.hip")
        out = os.path.join(tempfile.mkdtemp(prefix="lds_fill_"), "lds_fill.so")
        r = subprocess.run([B.hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lib = ctypes.CDLL(out)
        lib.lds_fill.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.lds_fill.restype = ctypes.c_int
        _LDS_LIB = lib
    return _LDS_LIB


def _fill_lds(value: int):
    lib = _lds_fill_lib()
    blocks = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    out = torch.empty(blocks, dtype=torch.int32, device="cuda")
    assert lib.lds_fill(value, blocks, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return out


LDS_SHAPES = [s for s in SHAPES if s[0] in (1, 6, 16, 32)]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape", LDS_SHAPES, ids=[SHAPE_IDS[SHAPES.index(s)] for s in LDS_SHAPES])
def test_outputs_do_not_depend_on_stale_lds(shape, prec):
    """The first layer's GEMM takes Tiles::K1P / 32 k-steps whatever D is; at D <= 32 the states slab's k tail past 32 is zero only
    if the launch wrote it.  Run the rollout step and the fused optimizer step once behind a kernel that zeroed every CU's LDS and
    once behind one that filled it with 0xFFFFFFFF (NaN in f32 and bf16): the outputs must be bit-identical (and finite)."""
    D, A, C, vh = shape
    bf16 = prec == "bf16"
    ora, pol = _policies(shape, bf16, seed=19)
    lay = pol.layout
    M = 1029
    g = torch.Generator().manual_seed(23)
    states, eps, fin = (torch.randn(M, D, generator=g).cuda(), torch.randn(M, lay.act_dim, generator=g).cuda(),
                        torch.randn(M, D, generator=g).cuda())
    mb = _step_case(shape, M, g, True, lambda s, a: {k: v.detach() for k, v in ora.evaluate(s, a).items()})
    tiles = pol.tiles()
    from rlinf_amd import ops

    def run(fill):
        rew = torch.zeros(M, C, device="cuda")
        flags = torch.ones(M, C, dtype=torch.bool, device="cuda")
        vals = torch.empty(M, lay.val_dim, device="cuda")
        grads = torch.where(_owned(pol), float("nan"), 0.0).repeat(ops.ppo_step_slabs(lay, M, bf16=bf16), 1).cuda()
        torch.cuda.synchronize()
        _fill_lds(fill)
        a, lp, v = ops.mlp_rollout_step(pol.flat.data, tiles, lay, states, eps,
                                        value_jobs=(dict(states=fin, rewards=rew, flags=flags, gamma=0.8), dict(states=fin, values=vals)))
        _fill_lds(fill)
        grads, row = _run_step(pol, shape, mb, bf16, grads=grads)
        torch.cuda.synchronize()
        return dict(action=a, logprob=lp, value=v, rewards=rew, values=vals, grads=grads.sum(0), row=row)

    clean, dirty = run(0), run(0xFFFFFFFF)
    bad = []
    for k in clean:
        assert k == "row" or torch.isfinite(clean[k]).all(), k
        if not torch.equal(clean[k].view(torch.int32), dirty[k].view(torch.int32)):
            nanrows = int((~torch.isfinite(dirty[k])).reshape(dirty[k].shape[0], -1).any(-1).sum()) if dirty[k].dim() else 0
            bad.append(f"{k}: {nanrows} non-finite rows / {dirty[k].shape[0]}")
    assert not bad, f"D={D} {prec}: outputs depend on what LDS held before the launch: " + "; ".join(bad)


# ---- whole loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hip_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("shape", [(6, 2, 1, True), (16, 9, 1, True), (8, 7, 1, False)], ids=["cartpole", "genesis", "libero-grpo"])
def test_whole_loop_at_reference_shapes(shape, hip_graph):
    """Rollout -> GAE (or GRPO) -> fused step -> clip + AdamW (its scalar path where n_params % 4 != 0) through the runner, eager
    and as replayed hipGraphs, against oracle.ppo_loop.iteration on identical seeds, weights, injected noise and shuffle order
    (the pattern of test_end_to_end.py::test_action_chunks_whole_loop_matches_oracle) at obs / action shapes other than 42 / 8."""
    from oracle import ppo_loop as L
    from test_end_to_end import _build, make_cfg
    D, A, C, vh = shape
    B, T, GB, group = 32, 12, 96, 4
    cfg = make_cfg(total_envs=B, steps=T, global_batch=GB, auto_reset=vh, hip_graph=hip_graph, done_mode=None if vh else "bernoulli")
    cfg.actor.model.obs_dim, cfg.actor.model.action_dim, cfg.actor.model.add_value_head = D, A, vh
    if not vh:
        cfg.algorithm.adv_type, cfg.algorithm.loss_type, cfg.algorithm.group_size = "grpo", "actor", group
        cfg.env.train.group_size = group
    env = L.synthetic_env_tensors(0, T, B, D, max_episode_steps=5, mode="periodic" if vh else "bernoulli", p_done=0.05)
    torch.manual_seed(11)
    ora = O.OracleMLPPolicy(D, A, C, add_value_head=vh)
    sd = copy.deepcopy(ora.state_dict())
    opt = O.build_adamw(ora)
    runner = _build(cfg, env, sd)
    w = runner.actor.worker
    model = w.model
    assert model.layout.obs_dim == D and model.layout.act_dim == A
    owned = _owned(model)
    for it in range(3 if hip_graph else 2):
        eps = torch.randn(T, B, A, generator=torch.Generator().manual_seed(100 + it))
        kw = dict(auto_reset=True) if vh else dict(auto_reset=False, max_episode_steps=5, adv_type="grpo", loss_type="actor",
                                                   group_size=group)
        batch, om = L.iteration(ora, opt, env, eps, gamma=0.8, gae_lambda=0.9, seed=1234, global_batch=GB, update_epoch=2, **kw)
        metrics = runner.run_step(eps.cuda())
        rb = w.rollout_batch
        tol = dict(rtol=2e-4, atol=2e-5) if it == 0 else dict(rtol=5e-3, atol=5e-4)
        torch.testing.assert_close(rb["forward_inputs"]["action"].cpu(), batch["forward_inputs"]["action"], **tol)
        torch.testing.assert_close(rb["prev_logprobs"].cpu(), batch["prev_logprobs"], **tol)
        if vh:
            torch.testing.assert_close(rb["prev_values"].cpu(), batch["prev_values"], **tol)
            torch.testing.assert_close(rb["rewards"].cpu(), batch["rewards"], **tol)
            torch.testing.assert_close(rb["returns"].cpu(), batch["returns"], **tol)
        else:
            assert not rb["prev_values"].any()
            assert torch.equal(rb["rewards"].cpu(), batch["rewards"]) and torch.equal(rb["loss_mask"].cpu(), batch["loss_mask"])
        assert torch.equal(rb["dones"].cpu(), batch["dones"])
        torch.testing.assert_close(rb["advantages"].cpu(), batch["advantages"], rtol=tol["rtol"] * 5, atol=tol["atol"] * 5)
        keys = ("actor/total_loss", "actor/grad_norm", "actor/policy_loss", "actor/approx_kl") + (("critic/value_loss",) if vh else ())
        for k in keys:
            want_k = sum(float(m[k]) for m in om) / len(om)
            assert metrics["train/" + k] == pytest.approx(want_k, rel=5e-3, abs=5e-5), k
        got = model.flat.detach().cpu()
        diff = (model.exposed_flat().cpu() - torch.cat([p.detach().reshape(-1) for p in ora.parameters()])).abs()
        steps_taken = len(om) * (it + 1)
        assert float(diff.max()) <= 2 * 3e-4 * steps_taken + 1e-6
        assert float((diff > 2e-5 * (it + 1)).float().mean()) < 0.02, float((diff > 2e-5 * (it + 1)).float().mean())
        assert not got[~owned].any()  # alignment gaps (and the phantom value net) stay zero
