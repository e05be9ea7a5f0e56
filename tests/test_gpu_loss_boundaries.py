"""The HIP loss entries ON the branches of their hand-written derivative: ties of torch.max / torch.min, the closed intervals of
the clamps, the Huber switch, the behaviour-weight threshold, |x| at 0.  `pytest -m gpu`.

csrc/ppo_loss_math.h computes the per-element derivative in the forward pass and promises autograd's tie rules.  The inputs come
from tests/helpers/loss_boundaries.py: dyadic rationals, so an element placed on a comparison sits on it bit for bit on host and
device (the only transcendental on a boundary is exp(0)), and every other element keeps a margin from every comparison -- asserted
in float64 from the inputs before anything is launched, together with the count of elements on each named boundary.

Reference: the oracle's torch-autograd restatements in f32 on the CPU (pinned to the reference at these inputs by
tests/test_loss_boundaries_host.py).  Bars: those of tests/test_gpu_losses.py for the same quantities -- loss and metrics rtol 1e-5 /
atol 1e-6, gradients rtol 1e-5 / atol 1e-7 -- and, where the value is exact by construction, equality:
  * count metrics (clip / dual-clip / behaviour-clip fractions, value_clip_ratio) as integers after multiplying by their
    denominator;
  * the device's gradient scales against 1 / the oracle's denominators;
  * the gradient of every critic element, and of every actor element whose ratio and behaviour weight are exactly 1: there the
    sum-form derivative is a product of dyadic numbers, so the oracle's gradient times its denominator is snapped to that grid
    (it must already lie within 2**-20 of it) and the device gradient must equal, bit for bit, that number times the device's own
    ACTOR_GRAD_SCALE / CRITIC_GRAD_SCALE times the upstream 0.5 -- the one rounding the backward kernel makes.  The reasoning
    loss publishes no gradient scale; its backward multiplies by fl32(1 / (denominator * tokens of the sequence)), a correctly
    rounded f64 division that the test restates from the mask.
"""

import pytest
import torch

from helpers import loss_boundaries as LB

pytestmark = pytest.mark.gpu
RTOL, ATOL, ATOL_GRAD = 1e-5, 1e-6, 1e-7
CASES = LB.cases()
GRID = 2.0 ** 13  # sum-form derivatives on a boundary: multiples of 2**-13 (advantages, errors and deltas on 2**-6, weights 1/2)


def test_the_table_covers_every_named_boundary():
    cov = LB.coverage(CASES)
    LB.assert_coverage(cov)
    for name, c in sorted(cov.items()):
        print(f"{name:72s} {c}")


def _dev(t, offset=False):
    if t is None:
        return None
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")  # the tensor starts 4 bytes into its allocation
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _close(got, want, what, atol=ATOL):
    torch.testing.assert_close(torch.as_tensor(got, dtype=torch.float32).cpu().reshape(()),
                               torch.as_tensor(want).float().reshape(()), rtol=RTOL, atol=atol, msg=lambda m: f"{what}: {m}")


def _same_count(got, want, den, what):
    g, w = float(got) * den, float(want) * den
    print(f"  {what}: device {g:.4f} oracle {w:.4f} (of {den:g})")
    assert abs(g - round(g)) < 1e-2 and abs(w - round(w)) < 1e-2, (what, g, w)
    assert round(g) == round(w), (what, g, w)


def _exact_grad(got, want, den, scale_dev, sel, what):
    """got == fl32(fl32(0.5 * scale_dev) * g) on ``sel``, g = the oracle's sum-form derivative snapped to the dyadic grid."""
    q = want.double() * den / LB.UPSTREAM
    g = (q * GRID).round() / GRID
    assert float((q - g).abs()[sel].max()) <= 2.0 ** -20, f"{what}: the oracle's own derivative is off the grid"
    expect = g.float() * (torch.tensor(LB.UPSTREAM, dtype=torch.float32) * torch.tensor(scale_dev, dtype=torch.float32))
    bad = (got != expect) & sel
    assert not bool(bad.any()), (what, int(bad.sum()), int(sel.sum()), got[bad][:4].tolist(), expect[bad][:4].tolist(),
                                 (got[bad][:4] / expect[bad][:4]).tolist())
    return int(sel.sum())


def _raw_flags(flags, raw_shape):
    """Flags per loss element -> per raw log-prob (an element's raw log-probs are adjacent)."""
    n = flags.numel()
    return flags.reshape(n, 1).expand(n, raw_shape.numel() // n).reshape(raw_shape)


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] != "token"], ids=lambda c: c["id"])
def test_embodied_losses_on_their_boundaries(case):
    from rlinf_amd import _lib, ops
    from rlinf_amd.algorithms import registry

    inp = LB.build(case)
    flags = LB.classify(case, inp)  # grid + margin, from the inputs, in float64, before the first launch
    want = LB.run_oracle(case, inp)
    kw = LB.loss_kwargs(case)
    dec = case["family"] == "decoupled"
    names = _lib.DPPO_OUT_NAMES if dec else _lib.PPO_OUT_NAMES
    lt, A, crit = case["logprob_type"], case["action_dim"], case["has_critic"]
    tens = {k: _dev(inp.get(k), case["offset"] and k in ("logprobs", "old_logprobs"))
            for k in ("logprobs", "old_logprobs", "advantages", "values", "prev_values", "returns", "loss_mask", "loss_mask_sum",
                      "proximal_logprobs", "versions")}
    den_a, den_c = LB.denominators(case, inp)
    mask = inp.get("loss_mask")
    sub = A if lt == "token_level" else 1
    n_valid = float(inp["n_adv"] * sub if mask is None else max(int(mask.sum()), 1))
    # elements whose derivative is exact: ratio == 1 and behaviour weight == 1
    exact = flags["actor/ratio==1"][0] & flags["actor/lp==old"][0]
    if dec and case["threshold"] is not None:  # (an element the threshold masks has derivative 0: exact as well)
        exact = exact | (flags[f"decoupled/{case['prox_mode']}: weight>threshold"][0] if case["prox_mode"] != "old"
                         else torch.zeros_like(exact))
    exact_raw = _raw_flags(exact, inp["logprobs"].shape)
    assert int(exact_raw.sum()) >= 2
    if not case["loss"]["critic_warmup"]:  # (under warm-up the actor term is a constant: its gradient is 0 by definition)
        assert int(((want["d_logprobs"] != 0) & exact_raw).sum()) >= 2, "the bit-for-bit comparison would compare zeros"

    entries = ["registry"] if dec else ["ops", "registry"]
    for entry in entries:
        lp = tens["logprobs"].detach().requires_grad_(True)
        v = tens["values"].detach().requires_grad_(True) if crit else None
        if entry == "ops":
            loss, out = ops.ppo_loss(lp, tens["old_logprobs"], tens["advantages"], logprob_type=lt, action_dim=A, values=v,
                                     prev_values=tens["prev_values"], returns=tens["returns"], loss_mask=tens["loss_mask"],
                                     loss_mask_sum=tens["loss_mask_sum"], has_critic=crit, **kw)
            metrics = {k: out[i] for k, i in names.items()}
        else:
            extra = {}
            if dec:
                extra = dict(proximal_logprobs=tens["proximal_logprobs"], versions=tens["versions"],
                             current_version=LB.CURRENT_VERSION if case["prox_mode"] == "versions" else None,
                             behave_weight_threshold=case["threshold"])
            loss, metrics = registry.policy_loss(
                task_type="embodied", loss_type="decoupled_actor_critic" if dec else ("actor_critic" if crit else "actor"),
                logprob_type=lt, reward_type="chunk_level" if lt == "chunk_level" else "action_level", single_action_dim=A,
                logprobs=lp, old_logprobs=tens["old_logprobs"], advantages=tens["advantages"], values=v,
                prev_values=tens["prev_values"], returns=tens["returns"], loss_mask=tens["loss_mask"],
                loss_mask_sum=tens["loss_mask_sum"], **extra, **kw)
            out = metrics.device_vector
        (loss * LB.UPSTREAM).backward()
        tag = f"{case['id']} [{entry}]"
        print(tag)
        _close(loss.detach(), want["loss"], f"{tag} loss")
        wm = want["metrics"]
        keys = [k for k in wm if k.startswith("actor/") and k != "actor/current_version"]
        keys += ["critic/value_loss", "critic/value_clip_ratio"] if crit else []
        if entry == "registry":
            assert {k for k in metrics if k.startswith("actor/")} == {k for k in wm if k.startswith("actor/")}, tag
        for k in keys:
            _close(metrics[k], wm[k], f"{tag} {k}")
        for k in ("actor/clip_fraction", "actor/dual_clip_fraction", "actor/behav_clip_fraction"):
            if k in wm:
                _same_count(metrics[k], wm[k], n_valid, f"{tag} {k}")
        if crit:
            _same_count(metrics["critic/value_clip_ratio"], wm["critic/value_clip_ratio"], float(inp["n_adv"]), f"{tag} value_clip_ratio")
        got_lp = lp.grad.cpu()
        torch.testing.assert_close(got_lp, want["d_logprobs"], rtol=RTOL, atol=ATOL_GRAD, msg=lambda m: f"{tag} d_logprobs: {m}")
        row = out.cpu()
        sa = float(row[_lib.PPO_ACTOR_GRAD_SCALE])
        assert sa == float(torch.tensor(1.0 / den_a, dtype=torch.float32)), (tag, sa, den_a)
        n_exact = _exact_grad(got_lp, want["d_logprobs"], den_a, sa, exact_raw, f"{tag} d_logprobs on ratio == 1")
        if crit:
            got_v = v.grad.cpu()
            torch.testing.assert_close(got_v, want["d_values"], rtol=RTOL, atol=ATOL_GRAD, msg=lambda m: f"{tag} d_values: {m}")
            sc = float(row[_lib.PPO_CRITIC_GRAD_SCALE])
            assert sc == float(torch.tensor(1.0 / den_c, dtype=torch.float32)), (tag, sc, den_c)
            n_exact += _exact_grad(got_v, want["d_values"], den_c, sc, torch.ones_like(got_v, dtype=torch.bool), f"{tag} d_values")
        print(f"  {n_exact} gradient entries compared bit for bit")


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] == "token"], ids=lambda c: c["id"])
def test_reasoning_loss_on_its_boundaries(case):
    """As above for token_ops.token_loss.  Bit for bit: every token whose ratio is exactly 1 (masked ones included: 0 on both
    sides), except under k3 the tokens off lp == ref, whose KL derivative exp(lp - ref) - 1 is no dyadic number.  The kernel
    forms g = fma(kl_beta, dk, g_actor) -- exact on the grid -- and the backward rounds once: fl32(g * fl32(w * 0.5)),
    w = fl32(1 / (den * cnt)): den = the tokens on (token-mean) or bsz, cnt = the sequence's tokens on (seq-mean-token-mean) or 1."""
    from rlinf_amd import _lib, token_ops

    inp = LB.build(case)
    flags = LB.classify(case, inp)
    want = LB.run_oracle(case, inp)
    loss_kw = case["loss"]
    params = token_ops.make_token_loss_params(
        loss_agg=case["agg"], clip_ratio_low=loss_kw["clip_ratio_low"], clip_ratio_high=loss_kw["clip_ratio_high"],
        clip_ratio_c=loss_kw["clip_ratio_c"], clip_log_ratio_min=loss_kw.get("clip_log_ratio_min"),
        clip_log_ratio_max=loss_kw.get("clip_log_ratio_max"), kl_penalty_type=case["kl"], kl_beta=LB.KL_BETA if case["kl"] else 0.0)
    lp = inp["logprobs"].cuda().requires_grad_(True)
    loss, out = token_ops.token_loss(lp, inp["old_logprobs"].cuda(), inp["advantages"].cuda(), _dev(inp["loss_mask"]), params,
                                     ref_logprobs=_dev(inp.get("ref_logprobs")))
    (loss * LB.UPSTREAM).backward()
    tag = case["id"]
    print(tag)
    wm = want["metrics"]
    _close(loss.detach(), want["loss"], f"{tag} loss")
    _close(out[_lib.TOK_OUT_NAMES["loss"]], wm["actor/final_loss"], f"{tag} final_loss")
    for k in ("actor/policy_loss", "actor/policy_loss_abs", "actor/ratio", "actor/ratio_abs", "actor/clipped_ratio",
              "actor/dual_cliped_ratio", "actor/approx_kl", "actor/clip_fraction", "actor/kl_loss"):
        _close(out[_lib.TOK_OUT_NAMES[k]], wm[k], f"{tag} {k}")
    mask = inp["loss_mask"]
    n_valid = float(lp.numel() if mask is None else int(mask.sum()))
    _same_count(out[_lib.TOK_OUT_NAMES["actor/clip_fraction"]], wm["actor/clip_fraction"], n_valid, f"{tag} clip_fraction")
    assert float(out[_lib.TOK_OUT_NAMES["actor/token_num"]]) == n_valid
    torch.testing.assert_close(lp.grad.cpu(), want["d_logprobs"], rtol=RTOL, atol=ATOL_GRAD, msg=lambda m: f"{tag} d_logprobs: {m}")
    on = mask if mask is not None else torch.ones_like(inp["logprobs"], dtype=torch.bool)
    cnt = on.sum(dim=1, keepdim=True).double()
    den = {"token-mean": torch.full_like(cnt, n_valid), "seq-mean-token-sum": torch.full_like(cnt, float(on.shape[0])),
           "seq-mean-token-mean": cnt * on.shape[0]}[case["agg"]]
    sel = flags["actor/ratio==1"][0]
    if case["kl"] == "k3":
        sel = sel & flags["kl/k3: lp==ref"][0]
    assert int((sel & on & (want["d_logprobs"] != 0)).sum()) >= 2
    got, total = lp.grad.cpu(), 0
    for r in range(on.shape[0]):  # one sequence = one denominator = one row weight
        row_sel = torch.zeros_like(sel)
        row_sel[r] = sel[r]
        w = float(torch.tensor(1.0 / float(den[r]), dtype=torch.float64).float())
        total += _exact_grad(got, want["d_logprobs"], float(den[r]), w, row_sel, f"{tag} d_logprobs on ratio == 1, sequence {r}")
    print(f"  {total} gradient entries compared bit for bit")
