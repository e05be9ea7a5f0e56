"""On-policy distillation (OPD) on the device: the advantage launch and the loss forward / backward of csrc/opd.hip, reached
through this package's registries (get_adv_and_returns("opd"), get_policy_loss("opd")).

    expected   tests/golden/opd.pt (the reference's compute_opd_advantages / compute_opd_actor_loss, recorded by
               tools/make_opd_golden.py) and a float64 restatement below: the reference's elementwise f32 graph, every sum in f64
    got        the HIP callees on device tensors"""

import os

import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = torch.load(os.path.join(GOLDEN_DIR, "opd.pt"))


def _adv_fn():
    from rlinf_amd.algorithms import get_adv_and_returns
    return get_adv_and_returns("opd")


def _loss_fn():
    from rlinf_amd.algorithms import get_policy_loss
    return get_policy_loss("opd")


def f64_opd(lp, adv, mask, msum, max_episode_steps):
    """losses.py:427-505 restated: v = (-lp) * adv and v / ratio in f32 as the reference's graph forms them, the aggregation in
    float64; the gradient chain d loss / d lp in float64.  Returns (loss, opd_reward, opd_reverse_kl, grad) as f64 CPU."""
    lp, adv = lp.detach().cpu(), adv.detach().cpu()
    m = mask.cpu().expand_as(lp).double()
    n = lp.numel()
    cnt = m.sum()
    v = (-lp) * adv
    if max_episode_steps is not None:
        ratio = (msum.cpu().expand_as(lp) * 1.0) / max_episode_steps
        loss = ((v / ratio) * m.float()).double().sum() / n
        grad = -(adv.double() * m / ratio.double()) / n
    else:
        total = (v.double() * m).sum()
        loss = total / cnt if cnt > 0 else total
        grad = -(adv.double() * m) / (cnt if cnt > 0 else 1.0)
    rew = (adv.double() * m).sum()
    rew = rew / cnt if cnt > 0 else rew
    return loss, rew, -rew, grad


def rel(got, want) -> float:
    got, want = float(got), float(want)
    if want != want:
        return 0.0 if got != got else float("inf")
    if want == 0.0:
        return abs(got)
    return abs(got - want) / abs(want)


def norm_rel(got, want) -> float:
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    if not torch.isfinite(want).all():
        same = torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
        fin = torch.isfinite(want)
        return norm_rel(got[fin], want[fin]) if same else float("inf")
    den = float(want.norm())
    return float((got - want).norm()) / den if den > 0 else float(got.norm())


def run_loss(case, dev=DEV):
    x = case["logprobs"].to(dev).requires_grad_(True)
    loss, metrics = _loss_fn()(logprobs=x, advantages=case["advantages"].to(dev), loss_mask=case["loss_mask"].to(dev),
                               loss_mask_sum=case["loss_mask_sum"].to(dev), max_episode_steps=case["max_episode_steps"])
    loss.backward()
    return loss.detach(), dict(metrics), x.grad


# ---- advantages -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLD["adv"]))
def test_advantages_bit_equal_to_golden_and_torch(name):
    c = GOLD["adv"][name]
    adv, ret = _adv_fn()(prev_logprobs=c["prev"].to(DEV), teacher_logprobs=c["teacher"].to(DEV), loss_mask=c["loss_mask"].to(DEV),
                         num_action_chunks=c["num_action_chunks"])
    assert ret is None and adv.dtype == torch.float32 and adv.is_cuda
    assert torch.equal(adv.cpu(), c["advantages"])
    T = c["loss_mask"].shape[0]
    want = (c["teacher"].to(DEV).float() - c["prev"].to(DEV).float()).reshape(*c["prev"].shape[:-1], c["num_action_chunks"], -1)[:T]
    assert torch.equal(adv, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("extra", [0, 1])
def test_advantages_T_and_T_plus_1_read_in_place(dtype, extra):
    """LIBERO OPD shape: 30 chunk steps x 512 envs x (8 chunks x 7 dims); the T+1 input's rows are read where they lie."""
    from rlinf_amd import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    T, B, C, A = 30, 512, 8, 7
    prev = -torch.rand(T + extra, B, C * A, device=DEV, generator=g).to(dtype) * 5
    teacher = -torch.rand(T + extra, B, C * A, device=DEV, generator=g).to(dtype) * 5
    mask = torch.rand(T, B, C, device=DEV, generator=g) < 0.9
    adv, _ = _adv_fn()(prev_logprobs=prev, teacher_logprobs=teacher, loss_mask=mask, num_action_chunks=C)
    want = (teacher.float() - prev.float()).reshape(T + extra, B, C, A)[:T]
    assert adv.shape == (T, B, C, A) and torch.equal(adv, want)
    # a time-strided view (every other row of a larger buffer) and an odd row length (scalar path)
    big_t = -torch.rand(2 * (T + 1), B, C * A, device=DEV, generator=g).to(dtype)
    big_p = -torch.rand(2 * (T + 1), B, C * A, device=DEV, generator=g).to(dtype)
    out = ops.opd_advantages(big_t[::2], big_p[::2], C, T)
    assert torch.equal(out, (big_t[::2].float() - big_p[::2].float()).reshape(T + 1, B, C, A)[:T])
    odd_t, odd_p = teacher[:, : B - 1, : 3 * 5].contiguous(), prev[:, : B - 1, : 3 * 5].contiguous()  # 511 x 15 per row
    out = ops.opd_advantages(odd_t, odd_p, 3, None)
    assert torch.equal(out, (odd_t.float() - odd_p.float()).reshape(T + extra, B - 1, 3, 5))


# ---- loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLD["loss"]))
def test_loss_against_golden_and_float64(name):
    c = GOLD["loss"][name]
    loss, metrics, grad = run_loss(c)
    assert set(metrics) == {"actor/policy_loss", "actor/opd_reward", "actor/opd_reverse_kl"}
    f_loss, f_rew, f_kl, f_grad = f64_opd(c["logprobs"], c["advantages"], c["loss_mask"], c["loss_mask_sum"],
                                          c["max_episode_steps"])
    for got, gold, f64 in ((loss, c["loss"], f_loss), (metrics["actor/policy_loss"], c["metrics"]["actor/policy_loss"], f_loss),
                           (metrics["actor/opd_reward"], c["metrics"]["actor/opd_reward"], f_rew),
                           (metrics["actor/opd_reverse_kl"], c["metrics"]["actor/opd_reverse_kl"], f_kl)):
        assert rel(got, gold) <= 1e-6, (name, float(got), float(gold))
        assert rel(got, f64) <= 1e-6, (name, float(got), float(f64))
    assert norm_rel(grad, c["grad"]) <= 1e-6, name
    assert norm_rel(grad, f_grad) <= 1e-6, name


def test_zero_mask_sum_returns_what_the_reference_returns():
    """ratio = 0 where loss_mask_sum is 0: the reference's loss and those rows' gradients are NaN / inf; the metrics do not
    involve the ratio and stay finite."""
    c = GOLD["loss"]["ratio_zero_sum"]
    loss, metrics, grad = run_loss(c)
    assert torch.isnan(loss) and torch.isnan(c["loss"])
    assert torch.equal(torch.isnan(grad.cpu()), torch.isnan(c["grad"])) and torch.equal(torch.isinf(grad.cpu()), torch.isinf(c["grad"]))
    assert metrics["actor/opd_reward"] == pytest.approx(float(c["metrics"]["actor/opd_reward"]), rel=1e-6)


def test_all_false_mask_is_the_masked_sum():
    c = GOLD["loss"]["mean_all_false"]
    loss, metrics, grad = run_loss(c)
    assert float(loss) == 0.0 and metrics["actor/opd_reward"] == 0.0 and metrics["actor/opd_reverse_kl"] == 0.0
    assert float(grad.abs().max()) == 0.0


def _libero_inputs(seed, bsz=30 * 512, C=8, A=7, max_steps=240):
    g = torch.Generator(device=DEV).manual_seed(seed)
    lp = -torch.rand(bsz, C, A, device=DEV, generator=g) * 6
    adv = torch.randn(bsz, C, A, device=DEV, generator=g) * 0.5
    mask = torch.rand(bsz, C, device=DEV, generator=g) < 0.85
    msum = torch.randint(1, max_steps + 1, (bsz, C), device=DEV, generator=g)
    return lp, adv, mask, msum


@pytest.mark.parametrize("max_episode_steps", [None, 240])
@pytest.mark.parametrize("form", ["row", "full"])
def test_loss_at_the_libero_opd_shape(max_episode_steps, form):
    """rollout_epoch 8 x 64 envs = 512, 240 / 8 = 30 chunk steps, 8 chunks x 7 action dims."""
    lp, adv, mask, msum = _libero_inputs(11)
    m, s = mask.unsqueeze(-1), msum.unsqueeze(-1)
    if form == "full":
        m = torch.rand(lp.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) < 0.8
        s = s.expand(lp.shape).contiguous()
    c = dict(logprobs=lp, advantages=adv, loss_mask=m, loss_mask_sum=s, max_episode_steps=max_episode_steps)
    loss, metrics, grad = run_loss(c)
    f_loss, f_rew, f_kl, f_grad = f64_opd(lp, adv, m, s, max_episode_steps)
    assert rel(loss, f_loss) <= 1e-6 and rel(metrics["actor/opd_reward"], f_rew) <= 1e-6
    assert rel(metrics["actor/opd_reverse_kl"], f_kl) <= 1e-6
    assert norm_rel(grad, f_grad) <= 1e-6


def test_two_runs_are_bit_identical_and_a_graph_replay_matches_eager():
    from rlinf_amd import ops
    T, B, C, A = 30, 512, 8, 7
    g = torch.Generator(device=DEV).manual_seed(3)
    teacher = -torch.rand(T + 1, B, C * A, device=DEV, generator=g).to(torch.bfloat16) * 5
    prev = -torch.rand(T + 1, B, C * A, device=DEV, generator=g).to(torch.bfloat16) * 5
    lp = -torch.rand(T * B, C, A, device=DEV, generator=g) * 6
    mask = torch.rand(T * B, C, 1, device=DEV, generator=g) < 0.85
    msum = torch.randint(1, 241, (T * B, C, 1), device=DEV, generator=g)

    def step():
        adv = ops.opd_advantages(teacher, prev, C, T).reshape(T * B, C, A)
        x = lp.detach().requires_grad_(True)
        loss, out = ops.opd_loss(x, adv, mask, action_dim=A, loss_mask_sum=msum, max_episode_steps=240)
        (gx,) = torch.autograd.grad(loss, x)
        return [adv, loss.detach(), out, gx]

    a, b = step(), step()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(captured, a):
        assert torch.equal(u, v)


# ---- the reference's assert messages ------------------------------------------------------------------------------------
def test_reference_assert_messages_on_device_inputs():
    adv_fn, loss_fn = _adv_fn(), _loss_fn()
    p = torch.zeros(3, 2, 14, device=DEV)
    with pytest.raises(AssertionError, match="requires post-rollout teacher_logprobs"):
        adv_fn(prev_logprobs=p, teacher_logprobs=None, num_action_chunks=2)
    with pytest.raises(AssertionError, match="requires prev_logprobs from student rollout"):
        adv_fn(prev_logprobs=None, teacher_logprobs=p, num_action_chunks=2)
    with pytest.raises(AssertionError, match="must match prev_logprobs shape"):
        adv_fn(prev_logprobs=p, teacher_logprobs=p[:2], num_action_chunks=2)
    with pytest.raises(AssertionError, match="set normalize_advantages to False"):
        adv_fn(prev_logprobs=p, teacher_logprobs=p, normalize_advantages=True, num_action_chunks=2)
    with pytest.raises(AssertionError, match="requires num_action_chunks"):
        adv_fn(prev_logprobs=p, teacher_logprobs=p)
    with pytest.raises(AssertionError, match="OPD token count 14 must be divisible by num_action_chunks 3"):
        adv_fn(prev_logprobs=p, teacher_logprobs=p, num_action_chunks=3)
    with pytest.raises(AssertionError, match="time dimension 3 must match loss_mask time dimension 1"):
        adv_fn(prev_logprobs=p, teacher_logprobs=p, num_action_chunks=2, loss_mask=torch.ones(1, 2, 2, dtype=torch.bool, device=DEV))
    lp = torch.zeros(4, 2, 7, device=DEV)
    m, s = torch.ones(4, 2, 1, dtype=torch.bool, device=DEV), torch.ones(4, 2, 1, dtype=torch.int64, device=DEV)
    with pytest.raises(AssertionError, match="logprobs must be float32"):
        loss_fn(logprobs=lp.double(), advantages=lp, loss_mask=m, loss_mask_sum=s)
    with pytest.raises(AssertionError, match="advantages must be float32"):
        loss_fn(logprobs=lp, advantages=lp.half(), loss_mask=m, loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD advantages shape"):
        loss_fn(logprobs=lp, advantages=lp[..., :1], loss_mask=m, loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD actor loss requires loss_mask."):
        loss_fn(logprobs=lp, advantages=lp, loss_mask=None, loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD actor loss requires loss_mask_sum."):
        loss_fn(logprobs=lp, advantages=lp, loss_mask=m, loss_mask_sum=None)
    with pytest.raises(AssertionError, match="OPD loss_mask rank 1 must match logprobs rank 3"):
        loss_fn(logprobs=lp, advantages=lp, loss_mask=m[:, 0, 0], loss_mask_sum=s)
    with pytest.raises(AssertionError, match="except the token dimension"):
        loss_fn(logprobs=lp, advantages=lp, loss_mask=m[:, :1], loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD loss_mask_sum token dimension 3 must be 1"):
        loss_fn(logprobs=lp, advantages=lp, loss_mask=m, loss_mask_sum=s.expand(4, 2, 3))
