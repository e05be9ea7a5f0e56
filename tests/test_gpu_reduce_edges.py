"""The two-stage reduction of csrc/rlx_reduce.h at the edges of its second stage, and the loss kernels' vector loads.

Statistics: sizes that give one partial row, a row count that is no multiple of the folding block's 256 threads, and more
elements than the 1024-row cap covers in one trip.  The values are small integers, so every sum is exact in float64 in ANY
order and the comparison with torch on the CPU is exact equality.
Losses: the float4 load path of the classic and of the decoupled (proximal_logprobs given) kernel against the scalar path on
the same values -- the additions run in the same element order, so every output has the same bits.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 65_537, 262_147]
_cache = {}


def _ints(n):
    """(x float32 with integer values in [-8, 8], mask) on the CPU, the same for every test that asks for size n."""
    if n not in _cache:
        g = torch.Generator().manual_seed(n)
        x = torch.randint(-8, 9, (n,), generator=g).float()
        m = torch.rand(n, generator=g) < 0.6
        m[0] = True  # never an empty selection: min / max of nothing is the kernels' -inf, not a torch value
        _cache[n] = (x, m)
    return _cache[n]


def _want(x, m):
    """count, sum, sum of squares, min, max in float64; the integer sums prove that float64 held them exactly."""
    sel = x if m is None else x[m]
    d = sel.double()
    i = sel.long()
    assert float(d.sum()) == int(i.sum()) and float(d.square().sum()) == int((i * i).sum())
    return float(sel.numel()), float(d.sum()), float(d.square().sum()), float(d.min()), float(d.max())


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_masked_stats_exact_at_fold_edges(n, masked):
    from rlinf_amd import ops
    x, m = _ints(n)
    m = m if masked else None
    cnt, s, sq, _, _ = _want(x, m)
    got = ops.masked_stats(x.cuda(), None if m is None else m.cuda()).cpu()
    assert got.dtype == torch.float64
    assert got.tolist() == [cnt, s, sq]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_rollout_metrics_exact_at_fold_edges(n, masked):
    from rlinf_amd import ops
    x, m = _ints(n)
    m = m if masked else None
    cnt, s, _, lo, hi = _want(x, m)
    got = ops.rollout_metrics([x.cuda()], None if m is None else m.cuda()).cpu()
    assert got.dtype == torch.float64
    assert got[0].tolist() == [s, cnt, -lo, hi]  # the row is (sum, count, -min, max)


def _shifted(t):
    """The same values in a view that starts one float into a larger buffer: contiguous, but only 4-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("decoupled", [False, True])
def test_loss_vector_loads_match_scalar_loads(decoupled):
    """raw_per_adv / sub_per_adv = 8, n_adv = 300: 16-byte aligned logprobs / old_logprobs / proximal_logprobs take the float4
    path, views one float into a buffer the scalar path; out, g_logp and g_value must be the same bits."""
    from rlinf_amd import ops
    g = torch.Generator().manual_seed(31)
    n_adv, A = 300, 8
    lp = (torch.randn(n_adv, A, generator=g) * 0.3 - 1.0).cuda()
    old = (lp.cpu() + torch.randn(n_adv, A, generator=g) * 0.05).cuda()
    prox = (lp.cpu() + torch.randn(n_adv, A, generator=g) * 0.03).cuda()
    adv, v, ret = (torch.randn(n_adv, 1, generator=g).cuda() for _ in range(3))
    pv = (v.cpu() + torch.randn(n_adv, 1, generator=g) * 0.7).cuda()
    mask = (torch.rand(n_adv, 1, generator=g) < 0.7).cuda()

    def run(place):
        a, b, c = place(lp), place(old), place(prox)
        a.requires_grad_(True)
        loss, out = ops.ppo_loss(a, b, adv, logprob_type="action_level", action_dim=A, clip_ratio_low=0.2, clip_ratio_high=0.28,
                                 clip_ratio_c=3.0, values=v.clone().requires_grad_(True), prev_values=pv, returns=ret,
                                 value_clip=0.5, huber_delta=1.0, loss_mask=mask,
                                 decoupled=dict(proximal_logprobs=c, behave_weight_threshold=1.05) if decoupled else None)
        g_logp, g_value, _ = loss.grad_fn.saved_tensors  # what the forward kernel wrote for the backward
        return out.clone(), g_logp.clone(), g_value.clone()

    def aligned(t):
        t = t.clone()
        assert t.data_ptr() % 16 == 0
        return t

    vec = run(aligned)
    scalar = run(_shifted)
    for name, a, b in zip(("out", "g_logp", "g_value"), vec, scalar):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert bool(torch.isfinite(vec[0]).all()) and float(vec[1].abs().max()) > 0.0
