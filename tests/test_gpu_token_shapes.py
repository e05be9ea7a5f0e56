"""The reasoning path's token kernels (token_ops.hip) at GRPO-step shapes, against float64 restatements (oracle/token_f64.py)
computed on the device from the same rounded inputs the kernels read.

The shapes are chosen so that every loop of every kernel runs more than once and every boundary of its data walk is hit:
  token_loss_rows_kernel      one 256-thread block per sequence            seq in {255, 256, 257, 1024, 1025, 3000, 4100}
  token_loss_finalize_kernel  one 256-thread block over the sequences      bsz in {255, 256, 257, 520}
  token_loss_bwd_kernel,      grid (bsz, ceil(seq / 1024) capped at 64)    seq 1025 / 3000 / 4100 (several y-blocks), 65537
  grpo_seq_adv_kernel                                                       (64 y-blocks, each striding twice, ragged last stripe)
  token_logprob_fwd/bwd       per row: unaligned head, full groups of 256 * 4 16-byte vectors (8192 bf16 / 4096 f32 elements),
                              leftover vectors, scalar tail                 V = 151936, row starts shifted so every head occurs;
                              a logit planted 20 above the rest of its row at each of those boundaries, so that an element
                              dropped or counted twice moves lse by O(1) instead of O(1/V)

Tolerances, each with its derivation next to the comparison:
  lse / log-prob / entropy   2e-5 absolute where |value| <= 32, the same number of f32 ulps (2e-5 / 2^-19 ~ 5) above that;
                             plus a bias bound on the mean signed error over all rows
  d_logits                   2e-5 relative + the rounding of the kernel's exponent argument (a few ulps of |lse|) times the
                             un-cancelled magnitude p * (|glp| + |gH| * (|x| + |H| + |lse|)); bf16 adds its rounding, 2^-8 of the value
  loss / metrics             1e-6 absolute + 1e-5 relative;  d_logprobs / d_entropy 1e-9 absolute + 2e-5 relative (the bounds of
                             tests/test_gpu_token_path.py against the f32 oracle, kept against f64)
  GRPO advantages            1e-6 absolute + 1e-5 relative

Budget on one MI355X: well under 90 s and 16 GB of device memory.  The largest cases carry "large" in their ids (-k large).
"""

import math

import numpy as np
import pytest
import torch

from oracle import token_f64 as T64
from rlinf_amd import token_ops
from rlinf_amd._lib import TOK_OUT_NAMES
from rlinf_amd.algorithms import registry
from rlinf_amd.utils import utils as UU

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 151936  # Qwen2.5 vocabulary
NT, UNROLL = 256, 4  # token_ops.hip: threads per row, 16-byte loads in flight per lane


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def assert_close(got, want, atol, rtol, what):
    """|got - want| <= atol + rtol * |want| elementwise (atol may be a tensor); NaN matches NaN, an infinity itself."""
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got == want) | (torch.isnan(got) & torch.isnan(want)) | ((got - want).abs() <= atol + rtol * want.abs())
    bad = ~ok
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} off; first at flat {i}: got {float(got.reshape(-1)[i])!r} "
                             f"want {float(want.reshape(-1)[i])!r}")


# ---- token log-prob / entropy / lse ----------------------------------------------------------------------------------------------
def logits_seen(x, temperature):
    """What the kernels read: x / T rounded to the logits' dtype.  f32: the correctly rounded quotient (torch's div).  bf16:
    bf16(f32(x) * f32(1 / T)) -- token_ops.hip's prep<bf16>, which differs from bf16(x / T) by one bf16 ulp on ~2^-15 of the
    elements (documented there); at 3e8 elements a planted peak would hit that, so the yardstick starts from the kernel's input."""
    if temperature == 1.0:
        return x.clone()
    if x.dtype == torch.float32:
        return x / temperature
    rt = float(np.float32(1.0) / np.float32(temperature))
    return (x.float() * rt).to(torch.bfloat16)


def row_geometry(ptr, esize):
    """token_logprob_fwd_kernel's split of a row that starts at byte address ptr -> (head, nfull, tail0, vec, group)."""
    vec = 16 // esize
    head = min(V, ((16 - ptr % 16) % 16) // esize)
    nvec = (V - head) // vec
    group = NT * UNROLL  # vectors per full group
    return head, nvec // group, head + nvec * vec, vec, group


def peak_positions(ptr, esize):
    """Every boundary of the row's walk: 0, the head's last element, the first vector, the first and last element of every full
    group, the first leftover vector (nfull * group), the last vector element, the scalar tail, V - 1."""
    head, nfull, tail0, vec, group = row_geometry(ptr, esize)
    pos = {0, head - 1, head, head + nfull * group * vec, head + nfull * group * vec + vec - 1, tail0 - 1, tail0, V - 1}
    for gi in range(nfull):
        pos.add(head + gi * group * vec)
        pos.add(head + (gi + 1) * group * vec - 1)
    return sorted(p for p in pos if 0 <= p < V)


def planted_rows(seed, n, dtype, scale):
    """n rows of V logits as a [n, 1, V] view into a [n, 1, V + 3] buffer (each row starts 3 elements after the previous one's
    slot, so heads of every residue occur), labels [n, 1].  8 of every 9 rows get one logit planted 20 above the row's maximum at
    a boundary of its walk: the rows of one head cycle through that head's list, with the label on the peak every other cycle.
    Labels also take the edges 0, V - 1 and -100."""
    g = gen(seed)
    buf = torch.empty(n, 1, V + 3, dtype=torch.float32, device=DEV)
    if scale == "llm":
        buf.uniform_(-30.0, 30.0, generator=g)  # LLM-like logit range
    else:
        buf.normal_(0.0, 3.0, generator=g)  # randn * 3
    buf = buf.to(dtype)
    x = buf[:, :, 1:V + 1]
    labels = torch.randint(0, V, (n, 1), device=DEV, generator=g)
    esize = x.element_size()
    rowmax = x.float().amax(-1)[:, 0].cpu()
    rows, cols, vals, heads = [], [], [], set()
    lab = labels[:, 0].cpu()
    nheads = 16 // esize  # the row start advances 3 elements a row: the head repeats every nheads rows
    for i in range(n):
        ptr = x.data_ptr() + i * x.stride(0) * esize
        heads.add(row_geometry(ptr, esize)[0])
        if i % 9 == 8:
            continue
        pos = peak_positions(ptr, esize)
        m = i // nheads
        p = pos[m % len(pos)]
        rows.append(i), cols.append(p), vals.append(float(rowmax[i]) + 20.0)
        if (m // len(pos)) % 2 == 0:
            lab[i] = p
    x[torch.tensor(rows, device=DEV), 0, torch.tensor(cols, device=DEV)] = torch.tensor(vals, device=DEV).to(dtype)
    lab[3::16] = 0
    lab[5::16] = V - 1
    lab[7::16] = -100
    labels = lab.to(DEV)[:, None]
    assert heads == set(range(nheads)), heads
    return x, labels


def lse_tol(ref):
    """2e-5 absolute for |value| <= 32 (the bound of tests/test_gpu_token_path.py at vocab <= 32003, about 5 f32 ulps there);
    beyond 32 the same number of ulps: the LLM-scale rows reach |lse| ~ 75 (x / 0.7 with a peak 20 above 30) and |log p| ~ 120,
    where one f32 ulp is 7.6e-6 and the final (r + log2 s) * ln 2 alone rounds twice."""
    return 2e-5 * torch.clamp(ref.abs() / 32.0, min=1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("temperature", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("scale", ["llm", "randn3"])
def test_logprob_fwd_planted_peaks(dtype, temperature, scale):
    n = 2048
    x, labels = planted_rows(11 + int(temperature * 10) + (0 if scale == "llm" else 100), n, dtype, scale)
    assert not x.is_contiguous()
    lp, ent, lse = token_ops.token_logprob_fwd(x, labels, temperature, with_entropy=True)
    xs = logits_seen(x, temperature)[:, 0]
    wlp, went, wlse = T64.logprob_entropy_lse(xs, labels[:, 0])
    lp, ent, lse = lp[:, 0], ent[:, 0], lse[:, 0]
    assert_close(lse, wlse, lse_tol(wlse), 0, "lse")
    assert_close(lp, wlp, lse_tol(wlp), 0, "logprob")
    # entropy: H = (log2 s - t / s) ln 2 with s, t summed in f32 over V / 256 terms per lane; |H| <= ln V = 11.9, the existing 2e-5
    assert_close(ent, went, 2e-5, 0, "entropy")
    # -100: the kernel writes -0.0, -cross_entropy(ignore_index) is -0.0 as well
    ign = labels[:, 0] == -100
    assert bool((lp[ign] == 0).all()) and bool(torch.signbit(lp[ign]).all()) and bool(torch.signbit(wlp[ign]).all())
    # bias: the per-element bounds above leave room for a systematic shift (a constant off in LOG2E / LN2, a rescale that is not
    # a power of two ...); the mean signed error over 2048 rows must stay a tenth of the smallest per-element bound
    for what, got, want in (("lse", lse, wlse), ("entropy", ent, went)):
        bias = float((got.double() - want).mean())
        assert abs(bias) < 2e-6, (what, bias)
    lp2, none, lse2 = token_ops.token_logprob_fwd(x, labels, temperature, with_entropy=False)
    assert none is None and torch.equal(lp2, lp[:, None]) and torch.equal(lse2[:, 0], lse)


def test_logprob_fwd_minus_inf_logits():
    """-inf logits (masked vocabulary entries) at the walk's boundaries: the reference's entropy_from_logits drops their p log p
    terms (finite entropy), -cross_entropy of a -inf label logit is -inf.  Pinned on both sides."""
    for dtype in (torch.float32, torch.bfloat16):
        n = 64
        x, labels = planted_rows(7, n, dtype, "llm")
        esize = x.element_size()
        lab = labels[:, 0].clone()
        for i in range(n):
            pos = peak_positions(x.data_ptr() + i * x.stride(0) * esize, esize)
            x[i, 0, torch.tensor(pos[1::2], device=DEV)] = float("-inf")
            x[i, 0, 1000 + 37 * i: 1000 + 37 * i + 500] = float("-inf")
            if i % 4 == 1:
                lab[i] = 1000 + 37 * i + 7
        labels = lab[:, None]
        lp, ent, lse = token_ops.token_logprob_fwd(x, labels, 1.0, with_entropy=True)
        wlp, went, wlse = T64.logprob_entropy_lse(x[:, 0], labels[:, 0])
        hit = torch.zeros(n, dtype=torch.bool, device=DEV)
        hit[1::4] = True
        assert bool(torch.isneginf(wlp[hit]).all()) and bool(torch.isneginf(lp[:, 0][hit]).all())
        assert bool(torch.isfinite(went).all()) and bool(torch.isfinite(ent).all())
        assert_close(ent[:, 0], went, 2e-5, 0, "entropy with -inf logits")
        assert_close(lse[:, 0], wlse, lse_tol(wlse), 0, "lse with -inf logits")
        assert_close(lp[:, 0][~hit], wlp[~hit], lse_tol(wlp[~hit]), 0, "logprob with -inf logits")


# ---- token log-prob backward -----------------------------------------------------------------------------------------------------
def grad_tol(xs, lse, ent, dlp, dent, want, temperature, dtype):
    """Per element: 2e-5 relative (tests/test_gpu_token_path.py's f32 bound) + the error of p itself times the un-cancelled size
    of the p-term.  p = exp2(fma(x, log2 e, -lse * log2 e)): the rounding of -lse * log2 e, of the fma and of lse itself
    (tolerated above at a few ulps of |lse|) enter p relatively; 2^-21 * (|x| + 2 |lse| + 4) covers them with a factor 4.
    The label entry glp * (1 - p) of a peaked row (p ~ 1 - 1e-9) and the entropy term's x + H - lse ~ 0 cancel, so this is the
    term that decides there.  bf16: the result is rounded once more to 8 significant bits, half an ulp = at most 2^-8 of the
    value."""
    p = torch.exp(xs - lse[:, None])
    a = p * (dlp.double().abs()[:, None] + dent.double().abs()[:, None] * (xs.abs() + ent.abs()[:, None] + lse.abs()[:, None]))
    tol = 1e-9 + 2e-5 * want.abs() + 2.0 ** -21 * (xs.abs() + 2 * lse.abs()[:, None] + 4) * a / temperature
    if dtype == torch.bfloat16:
        tol = tol + 2.0 ** -8 * want.abs()
    return tol


def upstream(n, seed, labels):
    """d_logprob / d_entropy that are not all ones: N(0, 1), zeros on -100 rows (the learner's masked tokens), a few rows with
    only one of the two."""
    g = gen(seed)
    dlp, dent = torch.randn(n, device=DEV, generator=g), torch.randn(n, device=DEV, generator=g)
    ign = labels == -100
    dlp[ign] = 0.0
    dent[ign] = 0.0
    dlp[1::32] = 0.0
    dent[2::32] = 0.0
    return dlp, dent


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("temperature", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
def test_logprob_bwd_planted_peaks(dtype, temperature, inplace):
    n = 2048
    x, labels = planted_rows(31 + int(temperature * 10), n, dtype, "llm")
    lab = labels[:, 0]
    lp, ent, lse = token_ops.token_logprob_fwd(x, labels, temperature, with_entropy=True)
    dlp, dent = upstream(n, 5, lab)
    xs = logits_seen(x, temperature)[:, 0]
    d = token_ops.token_logprob_bwd(x, labels, lse, ent, dlp[:, None], dent[:, None], temperature, out=x if inplace else None)
    assert d.dtype == dtype and d.shape == x.shape
    d = d[:, 0]
    chunk = 256
    for a in range(0, n, chunk):
        s = slice(a, a + chunk)
        want = T64.logits_grad_rows(xs[s], lab[s], dlp[s], dent[s], temperature)
        xs64 = xs[s].double()
        _, went, wlse = T64.logprob_entropy_lse(xs[s], lab[s])
        tol = grad_tol(xs64, wlse, went, dlp[s], dent[s], want, temperature, dtype)
        err = (d[s].double() - want).abs()
        bad = err > tol
        assert not bad.any(), (f"d_logits rows {a}..", int(bad.sum()), float((err / tol).max()))
    masked = (dlp == 0) & (dent == 0)
    assert int(masked.sum()) > 0 and float(d[masked].abs().max()) == 0.0  # masked rows: exact zeros, also in place


# ---- fused reasoning loss --------------------------------------------------------------------------------------------------------
LOSS_CASES = [
    # id, bsz, seq, agg, kl, entropy_bonus (None: no entropy), clip_ratio_c, clip_log_ratio_max, mask, fast_path
    ("b1-s4100", 1, 4100, "token-mean", None, 0.01, 3.0, 0.6, "ragged", True),
    ("b255-s3000", 255, 3000, "seq-mean-token-sum", "k1", 0.0, None, None, "prefix", True),
    ("b256-s1025", 256, 1025, "seq-mean-token-mean", "abs", 0.01, 3.0, None, "ragged", True),
    ("b257-s1025", 257, 1025, "token-mean", "k3", 0.02, 3.0, 0.6, "ragged", True),
    ("large-b520-s4100", 520, 4100, "seq-mean-token-mean", "k2", 0.01, 3.0, None, "prefix", True),
    ("b257-s1", 257, 1, "token-mean", "k1", None, 3.0, None, "prefix", True),
    ("b520-s255-row0off", 520, 255, "seq-mean-token-sum", "k3", 0.01, 3.0, 0.6, "row0", True),
    ("b256-s256-row0-nofast", 256, 256, "token-mean", None, 0.01, None, None, "row0", False),
    ("b255-s257", 255, 257, "seq-mean-token-sum", "abs", 0.0, None, 0.6, "ragged", True),
    ("b1-s1", 1, 1, "seq-mean-token-mean", "k2", 0.01, 3.0, None, "prefix", True),
    ("b520-s1024-row300off", 520, 1024, "seq-mean-token-mean", "k1", 0.01, 3.0, None, "row300", True),
    ("b256-s3000", 256, 3000, "token-mean", "k3", None, None, 0.6, "ragged", False),
]
RATIO_LO, RATIO_HI = 0.8, 1.28


def loss_inputs(seed, bsz, seq, mask_kind):
    g = gen(seed)
    old = -5.0 * torch.rand(bsz, seq, device=DEV, generator=g)
    lp = old + 0.4 * torch.randn(bsz, seq, device=DEV, generator=g)  # ratios ~ e^N(0, 0.4): every clip branch is taken
    adv = torch.randn(bsz, seq, device=DEV, generator=g)
    ent = 3.0 * torch.rand(bsz, seq, device=DEV, generator=g)
    ref = old + 0.2 * torch.randn(bsz, seq, device=DEV, generator=g)
    ref = ref + 25.0 * (torch.rand(bsz, seq, device=DEV, generator=g) < 0.05)  # some tokens beyond k3's +-20 clamp
    lens = torch.randint(1, seq + 1, (bsz,), device=DEV, generator=g)
    lens[::3] = seq
    mask = torch.arange(seq, device=DEV)[None, :] < lens[:, None]
    if mask_kind != "prefix":
        mask &= torch.rand(bsz, seq, device=DEV, generator=g) < 0.8
        mask[:, 0] |= mask_kind == "ragged"
    if mask_kind == "row0":
        mask[0] = False
    if mask_kind == "row300":
        mask[300] = False
    return lp, old, adv, ent, ref, mask


def near_kink(lp, old, ref, mask, clip_c, clip_max, kl):
    """Tokens whose f64 value lies within 2^-20 (16 f32 ulps) relative of a point where the loss's derivative jumps: the two
    ratio clips, the dual clip (ratio = clip_ratio_c), the log-ratio clamp, k3's +-20 / +-10 clamps.  The kernel decides those
    comparisons in f32 (ratio = expf(lp - old), bounds rounded to f32) and may take the other side."""
    d = 2.0 ** -20
    lr = lp - old
    if clip_max is not None:
        near = (lr - clip_max).abs() <= d * clip_max
        lr = lr.clamp(max=clip_max)
    else:
        near = torch.zeros_like(mask)
    r = lr.exp()
    for b in (RATIO_LO, RATIO_HI) + ((clip_c,) if clip_c is not None else ()):
        near |= (r - b).abs() <= d * b
    if kl == "k3":
        raw = lp - ref
        kld = raw.clamp(-20, 20).exp() - raw.clamp(-20, 20) - 1
        near |= ((raw.abs() - 20).abs() <= d * 20) | ((kld.abs() - 10).abs() <= d * 10 * 64)
    return near & mask


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_token_loss_vs_f64(case):
    cid, bsz, seq, agg, kl, bonus, clip_c, clip_max, mask_kind, fast = case
    lp0, old, adv, ent0, ref, mask = loss_inputs(100 + LOSS_CASES.index(case), bsz, seq, mask_kind)
    use_ent = bonus is not None
    beta = 0.1 if kl else 0.0
    # kernel, the way the learner calls it
    dlp = lp0.clone().requires_grad_(True)
    dent = ent0.clone().requires_grad_(True) if use_ent else None
    loss, metrics = registry.policy_loss(
        task_type="reasoning", loss_type="actor", loss_agg_func=UU.get_loss_agg_func(agg), logprobs=dlp, old_logprobs=old,
        advantages=adv, clip_ratio_c=clip_c, clip_ratio_low=0.2, clip_ratio_high=0.28, loss_mask=mask,
        clip_log_ratio_max=clip_max, fast_path_zero_loss_mask=fast, entropy=dent, entropy_bonus=bonus or 0.0,
        ref_logprobs=ref if kl else None, kl_beta=beta, kl_penalty_type=kl)
    (loss / 4).backward()
    out = metrics.device_vector.double()
    # f64 reference on the same f32 inputs
    lp64 = lp0.double().requires_grad_(True)
    ent64 = ent0.double().requires_grad_(True) if use_ent else None
    wloss, wm, went, wkl = T64.token_loss(lp64, old.double(), adv.double(), mask, loss_agg=agg, clip_ratio_low=0.2,
                                          clip_ratio_high=0.28, clip_ratio_c=clip_c, clip_log_ratio_max=clip_max,
                                          fast_path_zero_loss_mask=fast, entropy=ent64, entropy_bonus=bonus or 0.0,
                                          ref_logprobs=ref.double() if kl else None, kl_beta=beta, kl_penalty_type=kl)
    if wloss.requires_grad:
        (wloss / 4).backward()
    near = near_kink(lp0.double(), old.double(), ref.double(), mask, clip_c, clip_max, kl)
    n_near, n_on = int(near.sum()), int(mask.sum())
    # expected count: the ratio density near the clip bounds is ~1, the window 2 * 2^-20 per bound -> ~1e-5 of the tokens
    assert n_near <= 16 + 1e-5 * mask.numel(), (n_near, mask.numel())
    policy_on = not (fast and not bool(mask[0].any()))
    assert float(out[TOK_OUT_NAMES["policy_on"]]) == (1.0 if policy_on else 0.0)
    assert float(out[TOK_OUT_NAMES["actor/token_num"]]) == n_on
    # every slot of rlx_tok_out; a token that may flip a clip decision moves clip_fraction by 1 / n_on and the dual-clipped
    # ratio by up to clip_ratio_c / n_on (the loss itself is continuous there)
    flip = n_near / max(n_on, 1)
    for key, want, extra in (("loss", wloss, 0.0), ("actor/policy_loss", wm["actor/policy_loss"], 0.0),
                             ("actor/policy_loss_abs", wm["actor/policy_loss_abs"], 0.0), ("actor/ratio", wm["actor/ratio"], 0.0),
                             ("actor/ratio_abs", wm.get("actor/ratio_abs", torch.zeros(())), 0.0),
                             ("actor/clipped_ratio", wm["actor/clipped_ratio"], 0.0),
                             ("actor/dual_cliped_ratio", wm["actor/dual_cliped_ratio"], 3.0 * flip),
                             ("actor/approx_kl", wm["actor/approx_kl"], 0.0), ("actor/clip_fraction", wm["actor/clip_fraction"], flip),
                             ("actor/entropy_loss", went, 0.0), ("actor/kl_loss", wkl, 0.0)):
        assert_close(out[TOK_OUT_NAMES[key]], want.reshape(()), 1e-6 + extra, 1e-5, f"{cid} {key}")
    if not use_ent:
        assert float(out[TOK_OUT_NAMES["actor/entropy_loss"]]) == 0.0
    if agg == "seq-mean-token-mean" and mask_kind == "row300":
        # sequence 300 has no token: 0 / 0 in this aggregation, NaN on both sides; the other sequences' gradients are finite
        assert torch.isnan(loss) and torch.isnan(wloss)
        keep = torch.ones(bsz, dtype=torch.bool, device=DEV)
        keep[300] = False
    else:
        keep = torch.ones(bsz, dtype=torch.bool, device=DEV)
    zeros = torch.zeros_like(lp64)
    g_lp = lp64.grad if lp64.grad is not None else zeros
    ok = keep[:, None] & ~near
    assert_close(dlp.grad[ok], g_lp[ok], 1e-9, 2e-5, f"{cid} d_logprobs")
    if use_ent:
        g_ent = ent64.grad if ent64.grad is not None else zeros
        got = dent.grad if dent.grad is not None else torch.zeros_like(ent0)
        assert_close(got[keep], g_ent[keep], 1e-9, 2e-5, f"{cid} d_entropy")


# ---- GRPO advantages -------------------------------------------------------------------------------------------------------------
GRPO_CASES = [(512, 1023, 8), (512, 1024, 16), (256, 1025, 2), (64, 4100, 1), (512, 4100, 8), (96, 1024, 2),
              pytest.param(16, 65537, 16, id="large-16-65537-16"), (32, 65537, 2)]


@pytest.mark.parametrize("bsz,seq,group", GRPO_CASES)
def test_grpo_seq_adv_vs_f64(bsz, seq, group):
    g = gen(bsz * 7 + seq + group)
    rewards = torch.randn(bsz, device=DEV, generator=g)
    binary = torch.rand(bsz, device=DEV, generator=g) < 0.5
    rewards[: bsz // 2] = binary[: bsz // 2].float()  # half the groups with 0/1 correctness rewards
    if group > 1:
        # identical rewards in a group: std 0, advantage 0 / (0 + eps).  The values are exact in f32 sums (0, 1, -2.5): with a
        # reward like 0.3 the f32 group mean is not exactly 0.3 (for ~half of such values at group size 8), and the f32 reference
        # gives +-0.06..0.12 instead of 0 as well
        rewards[0:group] = 1.0
        rewards[group:2 * group] = 0.0
        rewards[bsz - group:] = -2.5
    lens = torch.randint(1, seq + 1, (bsz,), device=DEV, generator=g)
    lens[::5] = seq
    mask = torch.arange(seq, device=DEV)[None, :] < lens[:, None]
    mask[1::4] &= torch.rand(len(range(1, bsz, 4)), seq, device=DEV, generator=g) < 0.7
    mask[bsz // 2 + 1] = False  # an all-False row
    adv, ret = registry.calculate_adv_and_returns(task_type="reasoning", adv_type="grpo", rewards=rewards, loss_mask=mask,
                                                  group_size=group)
    assert ret is None and adv.shape == (bsz, seq)
    assert torch.equal(adv, token_ops.grpo_seq_adv(rewards, mask, group)) or group == 1
    want = T64.grpo_advantages(rewards, mask, group)
    if group == 1:
        # std of one element is NaN in the reference (torch's unbiased std), and NaN * 0 stays NaN: the whole tensor is NaN
        assert bool(torch.isnan(want).all()) and bool(torch.isnan(adv).all())
        return
    # group mean / std in sequential f32 sums of <= 16 terms: ~1e-6 relative on |adv| <= 4
    assert_close(adv, want, 1e-6, 1e-5, "advantages")
    assert float(adv[0:group].abs().max()) == 0.0 and float(adv[bsz - group:].abs().max()) == 0.0
    assert float(adv[bsz // 2 + 1].abs().max()) == 0.0


# ---- one micro-batch end to end at a configs[2]-like size ------------------------------------------------------------------------
def test_large_chain_logprobs_loss_backward_bf16():
    """8 x 1024 tokens x 151936 bf16 logits through token_logprobs (the autograd function) into the fused loss and .backward(),
    against the chain in f64: f64 log-probs / entropy of the same (scaled, bf16-rounded) logits, the f64 loss's gradient w.r.t.
    them, and the chunked f64 d_logits.  The old log-probs put every token's ratio at least 2e-3 away from a clip bound, so no
    clip decision depends on the kernel's ~1e-5 of log-prob error.  Tolerance: one bf16 ulp of each row's largest entry (the
    pattern of tests/test_gpu_token_path.py's bf16 backward test), every row."""
    bsz, seq, T = 8, 1024, 0.7
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    g = gen(99)
    x = torch.empty(bsz, seq, V, dtype=torch.bfloat16, device=DEV)
    for b in range(bsz):
        x[b] = (torch.rand(seq, V, device=DEV, generator=g) * 60.0 - 30.0).to(torch.bfloat16)
    labels = torch.randint(0, V, (bsz, seq), device=DEV, generator=g)
    labels[:, ::2] = x[:, ::2].argmax(-1)  # half the tokens are the mode, like sampled responses
    adv = torch.randn(bsz, seq, device=DEV, generator=g)
    mask = torch.rand(bsz, seq, device=DEV, generator=g) < 0.85
    xs = logits_seen(x, T).reshape(-1, V)
    lab = labels.reshape(-1)
    wlp, went, _ = T64.logprob_entropy_lse(xs, lab)
    lr = torch.rand(bsz * seq, device=DEV, generator=g).double() - 0.5
    for b in (math.log(RATIO_LO), math.log(RATIO_HI)):
        lr = torch.where((lr - b).abs() < 2e-3, lr + 4e-3, lr)
    old = (wlp - lr).float().reshape(bsz, seq)
    kw = dict(loss_agg_func=UU.get_loss_agg_func("token-mean"), clip_ratio_c=3.0, clip_ratio_low=0.2, clip_ratio_high=0.28,
              fast_path_zero_loss_mask=True, entropy_bonus=0.01)
    x.requires_grad_(True)
    lp, ent = token_ops.token_logprobs(x, labels, temperature=T, with_entropy=True)
    loss, _ = registry.policy_loss(task_type="reasoning", loss_type="actor", logprobs=lp, old_logprobs=old, advantages=adv,
                                   loss_mask=mask, entropy=ent, **kw)
    loss.backward()
    dx = x.grad.reshape(-1, V)
    assert dx.dtype == torch.bfloat16
    lp64 = wlp.reshape(bsz, seq).clone().requires_grad_(True)
    ent64 = went.reshape(bsz, seq).clone().requires_grad_(True)
    wloss, _, _, _ = T64.token_loss(lp64, old.double(), adv.double(), mask, loss_agg="token-mean", clip_ratio_low=0.2,
                                    clip_ratio_high=0.28, clip_ratio_c=3.0, fast_path_zero_loss_mask=True, entropy=ent64,
                                    entropy_bonus=0.01)
    wloss.backward()
    assert_close(loss, wloss, 1e-6, 1e-5, "loss")
    glp, gent = lp64.grad.reshape(-1), ent64.grad.reshape(-1)
    chunk = 256
    for a in range(0, bsz * seq, chunk):
        s = slice(a, a + chunk)
        want = T64.logits_grad_rows(xs[s], lab[s], glp[s], gent[s], T)
        ulp = want.abs().amax(-1, keepdim=True) * 2.0 ** -8
        err = (dx[s].double() - want).abs()
        row_ok = (err <= ulp + 1e-12).all(-1)
        assert bool(row_ok.all()), (f"rows {a}..", int((~row_ok).sum()), float((err / (ulp + 1e-12)).max()))
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    assert peak <= 16.0, f"the file's device-memory budget: {peak:.2f} GiB"  # the largest test of the file
