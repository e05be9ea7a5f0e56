"""The optimizer step (csrc/adamw_clip.hip) away from the MLP policy's own sizes: slab counts around the one-launch kernel's load
batches, sizes around every dispatch threshold, parameter groups that are not the policy's, the step's scalars, and a replayed graph.

Three forms hold the same arithmetic and are selected here by what the caller hands over:
  scalar      every buffer is a view one float into a larger allocation (data_ptr() % 16 == 4), or n % 4 != 0
  segment     16-byte aligned buffers, no sync words                    (grad_reduce_sqnorm + clip_adamw_seg_kernel)
  one launch  aligned buffers and ``ops.adamw_sync_words``              (reduce_clip_adamw_one_launch)
Which one ran is read from the sync words: word 0 (the exchange's epoch) advances by one per one-launch step and the whole buffer
stays zero when the library fell back; word 1 set means the exchange expired, which is a failure here.

References (all on the CPU):
  slab sum   the f32 loop acc = g[0]; acc = acc + g[k] in ascending k, then * grad_scale in f32: the documented order, bit-exact
  deferred   float64 sum_q scale[q] * (sum of group q's slabs) on the two ranges; allowance (per + groups + 2) * 2^-24 * sum |addend|
             (per - 1 adds inside a group, one multiply and one add per group that may contract, the grad_scale multiply)
  norm       float32(sqrt(float64 sum of squares of the f32 gradient)), 2^-23 relative (one rounding + one ulp)
  AdamW      torch.optim.AdamW in float64 on the float64 clipped gradient, one param group per range, with the bounds of
             test_clip_adamw_shapes: parameters t * (2^-21 |want| + 2^-14 lr), moments 2^-17 |want| + 2^-18 max |want|
             (t = steps this test applied)
  clipped g  4 * 2^-23 |want| where the clip is active: the coefficient is max_norm / (norm + 1e-6) in f32 from a norm that is
             within one ulp -- three roundings -- and the product one more
Between forms: bit-identical with the clip inactive; with it active the norm's last bit may differ (the header says so), so
4 * 2^-23 |ref| on gradient and moments and 4 * 2^-23 (|ref| + lr) on parameters against the segment form."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

U23, U24 = 2.0 ** -23, 2.0 ** -24
ONE_BLOCK = 2048            # parameters per block of the one-launch / segment kernels
ONE_LAUNCH_MAX = 512 * ONE_BLOCK
BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.01


def _ops():
    from rlinf_amd import ops
    return ops


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _slabs(n, nslab, seed):
    """[nslab, n] like test_clip_adamw_shapes: one base gradient, 0.5e-2 .. 1.5e-2 either sign, times a weight of its own per slab
    and element (a dropped, doubled or mis-strided slab moves the sum by ~1 / nslab); the LAST element carries a fifth of the norm."""
    g = torch.Generator().manual_seed(seed)
    base = (torch.rand(n, generator=g) + 0.5) * torch.where(torch.rand(n, generator=g) < 0.5, -1e-2, 1e-2)
    base[n - 1] = 0.05 + 0.005 * math.sqrt(n)
    return base.repeat(nslab, 1) * (torch.rand(nslab, n, generator=g) * 0.5 + 0.75)


def _state(n, seed):
    """Parameters and NON-ZERO moments of a size that keeps m / (sqrt(v) + eps) of order one."""
    g = torch.Generator().manual_seed(1000 + seed)
    p0 = torch.randn(n, generator=g) * 0.1
    m0 = torch.randn(n, generator=g) * 5e-3
    v0 = (torch.rand(n, generator=g) + 0.5) * 2.5e-5
    return p0, m0, v0


def _sum_f32(slabs, grad_scale=1.0):
    """The documented order in f32: ascending slabs, then the scale."""
    acc = slabs[0].clone()
    for k in range(1, slabs.shape[0]):
        acc = acc + slabs[k]
    return acc * torch.tensor(grad_scale, dtype=torch.float32)


def _clear_of_zero(g64):
    assert float(g64.abs().min()) >= 1e-3, "a summed gradient is within 1e-3 of zero: the inputs of this test are wrong"


def _scales(groups):
    return torch.tensor([(0.5, 0.25, 2.0, 1.5)[q % 4] * (1.0 + 0.125 * (q // 4)) for q in range(groups)])


def _deferred(groups, ranges):
    """A hand-built ``deferred`` dict (the keys of ops.deferred_actor_scale): the scales sit in column 1 of a [groups, 3] table."""
    rows = torch.zeros(groups, 3, device="cuda")
    rows[:, 1] = _scales(groups).cuda()
    return dict(scale=rows[0, 1:], stride=int(rows.stride(0)), groups=groups, ranges=list(ranges), keep=rows)


def _deferred_f64(slabs, groups, per, ranges, grad_scale):
    """float64 restatement of the deferred sum and its f32 allowance per element."""
    n = slabs.shape[1]
    inr = torch.zeros(n, dtype=torch.bool)
    for b, e in ranges:
        inr[b:e] = True
    s64 = slabs.double().view(groups, per, n)
    f = torch.where(inr[None, :], _scales(groups).double()[:, None], torch.ones((), dtype=torch.float64))
    g64 = (s64.sum(1) * f).sum(0) * grad_scale
    allow = (per + groups + 2) * U24 * (s64.abs() * f[:, None, :]).sum((0, 1)) * grad_scale
    return g64, allow


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def _reference(p0, m0, v0, g64, groups, step, *, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.5):
    """clip_grad_norm_ + the ``step``-th torch.optim.AdamW step in float64, one param group per non-empty range."""
    n = p0.numel()
    norm = float(g64.square().sum().sqrt())
    r = SimpleNamespace(norm=norm, applied=math.isfinite(norm), p=p0.double().clone(), m=m0.double().clone(), v=v0.double().clone(),
                        lr=torch.zeros(n, dtype=torch.float64), cov=torch.zeros(n, dtype=torch.bool))
    r.coef = min(1.0, max_grad_norm / (norm + 1e-6)) if (max_grad_norm and max_grad_norm > 0) else 1.0
    r.g = g64 * r.coef
    if not r.applied:
        return r
    live = [(b, e, lr) for b, e, lr in groups if e > b]
    for b, e, lr in live:
        r.lr[b:e], r.cov[b:e] = lr, True
    if not live:
        return r
    prm = [torch.nn.Parameter(r.p[b:e].clone()) for b, e, _ in live]
    opt = torch.optim.AdamW([{"params": [q], "lr": lr} for q, (_, _, lr) in zip(prm, live)], betas=betas, eps=eps,
                            weight_decay=weight_decay)
    for q, (b, e, _) in zip(prm, live):
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": r.m[b:e].clone(), "exp_avg_sq": r.v[b:e].clone()}
        q.grad = r.g[b:e].clone()
    opt.step()
    for q, (b, e, _) in zip(prm, live):
        r.p[b:e], r.m[b:e], r.v[b:e] = q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    return r


# ---- running one step in a chosen form ----------------------------------------------------------------------------------------
def _forms():
    """The three forms; without sync words (RLX_ADAMW_ONE_LAUNCH=0) the one-launch form does not exist and is left out."""
    return ("scalar", "segment") + (("one",) if _ops().adamw_sync_words(8, "cuda") is not None else ())


def _run(form, slabs, p0, m0, v0, groups, step, *, with_sync=None, step_state=None, **kw):
    """One ops.clip_adamw_step_ on device copies of the inputs.  form "scalar": misaligned views; "segment": aligned, no sync words;
    "one": aligned with sync words.  ``with_sync`` overrides whether sync words are passed (a misaligned one-launch request).
    Returns the results on the host; ``epoch`` is None without sync words, else the number of one-launch steps that ran."""
    ops = _ops()
    mis = form == "scalar"

    def place(t):
        buf = torch.empty(t.numel() + (1 if mis else 0), dtype=torch.float32, device="cuda")
        view = (buf[1:] if mis else buf).view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == (4 if mis else 0) or t.numel() == 0
        return view

    n = p0.numel()
    p, m, v, grads = place(p0), place(m0), place(v0), place(slabs)
    want_sync = (form == "one") if with_sync is None else with_sync
    sync = ops.adamw_sync_words(n, "cuda") if want_sync else None
    stats = torch.full((2,), -7.0, device="cuda")
    state = None if step_state is None else torch.tensor(step_state, dtype=torch.int32, device="cuda")
    ops.clip_adamw_step_(p, grads, m, v, groups, step, stats=stats, step_state=state, sync=sync, **kw)
    torch.cuda.synchronize()
    out = SimpleNamespace(form=form, p=p.cpu(), m=m.cpu(), v=v.cpu(), g=grads.reshape(-1)[:n].cpu(), stats=stats.cpu(), epoch=None,
                          state=None if state is None else state.cpu())
    if sync is not None:
        words = sync.cpu()
        assert int(words[1]) == 0, "the exchange expired (sticky word set): a workgroup of the one-launch step never became resident"
        out.epoch = int(words[0])
        assert out.epoch in (0, 1)
        if out.epoch == 0:
            assert not bool(words.any()), "the step fell back to two launches but touched the sync words"
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()), int((_bits(a) != _bits(b)).nonzero()[0]))


def _within(got, want, bar, what):
    err = (got.double() - want).abs()
    assert bool((err <= bar).all()), (what, float((err - bar).max()), int((err > bar).nonzero()[0]))


def _check(run, ref, inputs, *, grad="exact", g32=None, g_allow=None, norm_rel=U23, steps=1):
    """One form's results against the float64 reference.  grad: "exact" (clip inactive, plain slabs: the written-back gradient IS the
    f32 sum ``g32``), "clipped" (4 * 2^-23 |want|) or "allow" (the deferred sum's allowance ``g_allow``)."""
    p0, m0, v0 = inputs
    tag = run.form
    if not ref.applied:
        assert not math.isfinite(float(run.stats[0])) and float(run.stats[1]) == 0.0, (tag, run.stats)
        for got, was, nm in ((run.p, p0, "p"), (run.m, m0, "m"), (run.v, v0, "v")):
            _same_bits(got, was, f"{tag}: {nm} moved although the step was skipped")
        return
    want_norm = float(torch.tensor(ref.norm, dtype=torch.float64).float())
    assert abs(float(run.stats[0]) - want_norm) <= norm_rel * ref.norm, (tag, float(run.stats[0]), want_norm)
    assert float(run.stats[1]) == 1.0, (tag, run.stats)
    if grad == "exact":
        _same_bits(run.g, g32, f"{tag}: written-back gradient is not the ascending f32 slab sum")
    elif grad == "clipped":
        _within(run.g, ref.g, 4 * U23 * ref.g.abs(), f"{tag}: clipped gradient")
    else:
        _within(run.g, ref.g, g_allow, f"{tag}: deferred gradient")
    _within(run.p, ref.p, steps * (2.0 ** -21 * ref.p.abs() + 2.0 ** -14 * ref.lr) + 1e-30, f"{tag}: params")
    for got, want, nm in ((run.m, ref.m, "exp_avg"), (run.v, ref.v, "exp_avg_sq")):
        _within(got, want, 2.0 ** -17 * want.abs() + 2.0 ** -18 * float(want.abs().max()) + 1e-30, f"{tag}: {nm}")
    unc = ~ref.cov
    if bool(unc.any()):  # elements of no group: the bounds above would let them drift, the kernel must not touch them
        for got, was, nm in ((run.p, p0, "p"), (run.m, m0, "m"), (run.v, v0, "v")):
            _same_bits(got[unc], was[unc], f"{tag}: {nm} of an element that no group covers moved")


def _check_forms(runs, ref, *, clip_active):
    """The forms against each other (see the module docstring)."""
    if not ref.applied:
        return
    base = runs["segment"]
    for tag, r in runs.items():
        if tag == "segment":
            continue
        if not clip_active:
            for nm in ("p", "m", "v", "g"):
                _same_bits(getattr(r, nm), getattr(base, nm), f"{tag} vs segment, clip inactive: {nm}")
        else:
            for nm in ("m", "v", "g"):
                b = getattr(base, nm).double()
                _within(getattr(r, nm), b, 4 * U23 * b.abs(), f"{tag} vs segment: {nm}")
            b = base.p.double()
            _within(r.p, b, 4 * U23 * (b.abs() + ref.lr), f"{tag} vs segment: p")


def _three_forms(slabs, inputs, groups, step, *, need_one_launch, **kw):
    runs = {f: _run(f, slabs, *inputs, groups, step, **kw) for f in _forms()}
    if "one" in runs and need_one_launch:
        assert runs["one"].epoch == 1, "a plan of <= 128 blocks on an unmasked stream must take the one-launch form"
    return runs


# ---- 1. slab counts -----------------------------------------------------------------------------------------------------------
N_SLAB, N_SLAB_SCALAR = 8200, 8203  # 5 one-launch blocks, the last ragged; the second is scalar by n % 4
GROUPS_SLAB = lambda n: [(0, 1027, 3e-3), (1027, n, 1e-3)]  # noqa: E731


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("nslab", [1, 2, 9, 10, 11, 16, 24, 25, 26, 48, 49, 50])
def test_slab_counts(nslab, grad_scale):
    """Every slab count around the batches of sum_slabs_f4 (SB = 9: 10 | 11; SB = 24: 25 | 26, 49 | 50) in all three forms, with the
    clip inactive both ways (max_grad_norm = 0 with grad_scale 1, a max_norm nobody reaches with 0.5): the written-back gradient
    is the ascending f32 sum bit for bit, norm and AdamW follow it, the forms are bit-identical, and rlx_sum_slabs (plain, and as
    one deferred group of scale 1) gives the same bits."""
    ops = _ops()
    max_norm = 0.0 if grad_scale == 1.0 else 1e9
    kw = dict(betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=max_norm)
    for n in (N_SLAB, N_SLAB_SCALAR):
        slabs, inputs = _slabs(n, nslab, 7 * nslab), _state(n, nslab)
        plain = _sum_f32(slabs)
        g32 = _sum_f32(slabs, grad_scale)
        _clear_of_zero(g32.double())
        dev = slabs.cuda()
        _same_bits(ops.sum_slabs(dev).cpu(), plain, "rlx_sum_slabs")
        _same_bits(ops.sum_slabs(dev, deferred=dict(_deferred(1, [(3, n - 2), (5, 5)]), scale=torch.ones(1, device="cuda"))).cpu(),
                   plain, "rlx_sum_slabs_deferred, one group of scale 1")
        groups = GROUPS_SLAB(n)
        ref = _reference(*inputs, g32.double(), groups, 3, **kw)
        runs = _three_forms(slabs, inputs, groups, 3, need_one_launch=n % 4 == 0, grad_scale=grad_scale, **kw)
        if n % 4 != 0 and "one" in runs:
            assert runs["one"].epoch == 0, "n % 4 != 0 cannot be the one-launch form"
        for r in runs.values():
            _check(r, ref, inputs, grad="exact", g32=g32)
        _check_forms(runs, ref, clip_active=False)


@pytest.mark.parametrize("groups,per", [(1, 1), (2, 10), (2, 11), (4, 25), (3, 26), (25, 1)])
def test_slab_counts_deferred(groups, per):
    """Slab groups with device-side scales, two range sets: both ranges starting and ending inside a float4, and one empty range next
    to one that covers all but the ends.  rlx_sum_slabs_deferred and the gradient every form writes back against the float64
    restatement, within the f32 allowance; rlx_sum_slabs on the same slabs bit-exact; the norm within the same relative allowance
    (every addend of an element has one sign, so an element's relative error bounds the norm's) plus its own rounding; AdamW on
    the float64 gradient; segment, one-launch and scalar bit-identical (clip inactive).  At n = 8203 every request is the scalar
    form by n % 4, with the ranges reaching across what would be the float4 tail."""
    ops = _ops()
    nslab = groups * per
    grad_scale = 1.0 if nslab == 1 else 0.5
    kw = dict(betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=1e9)
    for n in (N_SLAB, N_SLAB_SCALAR):  # the second: scalar by n % 4, the ranges reach into what would be the float4 tail
        slabs, inputs = _slabs(n, nslab, 11 * nslab + groups), _state(n, nslab)
        _same_bits(ops.sum_slabs(slabs.cuda()).cpu(), _sum_f32(slabs), "rlx_sum_slabs")
        for ranges in ([(3, 1002), (2049, n - 2)], [(7, 7), (1, n - 1)]):
            g64, allow = _deferred_f64(slabs, groups, per, ranges, grad_scale)
            _clear_of_zero(g64)
            un64, un_allow = _deferred_f64(slabs, groups, per, ranges, 1.0)
            _within(ops.sum_slabs(slabs.cuda(), deferred=_deferred(groups, ranges)).cpu(), un64, un_allow, "rlx_sum_slabs_deferred")
            grp = GROUPS_SLAB(n)
            ref = _reference(*inputs, g64, grp, 3, **kw)
            runs = _three_forms(slabs, inputs, grp, 3, need_one_launch=n % 4 == 0, grad_scale=grad_scale,
                                deferred=_deferred(groups, ranges), **kw)
            if n % 4 != 0 and "one" in runs:
                assert runs["one"].epoch == 0, "n % 4 != 0 cannot be the one-launch form"
            for r in runs.values():
                _check(r, ref, inputs, grad="allow", g_allow=allow, norm_rel=(per + groups + 2) * U24 + U23)
            _check_forms(runs, ref, clip_active=False)


@pytest.mark.parametrize("nslab", [25, 26])
def test_non_finite_value_in_the_last_slab_skips_the_step(nslab):
    """An inf in the LAST slab only (the one a short batch or a wrong clamp would drop): non-finite norm, stats[1] == 0, parameters
    and moments bit-unchanged, no exception, in every form."""
    n = N_SLAB
    slabs, inputs = _slabs(n, nslab, 3 * nslab), _state(n, nslab)
    slabs[nslab - 1, n - 2] = float("inf")
    ref = _reference(*inputs, _sum_f32(slabs).double(), GROUPS_SLAB(n), 3)
    assert not ref.applied
    runs = _three_forms(slabs, inputs, GROUPS_SLAB(n), 3, need_one_launch=True, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.5)
    for r in runs.values():
        _check(r, ref, inputs)


# ---- 2. sizes -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_launch_runs_at(n):
    """Does a one-launch request of n parameters take the one-launch form on this device (its residency capacity decides)?"""
    slabs, inputs = _slabs(n, 1, 5), _state(n, 5)
    return _run("one", slabs, *inputs, [(0, n, 1e-3)], 1, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.1).epoch == 1


SIZES = [1, 3, 4, 5, 2047, 2048, 2052, 128 * ONE_BLOCK, 449 * ONE_BLOCK, 511 * ONE_BLOCK, ONE_LAUNCH_MAX, ONE_LAUNCH_MAX + 4,
         1_100_003, 1_100_004]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n, record_property):
    """Three slabs, the clip active, one step (the 7th) from non-zero moments, at every size where the host takes another path:
    below one float4, one and two one-launch blocks, 128 blocks (the largest plan that must be one launch), 449 (the first block
    whose slot is in the polling lanes' LAST group of 64), 511, 512 (= the exchange's slots) and past it, and past the 1024 norm
    partials of the two-launch kernels (grid-stride loops, partial 1023).  The form is asserted from the epoch word where the code
    fixes it and recorded where the device's residency capacity decides."""
    max_norm = 0.1
    kw = dict(betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=max_norm)
    slabs, inputs = _slabs(n, 3, n % 1009), _state(n, n % 1013)
    g32 = _sum_f32(slabs)
    _clear_of_zero(g32.double())
    cut = min(n, 1000)
    groups = [(0, cut, 3e-3), (cut, n, 1e-3)]
    ref = _reference(*inputs, g32.double(), groups, 7, **kw)
    assert ref.norm > max_norm, "the clip is meant to be active"
    runs = {f: _run(f, slabs, *inputs, groups, 7, **kw) for f in _forms()}
    if "one" in runs:
        runs["scalar+sync"] = _run("scalar", slabs, *inputs, groups, 7, with_sync=True, **kw)
        assert runs["scalar+sync"].epoch == 0, "misaligned buffers cannot be the one-launch form"
        epoch = runs["one"].epoch
        record_property("one_launch_form_ran", bool(epoch))
        if n % 4 != 0 or n > ONE_LAUNCH_MAX:
            assert epoch == 0, "one launch is impossible for n % 4 != 0 and for more than 512 blocks"
        elif n <= 128 * ONE_BLOCK:
            assert epoch == 1, "a plan of <= 128 blocks on an unmasked stream must take the one-launch form"
        elif epoch == 1:  # the capacity holds this plan: then it holds every smaller one
            for smaller in (s for s in SIZES if 128 * ONE_BLOCK < s < n):
                assert _one_launch_runs_at(smaller), f"one launch at {n // ONE_BLOCK} blocks but not at {smaller // ONE_BLOCK}"
    for r in runs.values():
        _check(r, ref, inputs, grad="clipped")
    _check_forms(runs, ref, clip_active=True)


# ---- 3. groups ----------------------------------------------------------------------------------------------------------------
N_GROUPS = 4104  # two full one-launch blocks and two float4 of a third
GROUP_SETS = {
    # boundaries on every residue mod 4; one-element groups at 4i + 1 and 4i + 2; an empty group; a learning rate each
    "a_every_residue": [(0, 5), (5, 6), (6, 6), (6, 1030), (1030, 1031), (1031, 2051), (2051, N_GROUPS)],
    "b_eight_groups": [(0, 5), (5, 6), (6, 6), (6, 1030), (1030, 1031), (1031, 2051), (2051, 3000), (3000, N_GROUPS)],
    "c_no_group": [],
    "d_gaps": [(3, 1001), (1500, 2049), (3001, 4100)],
    # groups strictly inside a float4 whose first and last element no group covers
    "e_inside_one_float4": [(401, 403), (2402, 2403), (3000, 3500), (4101, 4102)],
}


@pytest.mark.parametrize("case", sorted(GROUP_SETS))
def test_groups(case):
    """Parameter groups that are not the policy's, the clip active, in all three forms against the float64 reference: covered
    elements take their own group's learning rate, elements of no group keep parameter and moments bit for bit while their
    gradient is clipped, and with no group at all only gradient and stats are written.

    (e) was wrong in the float4 forms before this test: update_values_f4 took "first and last element resolve to the same group"
    to decide the middle two, also when both resolved to NO group, so a one- or two-element group strictly inside a float4 was
    skipped while the scalar form applied it.  The kernel now looks the middle elements up unless both ends are in one group."""
    n = N_GROUPS
    groups = [(b, e, 1e-3 * (k + 1)) for k, (b, e) in enumerate(GROUP_SETS[case])]
    kw = dict(betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.5)
    slabs, inputs = _slabs(n, 3, 41), _state(n, 41)
    g32 = _sum_f32(slabs)
    _clear_of_zero(g32.double())
    ref = _reference(*inputs, g32.double(), groups, 5, **kw)
    assert ref.norm > 0.5, "the clip is meant to be active"
    assert int(ref.cov.sum()) == sum(e - b for b, e in GROUP_SETS[case])
    runs = _three_forms(slabs, inputs, groups, 5, need_one_launch=True, **kw)
    for r in runs.values():
        _check(r, ref, inputs, grad="clipped")
        if ref.cov.any():
            assert not torch.equal(r.p[ref.cov], inputs[0][ref.cov])
    _check_forms(runs, ref, clip_active=True)


def test_nine_groups_are_refused():
    ops = _ops()
    n = N_GROUPS
    t = torch.zeros(n, device="cuda")
    groups = [(k * 100, (k + 1) * 100, 1e-3) for k in range(9)]
    with pytest.raises(ops.RlxError):
        ops.clip_adamw_step_(t, torch.ones(n, device="cuda"), t.clone(), t.clone(), groups, 1)
    assert not bool(t.any())


def test_empty_gradient_for_live_parameters_is_refused():
    """n > 0 parameters with an EMPTY gradient tensor (0 % n == 0): refused by the wrapper, nothing is launched on a buffer that
    does not hold n floats."""
    ops = _ops()
    n = N_GROUPS
    t = torch.zeros(n, device="cuda")
    stats = torch.full((2,), -7.0, device="cuda")
    with pytest.raises(ops.RlxError):
        ops.clip_adamw_step_(t, torch.ones(n, device="cuda")[:0], t.clone(), t.clone(), [(0, n, 1e-3)], 1, stats=stats)
    torch.cuda.synchronize()
    assert not bool(t.any()) and stats.tolist() == [-7.0, -7.0]


def test_overlapping_groups_are_refused():
    """Non-empty ranges that overlap are refused on the host (the float4 forms rely on disjoint ranges); an EMPTY range inside
    another one is not an overlap."""
    ops = _ops()
    n = N_GROUPS
    t = torch.zeros(n, device="cuda")
    stats = torch.full((2,), -7.0, device="cuda")
    for groups in ([(0, 100, 1e-3), (99, 200, 2e-3)], [(0, n, 1e-3), (401, 403, 2e-3)]):
        with pytest.raises(ops.RlxError, match="overlap"):
            ops.clip_adamw_step_(t, torch.ones(n, device="cuda"), t.clone(), t.clone(), groups, 1, stats=stats)
    torch.cuda.synchronize()
    assert not bool(t.any()) and stats.tolist() == [-7.0, -7.0]
    out = ops.clip_adamw_step_(t, torch.ones(n, device="cuda"), t.clone(), t.clone(), [(0, n, 1e-3), (50, 50, 2e-3)], 1, stats=stats)
    assert float(out[1]) == 1.0


# ---- 4. scalars ---------------------------------------------------------------------------------------------------------------
N_SCALARS = 4096


def _two_forms(slabs, inputs, groups, step, **kw):
    runs = {f: _run(f, slabs, *inputs, groups, step, **kw) for f in _forms() if f != "scalar"}
    if "one" in runs:
        assert runs["one"].epoch == 1
    return runs


@pytest.mark.parametrize("on_device", [False, True], ids=["host_step", "step_state"])
@pytest.mark.parametrize("step", [1, 2, 3, 1000, 65_536, 1_000_003])
def test_scalars(step, on_device):
    """The step's scalars over betas x weight_decay x eps x max_grad_norm at step counts from the first to far past where beta ** step
    underflows, the count given on the host or read from a device step_state of {step - 1, 0} (the host field then holds a wrong
    value on purpose): one slab, segment and one-launch forms, non-zero moments.  max_grad_norm 0 and 1e9 leave the gradient
    bit-exact (coefficient exactly 1); 0.5 clips."""
    n = N_SCALARS
    slabs, inputs = _slabs(n, 1, 23), _state(n, 23)
    g32 = _sum_f32(slabs)
    _clear_of_zero(g32.double())
    groups = [(0, 1001, 3e-3), (1001, n, 1e-3)]
    for betas in ((0.9, 0.999), (0.0, 0.5), (0.99, 0.9999)):
        for wd in (0.0, 0.1):
            for eps in (1e-8, 1e-3):
                for max_norm in (0.0, 1e9, 0.5):
                    kw = dict(betas=betas, eps=eps, weight_decay=wd, max_grad_norm=max_norm)
                    ref = _reference(*inputs, g32.double(), groups, step, **kw)
                    active = max_norm == 0.5
                    assert (ref.coef < 1.0) == active
                    runs = _two_forms(slabs, inputs, groups, 123 if on_device else step,
                                      step_state=[step - 1, 0] if on_device else None, **kw)
                    for r in runs.values():
                        _check(r, ref, inputs, grad="clipped" if active else "exact", g32=g32)
                        if on_device:
                            assert int(r.state[0]) + int(r.state[1]) == step, (r.form, r.state)
                    _check_forms(runs, ref, clip_active=active)


@pytest.mark.parametrize("max_norm", [0.0, 0.5])
def test_all_zero_gradient(max_norm):
    """Norm 0: the coefficient is min(max_norm / 1e-6, 1) = 1, the step is applied and nothing is NaN.  From zero moments only the
    decay moves the parameters -- p * float32(1 - lr * wd) bit for bit; from non-zero moments the float64 reference holds."""
    n = N_SCALARS
    slabs = torch.zeros(1, n)
    groups = [(0, 1001, 3e-3), (1001, n, 1e-3)]
    kw = dict(betas=BETAS, eps=EPS, weight_decay=0.1, max_grad_norm=max_norm)
    p0, m0, v0 = _state(n, 29)
    zero = torch.zeros(n)
    for inputs in ((p0, zero, zero), (p0, m0, v0)):
        ref = _reference(*inputs, torch.zeros(n, dtype=torch.float64), groups, 4, **kw)
        runs = _two_forms(slabs, inputs, groups, 4, **kw)
        for r in runs.values():
            assert float(r.stats[0]) == 0.0 and float(r.stats[1]) == 1.0
            for t in (r.p, r.m, r.v, r.g):
                assert bool(torch.isfinite(t).all())
            _check(r, ref, inputs, grad="exact", g32=zero)
            if inputs[1] is zero:
                decay = torch.cat([torch.full((e - b,), 1.0 - lr * 0.1, dtype=torch.float64).float() for b, e, lr in groups])
                _same_bits(r.p, p0 * decay, f"{r.form}: only the decay may move a parameter")
                assert not bool(r.m.any()) and not bool(r.v.any())
        _check_forms(runs, ref, clip_active=False)


def test_no_parameters_is_no_launch():
    """n = 0 returns before anything is launched: stats and sync words keep what they held."""
    ops = _ops()
    z = [torch.empty(0, device="cuda") for _ in range(4)]
    stats = torch.full((2,), -7.0, device="cuda")
    sync = ops.adamw_sync_words(0, "cuda")
    out = ops.clip_adamw_step_(z[0], z[1], z[2], z[3], [], 1, stats=stats, sync=sync)
    torch.cuda.synchronize()
    assert out is stats and stats.tolist() == [-7.0, -7.0]
    assert sync is None or not bool(sync.any())


# ---- 5. replay ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["segment", "one"])
def test_replayed_graph_equals_eager_steps(form):
    """25 plain slabs (one more than the first batch of the SB = 24 kernel) through PreparedAdamw: a hipGraph of 4 steps captured on a
    side stream and replayed 5 times with the slabs rewritten between replays, against the same 20 steps launched eagerly in the
    same form -- bit for bit, with the device step counter at 20 and, in the one-launch form, the epoch at 20 and no expiry.
    (Inside a replay the steps after the first read slab 0 as the previous step left it: the clipped sum.  Both runs do.)"""
    ops = _ops()
    n, nslab = N_SLAB, 25
    if form == "one" and ops.adamw_sync_words(n, "cuda") is None:
        pytest.skip("RLX_ADAMW_ONE_LAUNCH=0")
    p0, m0, v0 = _state(n, 31)
    fresh = [_slabs(n, nslab, 50 + r).cuda() for r in range(5)]
    results = []
    for replayed in (False, True):
        p, m, v = p0.cuda(), m0.cuda(), v0.cuda()
        grads = torch.zeros(nslab, n, device="cuda")
        stats, state = torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        ws = torch.empty(ops._lib.load().rlx_adamw_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        sync = ops.adamw_sync_words(n, "cuda") if form == "one" else None
        step = ops.PreparedAdamw(p, grads, m, v, GROUPS_SLAB(n), betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=0.5,
                                 grad_scale=0.5, stats=stats, step_state=state, workspace=ws, sync=sync)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if replayed:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    for _ in range(4):
                        step(side.cuda_stream)
            for r in range(5):
                grads.copy_(fresh[r])
                if replayed:
                    graph.replay()
                else:
                    for _ in range(4):
                        step(side.cuda_stream)
        side.synchronize()
        torch.cuda.synchronize()
        assert int(state[0]) + int(state[1]) == 20 and float(stats[1]) == 1.0, (replayed, state, stats)
        if sync is not None:
            assert int(sync[1]) == 0, "the exchange expired (sticky word set)"
            assert int(sync[0]) == 20, "a step of the one-launch request fell back to two launches"
        results.append([t.cpu() for t in (p, m, v, grads[0], stats)])
    assert not torch.equal(results[0][0], p0)
    for a, b, nm in zip(results[0], results[1], ("p", "m", "v", "g", "stats")):
        _same_bits(b, a, f"replayed vs eager: {nm}")
