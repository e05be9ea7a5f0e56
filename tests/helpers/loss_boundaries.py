"""Boundary inputs for the PPO loss kernels: one table, shared by the GPU test, the host test against the reference and the
table's own CPU test.

Every quantity is a dyadic rational (a multiple of 2**-6, magnitude <= 8), so every subtraction and every sum over the action
dimension is exact in f32 in any order: an element placed on a comparison of the kernel (``lp == old``, ``diff == value_clip``,
``|e| == huber_delta`` ...) sits on it bit for bit on the host and on the device.  The only transcendental evaluated ON a boundary
is exp(0) == 1.  Every other element keeps ``MARGIN`` from every comparison the kernel makes, measured in float64 by
``classify`` -- device expf and host expf differ in the last place, which is seven orders of magnitude less.

``cases()`` lists the parameter sets, ``build(case)`` the raw tensors the loss entries take, ``classify(case, inp)`` which elements
sit on which named boundary (and asserts the margin), ``run_oracle(case, inp)`` the expected loss / metrics / gradients from the
oracle's torch-autograd restatements in f32 (a tie is a property of f32 equality).
"""

from __future__ import annotations

import itertools
import math

import torch

from oracle import ppo_oracle as O
from oracle import token_oracle as TO

Q = 2.0 ** -6       # the grid every input lies on
MARGIN = 2.0 ** -6  # distance an element that is not ON a comparison keeps from it (log-ratio / value units)
N_ADV = 603         # two 256-thread blocks and a ragged tail of 91
UPSTREAM = 0.5      # (loss * 0.5).backward()

# one actor atom = (log-ratio against the policy the clip is taken against, advantage, mask bit)
_LR = (0.0, 0.0625, -0.0625, 0.125, -0.125, 0.5, -0.5, 1.5)
_ADV = (1.5, -0.75, 0.0, -0.0)
_FILL_LR, _FILL_ADV = 0.125, 1.0
_VERSIONS = (5.0, 4.0, -1.0, 3.0)  # current_version = 5: current, current - 1, unknown (-1), and alpha = 1/2
_OFFSETS = (0.0, 0.5, -0.25)       # proximal - behaviour log-prob ("given" proximal policy): weight 1, 1.65, 0.78
CURRENT_VERSION = 5
VALUE_CLIP = 0.5
_DELTAS = (1.0, 0.25, 0.125)       # above, equal to and below the |e| = 0.25 of the symmetric Huber tie
KL_BETA = 0.25

_CLIP_VARIANTS = {
    "clip": dict(clip_ratio_low=0.2, clip_ratio_high=0.2),
    "low0": dict(clip_ratio_low=0.0, clip_ratio_high=0.2),
    "high0": dict(clip_ratio_low=0.2, clip_ratio_high=0.0),
    "both0": dict(clip_ratio_low=0.0, clip_ratio_high=0.0),
    "logmin": dict(clip_ratio_low=0.2, clip_ratio_high=0.2, clip_log_ratio_min=-0.0625),
    "logmax": dict(clip_ratio_low=0.2, clip_ratio_high=0.2, clip_log_ratio_max=0.0625),
    "log00": dict(clip_ratio_low=0.2, clip_ratio_high=0.2, clip_log_ratio_min=0.0, clip_log_ratio_max=0.0),
}
_NO_LOG = ("clip", "low0", "high0", "both0")  # the decoupled loss has no log-ratio clamp


def _critic_atoms(delta: float):
    """(prev_value, value, return) rows for value_clip = 0.5 and this huber_delta."""
    d = delta
    return [
        (0.5, 0.5, 0.875),     # v == pv (on-policy)
        (0.25, 0.75, 1.125),   # v - pv == +value_clip
        (0.25, -0.25, -0.625), # v - pv == -value_clip
        (0.875, 1.0, 1.0 + d), # |ret - v| == delta, v inside the clip (both signs)
        (0.875, 1.0, 1.0 - d),
        (0.0, 1.0, 1.0 + d),   # |ret - v| == delta, v outside the clip
        (0.0, 1.0, 0.5 + d),   # |ret - vclip| == delta (both signs)
        (0.0, 1.0, 0.5 - d),
        (0.875, 1.0, 1.0),     # ret == v, inside / outside the clip
        (0.0, 1.0, 1.0),
        (0.0, 1.0, 0.75),      # e1 = -0.25, e2 = +0.25: equal Huber values, v outside the clip -> half the gradient
        (0.0, -1.0, -0.75),    # the same tie with the signs exchanged
        (0.0, 0.25, 2.25),     # filler
    ]


# --------------------------------------------------------------------------------------------------------------------------
def cases():
    """Every parameter set, as dicts: id, family ('ppo' | 'decoupled' | 'token'), group (the product it comes from), loss (keyword
    arguments of the loss), geometry.

    The axes a group names are crossed in full.  What cycles underneath them is picked by ``_cyc`` from a weighted sum of the
    axis indices, each cycler with weights of its own, chosen so that no cycler follows a single axis or another cycler
    (tests/test_loss_boundaries_table.py asserts it: within a group, under every value of one attribute every other attribute
    still takes at least two values)."""
    out = []

    def add(family, group, name, loss, **geom):
        out.append(dict(id=f"{family}-{name}", family=family, group=group, loss=loss, **geom))

    def _cyc(options, idx, weights):
        return options[sum(i * w for i, w in zip(idx, weights)) % len(options)]

    def axes(*lists):
        return itertools.product(*(list(enumerate(x)) for x in lists))

    # classic actor and actor-critic entries: every clip variant x dual clip x critic warm-up x (actor only | actor-critic) at
    # the VEC4 geometry; the mask and the Huber delta cycle
    for (a, cv), (b, c), (w, warm), (h, crit) in axes(_CLIP_VARIANTS, (None, 3.0), (False, True), (False, True)):
        idx = (a, b, w, h)
        loss = dict(_CLIP_VARIANTS[cv], clip_ratio_c=c, critic_warmup=warm, value_clip=VALUE_CLIP,
                    huber_delta=_cyc(_DELTAS, idx, (1, 1, 2, 0)))
        add("ppo", "grid", f"{cv}-c{c}-warm{int(warm)}-{'ac' if crit else 'a'}", loss, logprob_type="action_level", action_dim=4,
            chunks=3, mask_mode=_cyc(("mask", "none"), idx, (1, 1, 1, 1)), has_critic=crit, offset=False)
    # every geometry: the three log-prob levels x VEC4 and scalar forms x the three aggregations
    for (l, lt), (a, A), (m, mm) in axes(("action_level", "token_level", "chunk_level"), (4, 3), ("none", "mask", "ratio")):
        idx = (l, a, m)
        cv = _cyc(("clip", "both0", "low0", "log00", "high0"), idx, (4, 3, 4))
        loss = dict(_CLIP_VARIANTS[cv], clip_ratio_c=_cyc((3.0, None), idx, (0, 1, 1)), critic_warmup=False,
                    value_clip=VALUE_CLIP, huber_delta=_cyc(_DELTAS, idx, (2, 2, 1)))
        add("ppo", "geom", f"{lt}-A{A}-{mm}-{cv}", loss, logprob_type=lt, action_dim=A, chunks=2 if lt == "chunk_level" else 3,
            mask_mode=mm, has_critic=True, offset=False)
    # a log-prob buffer that starts 4 bytes into its allocation
    for i, cv in enumerate(("clip", "both0", "logmin")):
        loss = dict(_CLIP_VARIANTS[cv], clip_ratio_c=3.0, critic_warmup=False, value_clip=VALUE_CLIP, huber_delta=_DELTAS[i])
        add("ppo", "offset", f"offset-{cv}", loss, logprob_type="action_level", action_dim=4, chunks=3, mask_mode="mask",
            has_critic=True, offset=True)
    # decoupled actor-critic: proximal mode x log-prob level x threshold; clip variant, dual clip, warm-up, delta, action_dim and
    # aggregation cycle
    for (p, pm), (l, lt), (t, thr) in axes(("given", "old", "versions"), ("action_level", "token_level", "chunk_level"),
                                           (None, 1.0)):
        idx = (p, l, t)
        cv = _cyc(_NO_LOG, idx, (3, 2, 3))
        loss = dict(_CLIP_VARIANTS[cv], clip_ratio_c=_cyc((3.0, None), idx, (1, 1, 0)),
                    critic_warmup=_cyc((False, False, True), idx, (1, 2, 2)), value_clip=VALUE_CLIP,
                    huber_delta=_cyc(_DELTAS, idx, (1, 1, 2)))
        add("decoupled", "decoupled", f"{pm}-{lt}-thr{thr}-{cv}", loss, logprob_type=lt, action_dim=_cyc((4, 3), idx, (0, 1, 1)),
            chunks=2 if lt == "chunk_level" else 3, mask_mode=_cyc(("mask", "none", "ratio"), idx, (1, 1, 1)), has_critic=True,
            offset=False, prox_mode=pm, threshold=thr)
    # reasoning loss on [bsz, seq] tokens: aggregation x clip variant; dual clip, the KL kinds and the mask cycle
    for (g, agg), (a, cv) in axes(("token-mean", "seq-mean-token-sum", "seq-mean-token-mean"), _CLIP_VARIANTS):
        idx = (g, a)
        kl = _cyc(("k1", "abs", "k2", "k3", None), idx, (2, 1))
        loss = dict(_CLIP_VARIANTS[cv], clip_ratio_c=_cyc((None, 3.0), idx, (1, 1)))
        add("token", "token", f"{agg}-{cv}-kl{kl}", loss, agg=agg, kl=kl, mask_mode=_cyc(("mask", "mask", "none"), idx, (1, 1)))
    return out


def case_attributes(case: dict) -> dict:
    """The attributes of a case that vary within its group, flat: what tests/test_loss_boundaries_table.py checks for aliasing."""
    at = {k: case[k] for k in ("logprob_type", "action_dim", "mask_mode", "has_critic", "prox_mode", "threshold", "agg", "kl")
          if k in case}
    loss = case["loss"]
    at["clip"] = next(k for k, v in _CLIP_VARIANTS.items()
                      if v == {n: x for n, x in loss.items() if n.startswith(("clip_ratio_low", "clip_ratio_high", "clip_log"))})
    at["clip_ratio_c"] = loss["clip_ratio_c"]
    if case["family"] != "token":
        at["critic_warmup"], at["huber_delta"] = loss["critic_warmup"], loss["huber_delta"]
    return at


def _split(x: torch.Tensor, R: int, spread: torch.Tensor) -> torch.Tensor:
    """[n] -> [n, R] rows that sum to x: all of it in the first entry, or (where ``spread``) x + 1/4 and -1/4 in the first two."""
    rows = torch.zeros(x.numel(), R)
    rows[:, 0] = x
    if R > 1:
        rows[:, 0] += 0.25 * spread
        rows[:, 1] -= 0.25 * spread
    return rows


def build(case: dict) -> dict:
    """The raw f32 tensors of one case, as the loss entries take them (before the reference's input shaping)."""
    token = case["family"] == "token"
    if token:
        bsz, seq = 2, 301  # one block per sequence: the 256 threads go round twice, the second time with a ragged tail
        n, sub, R = bsz * seq, 1, 1
    else:
        lt, A, C = case["logprob_type"], case["action_dim"], case["chunks"]
        n = N_ADV
        sub, R = (A, 1) if lt == "token_level" else ((1, A) if lt == "action_level" else (1, C * A))
    i = torch.arange(n)
    tiled = i < (n // 64) * 64
    k = i % 64
    on = torch.where(tiled, k % 2 == 0, torch.ones_like(tiled))
    adv = torch.where(tiled, torch.tensor(_ADV)[(k // 16) % 4], torch.tensor(_FILL_ADV))
    # loss elements: ``sub`` per advantage element, the log-ratio atoms rotating under a shared advantage
    s = torch.arange(sub)
    lr = torch.where(tiled[:, None], torch.tensor(_LR)[((k // 2)[:, None] + s) % 8], torch.tensor(_FILL_LR))  # [n, sub]
    pm = case.get("prox_mode")
    scale = torch.ones(n, 1)
    off = torch.zeros(n, sub)
    versions = None
    if pm == "given":
        off = torch.where(tiled, torch.tensor(_OFFSETS)[(i // 128) % 3], torch.tensor(0.0))[:, None].expand(n, sub)
    elif pm == "versions":
        versions = torch.where(tiled, torch.tensor(_VERSIONS)[(i // 128) % 4], torch.tensor(float(CURRENT_VERSION)))
        # version 3 of 5: alpha = 1/2, the proximal policy lies half way -> lp - old is twice the log-ratio against it
        scale = torch.where(versions == 3.0, 2.0, 1.0)[:, None]
    e = torch.arange(n * sub)
    spread = (e % 2 == 0).float()
    old = -(1.0 + ((e[:, None] * R + torch.arange(R)) % 5) * 0.25)  # [n * sub, R]
    prox = old + _split(off.reshape(-1), R, spread)
    lp = prox + _split((lr * scale).reshape(-1), R, 1.0 - spread)
    inp = dict(n_adv=n, on_all=bool(on.all()))
    if token:
        inp.update(logprobs=lp.reshape(bsz, seq), old_logprobs=old.reshape(bsz, seq), advantages=adv.reshape(bsz, seq).clone(),
                   loss_mask=on.reshape(bsz, seq).clone() if case["mask_mode"] == "mask" else None)
        if case["kl"] is not None:  # lp == ref on every fourth token, else 1/4 or 1/2 away on either side
            d = torch.tensor([0.0, 0.25, -0.5, 0.0, -0.25, 0.5, 0.0])[e % 7]
            inp["ref_logprobs"] = (lp[:, 0] + d).reshape(bsz, seq)
        return inp
    rows = n if lt == "chunk_level" else n // C
    shape_adv = (rows,) if lt == "chunk_level" else (rows, C)
    inp.update(logprobs=lp.reshape(rows, -1), old_logprobs=old.reshape(rows, -1), advantages=adv.reshape(shape_adv).clone())
    if pm == "given":
        inp["proximal_logprobs"] = prox.reshape(rows, -1)
    if versions is not None:  # one version per advantage element, repeated over its raw log-probs (the learner's layout)
        inp["versions"] = versions[:, None].expand(n, sub * R).reshape(rows, -1).contiguous()
    if case["mask_mode"] != "none":
        inp["loss_mask"] = on.reshape(shape_adv).clone()
    if case["mask_mode"] == "ratio":  # loss_mask_sum / max_episode_steps = 32 / 64: the ratio aggregation divides by 1/2
        inp["loss_mask_sum"] = torch.full(shape_adv, 32, dtype=torch.int64)
    if case["has_critic"]:
        atoms = torch.tensor(_critic_atoms(case["loss"]["huber_delta"]))
        row = atoms[torch.where(tiled, (i // 2) % len(atoms), torch.tensor(len(atoms) - 1))]
        inp.update(prev_values=row[:, 0].reshape(shape_adv).clone(), values=row[:, 1].reshape(shape_adv).clone(),
                   returns=row[:, 2].reshape(shape_adv).clone())
    return inp


def loss_kwargs(case: dict) -> dict:
    """The keyword arguments of the loss this case runs with (embodied families)."""
    kw = {k: v for k, v in case["loss"].items() if v is not None}
    if not case["has_critic"]:
        kw.pop("value_clip"), kw.pop("huber_delta")
    if case["mask_mode"] == "ratio":
        kw["max_episode_steps"] = 64
    return kw


def shaped_inputs(case: dict, inp: dict, lp=None, v=None, dtype=torch.float32):
    """What the reference's preprocess_loss_inputs makes of the raw tensors (oracle restatement); ``lp`` / ``v`` replace the raw
    log-probs / values (leaves to differentiate)."""
    c = lambda t: None if t is None else (t.to(dtype) if t.is_floating_point() else t)  # noqa: E731
    A, lt = case["action_dim"], case["logprob_type"]
    lp = c(inp["logprobs"]) if lp is None else lp
    v = c(inp.get("values")) if v is None else v
    shaped = O.shape_loss_inputs(lp, c(inp["old_logprobs"]), c(inp["advantages"]), lt, A, loss_mask=inp.get("loss_mask"),
                                 loss_mask_sum=inp.get("loss_mask_sum"), values=v, prev_values=c(inp.get("prev_values")),
                                 returns=c(inp.get("returns")))
    p2 = v2 = None
    if case["family"] == "decoupled":
        p2, v2 = O.shape_decoupled_inputs(c(inp.get("proximal_logprobs")), c(inp.get("versions")), lt, A, lp.shape[0],
                                          shaped["logprobs"].shape)
    return shaped, p2, v2


def proximal(case: dict, lp, old, p2, versions):
    """The log-probs the clip is taken against, at the loss shape: the behaviour policy's, the given proximal policy's, or the
    interpolation by version distance (losses.py:72-89)."""
    if case["family"] != "decoupled":
        return old
    if p2 is not None:
        return p2
    if versions is None:
        return old
    vb = versions.expand_as(lp)
    diff, gap = CURRENT_VERSION - vb, (CURRENT_VERSION - 1.0) - vb
    alpha = torch.where((diff > 0) & (vb >= 0), gap / diff, torch.zeros_like(vb)).clamp(0.0, 1.0)
    return old + alpha * (lp - old)


# --------------------------------------------------------------------------------------------------------------------------
def _on_or_away(d: torch.Tensor, what: str, case: dict):
    bad = (d != 0) & (d.abs() < MARGIN)
    assert not bool(bad.any()), f"{case['id']}: {int(bad.sum())} element(s) within {MARGIN} of {what} without being on it"
    return d == 0


def classify(case: dict, inp: dict) -> dict:
    """name -> (on-the-boundary flags, loss-mask flags, advantage) in float64 from the inputs alone.  Asserts that every element
    is either exactly on a comparison of the kernel or at least MARGIN away from it, and that every input lies on the grid."""
    f64 = torch.float64
    for name, t in inp.items():
        if torch.is_tensor(t) and t.is_floating_point():
            assert bool(((t.double() / Q) == (t.double() / Q).round()).all()) and float(t.abs().max()) <= 8.0, (case["id"], name)
    out = {}
    loss = case["loss"]
    if case["family"] == "token":
        lp, old, adv = (inp[k].double() for k in ("logprobs", "old_logprobs", "advantages"))
        mask = inp["loss_mask"] if inp["loss_mask"] is not None else torch.ones_like(lp, dtype=torch.bool)
        px, versions = old, None
    else:
        sh, p2, versions = shaped_inputs(case, inp, dtype=f64)
        lp, old = sh["logprobs"], sh["old_logprobs"]
        adv = sh["advantages"].expand_as(lp)
        mask = sh["loss_mask"].expand_as(lp) if sh["loss_mask"] is not None else torch.ones_like(lp, dtype=torch.bool)
        px = proximal(case, lp, old, p2, versions)

    def put(name, flags, m=mask, a=adv):
        out[name] = (flags, m, a)

    lr = lp - px
    put("actor/lp==old", lp == old)
    if loss.get("clip_log_ratio_min") is not None:
        put("actor/log_ratio==clip_log_ratio_min", _on_or_away(lr - loss["clip_log_ratio_min"], "clip_log_ratio_min", case))
        lr = lr.clamp(min=loss["clip_log_ratio_min"])
    if loss.get("clip_log_ratio_max") is not None:
        put("actor/log_ratio==clip_log_ratio_max", _on_or_away(lr - loss["clip_log_ratio_max"], "clip_log_ratio_max", case))
        lr = lr.clamp(max=loss["clip_log_ratio_max"])
    if loss.get("clip_log_ratio_min") == 0.0 and loss.get("clip_log_ratio_max") == 0.0:
        put("actor/log_ratio==min==max==0", lp == px)
    lo, hi = 1.0 - loss["clip_ratio_low"], 1.0 + loss["clip_ratio_high"]
    at_lo = _on_or_away(lr - math.log(lo), "log(1 - clip_ratio_low)", case)
    at_hi = _on_or_away(lr - math.log(hi), "log(1 + clip_ratio_high)", case)
    put("actor/ratio==1", lr == 0)
    if lo == 1.0:
        put("actor/ratio==1-clip_ratio_low", at_lo)
    if hi == 1.0:
        put("actor/ratio==1+clip_ratio_high", at_hi)
    if lo == 1.0 and hi == 1.0:
        put("actor/ratio==lo==hi", at_lo & at_hi)
    if loss.get("clip_ratio_c") is not None:
        assert not bool(_on_or_away(lr - math.log(loss["clip_ratio_c"]), "log(clip_ratio_c)", case).any())
        put("actor/ratio==1 under dual clip", lr == 0)
    if loss.get("critic_warmup"):
        put("actor/ratio==1 under critic_warmup", lr == 0)
    put("actor/adv==0", (adv == 0) & (lr == 0))
    if case.get("mask_mode") == "ratio":
        put("actor/ratio==1 under the ratio aggregation", lr == 0)
    if case["family"] == "token":
        put(f"token/{case['agg']}: ratio==1", lr == 0)
        if case["kl"] is not None:
            put(f"kl/{case['kl']}: lp==ref", _on_or_away(inp["ref_logprobs"].double() - lp, "ref_logprobs", case))
        return out
    if case["family"] == "decoupled":
        pm = case["prox_mode"]
        put(f"decoupled/{pm}: lp==proximal", lr == 0)
        if case["threshold"] is not None:
            at = _on_or_away((px - old) - math.log(case["threshold"]), "log(behave_weight_threshold)", case)
            put(f"decoupled/{pm}: weight==threshold", at)
            if pm != "old":  # (proximal == old: the weight is 1 everywhere)
                put(f"decoupled/{pm}: weight>threshold", (px - old) > math.log(case["threshold"]))
        if versions is not None:
            vb = versions.expand_as(lp)
            put("decoupled/version==current", vb == CURRENT_VERSION)
            put("decoupled/version==current-1", vb == CURRENT_VERSION - 1)
            put("decoupled/version==-1", vb == -1)
    if case["has_critic"]:
        v, pv, ret = sh["values"], sh["prev_values"], sh["returns"]
        cm = sh["loss_mask"] if sh["loss_mask"] is not None else torch.ones_like(v, dtype=torch.bool)
        ca = torch.ones_like(v)  # the critic does not read the advantage
        vc, dl = loss["value_clip"], loss["huber_delta"]
        diff = v - pv
        e1, e2 = ret - v, ret - (pv + diff.clamp(-vc, vc))
        hub = lambda e: torch.where(e.abs() < dl, 0.5 * e ** 2, dl * (e.abs() - 0.5 * dl))  # noqa: E731
        tie = _on_or_away(hub(e1) - hub(e2), "the other Huber value", case)
        put("critic/v==pv", diff == 0, cm, ca)
        put("critic/diff==+value_clip", _on_or_away(diff - vc, "+value_clip", case), cm, ca)
        put("critic/diff==-value_clip", _on_or_away(diff + vc, "-value_clip", case), cm, ca)
        at1, at2 = _on_or_away(e1.abs() - dl, "huber_delta", case), _on_or_away(e2.abs() - dl, "huber_delta", case)
        put("critic/ret-v==+huber_delta", at1 & (e1 > 0), cm, ca)
        put("critic/ret-v==-huber_delta", at1 & (e1 < 0), cm, ca)
        put("critic/|ret-vclip|==huber_delta", at2 & (diff.abs() > vc), cm, ca)
        put("critic/ret==v", e1 == 0, cm, ca)
        sym = tie & (e1 == -e2) & (e1 != 0)
        rel = "above" if dl > 0.25 else ("equal to" if dl == 0.25 else "below")
        put(f"critic/half-gradient tie e1>0, huber_delta {rel} |e|", sym & (e1 > 0), cm, ca)
        put(f"critic/half-gradient tie e1<0, huber_delta {rel} |e|", sym & (e1 < 0), cm, ca)
    return out


def required_boundaries() -> dict:
    """name -> whether the sign of the advantage matters: every boundary the table must hold at least twice."""
    req = {"actor/lp==old": True, "actor/ratio==1": True, "actor/adv==0": False,
           "actor/ratio==1-clip_ratio_low": True, "actor/ratio==1+clip_ratio_high": True, "actor/ratio==lo==hi": True,
           "actor/log_ratio==clip_log_ratio_min": True, "actor/log_ratio==clip_log_ratio_max": True,
           "actor/log_ratio==min==max==0": True, "actor/ratio==1 under dual clip": True,
           "actor/ratio==1 under critic_warmup": True, "actor/ratio==1 under the ratio aggregation": True,
           "critic/v==pv": False, "critic/diff==+value_clip": False, "critic/diff==-value_clip": False,
           "critic/ret-v==+huber_delta": False, "critic/ret-v==-huber_delta": False, "critic/|ret-vclip|==huber_delta": False,
           "critic/ret==v": False, "decoupled/version==current": False, "decoupled/version==current-1": False,
           "decoupled/version==-1": False, "decoupled/given: weight>threshold": False}
    for rel in ("above", "equal to", "below"):
        for s in ("e1>0", "e1<0"):
            req[f"critic/half-gradient tie {s}, huber_delta {rel} |e|"] = False
    for pm in ("given", "old", "versions"):
        req[f"decoupled/{pm}: lp==proximal"] = True
        req[f"decoupled/{pm}: weight==threshold"] = False
    for agg in ("token-mean", "seq-mean-token-sum", "seq-mean-token-mean"):
        req[f"token/{agg}: ratio==1"] = True
    for kind in ("k1", "abs", "k2", "k3"):
        req[f"kl/{kind}: lp==ref"] = False
    return req


def coverage(all_cases=None) -> dict:
    """name -> dict(total, on, masked, pos, neg) summed over the cases: elements on the boundary, with the mask on / off, and with
    the mask on under a positive / negative advantage."""
    cov = {}
    for case in (cases() if all_cases is None else all_cases):
        for name, (flags, mask, adv) in classify(case, build(case)).items():
            c = cov.setdefault(name, dict(total=0, on=0, masked=0, pos=0, neg=0))
            c["total"] += int(flags.sum())
            c["on"] += int((flags & mask).sum())
            c["masked"] += int((flags & ~mask).sum())
            c["pos"] += int((flags & mask & (adv > 0)).sum())
            c["neg"] += int((flags & mask & (adv < 0)).sum())
    return cov


def assert_coverage(cov: dict):
    for name, signed in required_boundaries().items():
        assert name in cov, f"no case places an element on {name}"
        c = cov[name]
        assert c["total"] >= 2 and c["on"] >= 1 and c["masked"] >= 1, (name, c)
        if signed:
            assert c["pos"] >= 1 and c["neg"] >= 1, (name, c)


# --------------------------------------------------------------------------------------------------------------------------
def run_oracle(case: dict, inp: dict) -> dict:
    """Expected loss, metrics and gradients ((loss * UPSTREAM).backward()) from the oracle's torch graph, f32 on the CPU; plus
    the oracle's own loss denominators for the exact comparison of the boundary gradients."""
    lp = inp["logprobs"].clone().requires_grad_(True)
    if case["family"] == "token":
        # (without a mask the kernel takes every token; the reference's sequence aggregations need the mask spelled out)
        mask = inp["loss_mask"] if inp["loss_mask"] is not None else torch.ones_like(lp, dtype=torch.bool)
        loss, metrics = TO.reasoning_loss_from_logprobs(
            lp, None, inp["old_logprobs"], inp["advantages"], mask, loss_agg=case["agg"],
            clip_ratio_low=case["loss"]["clip_ratio_low"], clip_ratio_high=case["loss"]["clip_ratio_high"],
            clip_ratio_c=case["loss"]["clip_ratio_c"], clip_log_ratio_min=case["loss"].get("clip_log_ratio_min"),
            clip_log_ratio_max=case["loss"].get("clip_log_ratio_max"), ref_logprobs=inp.get("ref_logprobs"),
            kl_beta=KL_BETA if case["kl"] else 0.0, kl_penalty_type=case["kl"] or "low_var_kl")
        (loss * UPSTREAM).backward()
        return dict(loss=loss.detach(), metrics=metrics, d_logprobs=lp.grad, d_values=None)
    v = inp["values"].clone().requires_grad_(True) if case["has_critic"] else None
    shaped, p2, v2 = shaped_inputs(case, inp, lp=lp, v=v)
    kw = loss_kwargs(case)
    if case["family"] == "decoupled":
        loss, metrics = O.decoupled_actor_critic_loss(proximal_logprobs=p2, versions=v2, behave_weight_threshold=case["threshold"],
                                                      current_version=CURRENT_VERSION if case["prox_mode"] == "versions" else None,
                                                      **kw, **shaped)
    elif case["has_critic"]:
        loss, metrics = O.ppo_actor_critic_loss(**kw, **shaped)
    else:
        loss, metrics = O.ppo_actor_loss(**{k: shaped[k] for k in ("logprobs", "old_logprobs", "advantages", "loss_mask",
                                                                   "loss_mask_sum")}, **kw)
    if loss.requires_grad:
        (loss * UPSTREAM).backward()
    zero = lambda t, g: torch.zeros_like(t) if g is None else g  # noqa: E731  (critic warm-up: the actor term is a constant)
    return dict(loss=loss.detach(), metrics=metrics, d_logprobs=zero(lp, lp.grad),
                d_values=None if v is None else zero(v, v.grad))


def denominators(case: dict, inp: dict) -> tuple:
    """(actor, critic) denominators of the oracle's aggregation: what masked_mean / masked_mean_ratio divide the element sums by
    (the kept set of a behave_weight_threshold in float64: the margin decides it the same way in f32)."""
    n = inp["n_adv"]
    sub = case["action_dim"] if case["logprob_type"] == "token_level" else 1
    mask = inp.get("loss_mask")
    nm = n if mask is None else max(int(mask.sum()), 1)
    if case["mask_mode"] == "ratio":
        return float(n * sub), float(n)
    actor = float(n * sub if mask is None else nm)
    if case["family"] == "decoupled" and case["threshold"] is not None:  # masked_mean over behav_mask, built at the loss shape
        sh, p2, v2 = shaped_inputs(case, inp, dtype=torch.float64)
        px = proximal(case, sh["logprobs"], sh["old_logprobs"], p2, v2)
        keep = (px - sh["old_logprobs"]) <= math.log(case["threshold"])
        if sh["loss_mask"] is not None:
            keep = keep & sh["loss_mask"]
        actor = float(max(int(keep.sum()), 1))
    return actor, float(n if mask is None else nm)
