"""Built-in loss-scale processes behind the registry names "group_level", "agent_level" and "turn_level" (mirror of
rlinf/algorithms/loss_scales.py), served by grpo_dynamic.hip.

Each process takes the learner's scaling ``context`` and its dynamic rollout ``batch`` and rescales one batch tensor in place,
as the reference does.  The reference walks the turns in Python -- one indexed multiply per turn, and for "turn_level" one
``.item()`` per turn; here the (trajectory, sub-trajectory) grouping is built once on the host from the same ``.tolist()`` the
reference makes, and each process is one launch:
  * group_level: ``advantages *= num_seq * dp_world_size / actor_global_batch_size``;
  * agent_level: ``loss_scales[row] *= (1 / A_i) / T_ia`` (factors in f64 on the host, rounded to f32 once);
  * turn_level:  ``loss_scales[row] *= T_ia * |o_t| / sum_t |o_t|`` (counts and factors on the device); the one device read of
    the call is its "some group's token total is 0" flag, for the reference's ZeroDivisionError.
Every factor is the reference's Python float rounded to f32 and applied with one f32 multiply per element, which is what
torch's ``t *= python_float`` computes: the results are bit-identical.
"""

from __future__ import annotations

import torch

from .. import token_ops
from . import utils as _u
from .registry import register_loss_scale


def _in_place(t: torch.Tensor, dev, fn):
    """Apply ``fn`` to ``t`` on ``dev``; a CPU tensor is staged there and written back, so the caller's tensor changes in place
    as in the reference."""
    if t.device == dev and t.is_contiguous():
        fn(t)
        return
    work = t.to(dev).contiguous()
    fn(work)
    t.copy_(work)


def _groups(batch):
    sub = batch["extra:idx_to_sub_traj"]
    sub = sub.tolist() if isinstance(sub, torch.Tensor) else list(sub)  # the reference's one .tolist()
    return token_ops.loss_scale_groups(batch["idx_to_traj"], sub)


@register_loss_scale("group_level")
def group_scale(context, batch):
    """The outer 1 / G normalisation: ``batch["advantages"] *= num_seq * dp_world_size / actor_global_batch_size``."""
    folding_scale = context["folding_scale"]
    assert "group_level" not in folding_scale, (
        "`group_level` loss scaling can only be applied once. Apply the "
        "group-level factor before any `agent_level` or `turn_level` factor."
    )
    context["folding_scale"].append("group_level")

    num_sequence = len(batch["idx_to_traj"])
    dp_world_size = context.get("data_parallel_world_size", 1)
    group_scale = num_sequence * dp_world_size / context["actor_global_batch_size"]
    adv = batch["advantages"]
    _in_place(adv, _u.compute_device(adv), lambda t: token_ops.scale_rows_(t, group_scale))
    return batch


@register_loss_scale("agent_level")
def agent_scale(context: dict, batch: dict) -> dict:
    """``loss_scales[row] *= 1 / A_i / T_ia``: A_i distinct sub-trajectories in trajectory i, T_ia turns of sub-trajectory a."""
    folding_scale = context["folding_scale"]
    assert "group_level" in folding_scale and "agent_level" not in folding_scale, (
        "`agent_level` loss scaling requires `group_level` to be applied first, "
        "and it can only be applied once."
    )
    context["folding_scale"].append("agent_level")

    order, offsets, agents = _groups(batch)
    ls = batch["loss_scales"]
    dev = _u.compute_device(ls)
    factors = torch.from_numpy(token_ops.agent_level_factors(order, offsets, agents))
    factors = factors.pin_memory().to(dev, non_blocking=True)
    _in_place(ls, dev, lambda t: token_ops.scale_rows_(t, row_factors=factors))
    return batch


@register_loss_scale("turn_level")
def turn_scale(context: dict, batch: dict) -> dict:
    """``loss_scales[row] *= T_ia * |o_t| / sum_t |o_t|`` with |o_t| = response_mask[row].sum(): turn weights proportional to
    their response tokens.  A (trajectory, sub-trajectory) whose rows hold no response token raises ZeroDivisionError, as in
    the reference (whose earlier groups are scaled by then; here the groups with tokens are)."""
    folding_scale = context["folding_scale"]
    assert (
        "group_level" in folding_scale
        and "agent_level" in folding_scale
        and "turn_level" not in folding_scale
    ), (
        "`turn_level` loss scaling requires both `group_level` and "
        "`agent_level` to be applied first, and it can only be applied once."
    )
    context["folding_scale"].append("turn_level")

    order, offsets, _ = _groups(batch)
    ls = batch["loss_scales"]
    dev = _u.compute_device(ls)
    plan = token_ops.TurnScalePlan(order, offsets, dev)
    mask = _u.stage(batch["response_mask"], dev)
    flag = []
    _in_place(ls, dev, lambda t: flag.append(token_ops.turn_level_scale_(t, mask, plan)))
    if int(flag[0].item()):  # the call's one device -> host read
        raise ZeroDivisionError("division by zero")
    return batch
