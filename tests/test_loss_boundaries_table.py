"""The boundary table of tests/helpers/loss_boundaries.py on its own: grid, margin and coverage, from the inputs alone (CPU)."""

import pytest
import torch

from helpers import loss_boundaries as LB

CASES = LB.cases()


def test_case_ids_are_unique():
    ids = [c["id"] for c in CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("group", ["grid", "geom", "decoupled", "token"])
def test_no_attribute_of_a_case_follows_another(group):
    """Within a group, under every value of one attribute every other attribute takes at least two values: no cycling attribute
    is tied to an axis of the product or to another cycler (a mask that came only with critic_warmup=False, an actor-only entry
    that ran only under warm-up)."""
    attrs = [LB.case_attributes(c) for c in CASES if c["group"] == group]
    keys = [k for k in attrs[0] if len({a[k] for a in attrs}) > 1]
    assert len(keys) >= 5, keys
    for x in keys:
        for y in keys:
            for xv in {a[x] for a in attrs} if x != y else ():
                assert len({a[y] for a in attrs if a[x] == xv}) >= 2, f"{group}: {y} is fixed wherever {x} == {xv}"


def test_the_actor_only_entry_runs_with_a_gradient():
    """loss_type="actor" without critic warm-up (under it the actor term is a constant): every clip variant, with and without the
    dual clip and the mask, and the oracle's gradient there is not zero."""
    live = [c for c in CASES if not c.get("has_critic", True) and not c["loss"]["critic_warmup"]]
    seen = {(LB.case_attributes(c)["clip"], c["loss"]["clip_ratio_c"]) for c in live}
    assert len(seen) == 14, seen
    assert {(c["loss"]["clip_ratio_c"], c["mask_mode"]) for c in live} == {(None, "mask"), (None, "none"), (3.0, "mask"), (3.0, "none")}
    for c in live:
        want = LB.run_oracle(c, LB.build(c))
        assert int((want["d_logprobs"] != 0).sum()) >= 16 and want["d_values"] is None, c["id"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_every_element_is_on_a_boundary_or_a_margin_away(case):
    inp = LB.build(case)
    flags = LB.classify(case, inp)  # asserts the grid and the margin
    n_loss = inp["logprobs"].numel() if case["family"] == "token" else None
    for name, (on, mask, adv) in flags.items():
        assert on.shape == mask.shape == adv.shape, name
    if n_loss is None:  # more than one 256-thread block plus a ragged tail
        assert inp["n_adv"] > 512 and inp["n_adv"] % 256 not in (0, 255) and inp["n_adv"] % 4 != 0
    else:
        assert inp["logprobs"].shape[1] > 256 and inp["logprobs"].shape[1] % 256 != 0


def test_every_named_boundary_is_covered_at_least_twice():
    cov = LB.coverage(CASES)
    LB.assert_coverage(cov)
    for name, c in sorted(cov.items()):
        print(f"{name:70s} {c}")


def test_oracle_is_finite_and_ties_take_half_the_gradient():
    """The constructed critic tie of the table: pv = 0, v = 1, value_clip = 0.5, ret = 0.75 -> dv = 0.125 per unit of scale."""
    from oracle import ppo_oracle as O
    v = torch.tensor([1.0, -1.0], requires_grad=True)
    loss, _ = O.ppo_critic_loss(v, torch.tensor([0.75, -0.75]), torch.zeros(2), 0.5, 1.0)
    (g,) = torch.autograd.grad(loss * 2, v)
    assert torch.equal(g, torch.tensor([0.125, -0.125]))
    for case in CASES[::7]:
        want = LB.run_oracle(case, LB.build(case))
        assert bool(torch.isfinite(want["loss"])) and bool(torch.isfinite(want["d_logprobs"]).all()), case["id"]
