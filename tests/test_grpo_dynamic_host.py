"""CPU checks of multi-turn GRPO ("grpo_dynamic") and the loss-scale processes: registry names and lookup rules, the reference's
assertion messages (raised before any device is touched), the host CSR / grouping plans against a plain-Python grouping, and
ext.register() against stand-in registries with and without register_loss_scale."""

import os
import sys
import types

import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "grpo_dynamic.pt")


def _golden():
    return torch.load(GOLDEN, weights_only=False)


def test_registry_serves_grpo_dynamic_and_the_loss_scales_in_order():
    from rlinf_amd.algorithms import advantages, get_adv_and_returns, get_loss_scales, loss_scales
    assert get_adv_and_returns("grpo_dynamic").__wrapped__ is advantages.compute_grpo_dynamic_advantages.__wrapped__
    assert get_adv_and_returns("GRPO_Dynamic") is get_adv_and_returns("grpo_dynamic")  # advantages lower-case on lookup
    fns = get_loss_scales(["group_level", "agent_level", "turn_level"])
    assert fns == [loss_scales.group_scale, loss_scales.agent_scale, loss_scales.turn_scale]
    assert get_loss_scales(["turn_level", "group_level"]) == [loss_scales.turn_scale, loss_scales.group_scale]
    assert get_loss_scales([]) == []


def test_loss_scale_lookup_is_case_sensitive_and_names_are_lower_cased():
    from rlinf_amd.algorithms import registry as reg
    with pytest.raises(ValueError, match="^Loss scale process Turn_Level not registered$"):
        reg.get_loss_scales(["group_level", "Turn_Level"])
    want = _golden()["errors"]["unknown_scale"]
    try:
        reg.get_loss_scales(["group_level", "Turn_Level"])
    except ValueError as e:
        assert (type(e).__name__, str(e)) == (want["type"], want["message"])
    saved = dict(reg.LOSS_SCALE_REGISTRY)
    try:
        fn = lambda c, b: b  # noqa: E731
        assert reg.register_loss_scale("My_Scale")(fn) is fn
        assert reg.get_loss_scales(["my_scale"]) == [fn]
        with pytest.raises(ValueError, match="My_Scale not registered"):
            reg.get_loss_scales(["My_Scale"])
    finally:
        reg.LOSS_SCALE_REGISTRY.clear(), reg.LOSS_SCALE_REGISTRY.update(saved)


def test_rlinf_alias_serves_loss_scales():
    from rlinf_amd import compat
    compat.install_alias()
    try:
        import rlinf.algorithms.loss_scales as ls
        from rlinf.algorithms.registry import get_loss_scales
        assert get_loss_scales(["agent_level"]) == [ls.agent_scale]
    finally:
        compat.uninstall_alias()


def _raises_like(fn, want):
    with pytest.raises(Exception) as ei:
        fn()
    assert (type(ei.value).__name__, str(ei.value)) == (want["type"], want["message"])


def test_advantage_assertions_match_the_reference_before_any_device_work(monkeypatch):
    from rlinf_amd.algorithms import advantages as A
    from rlinf_amd.algorithms import calculate_adv_and_returns
    monkeypatch.setattr(A.token_ops, "GrpoDynamicPlan", None)  # reaching the device stage would fail differently
    err = _golden()["errors"]
    m = torch.ones(4, 5, dtype=torch.bool)
    f = A.compute_grpo_dynamic_advantages
    _raises_like(lambda: f(rewards=torch.zeros(4, 1), loss_mask=m, group_size=2, idx_to_traj=[0, 0, 1, 1, 1]),
                 err["size_mismatch"])
    _raises_like(lambda: f(rewards=torch.zeros(5, 1), loss_mask=m, group_size=2, idx_to_traj=[0, 0, 1, 2, 2]),
                 err["not_divisible"])
    _raises_like(lambda: f(rewards=torch.zeros(5, 1), loss_mask=m, group_size=2, idx_to_traj=[0, 0, 1, 1, 1],
                           advantage_mode="token"), err["invalid_mode"])
    # a 1-D integer tensor is accepted as idx_to_traj
    _raises_like(lambda: f(rewards=torch.zeros(5, 1), loss_mask=m, group_size=2, idx_to_traj=torch.tensor([0, 0, 1, 2, 2])),
                 err["not_divisible"])
    # the reasoning dispatcher's fast path checks the same things in the same order
    kw = dict(task_type="reasoning", adv_type="grpo_dynamic", rewards=torch.zeros(5), loss_mask=m.transpose(0, 1),
              num_sequence=5, group_size=2)
    _raises_like(lambda: calculate_adv_and_returns(idx_to_traj=[0, 0, 1, 2, 2], **kw), err["not_divisible"])
    _raises_like(lambda: calculate_adv_and_returns(idx_to_traj=[0, 0, 1, 1, 1], advantage_mode="token", **kw),
                 err["invalid_mode"])
    with pytest.raises(AssertionError, match="Unsupported reward shape"):
        calculate_adv_and_returns(idx_to_traj=[0, 0, 1, 1, 1], **dict(kw, rewards=torch.zeros(5, 1)))
    with pytest.raises(ZeroDivisionError):
        f(rewards=torch.zeros(5, 1), loss_mask=m, group_size=0, idx_to_traj=[0, 0, 1, 1, 1])


def _ctx(f):
    return {"folding_scale": list(f), "actor_global_batch_size": 8.0}


def test_folding_scale_ordering_errors_match_the_reference():
    from rlinf_amd.algorithms import loss_scales as ls
    err = _golden()["errors"]
    batch = {"idx_to_traj": [0, 1], "extra:idx_to_sub_traj": torch.zeros(2, dtype=torch.long),
             "response_mask": torch.ones(2, 3, dtype=torch.bool), "advantages": torch.ones(2, 3), "loss_scales": torch.ones(2, 3)}
    _raises_like(lambda: ls.agent_scale(_ctx([]), batch), err["agent_before_group"])
    _raises_like(lambda: ls.group_scale(_ctx(["group_level"]), batch), err["group_twice"])
    _raises_like(lambda: ls.turn_scale(_ctx(["group_level"]), batch), err["turn_before_agent"])
    _raises_like(lambda: ls.agent_scale(_ctx(["group_level", "agent_level"]), batch), err["agent_twice"])
    _raises_like(lambda: ls.turn_scale(_ctx(["group_level", "agent_level", "turn_level"]), batch), err["turn_twice"])


def _py_traj_groups(ids):
    out = {}
    for i, t in enumerate(ids):
        out.setdefault(t, []).append(i)
    return out


@pytest.mark.parametrize("ids", [[0, 0, 1, 3, 3], [3, 1, 0, 3, 2, 2, 1, 0, 3], [5, 4, 5, 0, 0, 7, 7, 7, 1], [0], list(range(9))[::-1],
                                 [int(x) for x in torch.randint(0, 50, (400,), generator=torch.Generator().manual_seed(1))]])
def test_grpo_dynamic_csr_matches_a_plain_python_grouping(ids):
    from rlinf_amd import token_ops
    order, off = token_ops.grpo_dynamic_csr(ids)
    want = _py_traj_groups(ids)
    assert len(off) == max(ids) + 2 and off[0] == 0 and off[-1] == len(ids)
    for t in range(max(ids) + 1):
        assert order[off[t]:off[t + 1]].tolist() == want.get(t, [])  # empty trajectories: an empty range
    order2, off2 = token_ops.grpo_dynamic_csr(torch.tensor(ids), num_traj=max(ids) + 3)
    assert order2.tolist() == order.tolist() and off2.tolist() == off.tolist() + [len(ids)] * 2


def test_grpo_dynamic_csr_rejects_bad_ids():
    from rlinf_amd import token_ops
    from rlinf_amd._lib import RlxError
    with pytest.raises(RlxError, match="negative"):
        token_ops.grpo_dynamic_csr([0, -1])
    with pytest.raises(RlxError, match="1-D integer"):
        token_ops.grpo_dynamic_csr(torch.zeros(3))


@pytest.mark.parametrize("seed,n,n_traj,n_sub", [(0, 9, 3, 2), (1, 200, 40, 4), (2, 57, 57, 1), (3, 300, 20, 7)])
def test_loss_scale_groups_and_agent_factors_match_a_plain_python_grouping(seed, n, n_traj, n_sub):
    from rlinf_amd import token_ops
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, n_traj, (n,), generator=g).tolist()
    sub = (torch.randint(0, n_sub, (n,), generator=g) * 3 - 2).tolist()  # arbitrary (also negative) agent ids
    order, off, agents = token_ops.loss_scale_groups(ids, sub)
    groups = {}
    for t, rows in _py_traj_groups(ids).items():
        per = {}
        for i in rows:
            per.setdefault(sub[i], []).append(i)
        for rows_a in per.values():
            groups[tuple(rows_a)] = len(per)
    got = {tuple(order[off[k]:off[k + 1]].tolist()): int(agents[k]) for k in range(len(off) - 1)}
    assert got == groups
    fac = token_ops.agent_level_factors(order, off, agents)
    for rows, a in groups.items():
        for i in rows:  # the reference's Python float, rounded to f32 once
            assert fac[i] == torch.tensor(1 / a / len(rows), dtype=torch.float32).item()


class _StubRegistry(types.ModuleType):
    def __init__(self, name, with_loss_scales):
        super().__init__(name)
        # an RLinf with the loss-scale registry also registers its own grpo_dynamic (advantages.py:167)
        self.ADV_REGISTRY, self.LOSS_REGISTRY = ({"grpo_dynamic": object()} if with_loss_scales else {}), {}
        if with_loss_scales:
            self.LOSS_SCALE_REGISTRY = {}

            def register_loss_scale(name):
                def deco(fn):
                    self.LOSS_SCALE_REGISTRY[name.lower()] = fn
                    return fn
                return deco
            self.register_loss_scale = register_loss_scale

    def register_advantage(self, name):
        def deco(fn):
            self.ADV_REGISTRY[name.lower()] = fn
            return fn
        return deco

    def register_policy_loss(self, name):
        def deco(fn):
            self.LOSS_REGISTRY[name] = fn
            return fn
        return deco


def _register_with_stub(with_loss_scales):
    from rlinf_amd import ext
    names = ("rlinf", "rlinf.algorithms", "rlinf.algorithms.registry", "rlinf.models")
    before = {n: sys.modules.get(n) for n in names}
    reg = _StubRegistry("rlinf.algorithms.registry", with_loss_scales)
    models = types.ModuleType("rlinf.models")
    models.register_model = lambda *a, **k: None
    pkg, algos = types.ModuleType("rlinf"), types.ModuleType("rlinf.algorithms")
    pkg.algorithms, pkg.models, algos.registry = algos, models, reg
    sys.modules.update({"rlinf": pkg, "rlinf.algorithms": algos, "rlinf.algorithms.registry": reg, "rlinf.models": models})
    try:
        try:
            ext.register()
        except RuntimeError as e:  # no HIP device here: register() installs the names, then says so
            assert "no HIP device" in str(e)
    finally:
        for n, m in before.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return reg


def test_ext_register_installs_grpo_dynamic_and_the_loss_scales_where_rlinf_has_them():
    from rlinf_amd.algorithms import advantages, loss_scales
    reg = _register_with_stub(True)
    assert reg.ADV_REGISTRY["grpo_dynamic"] is advantages.compute_grpo_dynamic_advantages
    assert reg.LOSS_SCALE_REGISTRY == {"group_level": loss_scales.group_scale, "agent_level": loss_scales.agent_scale,
                                       "turn_level": loss_scales.turn_scale}
    reg = _register_with_stub(False)  # an RLinf without grpo_dynamic and the loss-scale registry gets neither
    assert "grpo_dynamic" not in reg.ADV_REGISTRY
    assert not hasattr(reg, "LOSS_SCALE_REGISTRY") and "gae" in reg.ADV_REGISTRY


def test_golden_fixture_covers_the_issue_cases():
    d = _golden()
    assert {"turn_unsorted", "traj_unsorted", "traj_empty", "turn_single_turn_question", "turn_all_false_row",
            "turn_identical_group", "traj_bf16", "turn_bf16"} <= set(d["adv"])
    assert torch.isnan(d["adv"]["turn_single_turn_question"]["advantages"]).any()
    assert set(d["dispatch"]) and {"group", "group_agent", "group_agent_turn"} <= set(d["scale"])
