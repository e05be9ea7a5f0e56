"""Write tests/golden/grpo_dynamic.pt: the reference's multi-turn GRPO advantage and its loss-scale processes on seeded inputs.

    python -m tools.make_grpo_dynamic_golden

Runs only where the reference tree is readable (oracle.reference_loader); loss_scales.py is loaded by path from here.  The GPU
tests read the stored file, never the tree.  Recorded, per case, the inputs and what the reference returned:
  adv/<case>       compute_grpo_dynamic_advantages (advantages.py:167-299) with the callee contract: rewards [num_seq, 1],
                   loss_mask [seq_len, num_seq] -> [seq_len, num_seq]
  dispatch/<case>  registry.calculate_adv_and_returns(task_type="reasoning", adv_type="grpo_dynamic", ...) with the learner's
                   [num_seq] rewards and [num_seq, seq_len] mask -> [num_seq, seq_len]
  scale/<case>     a chain of loss-scale processes (loss_scales.py) on a dynamic batch: advantages and loss_scales after it
  errors/<case>    the exception type and message for inputs the reference rejects
Rewards are multiples of 1/4, so that every turn-mode sum the reference forms in f32 is exact and those advantages do not depend
on the order of its reductions (trajectory rewards are turn means, so trajectory-mode group means round in the reference's own
order).
"""

from __future__ import annotations

import importlib.util
import os

import torch

from oracle import reference_loader as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "grpo_dynamic.pt")


def load_loss_scales():
    RL.load()  # rlinf.algorithms.registry must be importable first
    path = os.path.join(RL.REFERENCE_ROOT, "rlinf/algorithms/loss_scales.py")
    spec = importlib.util.spec_from_file_location("rlinf.algorithms.loss_scales", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ids(g, num_traj, lo=1, hi=7, shuffle=False, empty=()):
    turns = torch.randint(lo, hi + 1, (num_traj,), generator=g).tolist()
    ids = [t for t in range(num_traj) if t not in empty for _ in range(turns[t])]
    if shuffle:
        ids = [ids[i] for i in torch.randperm(len(ids), generator=g).tolist()]
    return ids


def _rewards(g, n, dtype=torch.float32):
    return (torch.randint(-8, 9, (n,), generator=g).float() / 4).to(dtype)


def _mask(g, n, seq, p_on=0.8, false_rows=()):
    m = torch.rand(n, seq, generator=g) < p_on
    for r in false_rows:
        m[r] = False
    return m


def adv_cases(ref, g):
    A = ref.advantages.compute_grpo_dynamic_advantages
    cases = {}
    spec = {
        # name: (ids builder, group_size, seq_len, mode, dtype, extra)
        "turn_sorted": (lambda: _ids(g, 8), 4, 37, "turn", torch.float32, {}),
        "traj_sorted": (lambda: _ids(g, 8), 4, 37, "trajectory", torch.float32, {}),
        "turn_unsorted": (lambda: _ids(g, 12, shuffle=True), 4, 29, "turn", torch.float32, {}),
        "traj_unsorted": (lambda: _ids(g, 12, shuffle=True), 4, 29, "trajectory", torch.float32, {}),
        "traj_empty": (lambda: [0, 0, 1, 3, 3], 2, 9, "trajectory", torch.float32, {}),
        "turn_empty": (lambda: [0, 0, 1, 3, 3], 2, 9, "turn", torch.float32, {}),
        "traj_empty_g4": (lambda: _ids(g, 8, shuffle=True, empty=(2, 5)), 4, 16, "trajectory", torch.float32, {}),
        "turn_single_turn_question": (lambda: [2, 0, 3, 3, 4, 5, 5], 2, 11, "turn", torch.float32, {}),
        "traj_single_group_member": (lambda: _ids(g, 5, shuffle=True), 1, 7, "trajectory", torch.float32, {}),
        "turn_all_false_row": (lambda: _ids(g, 8), 2, 13, "turn", torch.float32, {"false_rows": (0, 3)}),
        "turn_identical_group": (lambda: _ids(g, 8), 4, 10, "turn", torch.float32, {"same_q0": 0.5}),
        "traj_identical_group": (lambda: _ids(g, 8), 4, 10, "trajectory", torch.float32, {"same_q0": 0.5}),
        "turn_bf16": (lambda: _ids(g, 8, shuffle=True), 4, 21, "turn", torch.bfloat16, {}),
        "traj_bf16": (lambda: _ids(g, 8, shuffle=True), 4, 21, "trajectory", torch.bfloat16, {}),
        "turn_default_mode": (lambda: _ids(g, 4), 2, 5, None, torch.float32, {}),
        "turn_g16": (lambda: _ids(g, 32, shuffle=True), 16, 33, "turn", torch.float32, {}),
    }
    for name, (ids_fn, G, seq, mode, dtype, extra) in spec.items():
        ids = ids_fn()
        n = len(ids)
        r = _rewards(g, n, dtype)
        if "same_q0" in extra:
            for i, t in enumerate(ids):
                if t // G == 0:
                    r[i] = extra["same_q0"]
        mask = _mask(g, n, seq, false_rows=extra.get("false_rows", ()))
        kw = dict(rewards=r.reshape(n, 1), loss_mask=mask.transpose(0, 1).contiguous(), group_size=G, idx_to_traj=ids)
        if mode is not None:
            kw["advantage_mode"] = mode
        adv, ret = A(**kw)
        assert ret is None and adv.dtype == dtype and adv.shape == (seq, n)
        cases[name] = dict(kw, advantages=adv)
    return cases


def dispatch_cases(ref, g):
    cases = {}
    for name, (num_traj, G, seq, mode, shuffle) in {
        "turn": (16, 4, 19, "turn", True),
        "trajectory": (16, 4, 19, "trajectory", True),
        "trajectory_g8": (16, 8, 64, "trajectory", False),
    }.items():
        ids = _ids(g, num_traj, shuffle=shuffle)
        n = len(ids)
        r, mask = _rewards(g, n), _mask(g, n, seq)
        kw = dict(task_type="reasoning", adv_type="grpo_dynamic", advantage_mode=mode, rewards=r, loss_mask=mask,
                  num_sequence=n, group_size=G, idx_to_traj=ids, kl_beta=0.0, kl_penalty_type="low_var_kl", logprob=None,
                  ref_logprob=None, use_reinpp_baseline=False)
        adv, ret = ref.registry.calculate_adv_and_returns(**kw)
        assert ret is None and adv.is_contiguous() and adv.shape == (n, seq)
        cases[name] = dict(kw, advantages=adv)
    return cases


def _batch(g, num_traj, G, seq, agents_max, false_rows=0, adv_dtype=torch.float32):
    """A dynamic batch; `false_rows` rows get an all-False mask, each the first row of a (trajectory, agent) group that has
    other rows, so that the group keeps some tokens."""
    ids = _ids(g, num_traj, shuffle=True)
    n = len(ids)
    sub = torch.randint(0, agents_max, (n,), generator=g)
    groups = {}
    for i, key in enumerate(zip(ids, sub.tolist())):
        groups.setdefault(key, []).append(i)
    picked = [rows[0] for rows in groups.values() if len(rows) > 1][:false_rows]
    assert len(picked) == false_rows
    mask = _mask(g, n, seq, p_on=0.6, false_rows=picked)
    adv = (torch.randn(n, seq, generator=g) * mask).to(adv_dtype)
    return dict(idx_to_traj=ids, **{"extra:idx_to_sub_traj": sub}, response_mask=mask, advantages=adv,
                loss_scales=torch.ones_like(adv).masked_fill(~mask, 0))


def scale_cases(ref, ls, g):
    reg = ref.registry
    cases = {}
    for name, (chain, num_traj, G, seq, agents_max, false_rows, agbs, dp) in {
        "group": (["group_level"], 8, 4, 23, 3, 0, 512 * 4 / 3, 2),
        "group_agent": (["group_level", "agent_level"], 8, 4, 23, 3, 2, 64.0, 1),
        "group_agent_turn": (["group_level", "agent_level", "turn_level"], 12, 4, 37, 3, 2, 512 * 4 / 3, 2),
        "group_agent_turn_one_agent": (["group_level", "agent_level", "turn_level"], 8, 4, 41, 1, 1, 24.0, 1),
        "group_agent_turn_ragged": (["group_level", "agent_level", "turn_level"], 16, 4, 7, 5, 3, 100.0 / 7, 4),
    }.items():
        batch = _batch(g, num_traj, G, seq, agents_max, false_rows)
        inputs = {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch.items()}
        context = {"folding_scale": [], "enable_scale_of_group": False, "actor_global_batch_size": agbs,
                   "data_parallel_world_size": dp}
        for fn in reg.get_loss_scales(chain):
            batch = fn(context, batch)
        cases[name] = dict(chain=chain, context=dict(actor_global_batch_size=agbs, data_parallel_world_size=dp),
                           inputs=inputs, advantages=batch["advantages"], loss_scales=batch["loss_scales"],
                           folding_scale=list(context["folding_scale"]))
    return cases


def _err(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001
        return dict(type=type(e).__name__, message=str(e))
    raise AssertionError("the reference accepted these inputs")


def error_cases(ref, ls, g):
    A = ref.advantages.compute_grpo_dynamic_advantages
    m = torch.ones(4, 5, dtype=torch.bool)
    out = {
        "size_mismatch": _err(lambda: A(rewards=torch.zeros(4, 1), loss_mask=m, group_size=2, idx_to_traj=[0, 0, 1, 1, 1])),
        "not_divisible": _err(lambda: A(rewards=torch.zeros(5, 1), loss_mask=m, group_size=2, idx_to_traj=[0, 0, 1, 2, 2])),
        "invalid_mode": _err(lambda: A(rewards=torch.zeros(5, 1), loss_mask=m, group_size=2, idx_to_traj=[0, 0, 1, 1, 1],
                                       advantage_mode="token")),
    }
    batch = _batch(g, 4, 2, 9, 2)
    ctx = lambda f: {"folding_scale": list(f), "actor_global_batch_size": 8.0}  # noqa: E731
    out["agent_before_group"] = _err(lambda: ls.agent_scale(ctx([]), batch))
    out["group_twice"] = _err(lambda: ls.group_scale(ctx(["group_level"]), batch))
    out["turn_before_agent"] = _err(lambda: ls.turn_scale(ctx(["group_level"]), batch))
    out["agent_twice"] = _err(lambda: ls.agent_scale(ctx(["group_level", "agent_level"]), batch))
    out["turn_twice"] = _err(lambda: ls.turn_scale(ctx(["group_level", "agent_level", "turn_level"]), batch))
    out["unknown_scale"] = _err(lambda: ref.registry.get_loss_scales(["group_level", "Turn_Level"]))
    zero = _batch(g, 4, 2, 9, 1)
    first = [i for i, t in enumerate(zero["idx_to_traj"]) if t == zero["idx_to_traj"][0]]
    zero["response_mask"][first] = False  # every row of one (trajectory, agent) group has no response token
    out["turn_zero_total"] = _err(lambda: ls.turn_scale(ctx(["group_level", "agent_level"]), zero))
    return out


def main():
    ref = RL.load()
    ls = load_loss_scales()
    g = torch.Generator().manual_seed(20261015)
    data = dict(adv=adv_cases(ref, g), dispatch=dispatch_cases(ref, g), scale=scale_cases(ref, ls, g),
                errors=error_cases(ref, ls, g))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(data, OUT)
    print(f"wrote {OUT}: " + ", ".join(f"{k} {len(v)}" for k, v in data.items()))


if __name__ == "__main__":
    main()
