"""The fused-step parity tests once more under the exact-f32 MFMA form (step::Form::F32: ppo_step_f32.hip, its plan in plan_step, its
weight image and the optimizer's refresh of it), which RLX_F32_EXACT_MFMA=1 selects once per process -- so no in-process test can
reach it.  One fresh child process per group (tests/helpers/exact_f32_child.py, started with the switch set) calls the existing test
functions over their non-bf16 parameter sets, assertions and bars verbatim, plus the plan edges only this form has, and leaves one
result line per case; every test_exact_f32[...] below only reads its line.

Child time limits: three times (the same cases in-process, where they run as F32X, summed per group from pytest --durations=0, + the
start-up of an empty child), rounded up to the next 30 s -- the project's bench puts the exact form at about 1.25 x F32X and shared
boxes vary by 12-18 %.  Measured on one MI355X:

    group       F32X in-process   + start-up 2.2 s   x 3      limit   child wall time (exact form)
    rollout     1.52 s            3.7 s              11.2 s   30 s    4.1 s
    step        2.80 s            5.0 s              15.0 s   30 s    5.4 s
    optimizer   2.47 s            4.7 s              14.0 s   30 s    4.9 s
    loop        0.61 s            2.8 s               8.4 s   30 s    5.0 s

(The step group's 2.80 s: 1.64 s for the existing functions + 1.16 s for the twenty plan-edge cases run in-process with F32X's own slab
counts.)  A child killed at its limit counts as hung unless its per-case seconds show steady progress; then split the group.
"""

import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import pytest

from conftest import ROOT
from helpers import exact_f32_child as X

LIMITS = {"rollout": 30, "step": 30, "optimizer": 30, "loop": 30}  # seconds per child (the table above)
EXPECTED = {"rollout": 17, "step": 44, "optimizer": 10, "loop": 6}
CASE_IDS = [c.id for g in X.GROUPS for c in X.cases(g)]

_RAN = {}      # group -> what its child left
_FAULT = None  # set once an exact-f32 child ended by a non-assertion exception, a signal, a non-zero exit or its time limit: names the
               # child and the case that ended it; no further child is started and nothing retries


def _run_child(group):
    global _FAULT
    if group in _RAN:
        return _RAN[group]
    rec = dict(facts=None, results={}, order=[], wall=None, ended=None)
    _RAN[group] = rec
    if _FAULT is not None:
        rec["ended"] = f"not started: {_FAULT}"
        return rec
    with tempfile.TemporaryDirectory(prefix="exact_f32_") as d:
        out = os.path.join(d, group + ".jsonl")
        cmd = [sys.executable, os.path.join(ROOT, "tests", "helpers", "exact_f32_child.py"), group, out]
        t0, how, tail = time.time(), None, ""
        try:
            r = subprocess.run(cmd, env=dict(os.environ, RLX_F32_EXACT_MFMA="1"), cwd=ROOT, capture_output=True, text=True,
                               timeout=LIMITS[group])
            tail = r.stderr[-1500:]
            if r.returncode != 0:
                how = f"signal {-r.returncode}" if r.returncode < 0 else f"exit status {r.returncode}"
        except subprocess.TimeoutExpired as e:
            how = f"its time limit of {LIMITS[group]} s"
            tail = (e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or ""))[-1500:]
        rec["wall"] = time.time() - t0
        if os.path.exists(out):
            with open(out) as f:
                for line in f:
                    try:
                        row = json.loads(line)
                    except ValueError:  # a line cut short by the child's end
                        continue
                    if "facts" in row:
                        rec["facts"] = row
                    else:
                        rec["results"][row["id"]] = row
                        rec["order"].append(row["id"])
    print(f"[exact-f32 child {group}] {len(rec['results'])} cases in {rec['wall']:.1f} s (limit {LIMITS[group]} s)"
          + (f", start-up {rec['facts']['startup_seconds']} s" if rec["facts"] else ""))
    if how is not None:
        ids = [c.id for c in X.cases(group)]
        errs = [i for i in rec["order"] if rec["results"][i]["outcome"] == "error"]
        at = errs[0] if errs else next((i for i in ids if i not in rec["results"]), "its teardown")
        rec["ended"] = _FAULT = f"the exact-f32 child '{group}' was ended by {how} at {at}; stderr: ...{tail}"
    return rec


@pytest.fixture(scope="session")
def exact_children():
    """group -> what that group's child left; a child runs at most once per session."""
    return _run_child


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_exact_f32(case_id, exact_children):
    rec = exact_children(case_id.split("::")[0])
    row = rec["results"].get(case_id)
    if row is None:
        pytest.fail(rec["ended"] or f"the child left no line for {case_id}", pytrace=False)
    print(f"[exact-f32] {case_id}: {row['outcome']} in {row['seconds']} s")
    if row["outcome"] != "passed":
        pytest.fail(f"{row['outcome']} under RLX_F32_EXACT_MFMA=1: {row['message']}"
                    + (f"\n{rec['ended']}" if row["outcome"] == "error" else ""), pytrace=False)


@pytest.mark.gpu
def test_the_children_ran_the_exact_form(exact_children):
    """A child that silently ran F32X would make this module pass while testing nothing new.  The f32 image of Form::F32 is 4 bytes
    per weight, exactly twice the bf16 image (the F32X image, three bf16 planes, is not); its plan allows 2 * num_cu / 20 slabs at
    6400 rows (25 at most: 256 rows per slab), F32X's ring plan fewer."""
    from rlinf_amd import _lib
    from rlinf_amd.models.embodiment.mlp_policy import MLPPolicy
    lib, lay = _lib.load(), MLPPolicy(42, 8, 1, True, False).layout
    cu, wave = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.rlx_device_info(ctypes.byref(cu), ctypes.byref(wave)) == 0
    here_f32, here_bf16 = lib.rlx_mlp_tiles_bytes_for(ctypes.byref(lay), 0), lib.rlx_mlp_tiles_bytes_for(ctypes.byref(lay), 1)
    here_slabs = lib.rlx_ppo_step_slabs_for(ctypes.byref(lay), X.FACTS_M, 0)
    assert here_f32 != 2 * here_bf16, "this process runs the exact form itself (RLX_F32_EXACT_MFMA is set): nothing to tell apart"
    for group in X.GROUPS:
        rec = exact_children(group)
        assert rec["facts"] is not None, rec["ended"] or f"the child '{group}' wrote no facts line"
        f = rec["facts"]["facts"]
        assert f["tiles_bytes_bf16"] == here_bf16 and f["tiles_bytes_f32"] == 2 * f["tiles_bytes_bf16"], (group, f)
        assert f["num_cu"] == cu.value, (group, f, cu.value)
        assert f["slabs_f32"] == min(2 * cu.value // 20, 25), (group, f, cu.value)
        assert f["slabs_f32"] != here_slabs, (group, f, here_slabs)


@pytest.mark.gpu
def test_every_case_was_reported(exact_children):
    """The ids the children wrote are the ids cases() lists, none missing and none extra, each with an outcome of its own -- and
    none skipped: a skip inside the child hides a case."""
    for group in X.GROUPS:
        rec = exact_children(group)
        want = [c.id for c in X.cases(group)]
        assert rec["order"] == want, (rec["ended"], sorted(set(want) - set(rec["order"])), sorted(set(rec["order"]) - set(want)))
        skipped = [i for i in want if rec["results"][i]["outcome"] == "skipped"]
        assert not skipped, skipped


def test_case_list_is_the_non_bf16_parameter_sets():
    """No GPU: the shared case list holds, for the existing functions, exactly the non-bf16 parameter sets of their own marks."""
    import test_gpu_fused_step as F
    import test_gpu_mlp_shapes as S
    assert CASE_IDS and len(set(CASE_IDS)) == len(CASE_IDS)
    for group in X.GROUPS:
        cs = X.cases(group)
        assert len(cs) == EXPECTED[group], (group, len(cs))
        assert all(c.id.startswith(group + "::") for c in cs)
        assert all(c.kwargs.get("prec", "f32") == "f32" and c.kwargs.get("bf16", False) is False for c in cs)
    by_fn = {}
    for group in X.GROUPS:
        for c in X.cases(group):
            by_fn.setdefault(c.fn.__name__, []).append(c.kwargs)
    n_shapes, n_lds = len(S.SHAPES), len(S.LDS_SHAPES)
    assert {k: len(v) for k, v in by_fn.items()} == {
        "test_rollout_step_shapes": n_shapes, "test_rollout_step_policy_and_value_jobs": 4,
        "test_outputs_do_not_depend_on_stale_lds": n_lds, "test_ppo_step_shapes": n_shapes,
        "test_ppo_step_gradients_and_metrics_vs_oracle": 4, "test_ppo_step_two_action_chunks": 5,
        "test_ppo_step_decoupled_loss_vs_oracle": 5, "test_ppo_step_matches_unfused_chain": 1,
        "plan_edge_case": len(X.EDGE_SHAPES) * len(X.EDGE_M) * 2, "test_clip_adamw_shapes": n_shapes,
        "test_optimizer_keeps_tile_image_in_step": 1, "test_whole_loop_at_reference_shapes": 6}
    assert [kw["shape"] for kw in by_fn["test_ppo_step_shapes"]] == S.SHAPES
    assert by_fn["test_ppo_step_matches_unfused_chain"] == [{}] and F.test_ppo_step_matches_unfused_chain is not None
