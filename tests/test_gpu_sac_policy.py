"""The SAC (Q-head) MLP policy on the GPU (csrc/sac_mlp.hip behind rlinf_amd/models/embodiment/sac_mlp_policy.py) against the
reference's own torch ``MLPPolicy(add_q_head=True)`` on the CPU (the staged files, through oracle.reference_loader).

Every comparison is against the reference run in FLOAT64.  The bound is four times the deviation of the reference's own FLOAT32
run from that float64 run on the same inputs, computed here (factor 4: another summation order across the 256-wide reductions and
another tanh / exp), with a floor of 1e-6 * max|x| for outputs (max-norm) and 1e-6 * ||g|| for gradients (2-norm, per tensor).
It is measured on the reference, never on the code under test.  Each comparison prints the reference's deviation and ours.

Measured on an MI355X (4863 comparisons; profiles/sac_mlp_tolerance_table.txt): all hold.  The tensors of one or two elements at
M = 1 are the tight ones: there the bound is four times ONE draw of the reference's rounding error, which can come out several
times below the reference's deviation on the neighbouring cases.  The kernels therefore keep their own error well below the
reference's float32 run where that is cheap (f64 tanh, LayerNorm statistics, head outputs and distribution epilogue; 32-deep MFMA
chains added up instead of one 128-step chain per output).

The HIP side of each group of cases runs in a child process with a time limit of its own (tests/helpers/sac_gpu_child.py): a
child that is killed by a signal or runs into its limit fails its tests, and no further child is started.
"""

import os
import subprocess
import sys
import tempfile

import pytest
import torch

from conftest import ROOT
from helpers import sac_cases as SC
from oracle import reference_loader as RL

pytestmark = pytest.mark.gpu

LIMITS = {"cases": 240, "calls": 90, "loop": 90}  # seconds; a cold start (import, HIP initialisation) is most of each
_RAN, _FAULT = {}, None


def _child(group):
    global _FAULT
    if group in _RAN:
        rec = _RAN[group]
    elif _FAULT is not None:
        pytest.fail(f"not started: {_FAULT}")
    else:
        rec = {}
        with tempfile.TemporaryDirectory(prefix="sac_gpu_") as d:
            path = os.path.join(d, group + ".pt")
            cmd = [sys.executable, os.path.join(ROOT, "tests", "helpers", "sac_gpu_child.py"), group, path]
            try:
                r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=LIMITS[group])
                if r.returncode != 0:
                    rec["error"] = f"child '{group}' ended with status {r.returncode}:\n{r.stderr[-2000:]}"
                    if r.returncode < 0 or r.returncode in (134, 139):
                        _FAULT = rec["error"]
                else:
                    rec["res"] = torch.load(path, weights_only=False)
            except subprocess.TimeoutExpired:
                rec["error"] = _FAULT = f"child '{group}' ran into its time limit of {LIMITS[group]} s"
        _RAN[group] = rec
    if "error" in rec:
        pytest.fail(rec["error"])
    return rec["res"]


@pytest.fixture(scope="module")
def ref():
    return RL.load().mlp_policy


_REF = {}


def _reference(key, fn, ref, *args):
    """The reference's float64 and float32 runs of one group, computed once and shared."""
    if key not in _REF:
        _REF[key] = tuple(fn(ref.MLPPolicy, ref.ForwardType, torch.device("cpu"), dt, *args) for dt in (torch.float64, torch.float32))
    return _REF[key]


def _check(where, name, ours, r64, r32, kind):
    """kind 'out': max-norm, floor 1e-6 max|x|; 'grad': 2-norm, floor 1e-6 ||g||."""
    assert ours.shape == r64.shape, f"{where} {name}: shape {tuple(ours.shape)} != {tuple(r64.shape)}"
    if r64.numel() == 0:
        return
    if kind == "out":
        norm, floor = (lambda t: t.abs().max().item()), 1e-6 * r64.abs().max().item()
    else:
        norm, floor = (lambda t: t.norm().item()), 1e-6 * r64.norm().item()
    ref_dev, our_dev = norm(r32 - r64), norm(ours - r64)
    bound = max(4 * ref_dev, floor)
    print(f"SACTOL {where:28s} {name:44s} ref32-ref64 {ref_dev:.3e}  ours-ref64 {our_dev:.3e}  bound {bound:.3e}")
    assert our_dev <= bound, f"{where} {name}: ours-ref64 {our_dev:.3e} > bound {bound:.3e} (ref32-ref64 {ref_dev:.3e})"


def _triple(group, key, fn, ref, *args):
    ours = _child(group)[key]
    r64, r32 = _reference((group, key), fn, ref, *args)
    assert sorted(ours) == sorted(r64), "the HIP module and the reference returned different sets of results"
    return ours, r64, r32


CASES = SC.all_cases()
IDS = [SC.case_id(*c) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_actor_forward(ref, case):
    """action everywhere; logprob where it is well conditioned: the 1e-6 floor inside the log makes it ill-conditioned once
    1 - a_n^2 < 1e-3 (judged on the float64 reference; the reference's own f32 run is off by up to 0.06 there)."""
    cid = SC.case_id(*case)
    ours, r64, r32 = _triple("cases", cid, SC.run_case, ref, *case)
    for suffix in ("", ".nograd"):
        _check(cid, "action" + suffix, ours["action" + suffix], r64["action"], r32["action"], "out")
        keep = (1 - r64["action"] ** 2) >= 1e-3  # action_scale 1, action_bias 0: the action is a_n
        excluded = 1 - keep.double().mean().item()
        print(f"SACTOL {cid:28s} logprob{suffix}: excluded share {excluded:.4f}")
        assert excluded <= 0.10
        _check(cid, "logprob" + suffix, ours["logprob" + suffix][keep], r64["logprob"][keep], r32["logprob"][keep], "out")
    assert torch.equal(ours["action"], ours["action.nograd"]) and torch.equal(ours["logprob"], ours["logprob.nograd"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_q_forward(ref, case):
    cid = SC.case_id(*case)
    ours, r64, r32 = _triple("cases", cid, SC.run_case, ref, *case)
    (D, A, C), m, _ = case
    assert ours["q/action_level"].shape == (m, 2 * C) and ours["q/chunk_level"].shape == (m, 2)
    for name in ("q/action_level", "q/chunk_level"):
        _check(cid, name, ours[name], r64[name], r32[name], "out")
    _check(cid, "q.nograd/action_level", ours["q.nograd/action_level"], r64["q/action_level"], r32["q/action_level"], "out")
    assert torch.equal(ours["q/action_level"], ours["q.nograd/action_level"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward(ref, case):
    """The critic, actor (through sac_q_forward(actions=pi) into the actor) and alpha losses: every parameter's gradient and
    d_actions; gradients of parameters a loss does not reach are None or zero exactly as the reference gives them."""
    cid = SC.case_id(*case)
    ours, r64, r32 = _triple("cases", cid, SC.run_case, ref, *case)
    for name in sorted(ours):
        if name.startswith(("action", "logprob", "q/", "q.")):
            continue
        tag, _, rest = name.partition("/")
        if tag.endswith(".none"):
            # None on the reference: ours is None or zero; a gradient on the reference: ours has one
            if r64[name].item() == 1.0:
                assert ours[name].item() == 1.0 or ours[tag[:-5] + "/" + rest].abs().max().item() == 0.0, name
            else:
                assert ours[name].item() == 0.0, f"{cid} {name}: the reference has a gradient, the HIP module gave None"
        elif rest in ("loss", "entropy"):
            _check(cid, name, ours[name], r64[name], r32[name], "out")
        else:
            _check(cid, name, ours[name], r64[name], r32[name], "grad")


def test_no_stale_weights(ref):
    ours, r64, r32 = _triple("calls", "stale", SC.run_stale, ref)
    for name in sorted(ours):
        if "logprob" in name:
            keep = (1 - r64[name.replace("logprob", "action")] ** 2) >= 1e-3
            _check("stale", name, ours[name][keep], r64[name][keep], r32[name][keep], "out")
        else:
            _check("stale", name, ours[name], r64[name], r32[name], "out")
    for what in ("q_target", "q_online", "action"):  # the updates were large enough to see
        assert (r64[f"after/{what}"] - r64[f"before/{what}"]).abs().max() > 1e-3


def test_predict_action_batch(ref):
    ours, r64, r32 = _triple("calls", "predict", SC.run_predict, ref)
    for mode in ("train", "eval"):
        assert ours[f"{mode}/keys"] == r64[f"{mode}/keys"]
        assert ours[f"{mode}/chunk_actions"].shape == (67, 2, 7)
        assert torch.equal(ours[f"{mode}/prev_values"], torch.zeros(67, 1, dtype=torch.float64))
        assert torch.equal(ours[f"{mode}/action"], ours[f"{mode}/model_action"])
        assert torch.equal(ours[f"{mode}/states"], r32[f"{mode}/states"])
        keep = (1 - r64[f"{mode}/action"] ** 2) >= 1e-3
        for name in ("chunk_actions", "action", "prev_values"):
            _check("predict", f"{mode}/{name}", ours[f"{mode}/{name}"], r64[f"{mode}/{name}"], r32[f"{mode}/{name}"], "out")
        name = f"{mode}/prev_logprobs"
        _check("predict", name, ours[name][keep], r64[name][keep], r32[name][keep], "out")


def test_five_step_loop(ref):
    ours, r64, r32 = _triple("loop", "loop", SC.run_loop, ref)
    for name in sorted(ours):
        _check("loop", name, ours[name], r64[name], r32[name], "out" if name.endswith("losses") else "grad")
