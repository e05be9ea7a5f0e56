"""Offline IQL on the GPU (csrc/iql_mlp.hip behind rlinf_amd/models/embodiment/iql_mlp.py and the learner
rlinf_amd/workers/actor/fsdp_iql_policy_worker.py) against the plain-torch restatement tests/helpers/iql_torch.py on the CPU.  The
reference's IQL files are not on the GPU machine; tests/test_iql_restatement_vs_reference.py pins the restatement to them bit for
bit where they exist, and tests/golden/iql_step.pt (recorded from the real reference) pins it on this machine.

Every comparison is against the restatement run in FLOAT64.  The bound is four times the deviation of the restatement's own
FLOAT32 run from that float64 run on the same inputs, with a floor of 1e-6 * max|x| for outputs (max-norm) and 1e-6 * ||g|| for
gradients and parameters (2-norm, per tensor).  It is measured on the restatement, never on the code under test.  Each comparison
prints both deviations (profiles/iql_tolerance_table.txt).  The eight metrics of the 5-step loop are compared per metric as the
vector of its five values: one metric of one step is a single draw of the float32 run's rounding error, which can come out many
times below its neighbours', and the five steps of one quantity have one scale.

The HIP side of each group runs in a child process with a time limit of its own (tests/helpers/iql_gpu_child.py): a child that is
killed by a signal or runs into its limit fails its tests, and no further child is started.
"""

import os
import subprocess
import sys
import tempfile

import pytest
import torch

from conftest import ROOT
from helpers import iql_cases as C
from helpers import iql_torch as T

pytestmark = pytest.mark.gpu

LIMITS = {"kernels": 240, "learner": 120}  # seconds; a cold start (import, HIP initialisation) is most of each
_RAN, _FAULT = {}, None


def _child(group):
    global _FAULT
    if group in _RAN:
        rec = _RAN[group]
    elif _FAULT is not None:
        pytest.fail(f"not started: {_FAULT}")
    else:
        rec = {}
        with tempfile.TemporaryDirectory(prefix="iql_gpu_") as d:
            path = os.path.join(d, group + ".pt")
            cmd = [sys.executable, os.path.join(ROOT, "tests", "helpers", "iql_gpu_child.py"), group, path]
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


_REF = {}


def _reference(key, fn, *args):
    """The restatement's float64 and float32 runs of one case, computed once and shared."""
    if key not in _REF:
        _REF[key] = tuple(fn(*args, dt) for dt in (torch.float64, torch.float32))
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
    print(f"IQLTOL {where:24s} {name:34s} ref32-ref64 {ref_dev:.3e}  ours-ref64 {our_dev:.3e}  bound {bound:.3e}")
    assert our_dev <= bound, f"{where} {name}: ours-ref64 {our_dev:.3e} > bound {bound:.3e} (ref32-ref64 {ref_dev:.3e})"


CASES = C.all_cases()
IDS = [C.case_id(*c) for c in CASES]


def _triple(case):
    cid = C.case_id(*case)
    r64, r32 = _reference(("case", cid), C.ref_case, *case)
    return cid, _child("kernels")[cid], r64, r32


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forwards(case):
    """All three kinds; saved activations or not is bit-equal; the value net over obs || next_obs in one launch is the two calls."""
    cid, ours, r64, r32 = _triple(case)
    for name in ("fwd/actor_mean", "fwd/value", "fwd/value_next", "fwd/critic"):
        _check(cid, name, ours[name], r64[name], r32[name], "out")
    for name in ("fwd/actor_mean", "fwd/value", "fwd/critic", "fwd/logprob"):
        assert torch.equal(ours[name], ours[name + ".saved"]), name
    assert torch.equal(ours["fwd/actor_mean"], ours["fwd/actor_mean.nolp"])
    assert torch.equal(ours["fwd/value_cat"], torch.cat([ours["fwd/value"], ours["fwd/value_next"]]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_actor_logprob(case):
    """Rows with every |a| <= 1 - 1e-3 under the bound; the others (the clamp constant differs between float32 and float64 there, by
    1.3e-2 in the log-prob) separately under their own bound: the same rule applied to those rows."""
    cid, ours, r64, r32 = _triple(case)
    shape, m, _ = case
    actions = T.make_batch(shape, m)["actions"]
    keep = (actions.abs() <= 1 - 1e-3).all(-1)
    excluded = 1 - keep.double().mean().item()
    print(f"IQLTOL {cid:24s} logprob: excluded share {excluded:.4f}")
    assert excluded <= 0.10
    if m >= 32:
        assert (actions == 1.0).any() and (actions == -1.0).any() and not keep.all()
    _check(cid, "fwd/logprob[kept]", ours["fwd/logprob"][keep], r64["fwd/logprob"][keep], r32["fwd/logprob"][keep], "out")
    if not keep.all():
        _check(cid, "fwd/logprob[excluded]", ours["fwd/logprob"][~keep], r64["fwd/logprob"][~keep], r32["fwd/logprob"][~keep], "out")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backwards(case):
    """Every parameter's gradient from seeded upstream gradients; the actor's through the log-prob, d actor_logstd included."""
    cid, ours, r64, r32 = _triple(case)
    names = [n for n in r64 if n.startswith("grad/")]
    assert sorted(n for n in ours if n.startswith("grad/")) == sorted(names) and len(names) == 9 + 6 + 12
    for name in names:
        _check(cid, name, ours[name], r64[name], r32[name], "grad")
    if case[2] == "logstd":  # 2.5 and -5.5 lie outside the clamp range: no gradient; exactly 2.0 is inside (clamp's gradient is inclusive)
        g = ours["grad/actor/actor_logstd"][0]
        assert g[0] == 0 and g[1] == 0 and g[2] != 0 and r64["grad/actor/actor_logstd"][0, 2] != 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loss_legs(case):
    cid, ours, r64, r32 = _triple(case)
    shape, m, _ = case
    a, b = C.aux(shape, m), T.make_batch(shape, m)
    if m >= 2:
        diff = torch.min(a["q_target"][0], a["q_target"][1]) - a["v"]
        assert (diff < 0).any() and (diff > 0).any()
    assert (torch.exp((a["q_min"] - a["new_v"]) * 3.0) > 100).any()
    if m >= 32:
        assert (b["masks"] == 0).any() and (b["masks"] == 1).any()
    assert torch.equal(ours["loss/value/q_min"], r64["loss/value/q_min"])
    for name in ("loss/value/d_v", "loss/actor/d_lp", "loss/critic/d_q"):
        _check(cid, name, ours[name], r64[name], r32[name], "out")
    for name, parts in (("loss/value/metrics", ("value_loss", "v")), ("loss/actor/metrics", ("actor_loss", "adv_mean")),
                        ("loss/critic/metrics", ("critic_loss", "q1", "q2"))):
        for i, part in enumerate(parts):
            _check(cid, f"{name}[{part}]", ours[name][i:i + 1], r64[name][i:i + 1], r32[name][i:i + 1], "out")
    if m == 1:  # Bessel's correction: torch gives NaN, and so must the kernel
        assert torch.isnan(r64["loss/actor/adv_std"]).all() and torch.isnan(ours["loss/actor/adv_std"]).all()
    else:
        _check(cid, "loss/actor/adv_std", ours["loss/actor/adv_std"], r64["loss/actor/adv_std"], r32["loss/actor/adv_std"], "out")


def test_soft_update_and_adam():
    """rlx_soft_update, and rlx_clip_adamw_step as the learner drives it (weight_decay 0, no clip, three slabs summed, the step count
    on the device) against torch.optim.Adam and torch's _foreach soft update on the CPU."""
    ours = _child("kernels")["optim"]
    (r64, _), (r32, _) = _reference(("optim",), lambda dt: C.ref_optim(dt))
    for name in sorted(r64):
        _check("optim", name, ours[name], r64[name], r32[name], "grad")


def _golden_check(m, r64):
    g = torch.load(os.path.join(ROOT, "tests", "golden", "iql_step.pt"), weights_only=False)[f"m{m}"]
    rel = lambda a, b: (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)  # noqa: E731
    assert rel(r64["metrics"], g["metrics"]) <= 1e-9 and rel(r64["lr_actor"], g["lr_actor"]) <= 1e-15
    for name, probe in g["params"].items():
        assert rel(C.probe(r64[name], name), probe) <= 1e-9, name


@pytest.mark.parametrize("m", (32, 67))
def test_five_step_loop(m):
    """5 updates of the learner at (17, 6): the four parameter sets, the target, the eight metrics and lr_actor per step."""
    ours = _child("learner")[f"loop-m{m}"]
    r64, r32 = _reference(("loop", m), lambda dt: C.ref_loop(m, dt))
    _golden_check(m, r64)  # the restatement's float64 run on this machine is the recorded run of the real reference
    assert sorted(ours) == sorted(r64)
    for name in sorted(r64):
        if name == "metrics":
            for i, metric in enumerate(T.METRICS):
                _check(f"loop-m{m}", f"metrics[{metric}]", ours[name][:, i], r64[name][:, i], r32[name][:, i], "out")
        elif name == "lr_actor":
            assert ((ours[name] - r64[name]).abs() <= 1e-15 * r64[name].abs()).all(), (ours[name], r64[name])
        else:
            _check(f"loop-m{m}", name, ours[name], r64[name], r32[name], "grad")
    assert r64["lr_actor"][0] != r64["lr_actor"][4]


def test_run_training_resumes_bit_equal():
    """3 calls x 4 steps on a synthetic data set, checkpoint, reload into a new learner, one more call == 16 steps uninterrupted."""
    res = _child("learner")["run_training"]
    assert [r["__global_step"] for r in res["a/results"]] == [4, 8, 12, 16] == [r["__global_step"] for r in res["b/results"]]
    assert res["a/results"] == res["b/results"]
    keys = [k[2:] for k in res if k.startswith("a/") and k != "a/results"]
    assert len(keys) == 4 + 9
    for k in keys:
        assert torch.equal(res["a/" + k], res["b/" + k]), k
    assert all(res[f"a/{n}/steps"].sum().item() == 16 for n in ("actor", "value", "critic"))
    for key in T.METRICS + ("lr_actor", "lr_value", "lr_critic"):
        assert key in res["a/results"][0]
