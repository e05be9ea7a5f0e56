"""CPU checks of the "grpo_video" and "raw" advantages: import-time registration (in a fresh interpreter, because another test
of this suite registers and pops its own "raw"), the reference's error texts raised before any device is touched, ext.register()
against stand-in registries with and without the two names, and the learner's forwarding of algorithm.advantage_mode."""

import contextlib
import os
import subprocess
import sys
import types

import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "adv_video_raw.pt")
SEVEN = {"gae", "grpo", "grpo_video", "grpo_dynamic", "reinpp", "opd", "raw"}  # rlinf/algorithms/advantages.py


@pytest.fixture
def builtins_installed():
    """The two names as the package installs them at import time, whatever earlier tests did to the registries; restored after."""
    from rlinf_amd.algorithms import advantages as A
    from rlinf_amd.algorithms import registry as R
    saved = dict(R.ADV_REGISTRY), dict(R._NATIVE_ADV), dict(R._NATIVE_ADV_REASONING)
    R.ADV_REGISTRY["grpo_video"], R.ADV_REGISTRY["raw"] = A.compute_grpo_video_advantages, A.compute_raw_advantages
    R._NATIVE_ADV["grpo_video"], R._NATIVE_ADV["raw"] = A._native_grpo_video, A._native_raw
    R._NATIVE_ADV_REASONING.pop("grpo_video", None)
    R._NATIVE_ADV_REASONING["raw"] = A._native_raw_reasoning
    try:
        yield R
    finally:
        for live, old in zip((R.ADV_REGISTRY, R._NATIVE_ADV, R._NATIVE_ADV_REASONING), saved):
            live.clear()
            live.update(old)


def test_import_registers_all_seven_reference_names_in_a_fresh_interpreter():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from rlinf_amd.algorithms import ADV_REGISTRY, registry as R\n"
            "print(sorted(ADV_REGISTRY)); print(sorted(R._NATIVE_ADV)); print(sorted(R._NATIVE_ADV_REASONING))\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    names, native, native_reasoning = (set(eval(line)) for line in out.stdout.strip().splitlines()[-3:])
    assert {"grpo_video", "raw"} <= names and SEVEN <= names
    assert {"grpo_video", "raw"} <= native
    assert "raw" in native_reasoning and "grpo_video" not in native_reasoning


def _embodied(adv_type, **extra):
    return dict(task_type="embodied", adv_type=adv_type, rewards=torch.rand(2, 4, 1), dones=torch.zeros(3, 4, 1, dtype=torch.bool),
                values=None, gamma=1, gae_lambda=1, group_size=2, reward_type="action_level",
                loss_mask=torch.ones(2, 4, 1, dtype=torch.bool), loss_mask_sum=None, **extra)


@pytest.mark.parametrize("tag,extra", [("mode_none", {"advantage_mode": None}), ("mode_missing", {}),
                                       ("mode_clip", {"advantage_mode": "clip"})])
def test_bad_advantage_mode_raises_the_reference_text_before_any_device_work(builtins_installed, monkeypatch, tag, extra):
    from rlinf_amd.algorithms import advantages as A
    monkeypatch.setattr(A.ops, "grpo_video_adv", None)  # reaching the launch would fail differently
    want = torch.load(GOLDEN, weights_only=False)["errors"][tag]
    with pytest.raises(ValueError) as ei:
        builtins_installed.calculate_adv_and_returns(**_embodied("grpo_video", **extra))
    assert (type(ei.value).__name__, str(ei.value)) == (want["type"], want["message"])
    with pytest.raises(ValueError) as ei:  # the callee contract on [T, B] views
        A.compute_grpo_video_advantages(rewards=torch.rand(2, 4), loss_mask=torch.ones(2, 4, dtype=torch.bool), group_size=2, **extra)
    assert str(ei.value) == want["message"]
    assert want["message"] == f"Unsupported grpo_video advantage_mode: {extra.get('advantage_mode')}"


def test_reasoning_batches_fail_the_way_the_reference_does(builtins_installed):
    gold = torch.load(GOLDEN, weights_only=False)["errors"]
    with pytest.raises(AssertionError, match="Unsupported adv_type grpo_video") as ei:
        builtins_installed.calculate_adv_and_returns(task_type="reasoning", adv_type="grpo_video", rewards=torch.rand(4),
                                                     loss_mask=torch.ones(4, 3, dtype=torch.bool), group_size=2,
                                                     advantage_mode="frame")
    assert str(ei.value) == gold["reasoning_grpo_video"]["message"]
    with pytest.raises(AssertionError, match="Unsupported reward shape") as ei:
        builtins_installed.calculate_adv_and_returns(task_type="reasoning", adv_type="raw", rewards=torch.rand(4, 1),
                                                     loss_mask=torch.ones(4, 3, dtype=torch.bool))
    assert str(ei.value) == gold["reasoning_raw_2d"]["message"]


def test_missing_loss_mask_fails(builtins_installed):
    kw = _embodied("grpo_video", advantage_mode="frame")
    kw["loss_mask"] = None
    with pytest.raises(TypeError, match="loss_mask"):
        builtins_installed.calculate_adv_and_returns(**kw)
    with pytest.raises(TypeError, match="loss_mask"):
        builtins_installed.calculate_adv_and_returns(**dict(kw, adv_type="raw"))


class _StubRegistry(types.ModuleType):
    def __init__(self, name, adv_names):
        super().__init__(name)
        self.ADV_REGISTRY, self.LOSS_REGISTRY = {n: object() for n in adv_names}, {}

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


def _register_with_stub(adv_names):
    from rlinf_amd import ext
    names = ("rlinf", "rlinf.algorithms", "rlinf.algorithms.registry", "rlinf.models")
    before = {n: sys.modules.get(n) for n in names}
    reg = _StubRegistry("rlinf.algorithms.registry", adv_names)
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


def test_ext_register_installs_the_two_names_only_where_rlinf_has_them():
    from rlinf_amd.algorithms import advantages as A
    reg = _register_with_stub(("grpo_video", "raw"))
    assert reg.ADV_REGISTRY["grpo_video"] is A.compute_grpo_video_advantages
    assert reg.ADV_REGISTRY["raw"] is A.compute_raw_advantages
    reg = _register_with_stub(("raw",))
    assert reg.ADV_REGISTRY["raw"] is A.compute_raw_advantages and "grpo_video" not in reg.ADV_REGISTRY
    reg = _register_with_stub(())
    assert "grpo_video" not in reg.ADV_REGISTRY and "raw" not in reg.ADV_REGISTRY and "gae" in reg.ADV_REGISTRY


@pytest.mark.parametrize("mode", ["video", None])
def test_learner_forwards_algorithm_advantage_mode(builtins_installed, mode):
    """EmbodiedFSDPActor._advantages_for hands cfg.algorithm.advantage_mode (None when the config has no such key) to the
    dispatcher, as the reference's learner does (embodied_fsdp_actor_worker.py:310).  A spy registered under "grpo_video" (the
    one name the generic route runs without the device score scan) records what it was given."""
    from rlinf_amd.config import DictConfig
    from rlinf_amd.workers.actor.embodied_fsdp_actor_worker import EmbodiedFSDPActor
    seen = {}

    @builtins_installed.register_advantage("grpo_video")
    def spy(rewards, loss_mask, group_size, **kwargs):
        seen.update(kwargs, group_size=group_size, shape=tuple(rewards.shape))
        return torch.zeros_like(rewards), None

    alg = dict(adv_type="grpo_video", group_size=2, reward_type="action_level")
    if mode is not None:
        alg["advantage_mode"] = mode
    me = types.SimpleNamespace(cfg=DictConfig(dict(runner=dict(task_type="embodied"), algorithm=alg)),
                               timer=lambda name: contextlib.nullcontext(), use_training_pipeline=False)
    batch = dict(rewards=torch.rand(3, 4, 2), dones=torch.zeros(4, 4, 2, dtype=torch.bool),
                 loss_mask=torch.ones(3, 4, 2, dtype=torch.bool))
    assert EmbodiedFSDPActor._advantages_for(me, batch, metrics=False) is None
    assert "advantage_mode" in seen and seen["advantage_mode"] == mode
    assert seen["group_size"] == 2 and seen["shape"] == (6, 4) and "normalize_advantages" not in seen
    assert tuple(batch["advantages"].shape) == (3, 4, 2)


def test_golden_fixture_covers_the_issue_cases():
    d = torch.load(GOLDEN, weights_only=False)
    video = d["video"]
    assert {k.rsplit("_", 1)[1] for k in video} == {"frame", "video"}
    kws = [c["kwargs"] for c in video.values()]
    assert {1, 2, 3, 8, 16} <= {k["group_size"] for k in kws}
    assert {1, 2, 5, 16} <= {k["rewards"].shape[2] for k in kws}
    assert {"action_level", "chunk_level"} == {k["reward_type"] for k in kws}
    masks = [k["loss_mask"] for k in kws + [c["kwargs"] for c in d["raw"].values()] + [c["kwargs"] for c in d["reasoning"].values()]]
    assert any(not m.any() for m in masks) and any(int(m.sum()) == 1 for m in masks) and any(m.all() for m in masks)
    assert torch.isnan(video["g1_c2_frame"]["advantages"]).all() and torch.isnan(video["g1_t1_video"]["advantages"]).all()
    assert any(k.endswith("_norm") for k in d["raw"]) and any(k.endswith("_plain") for k in d["raw"])
    assert any(k.endswith("_norm") for k in d["reasoning"]) and any(k.endswith("_plain") for k in d["reasoning"])
    assert torch.isnan(d["raw"]["g8_c2_mask_one_norm"]["advantages"]).all()  # exactly one valid element
    assert os.path.getsize(GOLDEN) < 316373  # no larger than its siblings
