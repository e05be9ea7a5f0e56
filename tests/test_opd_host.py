"""On-policy distillation (OPD) without a GPU: the registry names resolve, the reference's argument checks run on the host before
anything launches, the C entry points reject bad arguments, ext.register() installs both names in the reference's registries,
and this build's mlp_policy learner refuses adv_type 'opd' the way the reference's learner does for non-OpenVLA models."""

import ctypes
import sys
import types

import pytest
import torch


def test_both_names_resolve_in_this_package():
    from rlinf_amd.algorithms import advantages, get_adv_and_returns, get_policy_loss, losses
    from rlinf_amd.algorithms.registry import _NATIVE_LOSS
    assert get_adv_and_returns("opd").__wrapped__ is advantages.compute_opd_advantages.__wrapped__
    assert get_adv_and_returns("OPD") is get_adv_and_returns("opd")
    assert get_policy_loss("opd").__wrapped__ is losses.compute_opd_actor_loss.__wrapped__
    assert _NATIVE_LOSS["opd"] is losses._native_opd_loss


def test_advantage_checks_raise_the_reference_messages_on_the_host():
    from rlinf_amd.algorithms import get_adv_and_returns
    fn = get_adv_and_returns("opd")
    p = torch.zeros(3, 2, 14)
    with pytest.raises(AssertionError, match="OPD advantage computation requires post-rollout teacher_logprobs."):
        fn(prev_logprobs=p, teacher_logprobs=None, num_action_chunks=2)
    with pytest.raises(AssertionError, match="OPD advantage computation requires prev_logprobs from student rollout."):
        fn(prev_logprobs=None, teacher_logprobs=p, num_action_chunks=2)
    with pytest.raises(AssertionError, match=r"teacher_logprobs shape torch.Size\(\[2, 2, 14\]\) must match prev_logprobs shape"):
        fn(prev_logprobs=p, teacher_logprobs=p[:2], num_action_chunks=2)
    with pytest.raises(AssertionError, match="VLA-OPD uses raw reverse-KL rewards; set normalize_advantages to False."):
        fn(prev_logprobs=p, teacher_logprobs=p, normalize_advantages=True, num_action_chunks=2)
    with pytest.raises(AssertionError, match="OPD advantage computation requires num_action_chunks."):
        fn(prev_logprobs=p, teacher_logprobs=p)
    with pytest.raises(AssertionError, match="OPD token count 14 must be divisible by num_action_chunks 3."):
        fn(prev_logprobs=p, teacher_logprobs=p, num_action_chunks=3)
    with pytest.raises(AssertionError, match="OPD advantages time dimension 3 must match loss_mask time dimension 1 or include "
                                             "one bootstrap step."):
        fn(prev_logprobs=p, teacher_logprobs=p, num_action_chunks=2, loss_mask=torch.ones(1, 2, 2, dtype=torch.bool))


def test_loss_checks_raise_the_reference_messages_on_the_host():
    from rlinf_amd.algorithms import get_policy_loss
    fn = get_policy_loss("opd")
    lp = torch.zeros(4, 2, 7)
    m, s = torch.ones(4, 2, 1, dtype=torch.bool), torch.ones(4, 2, 1, dtype=torch.int64)
    with pytest.raises(AssertionError, match="logprobs must be float32 to keep numerical stability"):
        fn(logprobs=lp.double(), advantages=lp, loss_mask=m, loss_mask_sum=s)
    with pytest.raises(AssertionError, match="advantages must be float32 to keep numerical stability"):
        fn(logprobs=lp, advantages=lp.half(), loss_mask=m, loss_mask_sum=s)
    with pytest.raises(AssertionError, match=r"OPD advantages shape torch.Size\(\[4, 2, 1\]\) must match logprobs shape"):
        fn(logprobs=lp, advantages=lp[..., :1], loss_mask=m, loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD actor loss requires loss_mask."):
        fn(logprobs=lp, advantages=lp, loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD actor loss requires loss_mask_sum."):
        fn(logprobs=lp, advantages=lp, loss_mask=m)
    with pytest.raises(AssertionError, match="OPD loss_mask rank 1 must match logprobs rank 3."):
        fn(logprobs=lp, advantages=lp, loss_mask=m[:, 0, 0], loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD loss_mask shape .* must match logprobs shape .* except the token dimension."):
        fn(logprobs=lp, advantages=lp, loss_mask=m[:, :1], loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD loss_mask token dimension 3 must be 1 or match logprobs token dimension 7."):
        fn(logprobs=lp, advantages=lp, loss_mask=m.expand(4, 2, 3), loss_mask_sum=s)
    with pytest.raises(AssertionError, match="OPD loss_mask_sum rank 1 must match logprobs rank 3."):
        fn(logprobs=lp, advantages=lp, loss_mask=m, loss_mask_sum=s[:, 0, 0])
    with pytest.raises(AssertionError, match="OPD loss_mask_sum token dimension 3 must be 1"):
        fn(logprobs=lp, advantages=lp, loss_mask=m, loss_mask_sum=s.expand(4, 2, 3))
    # the embodied dispatcher's token-level shaping (utils.py:318-323): per-token advantages must match the log-probs
    from rlinf_amd.algorithms import policy_loss
    with pytest.raises(AssertionError, match=r"OPD advantages shape torch.Size\(\[4, 2\]\) must match logprobs shape"):
        policy_loss(loss_type="opd", task_type="embodied", logprob_type="token_level", single_action_dim=7,
                    logprobs=lp.reshape(4, 14), old_logprobs=lp.reshape(4, 14), advantages=torch.zeros(4, 2),
                    loss_mask=m[..., 0], loss_mask_sum=s[..., 0], max_episode_steps=10)


def test_c_entry_points_validate_without_a_gpu():
    from rlinf_amd import _lib
    lib = _lib.load()
    assert lib.rlx_version() >= 113
    one = ctypes.c_float(0)
    ptr = ctypes.addressof(one)
    assert lib.rlx_opd_advantages(None, 0, 4, None, 0, 4, 0, 4, None, None) == 0  # nothing to do
    assert lib.rlx_opd_advantages(ptr, 9, 4, ptr, 0, 4, 1, 4, ptr, None) == -22
    assert b"teacher_dtype" in lib.rlx_last_error()
    assert lib.rlx_opd_advantages(ptr, 0, 2, ptr, 0, 4, 1, 4, ptr, None) == -22
    assert b"row strides" in lib.rlx_last_error()
    ws = lib.rlx_opd_loss_workspace_bytes(100)
    assert ws >= 1024 * 3 * 8
    assert lib.rlx_opd_loss_fwd(ptr, ptr, ptr, 3, None, 1, 1, 14, 0, ptr, ptr, ws, None) == -22  # 14 % 3 != 0
    assert b"divisors" in lib.rlx_last_error()
    assert lib.rlx_opd_loss_fwd(ptr, ptr, ptr, 7, None, 7, 1, 14, 240, ptr, ptr, ws, None) == -22
    assert b"loss_mask_sum is NULL" in lib.rlx_last_error()
    assert lib.rlx_opd_loss_fwd(ptr, ptr, ptr, 7, ptr, 7, 1, 14, 240, ptr, ptr, 8, None) == -28  # workspace too small
    assert lib.rlx_opd_loss_fwd(ptr, ptr, ptr, 1, None, 1, 1, 1 << 31, 0, ptr, ptr, ws, None) == -22
    assert lib.rlx_opd_loss_bwd(None, None, 1, None, 1, 0, 0, 0, None, None, None, None) == 0  # empty
    assert lib.rlx_opd_loss_bwd(ptr, ptr, 1, None, 1, 2, 4, 0, ptr, None, ptr, None) == -22


def test_mlp_policy_learner_refuses_opd_with_the_reference_message():
    from test_end_to_end import make_cfg

    from rlinf_amd.config import validate_cfg
    cfg = make_cfg()
    cfg.algorithm.adv_type, cfg.algorithm.loss_type = "opd", "opd"
    cfg.algorithm.normalize_advantages = False
    with pytest.raises(AssertionError, match="OPD teacher logprob computation currently supports OpenVLA models."):
        validate_cfg(cfg)


class _StubRegistry(types.ModuleType):
    """The reference's registry semantics (registry.py:30-74): last registration wins, names lower-cased."""

    def __init__(self, name, builtin_opd=True):
        super().__init__(name)
        opd = {"opd": object()} if builtin_opd else {}  # the reference registers its own "opd" callees at import
        self.ADV_REGISTRY, self.LOSS_REGISTRY = dict(opd), dict(opd)

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


def _register(reg):
    from rlinf_amd import ext
    try:
        ext.register()
    except RuntimeError as e:  # no HIP device here: register() installs the names, then says so
        assert "no HIP device" in str(e)


def test_ext_register_installs_opd_in_the_reference_registries():
    from oracle import reference_loader as RL
    if RL.available():
        ref = RL.load()
        mr = RL.load_models_registry()
        reg = ref.registry
        saved = dict(reg.ADV_REGISTRY), dict(reg.LOSS_REGISTRY), dict(mr.models._MODEL_REGISTRY)
        assert "opd" in saved[0] and "opd" in saved[1]  # the reference's own callees, replaced below
        try:
            _register(reg)
            assert reg.ADV_REGISTRY["opd"].__module__ == "rlinf_amd.algorithms.advantages"  # through the reference's wrapper
            assert reg.ADV_REGISTRY["opd"].__name__ == "compute_opd_advantages"
            assert reg.LOSS_REGISTRY["opd"] is not saved[1]["opd"] and reg.LOSS_REGISTRY["opd"].__name__ == "_shaped_opd"
        finally:
            reg.ADV_REGISTRY.clear(), reg.ADV_REGISTRY.update(saved[0])
            reg.LOSS_REGISTRY.clear(), reg.LOSS_REGISTRY.update(saved[1])
            mr.models._MODEL_REGISTRY.clear(), mr.models._MODEL_REGISTRY.update(saved[2])
        return
    # no reference tree: stand-in `rlinf.algorithms.registry` / `rlinf.models` modules with the reference's registration rules
    for builtin_opd in (True, False):
        reg = _with_stub_registry(builtin_opd)
        if builtin_opd:
            assert reg.ADV_REGISTRY["opd"].__module__ == "rlinf_amd.algorithms.advantages"
            assert reg.ADV_REGISTRY["opd"].__name__ == "compute_opd_advantages"
            assert reg.LOSS_REGISTRY["opd"].__name__ == "_shaped_opd"
        else:  # an RLinf without OPD (no dispatcher arm for it) gets no "opd" callee
            assert "opd" not in reg.ADV_REGISTRY and "opd" not in reg.LOSS_REGISTRY
            assert "gae" in reg.ADV_REGISTRY and "actor_critic" in reg.LOSS_REGISTRY


def _with_stub_registry(builtin_opd):
    names = ("rlinf", "rlinf.algorithms", "rlinf.algorithms.registry", "rlinf.models")
    before = {n: sys.modules.get(n) for n in names}
    reg = _StubRegistry("rlinf.algorithms.registry", builtin_opd)
    models = types.ModuleType("rlinf.models")
    models.register_model = lambda *a, **k: None
    pkg, algos = types.ModuleType("rlinf"), types.ModuleType("rlinf.algorithms")
    pkg.algorithms, pkg.models, algos.registry = algos, models, reg
    sys.modules.update({"rlinf": pkg, "rlinf.algorithms": algos, "rlinf.algorithms.registry": reg, "rlinf.models": models})
    try:
        _register(reg)
    finally:
        for n, m in before.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return reg
