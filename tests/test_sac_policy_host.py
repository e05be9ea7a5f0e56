"""Host side (no launches) of the SAC (Q-head) MLP policy: the module rlinf_amd.ext's builder returns for ``add_q_head=True`` must
look to the reference's SAC learner like the reference's own ``MLPPolicy(add_q_head=True)`` (names, order, shapes, initial values
from the same RNG stream, state_dict with the action buffers, the critic optimizer group), the builder must route only the
default Q head to it, shapes outside the kernels' limits must be refused by name, the C entries must validate before any HIP
call -- and the loss restatement the GPU tests are measured with (tests/helpers/sac_losses.py) must be what the reference's own
learner methods compute."""

import copy
import ctypes
import os
import sys
import types

import pytest
import torch

from helpers import sac_cases as SC
from helpers import sac_losses as SL
from oracle import reference_loader as RL

needs_reference = pytest.mark.skipif(not RL.available(), reason="neither the reference tree nor its staged copy is present")
WORKER = "rlinf/workers/actor/fsdp_sac_policy_worker.py"
BUILDER = "rlinf/models/embodiment/mlp_policy/__init__.py"


class Cfg(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def refmod():
    return RL.load().mlp_policy


@needs_reference
@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "D%dA%dC%d" % s)
def test_init_parity_with_the_reference(refmod, shape):
    from rlinf_amd.models.embodiment.sac_mlp_policy import SacMLPPolicy

    args = (*shape, False, True)
    torch.manual_seed(5)
    theirs = refmod.MLPPolicy(*args)
    after_theirs = torch.rand(4)
    torch.manual_seed(5)
    ours = SacMLPPolicy(*args)
    after_ours = torch.rand(4)
    assert torch.equal(after_theirs, after_ours)  # the same number of RNG draws, in the same order
    want, got = list(theirs.named_parameters()), list(ours.named_parameters())
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, p), (_, q) in zip(want, got):
        assert p.shape == q.shape and p.requires_grad == q.requires_grad and torch.equal(p.detach(), q.detach()), n
    assert list(ours.state_dict()) == list(theirs.state_dict()) and "action_scale" in ours.state_dict()
    assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), theirs.state_dict().values()))
    names = [n for n, _ in got]
    assert names[0] == "q_head.qs.0.net.0.weight" and names[-2:] == ["actor_logstd.weight", "actor_logstd.bias"]
    assert len([n for n in names if "q_head" in n]) == 28  # the reference's critic optimizer group
    torch.manual_seed(6)
    other = refmod.MLPPolicy(*args)
    ours.load_state_dict(other.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), other.state_dict().values()))
    theirs.load_state_dict(ours.state_dict(), strict=True)  # and back: a checkpoint of ours is a checkpoint of theirs
    # the kernels' layouts cover every parameter once; the 256-wide weights start at multiples of 4
    assert ours._q_layout.n_params == sum(p.numel() for n, p in got if "q_head" in n)
    assert ours._actor_layout.n_params == sum(p.numel() for n, p in got if "q_head" not in n)
    assert all(ours._q_layout.off_w[y][l] % 4 == 0 for y in range(2) for l in range(4)) and ours._actor_layout.off_wh % 4 == 0
    target = copy.deepcopy(ours)  # the learner's target network
    assert list(target.state_dict()) == list(ours.state_dict()) and target._q_layout is not ours._q_layout


def test_forward_types_other_than_sac_are_refused():
    from rlinf_amd.models.embodiment.sac_mlp_policy import SacMLPPolicy

    model = SacMLPPolicy(9, 7, 2, False, True)
    for kind in ("default", "sft", "crossq", "crossq_q"):
        with pytest.raises(NotImplementedError):
            model(forward_type=kind)
    with pytest.raises(NotImplementedError):
        SacMLPPolicy(9, 7, 2, False, True, q_head_type="crossq")


def test_shapes_outside_the_kernels_limits_name_the_limit():
    from rlinf_amd.models.embodiment.mlp_policy_module import build_reference_named_mlp_policy as build
    from rlinf_amd.models.embodiment.sac_mlp_policy import SacMLPPolicy

    base = Cfg(obs_dim=42, action_dim=4, num_action_chunks=1, add_value_head=False, add_q_head=True)
    with pytest.raises(NotImplementedError, match="obs_dim <= 64"):
        build(Cfg(base, obs_dim=65), torch.float32)
    with pytest.raises(NotImplementedError, match=r"action_dim \* num_action_chunks <= 16 \(got 17\)"):
        build(Cfg(base, action_dim=17), torch.float32)
    with pytest.raises(NotImplementedError, match="critic_obs_dim must be None or obs_dim=42"):
        build(Cfg(base, critic_obs_dim=50), torch.float32)
    with pytest.raises(NotImplementedError, match="float32 only"):
        build(Cfg(base), torch.bfloat16)
    assert isinstance(build(Cfg(base, obs_dim=64, action_dim=8, num_action_chunks=2, critic_obs_dim=64), torch.float32), SacMLPPolicy)
    # the PPO classes keep refusing the Q head
    from rlinf_amd.models.embodiment.mlp_policy import MLPPolicy

    with pytest.raises(NotImplementedError):
        MLPPolicy(42, 8, 1, False, True)


@needs_reference
def test_the_reference_registry_routes_sac_to_the_hip_module(refmod, monkeypatch):
    if not os.path.isfile(os.path.join(RL.REFERENCE_ROOT, BUILDER)):
        pytest.skip("the reference's own MLP builder is not present on this machine")
    from rlinf_amd import ext
    from rlinf_amd.models.embodiment.sac_mlp_policy import SacMLPPolicy

    mr, reg = RL.load_models_registry(), RL.load().registry
    saved = dict(mr.models._MODEL_REGISTRY), dict(reg.ADV_REGISTRY), dict(reg.LOSS_REGISTRY)
    # the reference's own builder, compiled from its source; the three policies it imports and does not build here are stand-ins
    for name, cls in (("iql_mlp_policy", "IQLMLPPolicy"), ("rlt_mlp_policy", "RLTMLPPolicy"), ("rlt_td3_mlp_policy", "RLTTD3MLPPolicy")):
        mod = types.ModuleType(f"rlinf.models.embodiment.mlp_policy.{name}")
        setattr(mod, cls, type(cls, (), {}))
        monkeypatch.setitem(sys.modules, mod.__name__, mod)
    monkeypatch.setattr(sys.modules["rlinf.models.embodiment.mlp_policy"], "get_model", RL.load_function(BUILDER, "get_model", torch=torch),
                        raising=False)
    try:
        try:
            ext.register()
        except RuntimeError as e:  # without a HIP device the hook raises AFTER registering
            assert "no HIP device" in str(e)
        cfg = Cfg(model_type="mlp_policy", precision="32", obs_dim=42, action_dim=4, num_action_chunks=1, add_value_head=False,
                  add_q_head=True, is_lora=False, load_to_device=False)
        model = mr.models.get_model(cfg)  # the reference's own get_model (rlinf/models/__init__.py:337-352)
        assert isinstance(model, SacMLPPolicy) and model.q_out_dim == 1
        crossq = mr.models.get_model(Cfg(cfg, q_head_type="crossq"))
        assert type(crossq) is refmod.MLPPolicy
    finally:
        mr.models._MODEL_REGISTRY.clear(), mr.models._MODEL_REGISTRY.update(saved[0])
        reg.ADV_REGISTRY.clear(), reg.ADV_REGISTRY.update(saved[1])
        reg.LOSS_REGISTRY.clear(), reg.LOSS_REGISTRY.update(saved[2])


def test_sac_entries_validate_before_any_hip_call():
    from rlinf_amd import _lib
    from rlinf_amd.models.embodiment.sac_mlp_policy import SacMLPPolicy

    lib = _lib.load()
    assert lib.rlx_version() >= 118
    model = SacMLPPolicy(42, 4, 1, False, True)
    al, ql = model._actor_layout, model._q_layout
    fake = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    err = lambda: lib.rlx_last_error()  # noqa: E731
    assert lib.rlx_sac_actor_fwd(fake, None, fake, None, 4, 1.0, 0.0, fake, fake, None, None, None) == -22 and b"NULL layout" in err()
    assert lib.rlx_sac_actor_fwd(None, ctypes.byref(al), None, None, 4, 1.0, 0.0, None, None, None, None, None) == -22
    assert b"rlx_sac_actor_fwd: NULL" in err()
    assert lib.rlx_sac_actor_fwd(fake, ctypes.byref(al), fake, None, 4, 1.0, 0.0, fake, fake, fake, None, None) == -22 and b"aux" in err()
    assert lib.rlx_sac_actor_fwd(None, ctypes.byref(al), None, None, 0, 1.0, 0.0, None, None, None, None, None) == 0  # empty batch
    assert lib.rlx_sac_actor_fwd(fake, ctypes.byref(al), fake, None, -1, 1.0, 0.0, fake, fake, None, None, None) == -22
    assert lib.rlx_sac_actor_bwd(fake, ctypes.byref(al), fake, None, fake, fake, None, None, 0, 1.0, fake, 1, fake, 1 << 30, None) == -22
    assert b"empty batch" in err()
    assert lib.rlx_sac_actor_bwd(fake, ctypes.byref(al), fake, None, fake, fake, None, None, 64, 1.0, fake, 0, fake, 1 << 30, None) == -22
    assert b"slabs=0" in err()
    assert lib.rlx_sac_actor_bwd(fake, ctypes.byref(al), fake, None, fake, fake, None, None, 64, 1.0, fake, 1, fake, 16, None) == -28
    assert lib.rlx_sac_actor_bwd_workspace_bytes(ctypes.byref(al), 64) == (3 * 64 * 256 + 2 * 64 * 4) * 4
    assert lib.rlx_sac_q_fwd(None, ctypes.byref(ql), None, None, 4, None, None, None, None) == -22 and b"rlx_sac_q_fwd: NULL" in err()
    assert lib.rlx_sac_q_fwd(fake, ctypes.byref(ql), fake, fake, 4, fake, fake, None, None) == -22 and b"rstd" in err()
    assert lib.rlx_sac_q_bwd(fake, ctypes.byref(ql), fake, fake, fake, fake, None, 64, fake, 1, fake, fake, 1 << 30, None) == -22
    assert b"rlx_sac_q_bwd: NULL" in err()
    assert lib.rlx_sac_q_bwd(fake, ctypes.byref(ql), fake, fake, fake, fake, fake, 64, None, 1, None, fake, 16, None) == -28
    assert lib.rlx_sac_q_bwd_workspace_bytes(ctypes.byref(ql), 64) == 12 * 64 * 256 * 4
    assert [lib.rlx_sac_q_bwd_slabs(m) for m in (1, 512, 513, 1 << 20)] == [1, 1, 2, 64] == \
           [lib.rlx_sac_actor_bwd_slabs(m) for m in (1, 512, 513, 1 << 20)]
    for field, value, word in (("hidden", 128, b"hidden=128"), ("obs_dim", 65, b"obs_dim=65 out of range [1,64]"),
                               ("act_dim", 17, b"act_dim=17 out of range [1,16]"), ("n_params", 100, b"out of range")):
        for lay, call in ((copy.copy(al), lambda lay: lib.rlx_sac_actor_fwd(fake, ctypes.byref(lay), fake, None, 4, 1.0, 0.0, fake, fake,
                                                                             None, None, None)),
                          (copy.copy(ql), lambda lay: lib.rlx_sac_q_fwd(fake, ctypes.byref(lay), fake, fake, 4, fake, None, None, None))):
            setattr(lay, field, value)
            assert call(lay) == -22 and word in err(), (field, err())
    bad = copy.copy(ql)
    bad.off_w[1][2] += 2
    assert lib.rlx_sac_q_fwd(fake, ctypes.byref(bad), fake, fake, 4, fake, None, None, None) == -22 and b"multiples of 4" in err()
    # the ops wrappers refuse CPU tensors: there is no fallback
    from rlinf_amd import ops

    with pytest.raises(_lib.RlxError, match="no CPU fallback"):
        ops.sac_q_fwd(torch.zeros(ql.n_params), ql, torch.zeros(2, 42), torch.zeros(2, 4), False)
    with pytest.raises(_lib.RlxError, match="no CPU fallback"):
        model.sac_forward({"states": torch.zeros(2, 42)})


# ---- the loss restatement ------------------------------------------------------------------------------------------------
def _batch(shape, m):
    b = SC.make_batch(shape, m)
    return {k: b[k] for k in ("curr_obs", "next_obs", "actions", "rewards", "terminations")}


@needs_reference
def test_loss_restatement_variants(refmod):
    """agg_q min / mean, bootstrap always / standard, backup_entropy and rewards summed over the chunks, each against the formula
    written out on the model's own outputs."""
    shape, m, alpha, gamma = (9, 7, 2), 16, 0.2, 0.8
    ft, batch = refmod.ForwardType, _batch(shape, m)
    model = SC.make_model(refmod.MLPPolicy, shape, "perturbed")
    target = SC.make_model(refmod.MLPPolicy, shape, "perturbed", seed=8)
    assert batch["rewards"].shape == (m, 2) and batch["terminations"].any() and not batch["terminations"].all()
    for agg in ("min", "mean"):
        for boot in ("always", "standard"):
            for backup in (True, False):
                torch.manual_seed(1)
                loss = SL.critic_loss(model, target, ft, batch, alpha, gamma=gamma, agg_q=agg, bootstrap_type=boot, backup_entropy=backup)
                torch.manual_seed(1)
                with torch.no_grad():
                    a2, lp2, _ = model(forward_type=ft.SAC, obs=batch["next_obs"])
                    qn = target(forward_type=ft.SAC_Q, obs=batch["next_obs"], actions=a2)
                    qn = qn.min(1, keepdim=True)[0] if agg == "min" else qn.mean(1, keepdim=True)
                    if backup:
                        qn = qn - alpha * lp2.sum(-1, keepdim=True)
                    live = 1.0 if boot == "always" else (~batch["terminations"].any(-1, keepdim=True)).float()
                    want = batch["rewards"].sum(-1, keepdim=True) + live * gamma * qn
                    q = model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=batch["actions"])
                    torch.testing.assert_close(loss, ((q - want) ** 2).mean(), rtol=1e-6, atol=1e-7)
        torch.manual_seed(2)
        loss, entropy = SL.actor_loss(model, ft, batch, alpha, agg_q=agg)
        torch.manual_seed(2)
        with torch.no_grad():
            pi, lp, _ = model(forward_type=ft.SAC, obs=batch["curr_obs"])
            q = model(forward_type=ft.SAC_Q, obs=batch["curr_obs"], actions=pi)
            q = q.min(1, keepdim=True)[0] if agg == "min" else q.mean(1, keepdim=True)
            torch.testing.assert_close(loss, (alpha * lp.sum(-1, keepdim=True) - q).mean(), rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(entropy, -lp.sum(-1).mean(), rtol=1e-6, atol=1e-7)


@needs_reference
@pytest.mark.parametrize("agg_q,bootstrap_type,backup_entropy", [("min", "standard", True), ("mean", "always", False),
                                                                 ("min", "always", True), ("mean", "standard", True)])
def test_loss_restatement_is_the_reference_learner(refmod, agg_q, bootstrap_type, backup_entropy):
    """The reference's own forward_critic / forward_actor / forward_alpha, compiled from the worker's source over a stand-in
    ``self`` that holds the reference's torch model and a deep-copied target: the helper gives bit-equal losses and gradients."""
    if not os.path.isfile(os.path.join(RL.REFERENCE_ROOT, WORKER)):
        pytest.skip("the reference's SAC worker is not present on this machine (it is not staged for the GPU machine)")
    import torch.nn.functional as F

    shape, m, gamma = (9, 7, 2), 16, 0.8
    ft, batch = refmod.ForwardType, _batch(shape, m)
    supported = RL.load_models_registry().config.SupportedModel
    globs = dict(torch=torch, F=F, ForwardType=ft, SupportedModel=supported)
    methods = {n: RL.load_function(WORKER, f"EmbodiedSACFSDPPolicy.{n}", **globs) for n in ("forward_critic", "forward_actor", "forward_alpha")}

    class Temp:
        def __init__(self):
            self.base_alpha = torch.tensor(0.3, requires_grad=True)

        def compute_alpha(self):
            return F.softplus(self.base_alpha)

        alpha = property(lambda self: self.compute_alpha().item())

    def fresh():
        model = SC.make_model(refmod.MLPPolicy, shape, "perturbed")
        target = copy.deepcopy(model)
        with torch.no_grad():
            for p in target.parameters():
                p.mul_(0.9)
        return model, target, Temp()

    algorithm = Cfg(q_head_type="default", bootstrap_type=bootstrap_type, agg_q=agg_q, gamma=gamma, backup_entropy=backup_entropy)
    cfg = Cfg(algorithm=algorithm, actor=Cfg(model=Cfg(model_type="mlp_policy")))
    model, target, temp = fresh()
    me = types.SimpleNamespace(cfg=cfg, torch_dtype=torch.float32, model=model, target_model=target, entropy_temp=temp,
                               critic_subsample_size=-1, use_dsrl=False, target_entropy=-14.0, device=torch.device("cpu"))
    model2, target2, temp2 = fresh()

    def grads(mod):
        out = [None if p.grad is None else p.grad.clone() for p in mod.parameters()]
        mod.zero_grad(set_to_none=True)
        return out

    def same(a, b):
        return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))

    torch.manual_seed(3)
    theirs, _ = methods["forward_critic"](me, batch)
    theirs.backward()
    torch.manual_seed(3)
    ours = SL.critic_loss(model2, target2, ft, batch, temp2.alpha, gamma=gamma, agg_q=agg_q, bootstrap_type=bootstrap_type,
                          backup_entropy=backup_entropy)
    ours.backward()
    assert torch.equal(theirs, ours) and same(grads(model), grads(model2))

    torch.manual_seed(4)
    theirs, their_entropy, _ = methods["forward_actor"](me, batch)
    theirs.backward()
    torch.manual_seed(4)
    ours, our_entropy = SL.actor_loss(model2, ft, batch, temp2.alpha, agg_q=agg_q)
    ours.backward()
    assert torch.equal(theirs, ours) and torch.equal(their_entropy, our_entropy) and same(grads(model), grads(model2))

    torch.manual_seed(5)
    theirs = methods["forward_alpha"](me, batch)
    theirs.backward()
    torch.manual_seed(5)
    ours = SL.alpha_loss(model2, ft, batch, temp2.compute_alpha(), me.target_entropy)
    ours.backward()
    assert torch.equal(theirs, ours) and torch.equal(temp.base_alpha.grad, temp2.base_alpha.grad) and same(grads(model), grads(model2))
