"""Offline IQL, the parts that need no GPU: configuration refusals, the flat layouts, argument validation of every new entry before
any HIP call, the ctypes mirrors, initialisation parity of the host networks, the data set's batching, the golden file, and
negative controls that show the GPU loop test can see plumbing errors."""

import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import iql_cases as C
from helpers import iql_reference as R
from helpers import iql_torch as T
from rlinf_amd import _lib, ops
from rlinf_amd.config import validate_cfg, validate_offline_cfg
from rlinf_amd.data.offline_dataset import OfflineTransitionDataset
from rlinf_amd.models.embodiment import iql_mlp as IM

needs_reference = pytest.mark.skipif(not R.available(), reason="the reference tree with its IQL files is not on this machine")


def _cfg(**edits):
    cfg = C.loop_cfg(32)
    for path, value in edits.items():
        node, keys = cfg, path.split("__")
        for k in keys[:-1]:
            node = node[k]
        if value is KeyError:
            del node[keys[-1]]
        else:
            node[keys[-1]] = value
    return cfg


# ---- configuration ----------------------------------------------------------------------------------------------------------
def test_offline_cfg_is_accepted_and_dispatched():
    cfg = validate_cfg(_cfg(actor__use_fsdp_wrap=True, actor__offline_torch_compile=True, actor__offline_compile_mode="reduce-overhead"))
    assert cfg.runner.task_type == "offline" and cfg.runner.only_eval is False
    with pytest.raises(AssertionError, match="not served by this build"):
        validate_cfg(_cfg(runner__task_type="reasoning"))


@pytest.mark.parametrize("path,message", [
    ("actor__global_batch_size", "offline training requires actor.global_batch_size"),
    ("actor__micro_batch_size", "offline training requires actor.micro_batch_size"),
    ("runner__local_update_steps", "offline training requires runner.local_update_steps"),
    ("runner__max_steps", "offline training requires runner.max_steps"),
    ("runner__only_eval", "offline training requires runner.only_eval"),
    ("algorithm__gamma", "offline training requires algorithm.gamma"),
    ("actor__seed", "offline training requires actor.seed"),
])
def test_offline_cfg_reference_messages_missing(path, message):
    with pytest.raises(AssertionError, match=message):
        validate_offline_cfg(_cfg(**{path: KeyError}))


@pytest.mark.parametrize("edits,message", [
    ({"algorithm__gamma": "x"}, "algorithm.gamma must be numeric, got 'x'"),
    ({"actor__seed": "s"}, "actor.seed must be int-castable, got 's'"),
    ({"actor__global_batch_size": 0, "actor__micro_batch_size": 0}, "actor.global_batch_size must be > 0, got 0"),
    ({"actor__micro_batch_size": 0}, "actor.micro_batch_size must be > 0, got 0"),
    ({"runner__local_update_steps": 0}, "runner.local_update_steps must be > 0 for offline training"),
    ({"runner__max_steps": -1}, "runner.max_steps must be >= 0, got -1"),
    ({"actor__micro_batch_size": 64}, "actor.global_batch_size must be >= actor.micro_batch_size for offline training"),
])
def test_offline_cfg_reference_messages_ranges(edits, message):
    with pytest.raises(AssertionError, match=message.replace(".", r"\.")):
        validate_offline_cfg(_cfg(**edits))


@pytest.mark.parametrize("edits,message", [
    ({"algorithm__dropout_rate": 0.1}, "algorithm.dropout_rate=0.1 is not supported"),
    ({"algorithm__hidden_dims": [256, 256, 256]}, r"algorithm.hidden_dims=\[256, 256, 256\] is not supported"),
    ({"actor__model__iql_config__state_dependent_std": True}, "state_dependent_std=true is not supported"),
    ({"actor__model__num_action_chunks": 2}, "num_action_chunks=2 is not supported"),
    ({"actor__micro_batch_size": 16}, "actor.micro_batch_size must equal per-rank batch size"),
    ({"actor__model__obs_dim": 65}, r"actor.model.obs_dim=65 out of range \[1, 64\]"),
    ({"actor__model__action_dim": 33}, r"actor.model.action_dim=33 out of range \[1, 32\]"),
    ({"actor__model__precision": "bf16"}, "precision='bf16' is not supported"),
])
def test_offline_cfg_refusals_of_this_build(edits, message):
    with pytest.raises(ValueError, match=message):
        validate_offline_cfg(_cfg(**edits))


def test_offline_cfg_refuses_more_than_one_rank(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="actor world size 2 is not supported"):
        validate_offline_cfg(_cfg())


@pytest.mark.parametrize("kwargs,message", [
    (dict(obs_dim=0, action_dim=3), r"obs_dim=0 out of range \[1, 64\]"), (dict(obs_dim=65, action_dim=3), r"obs_dim=65 out of range"),
    (dict(obs_dim=4, action_dim=0), r"action_dim=0 out of range \[1, 32\]"), (dict(obs_dim=4, action_dim=33), "action_dim=33 out of range"),
    (dict(obs_dim=4, action_dim=3, num_action_chunks=2), "num_action_chunks=2 is not supported"),
    (dict(obs_dim=4, action_dim=3, hidden_dims=(128, 128)), "hidden width 256"),
    (dict(obs_dim=4, action_dim=3, dtype=torch.bfloat16), "float32"),
])
def test_network_limits_are_refused_by_name(kwargs, message):
    with pytest.raises(ValueError, match=message):
        IM.IqlNetworks(device="cpu", **kwargs)


# ---- layouts and the C ABI --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"D{s[0]}A{s[1]}")
def test_layout_offsets_and_alignment(shape):
    D, A = shape
    for kind, n_nets, nh, out, in_b in (("actor", 1, 3, A, 0), ("critic", 2, 2, 1, A), ("value", 1, 2, 1, 0)):
        lay, views = IM.iql_layout(kind, D, A)
        assert (lay.n_nets, lay.n_hidden, lay.out_dim, lay.in_a, lay.in_b, lay.hidden) == (n_nets, nh, out, D, in_b, 256)
        spans = sorted((o, o + int(np.prod(s))) for o, s in views.values())
        assert spans[0][0] == 0 and spans[-1][1] == lay.n_params
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), "the views tile the buffer without gaps or overlap"
        K = D + in_b
        for y in range(n_nets):
            for l in range(nh + 1):
                assert lay.off_w[y][l] % 4 == 0, "every weight starts on a 16-byte boundary"
                assert lay.off_b[y][l] + (out if l == nh else 256) <= lay.n_params
            assert lay.off_w[y][1] - lay.off_w[y][0] == 256 * K + 256
        assert (lay.off_logstd >= 0) == (kind == "actor")
        names = {"actor": 9, "critic": 12, "value": 6}[kind]
        assert len(views) == names
    lay, views = IM.iql_layout("critic", D, A)
    assert views["q1.net.0.weight"][1] == (256, D + A) and views["q2.net.4.bias"][1] == (1,)


def test_struct_mirrors_and_version():
    lib = _lib.load()
    assert lib.rlx_version() >= 119
    assert lib.rlx_abi_struct_sizes(None, 0) == 13
    n = lib.rlx_abi_struct_sizes_ext(None, 0)
    assert n >= 5
    sizes = (ctypes.c_size_t * n)()
    lib.rlx_abi_struct_sizes_ext(ctypes.cast(sizes, ctypes.c_void_p), n)
    assert sizes[4] == ctypes.sizeof(_lib.IqlMlpLayout) and sizes[2] == ctypes.sizeof(_lib.SacActorLayout)
    for name in ("rlx_iql_mlp_fwd", "rlx_iql_mlp_bwd", "rlx_iql_mlp_bwd_slabs", "rlx_iql_mlp_bwd_workspace_bytes", "rlx_iql_value_loss",
                 "rlx_iql_actor_loss", "rlx_iql_critic_loss", "rlx_soft_update"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert _lib.IQL_METRIC_NAMES == T.METRICS


def test_iql_entries_validate_before_any_hip_call():
    lib = _lib.load()
    al, cl, vl = (IM.iql_layout(k, 17, 6)[0] for k in ("actor", "critic", "value"))
    fake, big = ctypes.c_void_p(4096), 1 << 30  # never dereferenced: validation fails first
    err = lambda: lib.rlx_last_error()  # noqa: E731
    R_ = ctypes.byref
    # forward
    assert lib.rlx_iql_mlp_fwd(fake, None, fake, 4, None, None, 4, fake, None, None, None, None) == -22 and b"NULL layout" in err()
    assert lib.rlx_iql_mlp_fwd(None, R_(vl), None, 4, None, None, 4, None, None, None, None, None) == -22 and b"rlx_iql_mlp_fwd: NULL" in err()
    assert lib.rlx_iql_mlp_fwd(None, R_(vl), None, 0, None, None, 0, None, None, None, None, None) == 0  # empty batch
    assert lib.rlx_iql_mlp_fwd(fake, R_(vl), fake, -1, None, None, -1, fake, None, None, None, None) == -22 and b"negative batch m" in err()
    assert lib.rlx_iql_mlp_fwd(fake, R_(cl), fake, 4, None, None, 4, fake, None, None, None, None) == -22 and b"xb goes with in_b" in err()
    assert lib.rlx_iql_mlp_fwd(fake, R_(vl), fake, 4, None, fake, 4, fake, None, None, None, None) == -22 and b"xb goes with in_b" in err()
    assert lib.rlx_iql_mlp_fwd(fake, R_(vl), fake, 3, None, None, 4, fake, None, None, None, None) == -22 and b"m_first=3" in err()
    assert lib.rlx_iql_mlp_fwd(fake, R_(vl), fake, 4, fake, None, 4, fake, None, None, None, None) == -22 and b"m_first=4" in err()
    assert lib.rlx_iql_mlp_fwd(fake, R_(al), fake, 4, None, None, 4, fake, None, fake, None, None) == -22 and b"actions and logprob" in err()
    assert lib.rlx_iql_mlp_fwd(fake, R_(vl), fake, 4, None, None, 4, fake, None, fake, fake, None) == -22 and b"actor_logstd" in err()
    odd = ctypes.c_void_p(4096 + 4)
    assert lib.rlx_iql_mlp_fwd(odd, R_(vl), fake, 4, None, None, 4, fake, None, None, None, None) == -22 and b"params is misaligned" in err()
    assert lib.rlx_iql_mlp_bwd(fake, R_(vl), odd, None, fake, fake, None, 64, fake, 1, fake, big, None) == -22 and b"misaligned" in err()
    # backward
    assert lib.rlx_iql_mlp_bwd(fake, R_(vl), fake, None, fake, fake, None, 0, fake, 1, fake, big, None) == -22 and b"empty batch m" in err()
    assert lib.rlx_iql_mlp_bwd(fake, R_(vl), fake, None, fake, fake, None, 64, fake, 0, fake, big, None) == -22 and b"slabs=0" in err()
    assert lib.rlx_iql_mlp_bwd(fake, R_(vl), fake, None, fake, None, None, 64, fake, 1, fake, big, None) == -22 and b"rlx_iql_mlp_bwd: NULL" in err()
    assert lib.rlx_iql_mlp_bwd(fake, R_(vl), fake, None, fake, fake, fake, 64, fake, 1, fake, big, None) == -22 and b"d_logstd needs" in err()
    assert lib.rlx_iql_mlp_bwd(fake, R_(cl), fake, None, fake, fake, None, 64, fake, 1, fake, big, None) == -22 and b"xb goes with" in err()
    assert lib.rlx_iql_mlp_bwd(fake, R_(vl), fake, None, fake, fake, None, 64, fake, 1, fake, 16, None) == -28 and b"workspace" in err()
    assert lib.rlx_iql_mlp_bwd_workspace_bytes(R_(cl), 64) == 2 * 2 * 64 * 256 * 4 and lib.rlx_iql_mlp_bwd_workspace_bytes(R_(al), 64) == 3 * 64 * 256 * 4
    assert [lib.rlx_iql_mlp_bwd_slabs(m) for m in (1, 256, 512, 513, 1 << 20)] == [1, 1, 1, 2, 64]
    # loss legs and the soft update
    assert lib.rlx_iql_value_loss(fake, None, 4, 0.7, fake, fake, fake, None) == -22 and b"rlx_iql_value_loss: NULL" in err()
    assert lib.rlx_iql_value_loss(fake, fake, -1, 0.7, fake, fake, fake, None) == -22 and b"negative batch m" in err()
    assert lib.rlx_iql_value_loss(None, None, 0, 0.7, None, None, None, None) == 0
    assert lib.rlx_iql_actor_loss(fake, R_(vl), fake, fake, fake, fake, fake, 4, 3.0, fake, fake, fake, fake, None) == -22 and b"actor_logstd" in err()
    assert lib.rlx_iql_actor_loss(fake, R_(al), fake, fake, fake, None, fake, 4, 3.0, fake, fake, fake, fake, None) == -22 and b"rlx_iql_actor_loss: NULL" in err()
    assert lib.rlx_iql_actor_loss(fake, R_(al), fake, None, fake, fake, fake, 4, 3.0, fake, fake, fake, fake, None) == -22 and b"go with q_min" in err()
    assert lib.rlx_iql_actor_loss(fake, None, fake, fake, fake, fake, fake, 4, 3.0, fake, fake, fake, fake, None) == -22 and b"NULL layout" in err()
    assert lib.rlx_iql_actor_loss(None, R_(al), None, None, None, None, None, 0, 3.0, None, None, None, None, None) == 0
    assert lib.rlx_iql_critic_loss(fake, fake, None, fake, 4, 0.99, fake, fake, None) == -22 and b"rlx_iql_critic_loss: NULL" in err()
    assert lib.rlx_iql_critic_loss(fake, fake, fake, fake, -2, 0.99, fake, fake, None) == -22 and b"negative batch m" in err()
    assert lib.rlx_soft_update(None, fake, 8, 0.005, None) == -22 and b"rlx_soft_update: NULL" in err()
    assert lib.rlx_soft_update(fake, fake, -1, 0.005, None) == -22 and b"negative n" in err()
    assert lib.rlx_soft_update(fake, fake, 8, 1.5, None) == -22 and b"tau=1.5" in err()
    assert lib.rlx_soft_update(None, None, 0, 0.005, None) == 0
    # the layout's limits, by name
    for field, value, word in (("hidden", 128, b"hidden=128"), ("in_a", 65, b"in_a (obs_dim)=65 out of range [1,64]"), ("in_a", 0, b"in_a (obs_dim)=0"),
                               ("in_b", 33, b"in_b (action_dim)=33 out of range [0,32]"), ("out_dim", 33, b"out_dim=33 out of range [1,32]"),
                               ("n_nets", 3, b"n_nets=3"), ("n_hidden", 4, b"n_hidden=4"), ("n_params", 100, b"out of range"),
                               ("off_logstd", 5, b"off_logstd")):
        lay = copy.copy(cl)
        setattr(lay, field, value)
        assert lib.rlx_iql_mlp_fwd(fake, R_(lay), fake, 4, None, fake, 4, fake, None, None, None, None) == -22 and word in err(), (field, err())
    bad = copy.copy(cl)
    bad.off_w[1][2] += 2
    assert lib.rlx_iql_mlp_fwd(fake, R_(bad), fake, 4, None, fake, 4, fake, None, None, None, None) == -22 and b"multiples of 4" in err()


def test_ops_wrappers_refuse_cpu_tensors():
    al, cl, vl = (IM.iql_layout(k, 5, 2)[0] for k in ("actor", "critic", "value"))
    z = torch.zeros
    calls = (lambda: ops.iql_mlp_fwd(z(vl.n_params), vl, z(3, 5)),
             lambda: ops.iql_mlp_bwd(z(vl.n_params), vl, z(3, 5), None, z(1, 2, 3, 256), z(1, 3, 1)),
             lambda: ops.iql_value_loss(z(2, 3), z(3), 0.7, z(8)),
             lambda: ops.iql_actor_loss(z(al.n_params), al, z(3), z(3), z(3), z(3, 2), z(3, 2), 3.0, z(8)),
             lambda: ops.iql_logprob_bwd(z(al.n_params), al, z(3, 2), z(3, 2), z(3)),
             lambda: ops.iql_critic_loss(z(2, 3), z(3), z(3), z(3), 0.99, z(8)),
             lambda: ops.soft_update_(z(8), z(8), 0.005),
             lambda: IM.IqlNetworks(5, 2, "cpu").critic.forward(z(3, 5), actions=z(3, 2)))
    for call in calls:
        with pytest.raises(_lib.RlxError, match="no CPU fallback"):
            call()


# ---- the host networks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"D{s[0]}A{s[1]}")
def test_init_parity_with_the_restatement(shape):
    torch.manual_seed(9)
    L = T.IqlLearner(*shape)
    after = torch.rand(1)
    torch.manual_seed(9)
    nets = IM.IqlNetworks(shape[0], shape[1], "cpu")
    assert torch.equal(torch.rand(1), after), "the host networks take other draws from the generator than the restatement"
    for name, mod in L.modules().items():
        sd, views = mod.state_dict(), getattr(nets, name).views
        assert list(sd) == [k for k in sd if k in views] and len(sd) == len(views), name
        for k in sd:
            assert torch.equal(sd[k], views[k]), f"{name}.{k}"
    assert nets.target.flat.data_ptr() != nets.critic.flat.data_ptr() and torch.equal(nets.target.flat, nets.critic.flat)


@needs_reference
def test_init_parity_with_the_reference_and_strict_load():
    shape = (17, 6)
    ref = R.make_learner(shape, torch.float32, seed=21)
    torch.manual_seed(21)
    nets = IM.IqlNetworks(shape[0], shape[1], "cpu")
    for name, mod in ref.modules().items():
        sd = mod.state_dict()
        for k, v in getattr(nets, name).views.items():
            assert torch.equal(v, sd[k]), f"{name}.{k}"
    policy = nets.get_policy_state_dict()
    assert "value_head.mlp.6.weight" in policy and "value_head.mlp.6.bias" not in policy
    fresh = R.build_module("actor", *shape)
    result = fresh.load_state_dict(policy, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(fresh.state_dict()["value_head.mlp.0.weight"], ref.model.state_dict()["value_head.mlp.0.weight"])


# ---- the data set -----------------------------------------------------------------------------------------------------------
def _dataset(n=23, D=3, A=2):
    rng = np.random.default_rng(0)
    return OfflineTransitionDataset.from_arrays(rng.standard_normal((n, D)), rng.standard_normal((n, A)), np.arange(n, dtype=np.float64),
                                                np.ones(n), rng.standard_normal((n, D)), device="cpu")


def test_dataset_epoch_permutation_drop_last_and_resume(tmp_path):
    ds = _dataset()
    assert ds.get_obs_action_dims() == (3, 2) and ds.get_dataset_size() == 23 and ds.fields["rewards"].dtype == torch.float32
    with pytest.raises(ValueError, match=r"Dataset size \(23\) must be >= batch_size \(24\)\."):
        ds.configure(24)
    ds.configure(5, seed=42)
    assert ds.batches_per_epoch() == 4  # the last 3 rows of an epoch's order are dropped
    taken = [ds.next_indices().clone() for _ in range(9)]
    for e in range(2):
        g = torch.Generator().manual_seed(42 + e)
        order = torch.randperm(23, generator=g)
        assert torch.equal(torch.cat(taken[4 * e:4 * e + 4]), order[:20])
    assert (ds.epoch, ds.iter_offset) == (2, 1) and not torch.equal(taken[0], taken[4])
    other = _dataset()
    other.configure(5, seed=42)
    other.set_position(2, 1)  # what a checkpoint stores
    assert torch.equal(other.next_indices(), ds.next_indices())
    with pytest.raises(_lib.RlxError, match="no CPU fallback"):
        ds.next_batch()  # rows are gathered on the device
    # D4RL's key names: masks = 1 - terminals
    path = os.path.join(tmp_path, "d.npz")
    np.savez(path, observations=np.zeros((4, 3), np.float32), actions=np.zeros((4, 2), np.float32), rewards=np.ones(4, np.float32),
             terminals=np.array([0, 1, 0, 0], bool), next_observations=np.zeros((4, 3), np.float32))
    z = OfflineTransitionDataset.from_npz(path, device="cpu")
    assert z.fields["masks"].tolist() == [1.0, 0.0, 1.0, 1.0]


# ---- the golden file and the negative controls --------------------------------------------------------------------------------
_LOOPS = {}


def _loop(m, dtype, mistake=None):
    key = (m, dtype, mistake)
    if key not in _LOOPS:
        _LOOPS[key] = C.ref_loop(m, dtype, mistake)
    return _LOOPS[key]


@pytest.mark.parametrize("m", (32, 67))
def test_restatement_reproduces_the_golden_file(m):
    """tests/golden/iql_step.pt was recorded from the real reference (tools/make_iql_golden.py); the restatement's float64 run on
    whatever machine this is reproduces it to 1e-9 relative."""
    g = torch.load(os.path.join(ROOT, "tests", "golden", "iql_step.pt"), weights_only=False)[f"m{m}"]
    r64 = _loop(m, torch.float64)
    rel = lambda a, b: (a - b).abs().max().item() / b.abs().max().item()  # noqa: E731
    assert rel(r64["metrics"], g["metrics"]) <= 1e-9 and rel(r64["lr_actor"], g["lr_actor"]) <= 1e-15
    assert len(g["params"]) == 9 + 12 + 6 + 12
    for name, probe in g["params"].items():
        assert rel(C.probe(r64[name], name), probe) <= 1e-9, name
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "iql_step.pt")) < 316373


@pytest.mark.parametrize("mistake", ("stale_new_v", "no_soft_update", "constant_lr"))
@pytest.mark.parametrize("m", (32, 67))
def test_loop_test_sees_plumbing_errors(m, mistake):
    """A deliberate mistake in the restatement's float64 run moves at least one compared quantity by more than 10 x the bound the
    GPU loop test uses for it (4 x the float32 run's deviation, floored at 1e-6 of the quantity's norm)."""
    r64, r32, wrong = _loop(m, torch.float64), _loop(m, torch.float32), _loop(m, torch.float64, mistake)
    seen = []
    for name in r64:
        if name == "lr_actor":
            continue  # compared to 1e-15 there; the controls are about the numerical bounds
        cols = [(f"metrics[{k}]", (lambda t, i=i: t[:, i]), "out") for i, k in enumerate(T.METRICS)] if name == "metrics" else \
               [(name, (lambda t: t), "grad")]
        for label, pick, kind in cols:
            a, b, w = pick(r64[name]), pick(r32[name]), pick(wrong[name])
            norm = (lambda t: t.abs().max().item()) if kind == "out" else (lambda t: t.norm().item())
            bound = max(4 * norm(b - a), 1e-6 * norm(a))
            if norm(w - a) > 10 * bound:
                seen.append(label)
    assert seen, f"{mistake}: no compared quantity moves by more than 10 x its bound"
    expected = {"stale_new_v": "actor/", "no_soft_update": "target/", "constant_lr": "actor/"}[mistake]
    assert any(s.startswith(expected) for s in seen), (mistake, seen)


def test_shipped_config_validates():
    from rlinf_amd.config import load_config

    path = os.path.join(ROOT, "examples", "embodiment", "config", "d4rl_iql_mlp.yaml")
    cfg = validate_cfg(load_config(path))
    assert cfg.runner.task_type == "offline" and cfg.actor.micro_batch_size == 256 and cfg.actor.model.iql_config.hidden_dims == [256, 256]
    assert cfg.data.dataset_type in ("npz", "synthetic")
