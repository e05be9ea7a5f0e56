"""tests/helpers/iql_torch.py (the plain-torch restatement the GPU tests compare with) against the REAL reference on the CPU:
``iql_mlp_policy.py`` executed by path, the worker's update methods compiled over a stand-in ``self`` (helpers/iql_reference.py).
Same state-dict keys and initial values after the same seed, bit-equal forwards, and bit-equal parameters, target, Adam moments,
metrics and lr_actor after 5 update steps, in float64 and float32.  Skips where the reference tree is absent."""

import pytest
import torch

from helpers import iql_cases as C
from helpers import iql_reference as R
from helpers import iql_torch as T

pytestmark = pytest.mark.skipif(not R.available(), reason="the reference tree with its IQL files is not on this machine")

DTYPES = (torch.float64, torch.float32)


@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"D{s[0]}A{s[1]}")
def test_same_keys_and_initial_values(shape):
    torch.manual_seed(11)
    ref = R.make_learner(shape, torch.float32, seed=11)
    after_ref = torch.rand(1)
    torch.manual_seed(11)
    ours = T.IqlLearner(shape[0], shape[1], live_only=False)
    assert torch.equal(torch.rand(1), after_ref), "the restatement takes other draws from the generator than the reference"
    for name, mod in ours.modules().items():
        sd, rsd = mod.state_dict(), ref.modules()[name].state_dict()
        assert list(sd) != [] and sorted(sd) == sorted(rsd), name
        for k in sd:
            assert torch.equal(sd[k], rsd[k]), f"{name}.{k}"
    # the live-only form: the same live values under the same names
    torch.manual_seed(11)
    live = T.IqlLearner(shape[0], shape[1])
    for name, mod in live.modules().items():
        rsd = ref.modules()[name].state_dict()
        for k, v in mod.state_dict().items():
            assert torch.equal(v, rsd[k]), f"{name}.{k}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_forwards_are_bit_equal(dtype):
    shape, m = (17, 6), 67
    ref, ours = R.make_learner(shape, dtype), T.make_learner(shape, dtype)
    b = T.cast(T.make_batch(shape, m), dtype)
    ft = ref.ForwardType
    with torch.no_grad():
        assert torch.equal(ref.model(forward_type=ft.IQL_ACTOR, observations=b["obs"], actions=b["actions"]),
                           ours.actor.log_prob(b["obs"], b["actions"]))
        assert torch.equal(ref.value_model(forward_type=ft.IQL_VALUE, observations=b["obs"]), ours.value.v(b["obs"]))
        q1, q2 = ref.critic_model(observations=b["obs"], actions=b["actions"])
        o1, o2 = ours.critic(b["obs"], b["actions"])
        assert torch.equal(q1, o1) and torch.equal(q2, o2)
        diff = torch.linspace(-1, 1, 9, dtype=dtype)
        assert torch.equal(ref.iql_expectile_loss(diff, 0.8), T.expectile_loss(diff, 0.8))


@pytest.mark.parametrize("m", (32, 67))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_five_update_steps_are_bit_equal(dtype, m):
    out, ref = R.run_loop(m, dtype, C.loop_batches(m), T.cast, T.LOOP)
    L = T.make_learner((17, 6), dtype, "init", **T.LOOP)
    for i, b in enumerate(C.loop_batches(m)):
        b = T.cast(b, dtype)
        mt, lr = T.iql_update_step(L, b["obs"], b["actions"], b["rewards"], b["masks"], b["next_obs"])
        assert torch.equal(mt.double(), out["metrics"][i]), f"metrics of step {i}"
        assert lr == out["lr_actor"][i].item(), f"lr_actor of step {i}"
    assert out["lr_actor"][0] != out["lr_actor"][4], "the cosine schedule did not move"
    for name, mod in L.modules().items():
        rsd = ref.modules()[name].state_dict()
        for k, v in mod.state_dict().items():
            assert torch.equal(v, rsd[k]), f"{name}.{k} after 5 steps"
    for name, ours, theirs in (("actor", L.opt_actor, ref.optimizer), ("value", L.opt_value, ref.vf_optimizer),
                               ("critic", L.opt_critic, ref.qf_optimizer)):
        ref_params = dict(ref.modules()[name].named_parameters())
        for k, po in L.modules()[name].named_parameters():  # the live parameters; the reference's unused ones never get a state
            so, sr = ours.state[po], theirs.state[ref_params[k]]
            assert torch.equal(so["exp_avg"], sr["exp_avg"]) and torch.equal(so["exp_avg_sq"], sr["exp_avg_sq"]), f"{name}.{k}"
            assert float(so["step"]) == float(sr["step"]) == 5.0
