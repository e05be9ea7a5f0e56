"""The fused-step parity tests under the exact-f32 MFMA form (step::Form::F32, rlinf_amd/csrc/ppo_step_f32.hip).

RLX_F32_EXACT_MFMA is read once per process, so every in-process test that asks for "f32" runs the three-plane form (F32X).  This
script is the child process tests/test_gpu_exact_f32_form.py starts with RLX_F32_EXACT_MFMA=1, one per group:

    python tests/helpers/exact_f32_child.py <group> <result file>

It imports the existing test modules as plain modules and calls their test functions as ordinary functions -- the assertions and
bars are theirs, verbatim -- over the non-bf16 parameter sets of the functions' own parametrize marks, plus the plan edges only
this form has (plan_edge_case below).  The result file gets one JSON line of form facts, then one line per case (id, outcome,
message, seconds), flushed case by case.  An assertion failure (or pytest's Failed / Skipped) is that case's outcome and the child
goes on; any other exception (an RlxError carrying a HIP error, a torch RuntimeError) is recorded as "error" and ends the child at
once with a non-zero status, nothing more started on the GPU.

cases(group) is shared with the parent, so both sides agree on the ids.
"""

import itertools
import json
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (TESTS, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GROUPS = ("rollout", "step", "optimizer", "loop")
FACTS_M = 6400  # the slab count the facts line reports: 25 under Form::F32 on 256 CUs, 10 under F32X

# group -> (module, function); test_train_fwd_bwd_and_value_shapes and the other mlp_policy.hip entry points do not read the switch
_EXISTING = {
    "rollout": (("test_gpu_mlp_shapes", "test_rollout_step_shapes"),
                ("test_gpu_fused_step", "test_rollout_step_policy_and_value_jobs"),
                ("test_gpu_mlp_shapes", "test_outputs_do_not_depend_on_stale_lds")),
    "step": (("test_gpu_mlp_shapes", "test_ppo_step_shapes"),
             ("test_gpu_fused_step", "test_ppo_step_gradients_and_metrics_vs_oracle"),
             ("test_gpu_fused_step", "test_ppo_step_two_action_chunks"),
             ("test_gpu_fused_step", "test_ppo_step_decoupled_loss_vs_oracle"),
             ("test_gpu_fused_step", "test_ppo_step_matches_unfused_chain")),
    "optimizer": (("test_gpu_mlp_shapes", "test_clip_adamw_shapes"),
                  ("test_gpu_fused_step", "test_optimizer_keeps_tile_image_in_step")),
    "loop": (("test_gpu_mlp_shapes", "test_whole_loop_at_reference_shapes"),),
}

# ---- the edges only Form::F32 has (plan_step, ppo_step_common.h: 64-row tiles, rows_per_slab rounded to 32, up to 2 * num_cu / 20
# slabs) ----------------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(42, 8, 1, True),   # Kin % 4 != 0: the scalar path of the first layer's B operand in ppo_step_dw_kernel
               (16, 9, 1, True)]   # Kin % 4 == 0: its float4 path, with the OP = 16 head of the fused kernel
# M -> slabs; None: the device's cap, min(2 * num_cu // 20, 25)
EDGE_M = {63: 1,      # one ragged 64-row tile
          64: 1,      # exactly one tile
          65: 1,      # a second tile holding one row
          257: 2,     # 2 slabs of 160 + 97 rows: the slab boundary lies inside the third tile, the second slab's last chunk has 1 row
          6400: None}  # rows_per_slab = 256 and the 25-slab cap on 256 CUs: the largest grid of ppo_step_dw_kernel


def _num_cu():
    import ctypes

    from rlinf_amd import _lib
    cu, wave = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.load().rlx_device_info(ctypes.byref(cu), ctypes.byref(wave)) == 0
    return cu.value


def plan_edge_case(shape, M, with_mask):
    """rlx_ppo_step at a tile / slab edge of the exact-f32 plan, against float64 with the bars of test_ppo_step_shapes (4 x the CPU
    f32 oracle's own distance + 2^-16 of the magnitude): the slab count the case was built for, every owned element of every slab
    written and finite (slabs start NaN there), every gap / phantom element still exactly 0, the summed gradient tensor by tensor,
    the metric row with the clip fraction exact."""
    import test_gpu_mlp_shapes as S
    import torch

    from rlinf_amd import ops
    from rlinf_amd._lib import PPO_OUT_NAMES
    D, A, C, vh = shape
    ora, pol = S._policies(shape, False, seed=11)
    o64 = S._f64(ora)
    owned = S._owned(pol)
    want_slabs = EDGE_M[M] if EDGE_M[M] is not None else min(2 * _num_cu() // 20, 25)
    slabs = ops.ppo_step_slabs(pol.layout, M)
    assert slabs == want_slabs, f"M={M}: {slabs} slabs, the case was built for {want_slabs}"
    g = torch.Generator().manual_seed(5 + M)
    mb = S._step_case(shape, M, g, with_mask,
                      lambda s, a: {k: v.detach().float() for k, v in o64.evaluate(s.double(), a.double()).items()})
    grads, row = S._run_step(pol, shape, mb, False)
    slab = grads.cpu()
    assert slab.shape[0] == slabs
    assert torch.isfinite(slab[:, owned]).all(), "an owned gradient element was never written"
    assert not slab[:, ~owned].any(), "a gap / phantom gradient element was written"
    got, host = slab.sum(0), row.cpu()
    keys = ("actor/ratio", "actor/clipped_ratio", "actor/approx_kl", "actor/policy_loss") + (("critic/value_loss",) if vh else ())
    res = {}
    for tag, model, cast in (("f64", o64, torch.float64), ("f32", ora, torch.float32)):
        model.zero_grad()
        mb_t = {k: (v.to(cast) if v.is_floating_point() else v) for k, v in mb.items()}
        loss, metrics = S._oracle_loss(shape, model.evaluate(mb_t["states"], mb_t["action"]), mb_t)
        loss.backward()
        res[tag] = (float(loss.detach()), {k: float(v) for k, v in metrics.items()},
                    {n: p.grad.detach().clone() for n, p in model.named_parameters()})
    (l64, m64, g64), (l32, m32, g32) = res["f64"], res["f32"]
    for name, w in g64.items():
        o = pol.offsets[name]
        S._check_f32(f"grad {name} M={M}", got[o:o + w.numel()], w.reshape(-1), g32[name].reshape(-1))
    assert float(host[PPO_OUT_NAMES["actor/clip_fraction"]]) == m64["actor/clip_fraction"]  # same branches, row by row
    for key, k64, k32 in (("loss", l64, l32),) + tuple((k, m64[k], m32[k]) for k in keys):
        err, own = abs(float(host[PPO_OUT_NAMES[key]]) - k64), abs(k32 - k64)
        assert err <= S.F32_MULT * own + S.F32_FLOOR * abs(k64) + 1e-9, (key, M, err, own)


# ---- the shared case list ------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, id_, fn, kwargs):
        self.id, self.fn, self.kwargs = id_, fn, kwargs

    def __repr__(self):
        return self.id


def _value_id(name, k, v):
    return str(v) if isinstance(v, (str, int, float, bool)) or v is None else f"{name}{k}"


def _param_sets(fn):
    """The function's own parametrize marks -> [(id, kwargs)], the nearest decorator's id first (pytest's order)."""
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names, values = mark.args[0], list(mark.args[1])
        names = [n.strip() for n in names.split(",")] if isinstance(names, str) else list(names)
        ids = mark.kwargs.get("ids")
        axis = []
        for k, v in enumerate(values):
            vals = tuple(v) if len(names) > 1 else (v,)
            assert len(vals) == len(names), (fn.__name__, names, v)
            id_ = str(ids[k]) if ids is not None else "-".join(_value_id(n, k, x) for n, x in zip(names, vals))
            axis.append((id_, dict(zip(names, vals))))
        axes.append(axis)
    out = []
    for combo in itertools.product(*axes):
        kwargs = {}
        for _, kw in combo:
            kwargs.update(kw)
        out.append(("-".join(i for i, _ in combo), kwargs))
    return out


def _is_f32(kwargs):
    return kwargs.get("prec", "f32") == "f32" and kwargs.get("bf16", False) is False


def cases(group):
    """The cases of one group, in the order the child runs them: the non-bf16 parameter sets of the existing functions (prec ==
    "f32" / bf16 is False), then -- in the step group -- the plan edges."""
    import importlib
    out = []
    for mod, name in _EXISTING[group]:
        fn = getattr(importlib.import_module(mod), name)
        for id_, kwargs in _param_sets(fn):
            if _is_f32(kwargs):
                out.append(Case(f"{group}::{name}" + (f"[{id_}]" if id_ else ""), fn, kwargs))
    if group == "step":
        for shape in EDGE_SHAPES:
            for M in EDGE_M:
                for with_mask in (False, True):
                    sid = "D%d-A%d-C%d-%s" % (shape[0], shape[1], shape[2], "v" if shape[3] else "novalue")
                    out.append(Case(f"step::plan_edge_case[{sid}-M{M}-{'mask' if with_mask else 'nomask'}]", plan_edge_case,
                                    dict(shape=shape, M=M, with_mask=with_mask)))
    assert len({c.id for c in out}) == len(out), "case ids collide"
    return out


# ---- the child -----------------------------------------------------------------------------------------------------------------
def _facts():
    """What proves the form: the f32 image of Form::F32 is 4 bytes per weight, exactly twice the bf16 image (the F32X image, three
    bf16 planes, is not), and its plan allows 2 * num_cu / 20 slabs where F32X's ring plan stops at (num_cu - 1) / 25."""
    import ctypes

    from rlinf_amd import _lib
    from rlinf_amd.models.embodiment.mlp_policy import MLPPolicy
    lib, lay = _lib.load(), MLPPolicy(42, 8, 1, True, False).layout
    return dict(tiles_bytes_f32=int(lib.rlx_mlp_tiles_bytes_for(ctypes.byref(lay), 0)),
                tiles_bytes_bf16=int(lib.rlx_mlp_tiles_bytes_for(ctypes.byref(lay), 1)),
                slabs_f32=int(lib.rlx_ppo_step_slabs_for(ctypes.byref(lay), FACTS_M, 0)), num_cu=_num_cu())


def main(argv):
    group, path = argv[1], argv[2]
    assert group in GROUPS, group
    if os.environ.get("RLX_F32_EXACT_MFMA") != "1":
        sys.stderr.write("exact_f32_child: start me with RLX_F32_EXACT_MFMA=1\n")
        return 2
    import pytest
    import torch
    with open(path, "w") as f:
        def put(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            os.fsync(f.fileno())

        t0 = time.time()
        torch.cuda.init()
        put(dict(facts=_facts(), group=group, startup_seconds=round(time.time() - t0, 3)))
        for case in cases(group):
            t0 = time.time()
            outcome, message = "passed", ""
            try:
                case.fn(**case.kwargs)
                torch.cuda.synchronize()
            except (AssertionError, pytest.fail.Exception) as e:
                outcome, message = "failed", "".join(traceback.format_exception_only(type(e), e)).strip()
            except pytest.skip.Exception as e:
                outcome, message = "skipped", str(e)
            except BaseException as e:  # noqa: BLE001 -- a HIP error or worse: nothing more runs on the GPU
                put(dict(id=case.id, outcome="error", message=traceback.format_exc()[-2000:], seconds=round(time.time() - t0, 3)))
                sys.stderr.write(f"exact_f32_child[{group}]: {case.id} ended the child: {type(e).__name__}: {e}\n")
                sys.stderr.flush()
                os._exit(3)  # no interpreter teardown: it would touch the device again
            put(dict(id=case.id, outcome=outcome, message=message[:2000], seconds=round(time.time() - t0, 3)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
