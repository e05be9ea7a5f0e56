"""The hand-off stores of the optimizer step's launches (rlinf_amd/csrc/rlx_store.h): what the fused launch and the weight-gradient
launches leave for the next launch is written through to memory instead of staying dirty in L2.  A write-through store that is
clipped by its buffer range, skipped on a ragged block or mis-sized would leave bytes of the destination as they were, so

1. the fused step's results must not depend on what the workspace and the gradient slabs held before (all-zero against all-ones
   bytes), and
2. a chain of optimizer steps must leave the same parameters, moments and weight image whether launched eagerly or replayed from a
   captured graph, the image being the one a fresh pack of the parameters gives.

Nothing here is compared within a tolerance: every check is bit for bit."""

import pytest
import torch

pytestmark = pytest.mark.gpu

OBS, ACT = 42, 8


def _policy(bf16):
    from rlinf_amd.models.embodiment.mlp_policy import MLPPolicy
    torch.manual_seed(13)
    pol = MLPPolicy(OBS, ACT, 1, True, False, compute_dtype=torch.bfloat16 if bf16 else torch.float32)
    return pol.to("cuda")


def _loss_params():
    from rlinf_amd import ops
    return ops.make_ppo_params(logprob_type="action_level", action_dim=ACT, chunks=1, clip_ratio_low=0.2, clip_ratio_high=0.2,
                               value_clip=1.0, huber_delta=10.0, max_episode_steps=50, has_critic=True)


def _minibatch(M, seed):
    g = torch.Generator().manual_seed(seed)
    mb = dict(states=torch.randn(M, OBS, generator=g), action=torch.randn(M, ACT, generator=g) * 0.6,
              prev_logprobs=torch.randn(M, ACT, generator=g) * 0.1 - 1.0, advantages=torch.randn(M, 1, generator=g),
              prev_values=torch.randn(M, 1, generator=g), returns=torch.randn(M, 1, generator=g))
    return {k: v.cuda().contiguous() for k, v in mb.items()}


def _bits(t):
    return t.contiguous().view(torch.uint8)


# ---- 1. every hand-off byte is written ------------------------------------------------------------------------------------------
# bf16: 5 (one ragged tile), 33 (a second tile of one row), 700 (many tiles, ragged, the LDS weight-gradient kernel), 4136 (the
# smallest ragged shape on the ring path, which starts at 4096 rows).  Precision 32 takes the ring path at every size.
@pytest.mark.parametrize("M,bf16", [(5, True), (33, True), (700, True), (4136, True), (5, False), (33, False), (700, False)])
def test_step_results_do_not_depend_on_what_the_buffers_held(M, bf16):
    from rlinf_amd import ops
    from rlinf_amd._lib import PPO_OUT_FLOATS
    pol = _policy(bf16)
    lay, lp, mb = pol.layout, _loss_params(), _minibatch(M, 100 + M)
    params = pol.flat.data
    slabs = ops.ppo_step_slabs(lay, M, bf16=bf16)
    runs = []
    for fill in (0x00, 0xFF):
        ws = torch.full((ops.ppo_step_workspace_bytes(lay, M),), fill, dtype=torch.uint8, device="cuda")
        grads = torch.full((slabs * lay.n_params * 4,), fill, dtype=torch.uint8, device="cuda").view(torch.float32).view(slabs, lay.n_params)
        row = torch.zeros(PPO_OUT_FLOATS, device="cuda")
        ops.ppo_step(params, lay, lp, mb, grads, row, ws, grad_out=1.0, bf16=bf16)
        torch.cuda.synchronize()
        runs.append((grads.cpu(), row.cpu()))
    (g0, r0), (g1, r1) = runs
    assert torch.isfinite(g1).all() and torch.isfinite(r1).all()
    assert torch.isfinite(g0).all() and torch.isfinite(r0).all()
    assert bool(g0.any()), "the step left no gradient at all"
    diff = _bits(g0) != _bits(g1)
    assert not bool(diff.any()), f"{int(diff.sum())} gradient bytes depend on the buffers' previous content"
    assert torch.equal(_bits(r0), _bits(r1)), "the metric row depends on the buffers' previous content"


# ---- 2. optimizer outputs land where the next launch reads them --------------------------------------------------------------------
def _sync_words(n):
    """Sync words of the one-launch form, whatever the process's default form is."""
    from rlinf_amd import _lib
    return torch.zeros((int(_lib.load().rlx_adamw_sync_words(int(n))),), dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("M,bf16,one_launch", [(4136, True, True), (96, False, True), (96, True, False), (96, False, False)],
                         ids=["bf16-4136-one", "f32-96-one", "bf16-96-two", "f32-96-two"])
def test_six_steps_eager_equal_replayed_and_image_equals_a_fresh_pack(M, bf16, one_launch):
    """fused -> weight gradients -> optimizer, six times with six different minibatches: once launched eagerly, once as a graph of
    three steps replayed twice (the minibatch buffers rewritten in between).  Every launch reads what the one in front wrote."""
    from rlinf_amd import _lib, ops
    from rlinf_amd._lib import PPO_OUT_FLOATS
    pol = _policy(bf16)
    lay, lp = pol.layout, _loss_params()
    n = lay.n_params
    fresh = [_minibatch(M, 200 + k) for k in range(6)]
    groups = [(0, n // 2, 1e-3), (n // 2, n, 3e-3)]
    slabs = ops.ppo_step_slabs(lay, M, bf16=bf16)
    results = []
    for replayed in (False, True):
        p = pol.flat.data.clone()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        tiles = ops.mlp_pack_tiles(p, lay, bf16=bf16)
        bufs = [{k: torch.empty_like(t) for k, t in fresh[0].items()} for _ in range(3)]
        grads = torch.zeros(slabs, n, device="cuda")
        rows = torch.zeros(3, PPO_OUT_FLOATS, device="cuda")
        ws = torch.zeros(ops.ppo_step_workspace_bytes(lay, M), dtype=torch.uint8, device="cuda")
        stats, state = torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        aws = torch.empty(_lib.load().rlx_adamw_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        sync = _sync_words(n) if one_launch else None
        fused = [ops.PreparedPpoStep(p, lay, lp, bufs[k], grads, rows[k], ws, grad_out=1.0, tiles=tiles, bf16=bf16) for k in range(3)]
        adam = ops.PreparedAdamw(p, grads, m, v, groups, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=0.5,
                                 grad_scale=1.0, stats=stats, step_state=state, workspace=aws, tile_layout=lay, tiles=tiles, sync=sync)

        def three(stream):
            for k in range(3):
                fused[k](stream)
                adam(stream)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if replayed:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    three(side.cuda_stream)
                # the capture ran nothing; the buffers are as they were set up
            for r in range(2):
                for k in range(3):
                    for name, t in fresh[3 * r + k].items():
                        bufs[k][name].copy_(t)
                if replayed:
                    graph.replay()
                else:
                    three(side.cuda_stream)
        side.synchronize()
        torch.cuda.synchronize()
        assert int(state[0]) + int(state[1]) == 6 and float(stats[1]) == 1.0, (replayed, state, stats)
        if sync is not None:
            assert int(sync[1]) == 0, "the exchange expired (sticky word set)"
            assert int(sync[0]) == 6, "a step of the one-launch request fell back to two launches"
        packed = ops.mlp_pack_tiles(p, lay, bf16=bf16)
        torch.cuda.synchronize()
        assert torch.equal(_bits(tiles), _bits(packed)), "the weight image the optimizer kept is not a fresh pack of the parameters"
        results.append([t.cpu() for t in (p, m, v, tiles)])
    assert not torch.equal(results[0][0], pol.flat.data.cpu())
    for a, b, name in zip(results[0], results[1], ("parameters", "exp_avg", "exp_avg_sq", "weight image")):
        if name != "weight image":  # (its bytes are bf16 tiles, whatever dtype the tensor carries)
            assert torch.isfinite(a).all(), name
        assert torch.equal(_bits(a), _bits(b)), f"replayed vs eager: {name}"
