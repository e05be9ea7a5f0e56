"""The two device passes of the async-PPO rollout store against torch on the same tensors: rlx_version_stats (min bit-equal,
integer sum and histogram exact, half-to-even rounding, deterministic) and rlx_gather_rows_segmented (bit-equal to
torch.cat(dim=1) + flatten + index_select, and to rlx_gather_rows for a single slot)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _torch_stats(v: torch.Tensor, base: int, n_bins: int):
    r = torch.round(v.reshape(-1)).to(torch.int64)  # buffer.py:1185
    d = r - base
    inside = (d >= 0) & (d < n_bins)
    counts = torch.bincount(d[inside], minlength=n_bins).tolist()
    return dict(min=v.min(), sum=int(r.sum()), n=v.numel(), below=int((d < 0).sum()), above=int((d >= n_bins).sum()), counts=counts)


def _check_stats(v: torch.Tensor, base: int, n_bins: int = 64):
    from rlinf_amd import ops
    st = ops.version_stats(v, base, n_bins)
    want = _torch_stats(v.cpu(), base, n_bins)
    assert torch.tensor(st.min, dtype=torch.float32).view(torch.int32).item() == want["min"].view(torch.int32).item(), "min bits"
    assert (st.n, st.sum, st.below, st.above, st.n_bins, st.base) == (want["n"], want["sum"], want["below"], want["above"], n_bins, base)
    assert list(st.count[:n_bins]) == want["counts"]
    again = ops.version_stats(v, base, n_bins)
    assert bytes(st) == bytes(again), "two runs differ"
    return st


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 1023, 4097, 65536 + 3, 128 * 1024 * 8])
def test_version_stats_matches_torch_at_every_size(n):
    g = torch.Generator().manual_seed(n)
    v = torch.randint(3, 9, (n,), generator=g).float().to(DEV)
    _check_stats(v, 3, 6)
    _check_stats(v, 0)


def test_version_stats_on_trajectory_shaped_versions():
    """The bench shape, as the learner sees it: one version, then two halves one version apart."""
    v = torch.full((128, 1024, 8), 17.0, device=DEV)
    st = _check_stats(v, 10)
    assert st.count[7] == v.numel() and st.min == 17.0
    v[:64] = 16.0
    st = _check_stats(v, 10)
    assert (st.count[6], st.count[7]) == (v.numel() // 2, v.numel() // 2) and st.sum == 16 * (v.numel() // 2) + 17 * (v.numel() // 2)


def test_version_stats_rounds_half_to_even():
    v = torch.tensor([0.5, 1.5, 2.5, 3.5, 4.5, -0.5, -1.5, 2.4999998, 2.5000002, 7.0], device=DEV)
    st = _check_stats(v, -2, 12)
    # torch.round: 0, 2, 2, 4, 4, -0, -2, 2, 3, 7
    assert st.sum == 0 + 2 + 2 + 4 + 4 + 0 - 2 + 2 + 3 + 7
    assert st.count[0] == 1 and st.count[2] == 2 and st.count[4] == 3 and st.count[6] == 2


def test_version_stats_counts_below_and_above_the_bin_range():
    g = torch.Generator().manual_seed(5)
    v = (torch.randint(-20, 120, (100003,), generator=g).float() + torch.rand(100003, generator=g) * 0.4).to(DEV)
    st = _check_stats(v, 10, 64)
    assert st.below > 0 and st.above > 0
    assert st.below + st.above + sum(st.count[:64]) == v.numel()


def test_version_stats_at_an_unaligned_address():
    """A view that starts 4 bytes into an allocation: scalar head, 16-byte body, scalar tail."""
    g = torch.Generator().manual_seed(9)
    for off in (1, 2, 3):
        for n in (1, 2, 6, 1000, 4099):
            v = torch.randint(0, 5, (n + off,), generator=g).float().to(DEV)[off:]
            assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
            _check_stats(v, 0, 8)


# ---- segmented gather ----------------------------------------------------------------------------------------------------------
def _slots(T, envs, row_bytes, g, extra_row=False):
    """Per-slot contiguous [T(+1), B_s, row] blocks whose row type has the alignment of row_bytes."""
    rows = T + 1 if extra_row else T
    if row_bytes % 4 == 0:
        return [torch.randn(rows, b, row_bytes // 4, generator=g).to(DEV) for b in envs]
    return [torch.randint(0, 255, (rows, b, row_bytes), generator=g, dtype=torch.uint8).to(DEV) for b in envs]


def _want(slots, index, T):
    cat = torch.cat(slots, dim=1)
    if index is None:
        return cat
    return cat[:T].reshape(-1, *cat.shape[2:]).index_select(0, index)


ENVS = {1: [[5], [1]], 2: [[4, 4], [1, 7], [6, 1]], 3: [[3, 3, 3], [1, 5, 2]], 16: [[2] * 16, [1, 3, 2, 5, 1, 1, 4, 2, 3, 1, 6, 2, 1, 2, 3, 1]]}


@pytest.mark.parametrize("S", [1, 2, 3, 16])
@pytest.mark.parametrize("with_index", [False, True])
def test_segmented_gather_equals_cat_flatten_index_select(S, with_index):
    from rlinf_amd import ops
    T = 7
    for envs in ENVS[S]:
        g = torch.Generator().manual_seed(100 * S + len(envs) + sum(envs))
        sum_b = sum(envs)
        # T-row and (T + 1)-row fields in one launch, every row size
        fields = [_slots(T, envs, rb, g, extra_row=extra) for rb in (1, 4, 28, 32, 168, 256) for extra in (False, True)]
        index = None
        if with_index:
            index = torch.randperm(T * sum_b, generator=g)[: max(1, (T * sum_b * 3) // 4)].to(DEV)
        got = ops.gather_rows_segmented(fields, index)
        for f, out in zip(fields, got):
            assert torch.equal(out, _want(f, index, T)), (S, envs, f[0].shape, f[0].dtype)


def test_segmented_gather_sixteen_fields_and_more():
    from rlinf_amd import ops
    g = torch.Generator().manual_seed(3)
    T, envs = 5, [3, 1, 4]
    for n_fields in (16, 19):  # 19: a second launch
        fields = [_slots(T, envs, (1, 4, 28, 32, 168, 256)[i % 6], g, extra_row=bool(i % 2)) for i in range(n_fields)]
        index = torch.randperm(T * sum(envs), generator=g).to(DEV)
        for idx in (None, index):
            for f, out in zip(fields, ops.gather_rows_segmented(fields, idx)):
                assert torch.equal(out, _want(f, idx, T))


def test_segmented_gather_of_one_slot_equals_gather_rows():
    from rlinf_amd import ops
    g = torch.Generator().manual_seed(4)
    T, B = 9, 13
    fields = [_slots(T, [B], rb, g) for rb in (1, 4, 28, 32, 168, 256)]
    index = torch.randperm(T * B, generator=g).to(DEV)
    seg = ops.gather_rows_segmented(fields, index)
    plain = ops.gather_rows([f[0].reshape(T * B, -1) for f in fields], index)
    for a, b in zip(seg, plain):
        assert a.dtype == b.dtype and torch.equal(a.reshape(b.shape), b)
        assert a.contiguous().view(torch.uint8).reshape(-1).equal(b.contiguous().view(torch.uint8).reshape(-1))


def test_segmented_gather_at_unaligned_slot_addresses():
    """Slots that start 4 bytes into an allocation: the kernel falls back to the widest word every pointer allows."""
    from rlinf_amd import ops
    g = torch.Generator().manual_seed(6)
    T, envs = 4, [3, 2]
    slots = []
    for b in envs:
        raw = torch.randn(T * b * 8 + 1, generator=g).to(DEV)
        slots.append(raw[1:].view(T, b, 8))
        assert slots[-1].data_ptr() % 16 == 4
    index = torch.randperm(T * sum(envs), generator=g).to(DEV)
    assert torch.equal(ops.gather_rows_segmented([slots], index)[0], _want(slots, index, T))
    assert torch.equal(ops.gather_rows_segmented([slots], None)[0], _want(slots, None, T))


def test_segmented_gather_skips_rows_outside_the_field():
    """An index entry outside [0, t_rows * sum B) is not read: its destination row keeps what it held."""
    from rlinf_amd import ops
    T, envs = 3, [2, 2]
    slots = [torch.arange(T * b * 4, dtype=torch.float32, device=DEV).view(T, b, 4) + 1000 * s for s, b in enumerate(envs)]
    index = torch.tensor([0, T * 4, -1, 5, 1 << 40], dtype=torch.int64, device=DEV)
    out = torch.full((5, 4), -7.0, device=DEV)
    ops.gather_rows_segmented([slots], index, [out])
    flat = torch.cat(slots, dim=1).reshape(-1, 4)
    assert torch.equal(out[0], flat[0]) and torch.equal(out[3], flat[5])
    assert bool((out[[1, 2, 4]] == -7.0).all())


def test_segmented_gather_at_the_learner_field_set():
    """The async learner's slot fields at a mid-size shape: states 168 B, action / log-probs / versions 32 B, prev_values 4 B
    with its closing row, shuffled."""
    from rlinf_amd import ops
    g = torch.Generator().manual_seed(8)
    T, envs = 32, [64, 64]
    fields = [_slots(T, envs, 168, g), _slots(T, envs, 32, g), _slots(T, envs, 32, g), _slots(T, envs, 32, g),
              _slots(T, envs, 4, g, extra_row=True)]
    index = torch.randperm(T * sum(envs), generator=g).to(DEV)
    for f, out in zip(fields, ops.gather_rows_segmented(fields, index)):
        assert torch.equal(out, _want(f, index, T))
