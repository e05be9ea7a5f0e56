"""The one launcher every wrapper goes through (rlinf_amd/_lib.py: launch, workspace): how it marshals arguments, which stream it
launches on and how a library error surfaces.  Needs a real MI355X: run with `pytest -m gpu`."""

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1003  # odd, several wavefronts, one block


def _mods():
    from rlinf_amd import _lib, ops
    return _lib, ops


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, generator=g)
    mask = torch.rand(N, generator=g) < 0.6
    return x, mask


def _stats64(x, mask=None):
    v = x.double() if mask is None else x.double()[mask]
    return torch.stack([torch.tensor(float(v.numel()), dtype=torch.float64), v.sum(), v.square().sum()])


def test_error_names_the_call_and_carries_the_library_message(data):
    _lib, _ = _mods()
    x = data[0].cuda()
    dev = x.device
    stats = torch.zeros(3, dtype=torch.float64, device=dev)
    ws = _lib.workspace(dev, 8)
    with pytest.raises(_lib.RlxError) as e:
        _lib.launch("rlx_masked_stats", dev, x, None, N, stats, 0, ws, ws.numel())
    assert "rlx_masked_stats" in str(e.value) and "workspace too small" in str(e.value)


def test_none_is_null_and_a_tensor_is_its_pointer(data):
    _, ops = _mods()
    x, mask = data
    # the bars of test_gpu_advantages' masked_stats checks
    torch.testing.assert_close(ops.masked_stats(x.cuda(), None).cpu(), _stats64(x), rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(ops.masked_stats(x.cuda(), mask.cuda()).cpu(), _stats64(x, mask), rtol=1e-12, atol=1e-9)


def _normalized_on_the_default_stream(x):
    _, ops = _mods()
    stats = ops.masked_stats(x)
    want = ops.normalize_from_stats(x, stats)
    torch.cuda.synchronize(x.device)
    return stats, want


def test_the_stream_is_read_at_call_time(data):
    _, ops = _mods()
    x = data[0].cuda()
    stats, want = _normalized_on_the_default_stream(x)
    side = torch.cuda.Stream(x.device)
    with torch.cuda.stream(side):
        got = ops.normalize_from_stats(x, stats)
    side.synchronize()
    assert torch.equal(got, want)


def test_an_explicit_stream_is_used_as_given(data):
    _lib, _ = _mods()
    x = data[0].cuda()
    stats, want = _normalized_on_the_default_stream(x)
    side = torch.cuda.Stream(x.device)
    got = torch.empty_like(x)
    _lib.launch("rlx_normalize_from_stats", x.device, x, stats, got, N, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(got, want)


def test_a_cpu_tensor_is_refused_before_any_launch(data):
    _lib, ops = _mods()
    with pytest.raises(_lib.RlxError, match="no CPU fallback"):
        ops.masked_stats(data[0])
