"""GPU: the one call path of the binding (_lib.bind / _lib.call behind ops.call) on a device.  An argument that does not fit the header's declaration is
refused on the host, before any launch, and the stream that ops.call fills in is the current one.  Tiny inputs: random blobs, D = 8, 64 points."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("one-2-3-45_amd._lib")
ops = importlib.import_module("one-2-3-45_amd.ops")

D, P = 8, 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def test_misdeclared_arguments_are_refused_before_any_launch(dev):
    g = torch.Generator().manual_seed(0)
    blob = (0.1 * torch.randn(_lib.call("o2345_sdf_blob_floats"), generator=g)).to(dev)
    vol_cl = (0.1 * torch.randn(D, D, D, 16, generator=g)).to(dev)
    pts4 = (torch.rand(P, 4, generator=g) * 2 - 1).to(dev)
    pts = pts4[:, :3].contiguous()
    index = torch.arange(P - 1, -1, -1, dtype=torch.int32, device=dev)          # every slot, so that every output element is written
    want = _bits(ops.sdf_mlp(blob, vol_cl, pts, index=index)["sdf"])
    with pytest.raises(ValueError, match=r"o2345_sdf_\w+: index: expected .*int32.*int64"):
        ops.sdf_mlp(blob, vol_cl, pts, index=index.long())
    with pytest.raises(ValueError, match=r"o2345_sdf_\w+: pts: expected .*contiguous=False"):
        ops.sdf_mlp(blob, vol_cl, pts4[:, :3], index=index)
    assert torch.equal(_bits(ops.sdf_mlp(blob, vol_cl, pts, index=index)["sdf"]), want)


def test_the_stream_filled_in_is_the_current_one(dev):
    """The points are written on a side stream behind a queue of slow kernels; view_count, called under that stream, must see them.  A launch on any
    other stream (side streams do not synchronise with the default one) would read the zeros that are there before."""
    g = torch.Generator().manual_seed(1)
    V, H, W = 2, 16, 16
    proj = torch.tensor([[20.0, 0.0, 8.0, 24.0], [0.0, 20.0, 8.0, 24.0], [0.0, 0.0, 1.0, 3.0]]).repeat(V, 1, 1).contiguous().to(dev)     # K [I | (0, 0, 3)]
    maskvol = torch.ones(D ** 3, device=dev)
    real = (torch.rand(P, 3, generator=g) * 2 - 1).to(dev)
    want = ops.view_count(real, maskvol, D, proj, V, H, W).cpu()
    assert not torch.equal(want, ops.view_count(torch.zeros_like(real), maskvol, D, proj, V, H, W).cpu())      # the check below can tell the two apart
    pts = torch.zeros_like(real)
    busy = torch.ones(1 << 24, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy.cumsum(0)
        pts.copy_(real)
        out = ops.view_count(pts, maskvol, D, proj, V, H, W)
    s.synchronize()
    assert torch.equal(out.cpu(), want)
