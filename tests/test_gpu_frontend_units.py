"""The volume front end's glue kernels, one by one, against the float64 references of tests/frontend_ref.py (themselves checked on the CPU by
tests/test_frontend_ref_cpu.py, which also asserts that the shared seeded inputs exercise the edges named below).

Shapes are the smallest at which each kernel takes another path: maps of less than a wave, a ragged last wave, a ragged last block, dead waves that
still run the LDS transpose (csrc/featmaps.hip); row counts around one block's share and past the 1024-block cap of the partial sums (csrc/sparse.hip);
dilation boxes clipped by the volume on one or both sides and |sdf| == threshold (csrc/costvol.hip); pixel counts around the 64-pixel tile of the
layout kernels (csrc/block_kernels.h, csrc/color_maps.hip).

Tolerance: the convention of tests/test_gpu_parity.py -- per compared tensor, max |error| <= 2e-5 * max(1, max |reference|); integer, mask and pure
data-movement outputs bit for bit.  Every float comparison prints its measured error."""
import ctypes
import importlib

import pytest
import torch

import frontend_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


def close(got, ref, what, rel=2e-5):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    scale = max(1.0, ref.abs().max().item() if ref.numel() else 1.0)
    print(f"{what}: max err {err:.3e} (bound {rel * scale:.3e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel:.1e} * {scale:.3g}"
    return err


def on(dev, d):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ k_fpn_level<8|16>
@pytest.mark.parametrize("C,with_ss,shape", R.FPN_CASES)
def test_fpn_level(dev, ops, C, with_ss, shape):
    d = R.fpn_inputs(C, with_ss, shape)
    g = on(dev, d)
    got = ops.fpn_level(g["fine"], g["coarse"], g["weight"], g["bias"], g["fine_ss"], R.FPN_SLOPE)
    ref = R.fpn_level(d["fine"], d["coarse"], d["weight"], d["bias"], d["fine_ss"], R.FPN_SLOPE)
    close(got, ref, f"fpn_level C={C} ss={with_ss} {shape}")


def test_fpn_level_rejects_bad_shapes(dev, ops):
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(ValueError):
        ops.fpn_level(z(1, 8, 5, 6), z(1, 32, 2, 3), z(32, 8), z(32))            # odd H
    with pytest.raises(ValueError):
        ops.fpn_level(z(1, 4, 4, 6), z(1, 32, 2, 3), z(32, 4), z(32))            # C = 4
    with pytest.raises(ValueError):
        ops.fpn_level(z(1, 8, 4, 6), z(1, 32, 2, 2), z(32, 8), z(32))            # coarse map of the wrong shape


# ------------------------------------------------------------------------------------------------ k_pyramid_pack
def _pyramid_pack_into(ops, g, fm, cm):
    """ops.pyramid_pack's call on caller-allocated outputs."""
    L = importlib.import_module("one-2-3-45_amd._lib")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    V, _, H, W = g["s0"].shape
    with torch.cuda.device(cm.device):
        L.check(L.lib().o2345_pyramid_pack(p(g["f2"]), p(g["s1"]), p(g["s0"]), p(g["rgb"]), V, H, W, p(fm), p(cm),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pyramid_pack")


@pytest.mark.parametrize("want_nchw", [True, False])
@pytest.mark.parametrize("shape", R.PYRAMID_SHAPES)
def test_pyramid_pack(dev, ops, shape, want_nchw):
    V, H, W = shape
    d = R.pyramid_inputs(shape)
    g = on(dev, d)
    fm, cm = ops.pyramid_pack(g["f2"], g["s1"], g["s0"], g["rgb"], want_nchw=want_nchw)
    rfm, rcm = R.pyramid(d["f2"], d["s1"], d["s0"], d["rgb"])
    assert tuple(cm.shape) == (V, H, W, 64)
    close(cm, rcm, f"pyramid_pack cmaps {shape} nchw={want_nchw}")
    assert torch.equal(cm[..., :3].cpu(), d["rgb"].permute(0, 2, 3, 1))             # rgb passes through untouched
    assert torch.equal(cm[..., 51:59].cpu(), d["s0"].permute(0, 2, 3, 1))
    assert torch.equal(cm[..., 59:].cpu(), torch.zeros(V, H, W, 5))                 # pad channels exactly 0
    if want_nchw:
        close(fm, rfm, f"pyramid_pack fmaps {shape}")
        assert torch.equal(cm[..., 3:59].cpu(), fm.permute(0, 2, 3, 1).cpu())       # one value, written twice
    else:
        assert fm is None
    # every element of the outputs is written: the same call into sentinel-filled buffers gives the same bits
    cm2 = torch.full((V, H, W, 64), float("nan"), device=dev)
    fm2 = torch.full((V, 56, H, W), float("nan"), device=dev) if want_nchw else None
    _pyramid_pack_into(ops, g, fm2, cm2)
    assert not torch.isnan(cm2).any() and torch.equal(cm2, cm)
    if want_nchw:
        assert not torch.isnan(fm2).any() and torch.equal(fm2, fm)


def test_pyramid_pack_rejects_bad_shapes(dev, ops):
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(ValueError):
        ops.pyramid_pack(z(1, 32, 1, 2), z(1, 16, 3, 4), z(1, 8, 6, 8), z(1, 3, 6, 8))           # H = 6


# ------------------------------------------------------------------------------------------------ o2345_bn_act_rows
@pytest.mark.parametrize("cfg", list(R.BN_CONFIGS))
@pytest.mark.parametrize("C,n", [(C, n) for C in R.BN_CHANNELS for n in R.bn_sizes(C)])
def test_bn_act_rows(dev, ops, C, n, cfg):
    """The three configurations the product runs, at every row count where the kernels take another path.  With a single row every channel has zero
    variance and y is beta exactly: the x * scale + shift form that k_bn_act used to evaluate missed that by up to 1.7e-4 (8.5 times the bound; scale is
    gamma / sqrt(eps) = 316 gamma there); the centred form it evaluates now measures 1e-7 there and at most 1.1e-6 over all cases."""
    d = R.bn_inputs(C, n, cfg)
    g = on(dev, d)
    want_stats = cfg == "identity_stats"
    out = ops.bn_act_rows(g["x"], g["gamma"], g["beta"], R.BN_EPS, slope=d["slope"], abs_gamma=d["abs_gamma"], skip=g["skip"], want_stats=want_stats)
    y, mv = out if want_stats else (out, None)
    ry, rmean, rvar = R.bn_rows(d["x"], d["gamma"], d["beta"], R.BN_EPS, d["slope"], d["abs_gamma"], d["skip"])
    close(y, ry, f"bn_act_rows y C={C} n={n} {cfg}")
    if want_stats:
        assert tuple(mv.shape) == (2, C)
        close(mv[0], rmean, f"bn_act_rows mean C={C} n={n}")
        close(mv[1], rvar, f"bn_act_rows var C={C} n={n}")


@pytest.mark.parametrize("C", R.BN_CHANNELS)
def test_bn_act_rows_no_rows(dev, ops, C):
    x, g, b = torch.empty(0, C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    y = ops.bn_act_rows(x, g, b)
    assert tuple(y.shape) == (0, C) and y.dtype == torch.float32 and y.device == x.device
    y, mv = ops.bn_act_rows(x, g, b, slope=1.0, want_stats=True)
    assert tuple(y.shape) == (0, C) and torch.equal(mv.cpu(), torch.zeros(2, C))


def test_shim_batchnorm_running_statistics(dev):
    """spnn.BatchNorm: two training-mode forwards (2 rows, then 777), then an eval-mode forward, against nn.BatchNorm1d in float64."""
    ts = importlib.import_module("one-2-3-45_amd.shims.torchsparse")
    d = R.shim_bn_inputs()
    C = R.SHIM_BN_C
    bn, ref = ts.nn.BatchNorm(C).to(dev), torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"])
        ref.weight.copy_(d["gamma"]); ref.bias.copy_(d["beta"])
    sparse = lambda f: ts.SparseTensor(f.to(dev), torch.zeros(f.shape[0], 4, dtype=torch.int32, device=dev))
    for i, f in enumerate(d["batches"]):
        close(bn(sparse(f)).F, ref(f.double()).detach(), f"shim BatchNorm training forward {i} ({f.shape[0]} rows)")
        close(bn.running_mean, ref.running_mean, f"shim BatchNorm running_mean after forward {i}")
        close(bn.running_var, ref.running_var, f"shim BatchNorm running_var after forward {i}")
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 2
    bn.eval(); ref.eval()
    f = d["batches"][1]
    close(bn(sparse(f)).F, ref(f.double()).detach(), "shim BatchNorm eval forward")
    assert int(bn.num_batches_tracked) == 2


# ------------------------------------------------------------------------------------------------ k_prune_dilate
@pytest.mark.parametrize("D,r", R.PRUNE_CASES)
def test_prune_dilate(dev, ops, D, r):
    d = R.prune_inputs(D, r)
    got = ops.prune_dilate(d["sdf"].to(dev), d["mask"].to(dev), D, d["thr"], r)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), R.prune_dilate(d["sdf"], d["mask"], D, d["thr"], r))


def test_prune_dilate_corners(dev, ops):
    d = R.prune_corner_inputs()
    got = ops.prune_dilate(d["sdf"].to(dev), d["mask"].to(dev), d["D"], d["thr"], d["r"])
    assert torch.equal(got.cpu(), R.prune_dilate(d["sdf"], d["mask"], d["D"], d["thr"], d["r"]))


# ------------------------------------------------------------------------------------------------ layout kernels
@pytest.mark.parametrize("C,hw", R.NHWC_CASES)
def test_nchw_to_nhwc(dev, ops, C, hw):
    x = R.nhwc_inputs(C, hw)
    got = ops.nchw_to_nhwc(x.to(dev))
    assert got.is_contiguous() and torch.equal(got.cpu(), R.nchw_to_nhwc(x))


@pytest.mark.parametrize("shape", R.PACK_SHAPES)
def test_pack_color_maps(dev, ops, shape):
    d = R.pack_inputs(shape)
    got = ops.pack_color_maps(d["feat"].to(dev), d["rgb"].to(dev))
    assert torch.equal(got.cpu(), R.pack_color_maps(d["feat"], d["rgb"]))


@pytest.mark.parametrize("want_cf", [True, False])
@pytest.mark.parametrize("C,dims", R.SCATTER_CASES)
def test_scatter_dense(dev, ops, C, dims, want_cf):
    d = R.scatter_inputs(C, dims)
    cl, cf, mask = ops.scatter_dense(d["rows"].to(dev), d["row_of_voxel"].to(dev), dims, want_cf=want_cf)
    rcl, rcf, rmask = R.scatter_dense(d["rows"], d["row_of_voxel"], dims)
    assert torch.equal(cl.cpu(), rcl) and torch.equal(mask.cpu(), rmask)
    assert torch.equal(cf.cpu(), rcf) if want_cf else cf is None


@pytest.mark.parametrize("want_cf", [True, False])
@pytest.mark.parametrize("C", [8, 16])
def test_scatter_dense_no_rows(dev, ops, C, want_cf):
    dims = (5, 6, 7)
    row = torch.full((5 * 6 * 7,), -1, dtype=torch.int32)
    cl, cf, mask = ops.scatter_dense(torch.empty(0, C, device=dev), row.to(dev), dims, want_cf=want_cf)
    rcl, rcf, rmask = R.scatter_dense(torch.empty(0, C), row, dims)
    assert torch.equal(cl.cpu(), rcl) and torch.equal(mask.cpu(), rmask)
    assert torch.equal(cf.cpu(), rcf) if want_cf else cf is None
