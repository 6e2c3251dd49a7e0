"""The float64 references of tests/frontend_ref.py against independent implementations, on the CPU -- and the conditions that the shared seeded
inputs must meet so that tests/test_gpu_frontend_units.py exercises the edges it was written for (a seed that stops doing so fails HERE).

Each float test prints the error of ATen's float32 result against the float64 reference: the yardstick next to which the HIP kernels' errors are read."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fake_ops
import frontend_ref as R


def err(a, b):
    return (a.double() - b.double()).abs().max().item() if a.numel() else 0.0


def scale(ref):
    return max(1.0, ref.abs().max().item() if ref.numel() else 1.0)


# ------------------------------------------------------------------------------------------------ bilinear up-sampling
@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (6, 1), (3, 4), (9, 7)])
def test_bilinear_up_vs_aten_float64(factor, hw):
    x = torch.from_numpy(np.random.default_rng(hw[0] * 16 + hw[1]).normal(0, 1, (2, 3) + hw))
    want = F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=True)
    got = R.bilinear_up(x, factor)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert err(got, want) <= 1e-14 * scale(want)
    e32 = err(F.interpolate(x.float(), scale_factor=factor, mode="bilinear", align_corners=True), got)
    print(f"bilinear x{factor} {hw}: ATen fp32 err {e32:.3e}")


# ------------------------------------------------------------------------------------------------ fpn_level, pyramid
@pytest.mark.parametrize("C,with_ss,shape", R.FPN_CASES)
def test_fpn_level_vs_fake_ops(C, with_ss, shape):
    d = R.fpn_inputs(C, with_ss, shape)
    ref = R.fpn_level(d["fine"], d["coarse"], d["weight"], d["bias"], d["fine_ss"], R.FPN_SLOPE)
    f32 = fake_ops.fpn_level(d["fine"], d["coarse"], d["weight"], d["bias"], d["fine_ss"], R.FPN_SLOPE)          # ATen in float32: agreement to 1e-6 of the map's magnitude
    assert f32.dtype == torch.float32 and tuple(ref.shape) == (shape[0], 32, shape[1], shape[2])
    e = err(f32, ref)
    print(f"fpn_level C={C} ss={with_ss} {shape}: ATen fp32 err {e:.3e} (max |ref| {ref.abs().max():.3g})")
    assert e <= 1e-6 * scale(ref)
    if with_ss:                     # both leaky branches are taken often enough to matter
        t = R.fpn_preactivations(d)
        assert (t < 0).double().mean() >= 0.10 and (t > 0).double().mean() >= 0.10
        assert d["fine_ss"][:C].abs().max() <= 1.5 and (d["fine_ss"][:C] < 0).any() and (d["fine_ss"][:C] > 0).any()


@pytest.mark.parametrize("shape", R.PYRAMID_SHAPES)
def test_pyramid_vs_fake_ops(shape):
    d = R.pyramid_inputs(shape)
    fm, cm = R.pyramid(d["f2"], d["s1"], d["s0"], d["rgb"])
    fm32, cm32 = fake_ops.pyramid_pack(d["f2"], d["s1"], d["s0"], d["rgb"])
    V, H, W = shape
    assert tuple(fm.shape) == (V, 56, H, W) and tuple(cm.shape) == (V, H, W, 64)
    e = max(err(fm32, fm), err(cm32, cm))
    print(f"pyramid {shape}: ATen fp32 err {e:.3e} (max |ref| {fm.abs().max():.3g})")
    assert err(fm32, fm) <= 1e-6 * scale(fm) and err(cm32, cm) <= 1e-6 * scale(cm)
    assert torch.equal(cm[..., :3], d["rgb"].double().permute(0, 2, 3, 1)) and torch.equal(cm[..., 51:59], d["s0"].double().permute(0, 2, 3, 1))
    assert not cm[..., 59:].any()


# ------------------------------------------------------------------------------------------------ batch norm over rows
@pytest.mark.parametrize("C,n,cfg", R.BN_CASES)
def test_bn_rows_vs_aten(C, n, cfg):
    d = R.bn_inputs(C, n, cfg)
    y, mean, var = R.bn_rows(d["x"], d["gamma"], d["beta"], R.BN_EPS, d["slope"], d["abs_gamma"], d["skip"])
    # nn.functional.batch_norm in float64: the same definition, ATen's code
    g64 = d["gamma"].double().abs() + R.BN_EPS if d["abs_gamma"] else d["gamma"].double()
    if n > 1:                       # ATen refuses a single row in training mode
        a = F.batch_norm(d["x"].double(), None, None, g64, d["beta"].double(), training=True, eps=R.BN_EPS)
        a = R.leaky(a, d["slope"]) + (d["skip"].double() if d["skip"] is not None else 0.0)
        assert err(a, y) <= 1e-12 * scale(y)
        assert err(d["x"].double().var(0, unbiased=False), var) <= 1e-12 * scale(var)
    # the oracle-backed stand-in, in float32
    f32, mv32 = fake_ops.bn_act_rows(d["x"], d["gamma"], d["beta"], R.BN_EPS, d["slope"], d["abs_gamma"], d["skip"], want_stats=True)
    e = err(f32, y)
    print(f"bn_rows C={C} n={n} {cfg}: ATen fp32 err y {e:.3e} mean {err(mv32[0], mean):.3e} var {err(mv32[1], var):.3e} (max |y| {y.abs().max():.3g})")
    # float32 statistics over n rows, and the constant channel's float32 mean error times 1 / sqrt(eps) = 316: a loose bound, the float64 check is above
    assert e <= 1e-3 * scale(y) and err(mv32[0], mean) <= 1e-5 and err(mv32[1], var) <= 1e-4 * scale(var)
    # the input conditions
    c = R.bn_const_channel(C)
    assert var[c].item() == 0.0 and mean[c].item() == d["x"][0, c].item()
    if n > 1:
        assert (var[torch.arange(C) != c] > 0).all()
    if d["abs_gamma"]:
        assert (d["gamma"] < 0).any() and (d["gamma"] > 0).any()
    if cfg == "relu_skip":
        assert d["skip"] is not None and tuple(d["skip"].shape) == (n, C)


def test_bn_sizes_reach_the_grid_stride_loop():
    for C in R.BN_CHANNELS:
        rpb = 256 // C
        sizes = R.bn_sizes(C)
        assert -(-sizes[-2] // (rpb * 8)) <= 1024 < -(-sizes[-1] // (rpb * 8))          # blocks needed: under the cap, then over it
    assert R.bn_sizes(16)[-1] == 131109 and R.bn_sizes(64)[-1] == 32805


def test_shim_bn_inputs():
    d = R.shim_bn_inputs()
    assert [b.shape[0] for b in d["batches"]] == [2, 777] and all(b.shape[1] == 32 for b in d["batches"])
    assert (d["batches"][0].double().var(0, unbiased=False) > 1e-4).all()                 # no accidentally constant channel in the two-row batch


# ------------------------------------------------------------------------------------------------ prune_dilate
def _prune(d, r=None, inclusive=False):
    return R.prune_dilate(d["sdf"], d["mask"], d["D"], d["thr"], d["r"] if r is None else r, inclusive)


@pytest.mark.parametrize("D,r", R.PRUNE_CASES)
def test_prune_dilate_vs_max_pool(D, r):
    d = R.prune_inputs(D, r)
    want = fake_ops.prune_dilate(d["sdf"], d["mask"], D, d["thr"], r)
    got = _prune(d)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    # the input conditions
    sdf64 = (d["sdf"].double() * 64)
    assert torch.equal(sdf64, sdf64.round()) and d["sdf"].abs().max() <= 1.0                  # multiples of 1/64 in [-1, 1]
    assert int((d["sdf"].abs() == d["thr"]).sum()) >= 20
    assert int((_prune(d, inclusive=True) != got).sum()) >= 1                                  # `<=` instead of `<` changes the result
    assert 0 < int(got.sum()) < int((d["mask"] > 0).sum())                                     # neither empty nor everything the mask allows
    assert 0.2 < (d["mask"] == 0).double().mean() < 0.4
    if r >= 1:
        assert int((_prune(d, r=r - 1) != got).sum()) >= 20                                    # the radius matters


def test_prune_dilate_corners_vs_max_pool():
    d = R.prune_corner_inputs()
    D = d["D"]
    got = _prune(d)
    assert torch.equal(got, fake_ops.prune_dilate(d["sdf"], d["mask"], D, d["thr"], d["r"]))
    sub = (d["sdf"].abs() < d["thr"]).view(D, D, D)
    assert int(sub.sum()) == 8 and all(sub[x, y, z] for x in (0, D - 1) for y in (0, D - 1) for z in (0, D - 1))
    assert int((d["sdf"].abs() == d["thr"]).sum()) >= 20
    # what survives is the mask inside the eight (r + 1)^3 corner blocks, nothing else
    c = torch.arange(D)
    edge = (c <= d["r"]) | (c >= D - 1 - d["r"])
    block = edge[:, None, None] & edge[None, :, None] & edge[None, None, :]
    assert torch.equal(got.view(D, D, D).bool(), block & (d["mask"].view(D, D, D) > 0))


# ------------------------------------------------------------------------------------------------ layout references
def test_layout_references():
    x = R.nhwc_inputs(8, (5, 13))
    y = R.nchw_to_nhwc(x)
    assert y.is_contiguous() and all(y[v, h, w, c] == x[v, c, h, w] for v in range(2) for c in (0, 7) for h in (0, 4) for w in (0, 12))
    d = R.pack_inputs(R.PACK_SHAPES[0])
    assert torch.equal(R.pack_color_maps(d["feat"], d["rgb"]), fake_ops.pack_color_maps(d["feat"], d["rgb"]))
    for C, dims in R.SCATTER_CASES:
        s = R.scatter_inputs(C, dims)
        n = s["rows"].shape[0]
        kept = s["row_of_voxel"] >= 0
        assert 0.35 < (~kept).double().mean() < 0.65 and torch.equal(s["row_of_voxel"][kept].sort().values, torch.arange(n, dtype=torch.int32))
        cl, cf, mask = R.scatter_dense(s["rows"], s["row_of_voxel"], dims)
        wcl, wcf, wmask = fake_ops.scatter_dense(s["rows"], s["row_of_voxel"], dims)
        assert torch.equal(cl, wcl) and torch.equal(cf, wcf) and torch.equal(mask, wmask)
