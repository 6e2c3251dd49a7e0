"""k_color_pts skips, in the pooling pass, the views that every point of a tile sees with pooling weight exactly 0 (O2345_COLOR_SCHED bit 4 turns
the skipping off).  The claim is BIT-identity of colours and valid-view counts, in both numerical forms, with fewer (tile, view) pairs evaluated."""
import importlib

import numpy as np
import pytest
import torch

from scene_util import small_scene

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("one-2-3-45_amd")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


def _scene(V, dev, ops):
    s = small_scene(V=V, HW=40, D=16)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dev)
    sc = s["sc"]
    Kt, w2c = torch.from_numpy(sc["intrinsics"]), torch.from_numpy(sc["w2cs"])
    d = dict(vol_cl=s["dense"][0].permute(1, 2, 3, 0).contiguous().to(dev), maskvol=s["mask"][0, 0].contiguous().to(dev),
             proj=(Kt @ w2c[:, :3, :]).contiguous().to(dev), cam_pos=torch.inverse(w2c)[:, :3, 3].contiguous().to(dev),
             cmaps=ops.pack_color_maps(t(s["fmaps"]).contiguous(), t(sc["images"]).contiguous()),
             x3=t(pkg.weights.pack_color_x3_blob(s["color_sd"])), fp32=t(pkg.weights.pack_color_mfma_blob(s["color_sd"])))
    return s, d


def _points(V):
    """Tiles as the render path makes them: 32 neighbouring points (coherent visibility and pooling weights), plus incoherent tiles and a ragged end."""
    rng = np.random.default_rng(100 + V)
    centres = rng.uniform(-0.9, 0.9, (96, 3)).astype(np.float32)
    pts = (centres[:, None] + rng.normal(0, 1e-3, (96, 32, 3)).astype(np.float32)).reshape(-1, 3)
    pts[:32] = centres[0]                                                            # one tile of 32 copies of one point: every view has one weight
    pts[2048:2304] = rng.uniform(-0.9, 0.9, (256, 3)).astype(np.float32)
    return np.concatenate([pts, rng.uniform(-0.5, 0.5, (5, 3)).astype(np.float32)])


@pytest.mark.parametrize("prec", ["x3", "fp32"])
@pytest.mark.parametrize("V", [5, 8, 32])
def test_zero_weight_view_skipping_is_bit_identical(dev, ops, V, prec, lib_instance):
    s, d = _scene(V, dev, ops)
    p = torch.from_numpy(_points(V)).to(dev)
    qcam = torch.from_numpy(s["sc"]["query_c2w"][:3, 3].copy()).to(dev)
    blob, mfma = (d["x3"], "x3") if prec == "x3" else (d["fp32"], True)
    outs = {}
    for sched in ("10", "26"):
        lib_instance({"O2345_COLOR_SCHED": sched})
        st = ops.color_stats_buffer(dev)
        rgb, nv = ops.color_points(blob, d["vol_cl"], d["maskvol"], d["cmaps"], d["proj"], d["cam_pos"], p, query_cam=qcam, mfma=mfma, stats=st)
        outs[sched] = (rgb.clone(), nv.clone(), ops.color_stats_read(st))
    a, b = outs["10"], outs["26"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2]["pairs_network"] == b[2]["pairs_network"] and a[2]["tiles"] == b[2]["tiles"] == (p.shape[0] + 31) // 32
    assert a[2]["pairs_pooling"] < b[2]["pairs_pooling"], (a[2], b[2])            # something WAS skipped
    assert int((a[1] >= 2).sum()) > 500 and bool(torch.isfinite(a[0]).all())
