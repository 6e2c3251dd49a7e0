"""GPU: the tile queue of the colour kernel (csrc/common.h; k_color_pts).

With a queue the first part of the 32-point tile list is dealt to the waves as before and the tail -- at the share the product is built with, the whole
list -- is claimed, through eight device-side heads, by the waves that finish first.  A tile's outputs depend on the tile alone, so the claim here is
BIT-identity with the static schedule, whichever wave takes which tile, and that no tile is taken twice or left out:
  * outputs are pre-filled with NaN; every listed slot is bit-equal between the two schedules and every other slot is still NaN;
  * the colour kernel's four work counters (sums over the tiles) are equal, and ``tiles`` == ceil(n / 32);
  * a second call on the same queue memory equals the first (a queue that is not cleared would leave the second call's tail unevaluated);
  * ops.render_rays, whose queues are counters of the call's workspace, equals the library loaded with O2345_TILE_QUEUE=0 bit for bit, call after call.
List lengths n: 0, 1, 31, 32, 33, 160 (a tail of fewer than 8 tiles: some heads own nothing), 32 W - 1, 32 W, 32 W + 1 (W = waves per workgroup x
workgroups launched = every wave of the device) and about 40 tiles per wave; each with a host-side n and with a device-side count on a longer list."""
import importlib

import pytest
import torch

from scene_util import rays_for, small_scene
from test_gpu_color_zero_weight import _scene
from test_gpu_parity import dev, dev_scene, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

COLOR_WAVES = 12                                     # waves per workgroup of k_color_pts (768 threads)
PAD = 77                                             # list entries behind a device-side count


def _lengths(dev):
    W = COLOR_WAVES * torch.cuda.get_device_properties(dev).multi_processor_count
    return W, [0, 1, 31, 32, 33, 160, 32 * W - 1, 32 * W, 32 * W + 1, 32 * 40 * W + 13]


def _cloud(P, dev, seed):
    """P points in tiles of 32 neighbours (coherent visibility, as the render path makes them), every 7th tile scattered over the volume"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    nt = (P + 31) // 32
    centres = torch.rand(nt, 1, 3, generator=g) * 1.8 - 0.9
    pts = centres + 1e-3 * torch.randn(nt, 32, 3, generator=g)
    pts[::7] = torch.rand(pts[::7].shape, generator=g) * 1.8 - 0.9
    return pts.reshape(-1, 3)[:P].contiguous().to(dev)


_SHARED = {}


def _shared(dev, ops):
    """points and one order of their slots (lists are its prefixes): made once"""
    if "cloud" not in _SHARED:
        W, ns = _lengths(dev)
        P = (max(ns) + PAD + 1000 + 31) // 32 * 32
        # the cloud's tiles in a random order, each tile's 32 slots together: a tile of the list is a tile of neighbours, and its cost depends on where it lies
        tiles = torch.randperm(P // 32, generator=torch.Generator(device="cpu").manual_seed(5))
        perm = (tiles[:, None] * 32 + torch.arange(32)[None]).reshape(-1).to(torch.int32).to(dev)
        _SHARED["cloud"] = (_cloud(P, dev, 23), perm)
    return _SHARED["cloud"]


def _list_args(perm, n, device_count, dev):
    """-> (index, n_dev, listed slots) for a list of n entries: host-side n, or a device-side count on a list PAD entries longer"""
    if device_count:
        return perm[:n + PAD].contiguous(), torch.tensor([n], dtype=torch.int32, device=dev), perm[:n].long()
    return perm[:n].contiguous(), None, perm[:n].long()


def _check_slots(name, got, want, listed, P):
    """bit-equal in the listed slots (and no NaN there), NaN in every other slot, in both results"""
    rest = torch.ones(P, dtype=torch.bool, device=got.device)
    rest[listed] = False
    for t in (got, want):
        assert bool(torch.isnan(t[rest]).all()), f"{name}: a slot that is not listed was written"
        assert not bool(torch.isnan(t[listed]).any()), f"{name}: a listed slot was not written"
    assert torch.equal(got[listed], want[listed]), name


def _color_call(ops, d, blob, mfma, pts, qcam, index, n_dev, queue):
    P = pts.shape[0]
    out = (torch.full((P, 3), float("nan"), device=pts.device), torch.full((P,), 255, dtype=torch.uint8, device=pts.device))
    st = ops.color_stats_buffer(pts.device)
    ops.color_points(blob, d["vol_cl"], d["maskvol"], d["cmaps"], d["proj"], d["cam_pos"], pts, query_cam=qcam, index=index, n_dev=n_dev, mfma=mfma, stats=st,
                     tile_queue=queue, out=out)
    return out[0], out[1], ops.color_stats_read(st)


@pytest.fixture(scope="module")
def color_scene(dev, ops):
    s, d = _scene(8, dev, ops)
    return d, torch.from_numpy(s["sc"]["query_c2w"][:3, 3].copy()).to(dev)


@pytest.mark.parametrize("device_count", [False, True], ids=["host_n", "device_n"])
@pytest.mark.parametrize("prec", ["x3", "fp32"])
def test_color_points_queue_is_bit_identical(dev, ops, color_scene, prec, device_count):
    d, qcam = color_scene
    blob, mfma = (d["x3"], "x3") if prec == "x3" else (d["fp32"], True)
    pts, perm = _shared(dev, ops)
    P = pts.shape[0]
    queue = ops.tile_queue_buffer(dev)
    queue.fill_(123456)                                                 # the entry point clears it
    for n in _lengths(dev)[1]:
        index, n_dev, listed = _list_args(perm, n, device_count, dev)
        rgb0, nv0, st0 = _color_call(ops, d, blob, mfma, pts, qcam, index, n_dev, None)
        rgb1, nv1, st1 = _color_call(ops, d, blob, mfma, pts, qcam, index, n_dev, queue)
        _check_slots(f"rgb n={n}", rgb1, rgb0, listed, P)
        rest = torch.ones(P, dtype=torch.bool, device=dev)
        rest[listed] = False
        assert torch.equal(nv1, nv0) and bool((nv1[rest] == 255).all()) and bool((nv1[listed] <= 8).all()), n
        assert st1 == st0 and st1["tiles"] == (n + 31) // 32, (n, st0, st1)
        if n > 1000:
            assert st1["pairs_network"] < 8 * st1["tiles"], "the scene must have tiles of different cost"


def test_second_call_on_the_same_queue_equals_the_first(dev, ops, color_scene):
    d, qcam = color_scene
    pts, perm = _shared(dev, ops)
    W, _ = _lengths(dev)
    n = 32 * 3 * W + 17
    index, n_dev, listed = _list_args(perm, n, True, dev)
    queue = ops.tile_queue_buffer(dev)
    outs = []
    for _ in range(2):
        rgb, nv, st = _color_call(ops, d, d["x3"], "x3", pts, qcam, index, n_dev, queue)
        assert st["tiles"] == (n + 31) // 32
        outs.append(rgb)
    assert int(queue.sum()) > 0                                         # tiles did go through the heads
    _check_slots("second call", outs[1], outs[0], listed, pts.shape[0])


SCENE_KEYS = ("sdf_blob", "color_mfma_blob", "color_x3_blob", "vol_cl", "maskvol", "cmaps", "proj", "cam_pos")


def _render(ops, scene, ro, rd, near, far, qcam, **kw):
    return {k: v.clone() for k, v in ops.render_rays(scene, ro, rd, near, far, 16, 16, 7.4, 1.0, 1.0, qcam, want_z=True, want_scalars=True, **kw).items()}


@pytest.mark.parametrize("R", [4096, 4160])
def test_render_rays_equals_the_static_schedule(dev, ops, lib_instance, R):
    s = small_scene()
    d = dev_scene(s, dev, ops)
    scene = {k: d[k] for k in SCENE_KEYS}
    qcam = torch.from_numpy(s["sc"]["query_c2w"][:3, 3].copy()).to(dev)
    ro, rd = (torch.from_numpy(a).to(dev) for a in rays_for(s, R, seed=R, center=True))
    near, far = (float(v) for v in s["sc"]["query_near_far"][:2])
    L = importlib.import_module("one-2-3-45_amd._lib")
    runs = {}
    for knob in ("1", "0"):
        if knob == "0":
            assert b"tile_queue=0" in lib_instance({"O2345_TILE_QUEUE": "0"}).o2345_knobs()
        else:
            assert b"tile_queue=1" in L.lib().o2345_knobs()
        st = ops.color_stats_buffer(dev)
        first = _render(ops, scene, ro, rd, near, far, qcam, color_stats=st)
        second = _render(ops, scene, ro, rd, near, far, qcam)                      # the same workspace: its queues were used by the first call
        seg = _render(ops, scene, ro, rd, near, far, qcam, segment_rays=64) if R % 64 == 0 else None
        runs[knob] = (first, second, seg, ops.color_stats_read(st))
    q, p = runs["1"], runs["0"]
    assert float(q[0]["weights_sum"].max()) > 0.5 and q[3]["tiles"] > 100
    # (the pair counters are not compared: the sampler appends to the occupied-point list with atomics, so which 32 points share a tile varies from call to call)
    assert q[3]["tiles"] == p[3]["tiles"]
    for k, v in p[0].items():
        assert torch.equal(q[0][k], v), k
        assert torch.equal(q[1][k], v) and torch.equal(p[1][k], v), k
    if q[2] is not None:
        for k, v in p[2].items():
            assert torch.equal(q[2][k], v), k
