"""GPU: the surface renderer (csrc/surface_trace.hip) against its host twin (one-2-3-45_amd/surface.py), which defines the result: fp64 in a defined order on
both sides, so every comparison is EXACT (bytes, whole info dicts).  Expected values are the twin applied to the same inputs (the twin itself is checked
against closed forms in tests/test_surface.py), an independent construction (marching cubes along lattice lines), or facts of the definition."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from guard_util import Guard
from mesh_components_util import spheres_field
from mesh_scene_util import dev, stored_scene  # noqa: F401 (dev: a fixture)
from test_surface import look_at, sphere_lattice

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
S = importlib.import_module("one-2-3-45_amd.surface")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")
STATS_BYTES = ctypes.sizeof(_lib.STRUCTS["O2345SurfaceStats"])        # the block at its exact size: one byte more written and a guard band shows it

NS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)                  # the lane, wave and block boundaries
R = 24
NEAR, FAR = 0.25, 1.0e9


@pytest.fixture(scope="module")
def field(dev):
    """the R = 24 spheres-and-specks field (negative inside), 33 x 32 rays of a camera that sees all of it, with every kind of ray among the first 63"""
    u = spheres_field(R)
    K = np.array([[30.0, 0, 16.0], [0, 30.0, 16.5], [0, 0, 1.0]])
    c2w = look_at((1.9, 1.1, 0.9), (0.0, 0.0, 0.0))
    o, d = S.camera_rays(K, c2w, 33, 32)
    o, d = o.copy(), d.copy()
    d[5, 1] = np.nan                                          # bad rays
    o[6, 0] = np.inf
    o[9], d[9] = (1.5, 0.0, -3.0), (0.0, 0.0, 1.0)            # parallel to an axis, outside its slab: a box miss
    o[11], d[11] = (-0.4, 0.0, 0.0), (0.0, 0.0, 1.0)          # starts inside the large sphere: an entry hit
    o[12], d[12] = (0.9, 0.9, -3.0), (0.0, 0.0, 1.0)          # marches through
    o[13], d[13] = (0.9, 0.9, -3.0), (0.0, 0.0, 1e-7)         # crosses the box in more than 2^20 steps: a bad ray
    o.setflags(write=False); d.setflags(write=False)
    u_nan = np.array(u)
    shell = np.abs(u) < 0.04
    shell[:9] = False
    u_nan[shell] = np.nan                                     # the nodes next to the surfaces on the camera's side: rays through their cells stall
    u_nan[3, 3, 3] = np.inf
    u_nan.setflags(write=False)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return dict(u=u, u_nan=u_nan, o=o, d=d, du=t(u), du_nan=t(u_nan), do=t(o), dd=t(d), twins={})


def _twin(F, n, skip, which="u", **kw):
    key = (n, skip, which, tuple(sorted(kw.items())))
    if key not in F["twins"]:
        out = S.trace_rays(F[which], F["o"][:n], F["d"][:n], NEAR, FAR, skip=skip, **kw)
        for a in out[:3]:
            a.setflags(write=False)
        F["twins"][key] = out
    return F["twins"][key]


def _same(out, twin):
    for k, w in zip(("depth", "kind", "point"), twin[:3]):
        g = out[k].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), k
    assert out["info"] == twin[3], (out["info"], twin[3])


def _hit_list_ok(out):
    n_hits = int(out["n_hits"].item())
    kind = out["kind"].cpu().numpy()
    assert out["hits"].dtype == torch.int32 and out["hits"].shape[0] == kind.shape[0]
    assert n_hits == out["info"]["hits"] + out["info"]["entry_hits"]
    assert np.array_equal(np.sort(out["hits"][:n_hits].cpu().numpy()), np.flatnonzero(kind != 0))          # exactly the slots with kind != 0, each once


@pytest.mark.parametrize("skip", [True, False])
def test_trace_equals_twin_at_every_lane_wave_and_block_boundary(field, skip):
    F = field
    for n in NS:
        out = ops.surface_trace(F["du"], F["do"][:n].contiguous(), F["dd"][:n].contiguous(), NEAR, FAR, skip=skip)
        _same(out, _twin(F, n, skip))
        _hit_list_ok(out)
    info = out["info"]
    print(skip, info)
    assert info["hits"] > 100 and info["entry_hits"] >= 1 and info["box_misses"] >= 1 and info["misses"] > 100 and info["bad_rays"] == 3
    if skip:
        assert info["lookups"] < info["samples"]
    else:
        assert info["lookups"] == info["samples"]


def test_trace_equals_twin_on_other_inputs(field):
    F = field
    n = 1025
    o, d = F["do"][:n].contiguous(), F["dd"][:n].contiguous()
    for kw in (dict(stride=2.0, refine=3), dict(stride=0.5, refine=0), dict(level=0.05), dict(refine=32),
               dict(bound_min=(-1.0, -1.5, -1.25), bound_max=(1.5, 1.0, 1.0))):
        for skip in (True, False):
            _same(ops.surface_trace(F["du"], o, d, NEAR, FAR, skip=skip, **kw), _twin(F, n, skip, **kw))
    # NaN and infinite nodes: stalled rays, the same bytes
    for skip in (True, False):
        out = ops.surface_trace(F["du_nan"], o, d, NEAR, FAR, skip=skip)
        _same(out, _twin(F, n, skip, "u_nan"))
        _hit_list_ok(out)
    assert out["info"]["stalled"] > 0
    # the negated lattice with inside_positive: the bytes of the plain call
    out = ops.surface_trace(-F["du"], o, d, NEAR, FAR, inside_positive=True)
    _same(out, _twin(F, n, True))
    # waves over 8 x 8 pixel tiles instead of rows: the same bytes, at an image that no tile size divides
    n = 33 * 31
    out = ops.surface_trace(F["du"], F["do"][:n].contiguous(), F["dd"][:n].contiguous(), NEAR, FAR, image_hw=(33, 31))
    _same(out, _twin(F, n, True))
    _hit_list_ok(out)
    out = ops.surface_trace(F["du"], F["do"][:n].contiguous(), F["dd"][:n].contiguous(), NEAR, FAR, image_hw=(1, n))
    _same(out, _twin(F, n, True))
    # near above far: every ray misses the box
    out = ops.surface_trace(F["du"], o, d, 5.0, 1.0)
    assert out["info"]["box_misses"] + out["info"]["bad_rays"] == 1025 and out["info"]["samples"] == 0 and not out["kind"].any()


def test_two_runs_and_a_second_stream_give_identical_bytes(field, dev):
    F = field
    n = 1025
    o, d = F["do"][:n].contiguous(), F["dd"][:n].contiguous()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    want = _twin(F, n, True)
    for stream in (None, None, side):
        with torch.cuda.stream(stream):
            out = ops.surface_trace(F["du"], o, d, NEAR, FAR)
            _same(out, want)
            _hit_list_ok(out)
    torch.cuda.synchronize()


def test_bricks_equal_twin(dev):
    for Rn in (2, 3, 9, 10, 17, 24, 40):
        u = np.array(spheres_field(Rn) if Rn >= 24 else sphere_lattice(Rn))
        if Rn >= 9:
            u[Rn - 1, 0, Rn - 2] = np.nan
        for kw in (dict(), dict(level=0.1), dict(level=-0.2, inside_positive=True)):
            got = ops.surface_bricks(torch.from_numpy(u).to(dev), **kw)
            want = S.brick_flags(u, **kw)
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), (Rn, kw)
    plain = S.brick_flags(spheres_field(40))
    assert 0 < int(plain.sum()) < plain.size                             # both kinds of brick took part


SHAPES = ((1, 1), (7, 9), (64, 65))


def test_camera_rays_equal_twin(dev):
    c2w = look_at((1.9, 1.1, 0.9), (0.1, 0.0, -0.1)).astype(np.float32)
    for H, W in SHAPES:
        for K in (np.array([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1.0]], np.float32), np.array([[41.5, 0, 3.25], [0, -17.0, 8.0], [0, 0, 1.0]], np.float32)):
            o, d = ops.camera_rays(K, c2w, H, W, dev)
            wo, wd = S.camera_rays(K, c2w, H, W)
            assert o.cpu().numpy().tobytes() == wo.tobytes() and d.cpu().numpy().tobytes() == wd.tobytes(), (H, W)
            o, d = ops.camera_rays(torch.from_numpy(K), torch.from_numpy(c2w[:3]), H, W, dev)
            assert d.cpu().numpy().tobytes() == wd.tobytes()
    K[0, 1] = 0.5
    with pytest.raises(ValueError):
        ops.camera_rays(K, c2w, 4, 4, dev)


def _pack_inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    n = H * W
    kind = rng.integers(0, 3, n).astype(np.uint8)
    depth = rng.uniform(0.5, 3.0, n).astype(np.float32)
    rgb = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    grad = rng.standard_normal((n, 3)).astype(np.float32)
    grad[rng.integers(0, n, max(1, n // 7))] = 0.0                       # zero gradients: n = 0
    grad[rng.integers(0, n, max(1, n // 9)), 1] = np.nan                 # non-finite ones too
    rgb[rng.integers(0, n, max(1, n // 5))] = (0.0, 1.0, 0.5)
    return kind, depth, rgb, grad


def test_pack_equals_twin(dev):
    t = lambda a: torch.from_numpy(a).to(dev)
    for k, (H, W) in enumerate(SHAPES):
        kind, depth, rgb, grad = _pack_inputs(H, W, k)
        for bg in ((0, 0, 0, 0), (255, 7, 130, 200)):
            got = ops.surface_pack(t(kind), t(depth), t(rgb), t(grad), H, W, background=bg)
            want = S.pack_images(kind, depth, rgb, grad, H, W, background=bg)
            for g, w in zip(got, want):
                g = g.cpu().numpy()
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (H, W, bg)
    with pytest.raises(ValueError):
        ops.surface_pack(t(kind), t(depth), t(rgb), t(grad), H, W, background=(0, 0, 256, 0))


def test_hits_along_lattice_lines_are_the_marching_cubes_vertices(field, dev):
    """Rays along lattice lines (x_i, y_j, -2) + t (0, 0, 1): between two nodes of a line the trilinear value is the linear function marching cubes
    interpolates, so the hit is the first z-edge vertex of that line -- an independent check of the lookup's indexing.  For the rays to run ALONG lattice
    lines their x and y must be lattice coordinates exactly, which float32 cannot hold for -1 + 2 i / 23: the box is (0, 0, -1) .. (23, 23, 1), so that
    x_i = i.  The outputs are float32, which cannot carry 1e-9 either (an ulp of the depth is 2.4e-7): the device must equal the twin byte for byte, the
    twin's depth before its rounding is compared to 1e-9, and the device's float32 depth is that of the marching-cubes vertex to one ulp."""
    F = field
    verts, _ = ops.marching_cubes(F["du"], 0.0)
    verts = verts.cpu().numpy()
    ii, jj = np.meshgrid(np.arange(4, 14), np.arange(7, 17), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    o = np.stack([ii, jj, np.full(100, -2.0)], 1).astype(np.float32)
    d = np.tile(np.float32([0, 0, 1]), (100, 1))
    b0, b1 = (0.0, 0.0, -1.0), (23.0, 23.0, 1.0)
    out = ops.surface_trace(F["du"], torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), 0.0, 10.0, stride=1.0, bound_min=b0, bound_max=b1)
    twin = S.trace_rays(F["u"], o, d, 0.0, 10.0, stride=1.0, bound_min=b0, bound_max=b1, want_t=True)
    _same(out, twin)
    depth, kind = out["depth"].cpu().numpy(), out["kind"].cpu().numpy()
    n_hit = 0
    for r in range(100):
        on_line = verts[(verts[:, 0] == ii[r]) & (verts[:, 1] == jj[r]), 2]
        if on_line.size == 0:
            assert kind[r] == 0, r                                     # no vertex on the line: the ray must miss
            continue
        z_mc = on_line.min()
        assert kind[r] == 1, r
        z = (twin[4][r] - 2.0 + 1.0) / 2.0 * (R - 1)
        assert abs(z - z_mc) <= 1e-9, (r, z, z_mc)
        t_mc = np.float32(2.0 + (z_mc / (R - 1) * 2.0 - 1.0))
        assert abs(depth[r] - t_mc) <= np.spacing(t_mc), r
        n_hit += 1
    assert 20 <= n_hit <= 95                                           # both kinds of line are among the hundred


# ---- canaries: every buffer the new entries are handed, at its exact size, carved out of pattern-filled allocations ------------------------------------
def _np(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def test_no_kernel_writes_outside_its_buffers(field, dev):
    F = field
    L = _lib.lib()
    g = Guard(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    Hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    b0, b1 = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    nb = (R - 1 + 7) // 8
    u = g.buf(F["u"], what="u")
    flags = g.buf(nbytes=nb ** 3, what="flags")
    _lib.check(L.o2345_surface_bricks(P(u), R, 0.0, 0, P(flags), s), "surface_bricks")
    assert not g.damaged() and np.array_equal(_np(flags, np.uint8, (nb, nb, nb)), S.brick_flags(F["u"]))
    for n in NS:
        for skip in (True, False):
            o, d = g.buf(F["o"][:n], what=("o", n)), g.buf(F["d"][:n], what=("d", n))
            wsb = L.o2345_surface_trace_workspace_bytes(n)
            assert wsb >= max(4 * n, 16) and wsb % 16 == 0
            ws, stats = g.buf(nbytes=wsb, what=("workspace", n)), g.buf(nbytes=STATS_BYTES, what=("stats", n))
            depth, kind, point = g.buf(nbytes=4 * n, what=("depth", n)), g.buf(nbytes=n, what=("kind", n)), g.buf(nbytes=12 * n, what=("point", n))
            _lib.check(L.o2345_surface_trace(P(u), R, P(flags) if skip else None, P(o), P(d), n, 0, 0, NEAR, FAR, 1.0, 8, 0.0, 0, Hp(b0), Hp(b1), P(ws),
                                             wsb, P(depth), P(kind), P(point), P(stats), s), "surface_trace")
            bad = g.damaged()
            assert not bad, bad
            w = _twin(F, n, skip)
            assert _np(depth, np.float32, (n,)).tobytes() == w[0].tobytes() and _np(kind, np.uint8, (n,)).tobytes() == w[1].tobytes()
            assert _np(point, np.float32, (n, 3)).tobytes() == w[2].tobytes() and ops.surface_info(stats.cpu().numpy(), n) == w[3]
            assert _np(u, np.float32, (R, R, R)).tobytes() == F["u"].tobytes()                    # the inputs are only read
    # the tiled mapping, at an image with partial tiles on both edges
    n = 33 * 31
    o, d = g.buf(F["o"][:n], what="o tiled"), g.buf(F["d"][:n], what="d tiled")
    wsb = L.o2345_surface_trace_workspace_bytes(n)
    ws, stats = g.buf(nbytes=wsb, what="workspace tiled"), g.buf(nbytes=STATS_BYTES, what="stats tiled")
    depth, kind, point = g.buf(nbytes=4 * n, what="depth tiled"), g.buf(nbytes=n, what="kind tiled"), g.buf(nbytes=12 * n, what="point tiled")
    _lib.check(L.o2345_surface_trace(P(u), R, P(flags), P(o), P(d), n, 33, 31, NEAR, FAR, 1.0, 8, 0.0, 0, Hp(b0), Hp(b1), P(ws), wsb, P(depth), P(kind),
                                     P(point), P(stats), s), "surface_trace")
    assert not g.damaged() and _np(depth, np.float32, (n,)).tobytes() == _twin(F, n, True)[0].tobytes()
    # rays and packer
    c2w = look_at((1.9, 1.1, 0.9), (0.0, 0.0, 0.0)).astype(np.float32)
    for k, (H, W) in enumerate(SHAPES):
        K = np.array([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1.0]], np.float32)
        n = H * W
        ro, rd = g.buf(nbytes=12 * n, what=("rays_o", n)), g.buf(nbytes=12 * n, what=("rays_d", n))
        _lib.check(L.o2345_camera_rays(Hp(K), Hp(c2w), H, W, P(ro), P(rd), s), "camera_rays")
        wo, wd = S.camera_rays(K, c2w, H, W)
        assert not g.damaged() and _np(ro, np.float32, (n, 3)).tobytes() == wo.tobytes() and _np(rd, np.float32, (n, 3)).tobytes() == wd.tobytes()
        kind_h, depth_h, rgb_h, grad_h = _pack_inputs(H, W, k)
        ins = [g.buf(a, what=("pack in", n)) for a in (kind_h, depth_h, rgb_h, grad_h)]
        color, normal, dout = g.buf(nbytes=4 * n, what=("color", n)), g.buf(nbytes=4 * n, what=("normal", n)), g.buf(nbytes=4 * n, what=("depth_out", n))
        bg = np.array([1, 2, 3, 4], np.uint8)
        _lib.check(L.o2345_surface_pack(P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), H, W, Hp(bg), P(color), P(normal), P(dout), s), "surface_pack")
        want = S.pack_images(kind_h, depth_h, rgb_h, grad_h, H, W, background=bg)
        bad = g.damaged()
        assert not bad, bad
        assert _np(color, np.uint8, (H, W, 4)).tobytes() == want[0].tobytes() and _np(normal, np.uint8, (H, W, 4)).tobytes() == want[1].tobytes()
        assert _np(dout, np.float32, (H, W)).tobytes() == want[2].tobytes()


def test_errors_are_statuses(field, dev):
    F = field
    o, d = F["do"][:70].contiguous(), F["dd"][:70].contiguous()
    for kw in (dict(stride=0.0), dict(stride=9.0), dict(refine=33), dict(refine=-1), dict(level=float("nan")), dict(bound_min=(1.0, -1.0, -1.0)),
               dict(image_hw=(7, 9)), dict(flags=torch.zeros(2, 2, 2, dtype=torch.uint8, device=dev))):
        with pytest.raises(ValueError):
            ops.surface_trace(F["du"], o, d, NEAR, FAR, **kw)
    with pytest.raises(ValueError):
        ops.surface_trace(F["du"], o, d, float("nan"), FAR)
    with pytest.raises(ValueError):
        ops.surface_trace(F["du"][:, :, :5].contiguous(), o, d, NEAR, FAR)
    with pytest.raises(ValueError):
        ops.surface_trace(F["du"], o, d[:5].contiguous(), NEAR, FAR)
    L = _lib.lib()
    assert L.o2345_surface_trace_workspace_bytes(-1) == 0 and L.o2345_surface_trace_workspace_bytes(2 ** 31) == 0
    _same(ops.surface_trace(F["du"], o, d, NEAR, FAR), _twin(F, 70, True))             # and the next call works


# ---- the pipeline on the stored small scene (D = 20, lattice 64^3, the 48 x 48 query camera) -----------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    S0 = stored_scene(dev, extract=False)
    s = S0["host"]
    return dict(vol=S0["vol"], proj=S0["proj"], cam_pos=S0["cam_pos"], K=s["sc"]["query_intrinsic"], c2w=s["sc"]["query_c2w"], H=s["H"], W=s["W"])


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_render_surface_equals_the_twin_and_the_networks_at_the_hit_points(scene, dev, prec, monkeypatch):
    Sc = scene
    H, W, K, c2w = Sc["H"], Sc["W"], Sc["K"], Sc["c2w"]
    wt = pipeline.SceneWeights(dev, seed=0, sdf_precision=prec, color_precision=prec)
    r = pipeline.render_surface(wt, Sc["vol"], Sc["proj"], Sc["cam_pos"], K, c2w, H, W, resolution=64, background=(9, 8, 7, 6))
    u = r["u"]
    assert u.dtype == torch.float32 and tuple(u.shape) == (64, 64, 64)
    ro, rd = S.camera_rays(K, c2w, H, W)
    depth, kind, point, info = S.trace_rays(u.cpu().numpy(), ro, rd, 0.0, 1.0e6, stride=config.SURFACE_STRIDE, refine=config.SURFACE_REFINE, inside_positive=True)
    print(prec, info)
    assert info["hits"] > 100 and info["misses"] + info["box_misses"] > 0
    assert r["info"] == info
    assert r["kind"].cpu().numpy().tobytes() == kind.tobytes() and tuple(r["kind"].shape) == (H, W)
    assert r["point"].cpu().numpy().tobytes() == point.tobytes() and tuple(r["point"].shape) == (H, W, 3)
    assert r["depth"].cpu().numpy().tobytes() == depth.tobytes() and tuple(r["depth"].shape) == (H, W)
    # colour and normal: the two networks called directly on the hit points, through the packer twin
    hit = np.flatnonzero(kind != 0)
    pts = torch.from_numpy(point[hit]).to(dev)
    g = ops.sdf_mlp(wt.sdf_blob, Sc["vol"]["vol_cl"], pts, variant=2, precision=prec)["grad"]
    blob, mfma = wt.color_network()
    cam = torch.from_numpy(np.asarray(c2w, np.float32)[:3, 3].copy()).to(dev)
    rgb, _ = ops.color_points(blob, Sc["vol"]["vol_cl"], Sc["vol"]["maskvol"], Sc["vol"]["cmaps"], Sc["proj"], Sc["cam_pos"], pts, query_cam=cam,
                              want_nviews=False, mfma=mfma)
    full_rgb, full_g = np.zeros((H * W, 3), np.float32), np.zeros((H * W, 3), np.float32)
    full_rgb[hit], full_g[hit] = rgb.cpu().numpy(), g.cpu().numpy()
    color, normal, dimg = S.pack_images(kind, depth, full_rgb, full_g, H, W, background=(9, 8, 7, 6))
    assert r["color"].cpu().numpy().tobytes() == color.tobytes() and r["normal"].cpu().numpy().tobytes() == normal.tobytes()
    assert r["depth"].cpu().numpy().tobytes() == dimg.tobytes()
    assert len(np.unique(color.reshape(-1, 4)[hit], axis=0)) > 10 and (color.reshape(-1, 4)[kind == 0] == (9, 8, 7, 6)).all()
    # a lattice passed in is reused: no lattice kernel runs, and the images are the same bytes
    real = ops.sdf_mlp

    def no_lattice(blob, vol_cl, pts=None, *a, **k):
        assert pts is not None, "render_surface(u=...) must not evaluate the lattice"
        return real(blob, vol_cl, pts, *a, **k)
    monkeypatch.setattr(ops, "sdf_mlp", no_lattice)
    r2 = pipeline.render_surface(wt, Sc["vol"], Sc["proj"], Sc["cam_pos"], K, c2w, H, W, resolution=64, u=u, background=(9, 8, 7, 6))
    assert r2["u"] is u and r2["info"] == info
    for k in ("color", "normal", "depth", "kind", "point"):
        assert torch.equal(r2[k], r[k]), k
    monkeypatch.setattr(ops, "sdf_mlp", real)
    # the lattice extract_mesh returns is the one render_surface computes
    assert torch.equal(pipeline.extract_mesh(wt, Sc["vol"], Sc["proj"], Sc["cam_pos"], 64)[3], u)
    # a turntable: the lattice once, every view the render_surface of its camera
    views, c2ws = pipeline.render_turntable(wt, Sc["vol"], Sc["proj"], Sc["cam_pos"], K, H, W, 3, elevation_deg=30.0, radius=2.2, resolution=64, u=u)
    assert len(views) == 3 and c2ws.tobytes() == S.orbit_c2w(3, 30.0, 2.2).tobytes()
    one = pipeline.render_surface(wt, Sc["vol"], Sc["proj"], Sc["cam_pos"], K, c2ws[1], H, W, u=u)
    assert torch.equal(views[1]["color"], one["color"]) and torch.equal(views[1]["depth"], one["depth"]) and views[1]["info"]["hits"] > 0


def test_reconstruct_folder_writes_previews(tmp_path, dev, monkeypatch):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    assert config.PREVIEW_VIEWS == 0                                       # the environment of the test run leaves it unset
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64, preview_views=2)
    assert len(out["previews"]) == 2
    for k, p in enumerate(out["previews"]):
        assert p["path"] == str(tmp_path / f"preview_{k:03d}.png")
        img = mio.read_png(p["path"])
        assert img.dtype == np.uint8 and img.shape == (256, 256, 4) and img.tobytes() == p["color"].tobytes()
        assert p["normal"].shape == (256, 256, 4) and p["depth"].shape == (256, 256) and p["depth"].dtype == np.float32
        assert p["info"]["hits"] > 0 and ((p["color"][..., 3] == 255) == (p["depth"] > 0)).all()
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    assert out["previews"][0]["c2w"].tobytes() == s["query_c2w"].numpy().astype(np.float32).tobytes()          # view 0 is the folder's query camera
    # off: the new ops are not reached, and the result keeps its keys
    for name in ("surface_bricks", "surface_trace", "camera_rays", "surface_pack"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"preview_views = 0 must not reach ops.{_n}"))
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64)
    off = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "c.ply"), D=48, resolution=64, preview_views=0)
    assert "previews" not in plain and set(plain) == set(off) == set(out) - {"previews"}
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read() == open(tmp_path / "c.ply", "rb").read()
    assert not (tmp_path / "preview_002.png").exists()
