"""GPU: the texture atlas of the exported mesh (csrc/mesh_texture.hip) against the host twins (mesh_io.texture_points / pack_texture / texture_corners /
obj_texture_text_numpy), which define the result.  Everything outside the two networks is fp64 in a defined order, or integer: every comparison is EXACT
(bytes).  Expected values are the host twins applied to the same inputs, or the library's own network kernels at the twin's points, never the code
under test."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from guard_util import Guard
from mesh_scene_util import args as _args, colours_at, dev, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("one-2-3-45_amd")
ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")
STATS_BYTES = ctypes.sizeof(_lib.STRUCTS["O2345TextureStats"])        # the block at its exact size: one byte more written and a guard band shows it

# c = 4: 16 texels per cell, 16 cells per 256-thread block -- 31 and 32 triangles end at the block's last thread, 33 start the next block;
# c = 8: 64 texels per cell, 4 cells per block -- 5 / 6 end inside the block, 7 / 8 at its end, 9 just after;  c = 5: 25 texels, no power of two.
COUNTS = (1, 2, 3, 5, 6, 7, 8, 9, 31, 32, 33, 41)
TEXELS = (4, 5, 8)
R = 64


def _mesh(nt, seed):
    """nt triangles over nt + 2 vertices inside an R = 64 grid, some at its rim so that extrapolating gutter texels meet the clamp on both sides"""
    rng = np.random.default_rng(seed)
    v = np.clip(rng.uniform(0.0, R - 1.0, 3) + rng.uniform(-4, 4, (nt + 2, 3)), 0.0, R - 1.0)
    v[0] = [0.0, 1.0, R - 1.0]
    f = np.stack([np.arange(nt), np.arange(nt) + 1, np.arange(nt) + 2], 1)
    f[1::2] = f[1::2, ::-1]
    v.setflags(write=False)
    return v, f


_twins = {}


def _twin_points(nt, c):
    """the twin's texel points of _mesh(nt), computed once per (nt, c) and shared by the tests"""
    if (nt, c) not in _twins:
        v, f = _mesh(nt, nt)
        out = mio.texture_points(v, f, c, R, ((-1.0, -2.0, -1.0), (1.0, 2.0, 3.0)))
        for a in out:
            a.setflags(write=False)
        _twins[(nt, c)] = out
    return _twins[(nt, c)]


def _B(t):
    return t.contiguous().cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("c", TEXELS)
def test_points_equal_the_twin_at_small_counts_and_block_boundaries(dev, c, dtype):
    clamped = 0
    for nt in COUNTS:
        v, f = _mesh(nt, nt)
        verts, tris = torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(f).to(dev).to(dtype)
        pts, world, stats = ops.mesh_texture_points(verts, tris, c, R, (-1.0, -2.0, -1.0), (1.0, 2.0, 3.0))
        wp, ww = _twin_points(nt, c)
        assert pts.dtype == torch.float64 and world.dtype == torch.float32 and tuple(pts.shape) == wp.shape == tuple(world.shape)
        assert _B(pts) == wp.tobytes() and _B(world) == ww.tobytes(), (nt, c)
        assert _B(stats) == bytes(STATS_BYTES)
        assert _B(verts) == v.tobytes() and np.array_equal(tris.cpu().numpy(), f)                 # inputs are only read
        clamped += int(((wp == 0.0) | (wp == R - 1.0)).sum())
    assert clamped > 0                                                    # the clamp had something to do


@pytest.fixture(scope="module")
def spheres(dev):
    from mesh_components_util import spheres_field
    u = torch.from_numpy(np.array(spheres_field(40))).to(dev)
    v, t = ops.marching_cubes(u, 0.0)
    hv, hf = v.cpu().numpy(), t.cpu().numpy()
    assert hf.shape[0] > 2000
    want = mio.texture_points(hv, hf, 4, 40)
    return dict(v=v, t=t, hv=hv, hf=hf, want=want)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_points_equal_the_twin_on_a_marching_cubes_mesh(dev, spheres, dtype):
    S = spheres
    tris = S["t"].to(dtype)
    pts, world, _ = ops.mesh_texture_points(S["v"], tris, 4, 40)
    assert _B(pts) == S["want"][0].tobytes() and _B(world) == S["want"][1].tobytes()
    assert _B(S["v"]) == S["hv"].tobytes() and np.array_equal(tris.cpu().numpy(), S["hf"])
    # the colour network would see the points the pipeline's own expression gives for the (-1, 1) box
    assert torch.equal(world, (pts / 39.0 * 2.0 - 1.0).to(torch.float32))


def _mats():
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 0.9; scale[:3, 3] = [0.01, 0.02, -0.03]
    trans = np.eye(4, dtype=np.float32); trans[:3, :3] = np.array([[0.0, -1.1, 0.0], [1.0, 0.0, 0.1], [0.0, 0.2, 1.0]], np.float32); trans[:3, 3] = [0.5, -0.25, 0.125]
    return scale, trans


@pytest.mark.parametrize("c", TEXELS)
def test_pack_equals_the_twin(dev, c):
    rng = np.random.default_rng(c)
    for nt in COUNTS:
        L = mio.texture_layout(nt, c)
        rgb = rng.uniform(-0.5, 1.5, (L["texels"], 3)).astype(np.float32)
        rgb[0] = [1.0, 0.0, -0.25]
        rgb[-1] = [1.0, 1.0, 1.25]
        d = torch.from_numpy(rgb).to(dev)
        img = ops.mesh_texture_pack(d, nt, c)
        assert img.dtype == torch.uint8 and tuple(img.shape) == (L["height"], L["width"], 4)
        assert _B(img) == mio.pack_texture(rgb, nt, c).tobytes(), (nt, c)
        assert _B(d) == rgb.tobytes()


@pytest.mark.parametrize("with_mats", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("c", TEXELS)
def test_corners_and_obj_text_equal_the_twin(dev, c, with_normals, with_mats):
    scale, trans = _mats() if with_mats else (None, None)
    for nt in COUNTS:
        v, f = _mesh(nt, nt)
        rng = np.random.default_rng(nt)
        g = (rng.normal(0, 1, (nt + 2, 3)) * rng.uniform(1e-3, 50, (nt + 2, 1))).astype(np.float32) if with_normals else None
        if with_normals:
            g[1] = 0.0                                                    # a zero gradient: (0, 1, 0)
        verts, tris = torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(f).to(dev)
        pos, uv, nrm, idx, bounds = ops.mesh_texture_corners(verts, tris, c, R, scale_mat=scale, trans_mat=trans, grad=None if g is None else torch.from_numpy(g).to(dev))
        wpos, wuv, wnrm, wb = mio.texture_corners(v, f, c, R, scale_mat=scale, trans_mat=trans, grad=g)
        assert _B(pos) == wpos.tobytes() and _B(uv) == wuv.tobytes() and _B(bounds) == wb.astype(np.float32).tobytes(), (nt, c)
        assert (nrm is None) == (not with_normals) and (nrm is None or _B(nrm) == wnrm.tobytes())
        assert np.array_equal(idx.cpu().numpy().reshape(-1), np.arange(3 * nt))
        # the welded export of the same mesh, gathered by corner in the reversed winding: the same bits
        wp, _, wn, widx, _ = ops.mesh_asset_pack(verts, tris, R, scale_mat=scale, trans_mat=trans, grad=None if g is None else torch.from_numpy(g).to(dev))
        gather = widx.reshape(-1).long()
        assert torch.equal(pos, wp[gather]) and (nrm is None or torch.equal(nrm, wn[gather]))
        assert np.array_equal(widx.cpu().numpy(), f[:, ::-1])
        # OBJ records
        text = ops.obj_texture_text(pos, uv, nrm, bounds=bounds)
        K = mio.obj_coordinate_digits(wb)
        assert _B(text) == mio.obj_texture_text_numpy(wpos, wuv, wnrm, K), (nt, c)
        assert text.numel() == mio.obj_texture_text_bytes(3 * nt, K, with_normals)


# ---- the pipeline on the stored small scene (D = 20, R = 64), the scene of tests/test_gpu_mesh_project.py -------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    return dict(stored_scene(dev, extract=False), cache={})


def _expected_image(S, project):
    """(mesh of the call, the image the definition gives): pack_texture of the colour network at the twin's texel points [after ops.mesh_project]"""
    key = ("image", project)
    if key not in S["cache"]:
        dev = S["vol"]["vol_cl"].device
        v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=2, project_iterations=project)
        hv, hf = v.cpu().numpy(), t.cpu().numpy()
        assert 100 < hf.shape[0] < 20000
        pts, world = mio.texture_points(hv, hf, 4, S["R"])
        world = torch.from_numpy(world).to(dev)
        if project:
            p, _ = ops.mesh_project(S["wt"].sdf_blob, S["vol"]["vol_cl"], torch.from_numpy(pts).to(dev), S["R"], project, max_move=2.0, precision=S["wt"].sdf_precision)
            world = (p / (S["R"] - 1.0) * 2.0 - 1.0).to(torch.float32).contiguous()
        image = mio.pack_texture(colours_at(S, world)[0].cpu().numpy(), hf.shape[0], 4)
        S["cache"][key] = (v, t, hv, hf, image)
    return S["cache"][key]


@pytest.mark.parametrize("project", [0, 2])
def test_textured_glb_end_to_end(scene, tmp_path, project):
    S = scene
    v, t, hv, hf, image = _expected_image(S, project)
    nt = hf.shape[0]
    path, welded = str(tmp_path / "t.glb"), str(tmp_path / "w.glb")
    kw = dict(decimate_cell=2, project_iterations=project, normals=True)
    assert pipeline.export_mesh_asset(path, *_args(S), texture_texel=4, **kw) == (3 * nt, nt)
    assert pipeline.export_mesh_asset(welded, *_args(S), **kw) == (hv.shape[0], nt)
    p, f, col, nr = mio.read_glb(path)
    uv, img, sampler = mio.read_glb_texture(path)
    L = mio.texture_layout(nt, 4)
    assert col is None and img.shape == (L["height"], L["width"], 4) and np.array_equal(f.reshape(-1), np.arange(3 * nt))
    assert img.tobytes() == image.tobytes()
    assert (image[..., 3] == 255).sum() == L["texels"] and image[..., :3].max() > 0
    wp, wf, wcol, wn = mio.read_glb(welded)
    assert wcol is not None and p.tobytes() == wp[wf.reshape(-1)].tobytes() and nr.tobytes() == wn[wf.reshape(-1)].tobytes()
    wpos, wuv, _, _ = mio.texture_corners(hv, hf, 4, S["R"])
    assert p.tobytes() == wpos.tobytes() and uv.tobytes() == wuv.tobytes()
    if project:
        assert image.tobytes() != _expected_image(S, 0)[4].tobytes()


def test_two_runs_and_a_second_stream_give_identical_files_and_the_obj_agrees(scene, dev, tmp_path):
    S = scene
    B = lambda p: open(p, "rb").read()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    files = []
    for k, stream in enumerate((None, None, side)):
        with torch.cuda.stream(stream):
            d = tmp_path / f"run{k}"
            os.mkdir(d)
            for ext in (".glb", ".obj"):
                pipeline.export_mesh_asset(str(d / ("mesh" + ext)), *_args(S), decimate_cell=2, texture_texel=4, normals=True)
            assert sorted(os.listdir(d)) == ["mesh.glb", "mesh.mtl", "mesh.obj", "mesh.png"]
            files.append([B(d / n) for n in sorted(os.listdir(d))])
    assert files[0] == files[1] == files[2]
    d = tmp_path / "run0"
    p, f, _, nr = mio.read_glb(str(d / "mesh.glb"))
    uv, img, _ = mio.read_glb_texture(str(d / "mesh.glb"))
    op, ouv, on, of, oimg = mio.read_obj_texture(str(d / "mesh.obj"))
    assert np.array_equal(oimg, img) and np.array_equal(of, f) and B(d / "mesh.png") == mio.png_bytes(img, 1)
    assert np.abs(op - p).max() <= 0.5e-8 and np.abs(on - nr).max() <= 0.5e-8 and np.abs(ouv - uv).max() <= 0.5e-8 + 6e-8
    K = mio.obj_coordinate_digits(p)
    assert B(d / "mesh.obj") == mio.obj_texture_header(str(d / "mesh.obj")) + mio.obj_texture_text_numpy(p, uv, nr, K)
    # smoothing comes last: the image is the unsmoothed surface's, the positions move
    sm = str(tmp_path / "s.glb")
    pipeline.export_mesh_asset(sm, *_args(S), decimate_cell=2, texture_texel=4, smooth_iterations=2)
    assert np.array_equal(mio.read_glb_texture(sm)[1], img) and mio.read_glb(sm)[0].tobytes() != p.tobytes()


def test_off_is_todays_path(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    assert config.MESH_TEXTURE_TEXEL == 0                                 # the environment of the test run leaves it unset
    for name in ("mesh_texture_points", "mesh_texture_pack", "mesh_texture_corners", "obj_texture_text"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"texture off must not reach ops.{_n}"))
    for ext in (".glb", ".obj", ".ply"):
        plain = str(tmp_path / ("plain" + ext))
        n = pipeline.export_mesh_asset(plain, *_args(S), decimate_cell=2)
        for k, texel in enumerate((0, None)):
            p = str(tmp_path / (f"off{k}" + ext))
            assert pipeline.export_mesh_asset(p, *_args(S), decimate_cell=2, texture_texel=texel) == n and B(p) == B(plain)
    assert sorted(x for x in os.listdir(tmp_path) if x.endswith((".png", ".mtl"))) == []
    with pytest.raises(ValueError, match="ply"):
        pipeline.export_mesh_asset(str(tmp_path / "x.ply"), *_args(S), texture_texel=4)
    for bad in (3, 65):
        with pytest.raises(ValueError):
            pipeline.export_mesh_asset(str(tmp_path / "x.glb"), *_args(S), texture_texel=bad)
    assert not os.path.exists(tmp_path / "x.glb") and not os.path.exists(tmp_path / "x.ply")


def test_config_default_reaches_the_pipeline(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    want, plain, got, off = (str(tmp_path / n) for n in ("want.glb", "plain.glb", "got.glb", "off.glb"))
    pipeline.export_mesh_asset(want, *_args(S), decimate_cell=2, texture_texel=4)
    pipeline.export_mesh_asset(plain, *_args(S), decimate_cell=2)
    monkeypatch.setattr(config, "MESH_TEXTURE_TEXEL", 4)
    pipeline.export_mesh_asset(got, *_args(S), decimate_cell=2)
    pipeline.export_mesh_asset(off, *_args(S), decimate_cell=2, texture_texel=0)         # an explicit 0 wins
    assert B(got) == B(want) != B(plain) and B(off) == B(plain)
    monkeypatch.setattr(config, "MESH_TEXTURE_PNG_LEVEL", 0)
    pipeline.export_mesh_asset(got, *_args(S), decimate_cell=2)
    assert len(B(got)) > len(B(want)) and np.array_equal(mio.read_glb_texture(got)[1], mio.read_glb_texture(want)[1])


def test_reconstruct_folder_reports_the_texture(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    os.mkdir(tmp_path / "a")
    os.mkdir(tmp_path / "b")
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a" / "m.ply"), D=48, resolution=64, output_format=".glb", decimate_cell=2)
    assert plain["texture"] is None and plain["triangles"] > 0
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b" / "m.ply"), D=48, resolution=64, output_format=".glb", decimate_cell=2,
                                      texture_texel=4)
    L = mio.texture_layout(plain["triangles"], 4)
    assert out["texture"] == {"width": L["width"], "height": L["height"], "texel": 4, "texels": L["texels"]}
    assert {k: v for k, v in out.items() if k not in ("texture", "ply", "asset")} == {k: v for k, v in plain.items() if k not in ("texture", "ply", "asset")}
    assert open(out["ply"], "rb").read() == open(plain["ply"], "rb").read()               # the PLY stays vertex-coloured
    uv, img, _ = mio.read_glb_texture(out["asset"])
    assert img.shape[:2] == (L["height"], L["width"]) and uv.shape == (3 * plain["triangles"], 2) and mio.read_glb_texture(plain["asset"]) is None
    # without an asset there is nothing to texture
    none = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "c.ply"), D=48, resolution=64, decimate_cell=2, texture_texel=4)
    assert none["texture"] is None and "asset" not in none


def test_errors_are_statuses_not_faults(dev, tmp_path):
    v, f = _mesh(33, 33)
    good_v, good_t = torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(f).to(dev)
    for bad in (float("nan"), float("inf")):
        bv = good_v.clone()
        bv[20, 1] = bad
        with pytest.raises(RuntimeError, match="non-finite"):
            ops.mesh_texture_points(bv, good_t, 4, R)
    for bad in (35, -1, 2 ** 31 + 5):
        bt = good_t.clone()
        bt[17, 2] = bad
        with pytest.raises(RuntimeError, match="index"):
            ops.mesh_texture_points(good_v, bt, 4, R)
        # the unchecked form hands the counters on: the export raises after its copy, and the corners never dereference the index
        pts, world, stats = ops.mesh_texture_points(good_v, bt, 4, R, validate=False)
        rgb = torch.zeros(pts.shape[0], 3, device=dev)
        with pytest.raises(RuntimeError, match="index"):
            mio.export_asset(str(tmp_path / "bad.glb"), good_v, bt, R, texture={"texel": 4, "rgb": rgb, "stats": stats})
    # and the next call works
    pts, world, _ = ops.mesh_texture_points(good_v, good_t, 4, R)
    assert _B(pts) == mio.texture_points(v, f, 4, R)[0].tobytes()
    with pytest.raises(ValueError, match="CUDA"):
        ops.mesh_texture_points(good_v.cpu(), good_t.cpu(), 4, R)
    with pytest.raises(ValueError, match="CUDA"):
        ops.mesh_texture_pack(torch.zeros(17 * 16, 3), 33, 4)
    for call in (lambda: ops.mesh_texture_points(good_v.float(), good_t, 4, R), lambda: ops.mesh_texture_points(good_v, good_t.float(), 4, R),
                 lambda: ops.mesh_texture_points(good_v, good_t, 3, R), lambda: ops.mesh_texture_points(good_v, good_t, 65, R),
                 lambda: ops.mesh_texture_points(good_v, good_t, 4, 1), lambda: ops.mesh_texture_points(good_v, good_t, 4, R, (1.0, -1.0, -1.0)),
                 lambda: ops.mesh_texture_pack(torch.zeros(5, 3, device=dev), 33, 4), lambda: ops.mesh_texture_corners(good_v, good_t[:0], 4, R),
                 lambda: ops.mesh_texture_corners(good_v, good_t, 4, R, grad=torch.zeros(3, 3, device=dev))):
        with pytest.raises(ValueError):
            call()
    # through the C ABI: refused layouts and null pointers are statuses
    L = _lib.lib()
    w, h = ctypes.c_int(), ctypes.c_int()
    assert L.o2345_mesh_texture_texels(33, 4, ctypes.byref(w), ctypes.byref(h)) == 17 * 16 and (w.value, h.value) == (20, 16)
    for nt, c in ((0, 4), (33, 3), (33, 65), (2 * 256 * 256 + 1, 64), (2 ** 45, 4)):
        assert L.o2345_mesh_texture_texels(nt, c, None, None) == 0
    assert L.o2345_mesh_texture_texels(2 * 256 * 256, 64, ctypes.byref(w), None) == 2 ** 28 and w.value == 16384
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.o2345_mesh_texture_pack(None, 33, 4, None, s) == -1 and "null" in L.o2345_last_error().decode()
    assert L.o2345_mesh_texture_pack(None, 33, 3, None, s) == -1 and "layout" in L.o2345_last_error().decode()
    assert L.o2345_obj_texture_text_bytes(4, 1, 0) == 0 and L.o2345_obj_texture_text_bytes(3, 0, 0) == 0


# ---- guard bands (tests/guard_util.py): every output and the workspace at their EXACT sizes ---------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_kernel_writes_outside_its_buffers(dev, dtype):
    L = _lib.lib()
    g = Guard(dev)
    b0, b1 = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ib = 8 if dtype == torch.int64 else 4
    for nt, c in ((1, 4), (33, 4), (35, 5), (9, 8), (1, 64)):
        v, f = _mesh(nt, nt)
        lay = mio.texture_layout(nt, c)
        n, W, Hh = lay["texels"], lay["width"], lay["height"]
        verts, tris = torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(f).to(dev).to(dtype)
        rng = np.random.default_rng(nt)
        rgb = torch.from_numpy(rng.uniform(0, 1, (n, 3)).astype(np.float32)).to(dev)
        grad = torch.from_numpy(rng.normal(0, 1, (nt + 2, 3)).astype(np.float32)).to(dev)
        wsb = L.o2345_mesh_bounds_workspace_bytes(3 * nt)
        pts, world, stats = g.buf(24 * n, ("points", nt)), g.buf(12 * n, ("world", nt)), g.buf(STATS_BYTES, ("stats", nt))
        image = g.buf(4 * W * Hh, ("image", nt))
        pos, uv, nrm, idx = g.buf(36 * nt, ("positions", nt)), g.buf(24 * nt, ("uv", nt)), g.buf(36 * nt, ("normals", nt)), g.buf(12 * nt, ("indices", nt))
        bounds, ws = g.buf(24, ("bounds", nt)), g.buf(wsb, ("workspace", nt))
        _lib.check(L.o2345_mesh_texture_points(P(verts), nt + 2, P(tris), ib, nt, c, R, H(b0), H(b1), P(pts), P(world), P(stats), s), "mesh_texture_points")
        _lib.check(L.o2345_mesh_texture_pack(P(rgb), nt, c, P(image), s), "mesh_texture_pack")
        _lib.check(L.o2345_mesh_texture_corners(P(verts), nt + 2, P(tris), ib, nt, c, R, H(b0), H(b1), None, None, P(grad), P(pos), P(uv), P(nrm), P(idx), P(bounds),
                                                P(ws), wsb, s), "mesh_texture_corners")
        K = 1
        tb = L.o2345_obj_texture_text_bytes(3 * nt, K, 1)
        text = g.buf(tb, ("text", nt))
        _lib.check(L.o2345_obj_texture_text(P(pos), P(uv), P(nrm), 3 * nt, K, P(text), s), "obj_texture_text")
        bad = g.damaged()
        assert not bad, bad
        wp, ww = mio.texture_points(v, f, c, R)
        wpos, wuv, wnrm, wb = mio.texture_corners(v, f, c, R, grad=grad.cpu().numpy())
        assert _B(pts) == wp.tobytes() and _B(world) == ww.tobytes() and _B(stats) == bytes(STATS_BYTES)
        assert _B(image) == mio.pack_texture(rgb.cpu().numpy(), nt, c).tobytes()
        assert _B(pos) == wpos.tobytes() and _B(uv) == wuv.tobytes() and _B(nrm) == wnrm.tobytes() and _B(bounds) == wb.tobytes()
        assert _B(text) == mio.obj_texture_text_numpy(wpos, wuv, wnrm, K)
        assert _B(verts) == v.tobytes() and np.array_equal(tris.cpu().numpy(), f)
    assert len(g.live) == 11 * 5
