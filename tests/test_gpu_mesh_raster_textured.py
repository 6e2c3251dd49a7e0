"""GPU: the textured shading stage (csrc/mesh_raster.hip: k_rs_shade_tex, o2345_mesh_raster_shade_textured) against the host twin
(one-2-3-45_amd/raster.py: shade_textured / rasterize_textured), which defines the result.  Every array and both sets of counts are compared EXACTLY
(bytes, whole dicts).  Expected values are the twin applied to the same inputs (itself checked against hand cases and properties of the bake in
tests/test_mesh_raster_textured.py), never the code under test; a twin result is computed once per case."""
import importlib

import numpy as np
import pytest
import torch

import mesh_raster_textured_util as TU
import mesh_raster_util as RU
from guard_util import Guard
from mesh_scene_util import args as _args, dev, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
raster = importlib.import_module("one-2-3-45_amd.raster")
surface = importlib.import_module("one-2-3-45_amd.surface")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

SIZES = ((8, 8), (29, 37), (48, 64))                          # H x W: one tile, not multiples of the tile, not square
NC, NT = len(raster.COUNTS), len(raster.TEX_COUNTS)
# (texel, odd, normal map, nt): texel 4 (the B leg is one texel) and 5; one triangle; an odd count (the last cell's B half repeats); 3 and 11 triangles
# have an atlas that is not square; with and without the normal map
CASES = ((4, True, False, None), (5, False, True, None), (4, True, True, 1), (5, True, False, 3), (4, True, True, 11), (5, False, False, 6))
MAPPED = ("nrm", "tan", "nimage")


def _host(out):
    return {k: x.cpu().numpy() if torch.is_tensor(x) else x for k, x in out.items()}


def _camera_args(K, M):
    """the two host arrays of the C ABI: K float32 [3,3] and the 3 x 4 of c2w"""
    return np.ascontiguousarray(K, np.float32), np.ascontiguousarray(np.asarray(M, np.float32)[:3])


def _shade(dev, verts, tris, face, bary, uv, image, frames, cam, H, W, ambient, g=None, stream=None):
    """the new entry itself on host arrays, every buffer at its exact size (inputs and outputs inside guard bands when ``g`` is given) -> the arrays and
    the counters on the host; the inputs are checked to be unwritten"""
    nv, nt, n = verts.shape[0], tris.shape[0], H * W
    ib = tris.dtype.itemsize
    inputs = dict(verts=np.ascontiguousarray(verts, np.float64), tris=np.ascontiguousarray(tris), face=np.ascontiguousarray(face, np.int32),
                  bary=np.ascontiguousarray(bary, np.float32), uv=np.ascontiguousarray(uv, np.float32), image=np.ascontiguousarray(image))
    if frames is not None:
        inputs.update(nrm=np.ascontiguousarray(frames[0], np.float32), tan=np.ascontiguousarray(frames[1], np.float32), nimage=np.ascontiguousarray(frames[2]))
    up = (lambda a, what: g.buf(src=a, what=what).view(getattr(torch, str(a.dtype)))) if g else (lambda a, what: torch.from_numpy(a.copy()).to(dev).view(-1))
    d = {k: up(a, k) for k, a in inputs.items()}
    new = (lambda nb, what: g.buf(nb, what)) if g else (lambda nb, what: torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev))
    kind, rgb, nrm, lit = new(n, "kind"), new(12 * n, "rgb").view(torch.float32), new(12 * n, "nrm").view(torch.float32), new(12 * n, "lit").view(torch.float32)
    counters = new(8 * NT, "counters").view(torch.int64)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _lib.call("o2345_mesh_raster_shade_textured", d["verts"], d["tris"], ib, nv, nt, d["face"], d["bary"], d["uv"], d["image"], image.shape[0], image.shape[1],
                  d.get("nimage"), d.get("nrm"), d.get("tan"), *cam, H, W, float(ambient), kind, rgb, nrm, lit, counters)
    torch.cuda.synchronize()
    for k, a in inputs.items():
        assert d[k].cpu().numpy().tobytes() == a.tobytes(), k
    c = counters.tolist()
    assert c[3] == 0
    return dict(kind=kind.cpu().numpy(), rgb=rgb.cpu().numpy().reshape(n, 3), nrm=nrm.cpu().numpy().reshape(n, 3), lit=lit.cpu().numpy().reshape(n, 3),
                tex_info=dict(zip(raster.TEX_COUNTS[:3], c)))


def _raw(dev, a, K, M, H, W, near, dtype, cull=0, ray_depth=False, ambient=0.25, g=None, stream=None):
    """count and emit as ops.mesh_raster runs them, then the new entry -> the twin's dict on the host"""
    verts = a["pos"].astype(np.float64)
    nv, nt = verts.shape[0], verts.shape[0] // 3
    tris = np.arange(nv, dtype=np.int64 if dtype == torch.int64 else np.int32).reshape(-1, 3)
    dv, dt = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    cam = _camera_args(K, M)
    cull = raster.mirrored_cull(cull, M)
    wsb = _lib.call("o2345_mesh_raster_workspace_bytes", nv, nt, H, W)
    ws, counts = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.empty(NC, dtype=torch.int64, device=dev)
    face, depth, bary = torch.empty(H, W, dtype=torch.int32, device=dev), torch.empty(H, W, device=dev), torch.empty(H, W, 3, device=dev)
    _lib.call("o2345_mesh_raster_count", dv, dt, tris.dtype.itemsize, nv, nt, *cam, H, W, near, cull, ws, wsb, counts)
    n_pairs = counts.tolist()[raster.COUNTS.index("pairs")]
    lists = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
    _lib.call("o2345_mesh_raster_emit", nv, nt, *cam, H, W, near, cull, int(ray_depth), ws, wsb, n_pairs, lists if n_pairs else None, face, depth, bary, counts)
    hf, hb = face.cpu().numpy(), bary.cpu().numpy()
    frames = tuple(a[k] for k in MAPPED) if "tan" in a else None
    out = _shade(dev, verts, tris, hf, hb, a["uv"], a["image"], frames, cam, H, W, ambient, g, stream)
    return dict(out, face=hf, depth=depth.cpu().numpy(), bary=hb, info=dict(zip(raster.COUNTS, counts.tolist())))


def _variant(k, dtype):
    """cull, depth mode and ambient alternate with the case and the index width, so that every value of each occurs at every size"""
    j = k + (dtype == torch.int64)
    return j % 3, bool(j % 2), (0.25, 0.0, 1.0)[(j // 2) % 3]


@pytest.mark.parametrize("size", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_every_case_equals_the_twin(dev, dtype, size):
    H, W = size
    hits = 0
    for k, (texel, odd, nm, nt) in enumerate(CASES):
        cull, ray_depth, ambient = _variant(k, dtype)
        a = TU.asset(texel, odd, nm, nt=nt)
        K, _, M, near = TU.camera(a, H, W)
        want = TU.twin(texel, odd, nm, H=H, W=W, cull=cull, ambient=ambient, ray_depth=ray_depth, nt=nt)
        TU.assert_equal_results(_raw(dev, a, K, M, H, W, near, dtype, cull, ray_depth, ambient), want, (texel, odd, nm, nt, cull))
        if dtype == torch.int32:
            t = lambda x: torch.from_numpy(np.array(x)).to(dev)
            kw = dict(normals=t(a["nrm"]), tangents=t(a["tan"]), normal_image=t(a["nimage"])) if nm else {}
            got = _host(ops.mesh_raster_textured(t(a["pos"]), t(a["uv"]), t(a["image"]), K, M, H, W, near=near, cull=cull, ray_depth=ray_depth, ambient=ambient, **kw))
            TU.assert_equal_results(got, want, (texel, odd, nm, nt, cull, "op"))
        hits += want["info"]["pixels"]
    assert hits > H * W // 2


def _edge_inputs(mapped):
    c = TU.edge_case()
    rng = np.random.default_rng(4)
    image = rng.integers(0, 256, (5, 11, 4)).astype(np.uint8) if mapped else TU.hand_image()
    frames = None
    if mapped:
        nimage = rng.integers(0, 256, (5, 11, 4)).astype(np.uint8)
        N, T = rng.normal(0.0, 1.0, (12, 3)).astype(np.float32), rng.normal(0.0, 1.0, (12, 4)).astype(np.float32)
        T[3:6, :3] = N[3:6]                                                     # T parallel to N: B = 0
        T[9:12] = (1.0, -0.0, 0.0, 1.0)                                         # triangle 3 carries the degenerate mark
        N[9:12] = (0.0, 1.0, 0.0)
        frames = (N, T, nimage)
    return c, image, frames


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_uv_at_the_edges_and_a_degenerate_frame(dev, dtype, mapped):
    """uv at 0 and 1, outside [0, 1] by a little and by 1e30, NaN and infinite; face ids that are no triangle; a frame with the degenerate mark; ambient 0
    and 1 -- face and bary written by hand, on an image that is neither square nor a multiple of anything"""
    c, image, frames = _edge_inputs(mapped)
    cam = _camera_args(RU.HAND_K, RU.HAND_C2W)
    tris = c["tris"].astype(dtype)
    tris[1, 2] = 12 if dtype == np.int32 else -(1 << 40)                        # triangle 1 has an index outside the vertices: a miss, never dereferenced
    n = c["face"].shape[1]
    for ambient in (0.0, 1.0, 0.25):
        kw = dict(normals=frames[0], tangents=frames[1], normal_image=frames[2]) if mapped else {}
        kind, rgb, nrm, lit, counts = raster.shade_textured(c["verts"], tris, c["face"], c["bary"], c["uv"], image, RU.HAND_K, RU.HAND_C2W, ambient=ambient, **kw)
        got = _shade(dev, c["verts"], tris, c["face"], c["bary"], c["uv"], image, frames, cam, 1, n, ambient)
        assert got["tex_info"] == counts and counts["bad_uv"] == 5 and (counts["flat_frame"] >= 5) == mapped
        assert kind.tolist() == [1] * 5 + [0] * 5 + [1] * 10 + [0, 0]
        for k, want in (("kind", kind), ("rgb", rgb), ("nrm", nrm), ("lit", lit)):
            assert got[k].tobytes() == want.tobytes(), (k, ambient)


def test_no_write_outside_the_buffers_and_no_write_to_the_inputs(dev):
    g = Guard(dev)
    for k, (texel, odd, nm, nt) in enumerate(CASES):
        H, W = SIZES[k % 3]
        a = TU.asset(texel, odd, nm, nt=nt)
        K, _, M, near = TU.camera(a, H, W)
        got = _raw(dev, a, K, M, H, W, near, (torch.int32, torch.int64)[k % 2], g=g)
        bad = g.damaged()
        assert not bad, bad
        TU.assert_equal_results(got, TU.twin(texel, odd, nm, H=H, W=W, nt=nt), (texel, odd, nm, nt))
    c, image, frames = _edge_inputs(True)
    _shade(dev, c["verts"], c["tris"], c["face"], c["bary"], c["uv"], image, frames, _camera_args(RU.HAND_K, RU.HAND_C2W), 1, c["face"].shape[1], 0.25, g=g)
    assert not g.damaged()
    assert len(g.live) == sum(11 + 3 * nm for _, _, nm, _ in CASES) + 14


def test_a_second_stream_and_a_second_run_give_identical_bytes(dev):
    side = torch.cuda.Stream(device=dev)
    a = TU.asset(5, False, True)
    K, _, M, near = TU.camera(a, 29, 37)
    runs = [_raw(dev, a, K, M, 29, 37, near, torch.int64, stream=st) for st in (None, None, side)]
    for r in runs:
        TU.assert_equal_results(r, TU.twin(5, False, True), "stream")


def test_render_textured_mesh_and_the_turntable(dev):
    a = TU.asset(5, False, True)
    K, c2w, M, near = TU.camera(a, 29, 37)
    kw = dict(normals=a["nrm"], tangents=a["tan"], normal_image=a["nimage"])
    want = raster.render_textured(a["pos"], a["uv"], a["image"], K, M, 29, 37, background=(9, 8, 7, 6), near=near, cull=1, ray_depth=True, ambient=0.5, **kw)
    host = {k: a[k] for k in ("pos", "uv", "image") + MAPPED}
    on_device = {k: torch.from_numpy(np.array(x)).to(dev) for k, x in host.items()}
    for asset in (host, on_device):
        got = pipeline.render_textured_mesh(asset, K, M, 29, 37, background=(9, 8, 7, 6), near=near, cull=1, ambient=0.5)
        assert set(got) == set(want)
        for k in ("color", "lit", "normal", "depth", "face"):
            assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        assert got["info"] == want["info"] and got["tex_info"] == want["tex_info"] and want["info"]["culled"] > 0
    plain = pipeline.render_textured_mesh({k: host[k] for k in ("pos", "uv", "image")}, K, M, 29, 37, near=near)
    flat = raster.render_textured(a["pos"], a["uv"], a["image"], K, M, 29, 37, near=near, ray_depth=True)
    assert plain["normal"].cpu().numpy().tobytes() == flat["normal"].tobytes() and plain["lit"].cpu().numpy().tobytes() == flat["lit"].tobytes()
    views, c2ws = pipeline.render_textured_turntable(on_device, K, 29, 37, 5, elevation_deg=25.0, radius=2.0, scale_mat=a["scale_mat"], trans_mat=a["trans_mat"])
    assert len(views) == 5 and c2ws.tobytes() == surface.orbit_c2w(5, 25.0, 2.0).tobytes() and np.array_equal(c2ws[1], c2w)
    one = raster.render_textured(a["pos"], a["uv"], a["image"], K, M, 29, 37, near=near, ray_depth=True, **kw)
    assert views[1]["lit"].cpu().numpy().tobytes() == one["lit"].tobytes() and views[1]["depth"].cpu().numpy().tobytes() == one["depth"].tobytes()
    with pytest.raises(ValueError):
        pipeline.render_textured_mesh({k: host[k] for k in ("pos", "uv", "image", "tan")}, K, M, 29, 37)


@pytest.fixture(scope="module")
def exported(dev, tmp_path_factory):
    """the stored small scene, decimated, with an atlas of texel 4 and a normal map: the file, and the buffers it was written from"""
    S = stored_scene(dev, extract=False)
    opts = config.mesh_options(None, None, 2, None, None, 4, None)
    m = pipeline._mesh_fields(*_args(S), opts, normal_map=True)
    path = str(tmp_path_factory.mktemp("textured") / "mesh.glb")
    mio.export_asset(path, m.verts_idx, m.tris, S["R"], vertex_colors=m.rgb, texture=m.texture)
    buffers = mio.textured_asset_buffers(m.verts_idx, m.tris, S["R"], texture=m.texture)
    return dict(path=path, buffers=buffers, nt=int(m.tris.shape[0]))


def test_the_file_on_disk_and_the_device_buffers_render_alike(dev, exported):
    b = exported["buffers"]
    assert set(MAPPED) <= set(b) and exported["nt"] > 100 and b["pos"].shape[0] == 3 * exported["nt"]
    disk = mio.read_textured_glb(exported["path"])
    for k in ("pos", "uv", "image") + MAPPED:
        assert disk[k].tobytes() == b[k].cpu().numpy().tobytes(), k
    K, c2w = RU.orbit_camera(48, 64, view=2, n=4, elevation=25.0, radius=1.6)
    M, s, mirrored = raster.asset_camera(c2w)
    assert s == 1.0 and mirrored
    from_disk = pipeline.render_textured_mesh(exported["path"], K, M, 48, 64, near=0.05, cull=1)
    from_buffers = pipeline.render_textured_mesh(b, K, M, 48, 64, near=0.05, cull=1)
    want = raster.render_textured(disk["pos"], disk["uv"], disk["image"], K, M, 48, 64, near=0.05, cull=1, ray_depth=True, normals=disk["nrm"],
                                  tangents=disk["tan"], normal_image=disk["nimage"])
    for k in ("color", "lit", "normal", "depth", "face"):
        assert from_disk[k].cpu().numpy().tobytes() == from_buffers[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert from_disk["info"] == from_buffers["info"] == want["info"] and from_disk["tex_info"] == from_buffers["tex_info"] == want["tex_info"]
    assert want["info"]["pixels"] > 100 and want["tex_info"]["bad_uv"] == 0


def test_every_refusal_is_a_status_and_launches_nothing(dev):
    a = TU.asset(5, True, True, nt=3)
    K, _, M, near = TU.camera(a, 8, 8)
    cam, n, nt = _camera_args(K, M), 64, 3
    t = lambda x: torch.from_numpy(np.array(x)).to(dev)
    verts, tris = t(a["pos"].astype(np.float64)), torch.arange(9, dtype=torch.int32, device=dev).view(3, 3)
    uv, image, nrm, tan, nimage = (t(a[k]) for k in ("uv", "image") + MAPPED)
    face, bary = torch.zeros(n, dtype=torch.int32, device=dev), torch.full((3 * n,), 1.0 / 3.0, device=dev)
    outs = [torch.full((m,), 0xA5, dtype=torch.uint8, device=dev) for m in (n, 12 * n, 12 * n, 12 * n, 8 * NT)]
    kind, rgb, shn, lit, counters = outs[0], outs[1].view(torch.float32), outs[2].view(torch.float32), outs[3].view(torch.float32), outs[4].view(torch.int64)

    def shade(verts=verts, tris=tris, ib=4, nv=9, nt=nt, face=face, bary=bary, uv=uv, image=image, th=image.shape[0], tw=image.shape[1], nimage=nimage, nrm=nrm,
              tan=tan, cam=cam, H=8, W=8, ambient=0.25, kind=kind, rgb=rgb, shn=shn, lit=lit, counters=counters):
        _lib.call("o2345_mesh_raster_shade_textured", verts, tris, ib, nv, nt, face, bary, uv, image, th, tw, nimage, nrm, tan, *cam, H, W, ambient, kind, rgb, shn,
                  lit, counters)

    def changed(which, at, x):
        """the camera with entry ``at`` of K (which = 0) or of c2w (which = 1) replaced"""
        new = [a.copy() for a in cam]
        new[which][at] = x
        return tuple(new)
    bad = [(dict(cam=changed(0, (0, 0), 0.0)), "fx and fy"), (dict(cam=changed(0, (0, 2), float("nan"))), "finite"), (dict(cam=changed(1, (0, 1), 1e-3)), "rotation"),
           (dict(cam=changed(1, (0, 0), 2.0)), "rotation"), (dict(cam=(None, cam[1])), "null pointer"), (dict(cam=(cam[0], None)), "null pointer"),
           (dict(cam=changed(0, (0, 1), 0.5)), "without skew"), (dict(cam=changed(0, (2, 2), 2.0)), "without skew"), (dict(H=0), "image size"), (dict(H=1 << 16, W=1 << 15), "image size"), (dict(ib=2), "index_bytes"),
           (dict(nv=1 << 30), "bad sizes"), (dict(nt=-1), "bad sizes"), (dict(th=0), "atlas size"), (dict(tw=16385), "atlas size"), (dict(th=-5), "atlas size"),
           (dict(nimage=None), "together"), (dict(nrm=None), "together"), (dict(tan=None), "together"), (dict(nimage=None, nrm=None), "together"),
           (dict(ambient=-0.01), "ambient"), (dict(ambient=1.5), "ambient"), (dict(ambient=float("nan")), "ambient"), (dict(ambient=float("inf")), "ambient"),
           (dict(face=None), "null pointer"), (dict(bary=None), "null pointer"), (dict(uv=None), "null pointer"), (dict(image=None), "null pointer"),
           (dict(verts=None), "null pointer"), (dict(tris=None), "null pointer"), (dict(kind=None), "null pointer"), (dict(lit=None), "null pointer"),
           (dict(counters=None), "null pointer"), (dict(image=outs[1][1:1 + image.numel()]), "aligned")]
    for kw, message in bad:
        with pytest.raises(RuntimeError, match=message):
            shade(**kw)
    torch.cuda.synchronize()
    assert all(bool((o == 0xA5).all()) for o in outs)                           # nothing was launched, not even the counters' memset
    shade()
    shade(nimage=None, nrm=None, tan=None)
    torch.cuda.synchronize()
    assert counters.tolist()[3] == 0 and int(kind.sum()) == n
    # a reflected camera is accepted: R^T R is all that is tested
    assert abs(np.linalg.det(np.asarray(M, np.float64)[:, :3]) + 1.0) < 1e-5
    # the Python side refuses before anything is launched
    go = dict(positions=t(a["pos"]), uv=uv, image=image, K=K, c2w=M, H=8, W=8, near=near)
    for kw in (dict(ambient=2.0), dict(normal_image=nimage), dict(normals=nrm, tangents=tan), dict(normals=nrm, tangents=tan, normal_image=nimage[:-1]),
               dict(uv=uv[:-1]), dict(image=image[..., :3]), dict(image=image.float()), dict(positions=t(a["pos"]).double()), dict(cull=3), dict(near=0.0),
               dict(c2w=2.0 * np.eye(4, dtype=np.float32)), dict(normals=nrm[:-1], tangents=tan, normal_image=nimage)):
        with pytest.raises(ValueError):
            ops.mesh_raster_textured(**{**go, **kw})


def test_reconstruct_folder_writes_textured_previews(tmp_path, dev, monkeypatch):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    assert config.TEXTURED_PREVIEW_VIEWS == 0                               # the environment of the test run leaves it unset
    kw = dict(D=48, resolution=64, simplify_faces=600, output_format=".glb", texture_texel=4, normal_map=True)
    (tmp_path / "on").mkdir(); (tmp_path / "off").mkdir()
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "on" / "a.ply"), textured_preview_views=2, **kw)
    assert len(out["textured_previews"]) == 2
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    K = s["query_intrinsic"].numpy()[:3, :3]
    for k, p in enumerate(out["textured_previews"]):
        assert p["path"] == str(tmp_path / "on" / f"textured_{k:03d}.png") and p["lit_path"] == str(tmp_path / "on" / f"textured_lit_{k:03d}.png")
        M, scale, _ = raster.asset_camera(p["c2w"], s["scale_mat"], s["trans_mat"])
        assert M.tobytes() == p["c2w_asset"].tobytes()
        want = pipeline.render_textured_mesh(out["asset"], K, M, 256, 256, near=1e-3 * scale)          # the file on disk, as a viewer reads it
        assert mio.read_png(p["path"]).tobytes() == want["color"].cpu().numpy().tobytes() == p["color"].tobytes()
        assert mio.read_png(p["lit_path"]).tobytes() == want["lit"].cpu().numpy().tobytes() == p["lit"].tobytes()
        assert p["info"] == want["info"] and p["tex_info"] == want["tex_info"] and p["info"]["pixels"] > 1000 and p["tex_info"]["bad_uv"] == 0
        assert p["color"].tobytes() != p["lit"].tobytes()
    assert out["textured_previews"][0]["c2w"].tobytes() == s["query_c2w"].numpy().astype(np.float32).tobytes()
    # off: the new op is not reached, the result has no new key, and the files keep their bytes
    monkeypatch.setattr(ops, "mesh_raster_textured", lambda *a, **k: pytest.fail("textured_preview_views = 0 must not reach ops.mesh_raster_textured"))
    off = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "off" / "a.ply"), **kw)
    assert set(off) == set(out) - {"textured_previews"}
    for name in ("a.ply", "mesh.glb"):
        assert open(tmp_path / "on" / name, "rb").read() == open(tmp_path / "off" / name, "rb").read()
    assert not (tmp_path / "off" / "textured_000.png").exists()
    with pytest.raises(ValueError, match="texture_texel"):
        pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "off" / "b.ply"), D=48, resolution=64, textured_preview_views=1)
