"""GPU: the mesh rasterizer (csrc/mesh_raster.hip) against the host twin (one-2-3-45_amd/raster.py), which defines the result.  Face ids, depths,
barycentrics, the shading arrays and the counts are compared EXACTLY (bytes, whole dicts).  Expected values are the twin applied to the same inputs
(itself checked against hand images and properties in tests/test_mesh_raster.py), never the code under test; a twin result is computed once."""
import importlib

import numpy as np
import pytest
import torch

import mesh_raster_util as U
from guard_util import PRE, Guard
from mesh_scene_util import args as _args, dev, dev_tris as _dev_tris, stored_scene  # noqa: F401 (dev: a fixture)
from test_mesh_raster import cross_check

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
raster = importlib.import_module("one-2-3-45_amd.raster")
surface = importlib.import_module("one-2-3-45_amd.surface")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

SIZES = ((8, 8), (29, 37), (48, 64))                          # H x W: one tile, not multiples of the tile, not square
NC = len(raster.COUNTS)


def _host(out):
    return {k: x.cpu().numpy() if torch.is_tensor(x) else x for k, x in out.items()}


def _camera_args(s):
    """the two host arrays of the C ABI: K float32 [3,3] and the 3 x 4 of c2w"""
    return np.ascontiguousarray(s["K"], np.float32), np.ascontiguousarray(np.asarray(s["c2w"], np.float32)[:3])


def _raw(dev, s, dtype, cull=0, ray_depth=False, attrs=False, g=None, stream=None):
    """the four entries themselves, every buffer at its exact size (inside guard bands when ``g`` is given) -> the twin's dict on the host"""
    hv, hf, H, W = s["verts"], s["tris"], s["H"], s["W"]
    nv, nt, n = hv.shape[0], hf.shape[0], s["H"] * s["W"]
    ib = 8 if dtype == torch.int64 else 4
    verts, tris = torch.from_numpy(np.array(hv, np.float64)).to(dev), _dev_tris(hf, dev, dtype)
    col, nrm = (torch.from_numpy(a).to(dev) for a in U.attributes(nv)) if attrs else (None, None)
    wsb = _lib.call("o2345_mesh_raster_workspace_bytes", nv, nt, H, W)
    assert wsb > 0 and PRE % 16 == 0
    new = (lambda nb, what: g.buf(nb, (what, nv, nt, H, W))) if g else (lambda nb, what: torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev))
    ws, counts = new(wsb, "workspace"), new(8 * NC, "counts").view(torch.int64)
    face, depth, bary = new(4 * n, "face").view(torch.int32), new(4 * n, "depth").view(torch.float32), new(12 * n, "bary").view(torch.float32)
    kind, rgb, shn = new(n, "kind"), new(12 * n, "rgb").view(torch.float32), new(12 * n, "nrm").view(torch.float32)
    cam = _camera_args(s)
    torch.cuda.synchronize()                                              # the buffers were filled on the current stream
    with torch.cuda.stream(stream):
        _lib.call("o2345_mesh_raster_count", verts, tris, ib, nv, nt, *cam, H, W, s["near"], cull, ws, wsb, counts)
        n_pairs = counts.tolist()[raster.COUNTS.index("pairs")]
        lists = new(4 * n_pairs, "lists").view(torch.int32) if n_pairs else None
        torch.cuda.synchronize()
        _lib.call("o2345_mesh_raster_emit", nv, nt, *cam, H, W, s["near"], cull, int(ray_depth), ws, wsb, n_pairs, lists, face, depth, bary, counts)
        _lib.call("o2345_mesh_raster_shade", verts, tris, ib, nv, nt, face, bary, H, W, col, nrm, kind, rgb, shn)
    torch.cuda.synchronize()
    assert verts.cpu().numpy().tobytes() == np.ascontiguousarray(hv, np.float64).tobytes() and np.array_equal(tris.cpu().numpy(), hf)
    return dict(face=face.cpu().numpy().reshape(H, W), depth=depth.cpu().numpy().reshape(H, W), bary=bary.cpu().numpy().reshape(H, W, 3), kind=kind.cpu().numpy(),
                rgb=rgb.cpu().numpy().reshape(n, 3), nrm=shn.cpu().numpy().reshape(n, 3), info=dict(zip(raster.COUNTS, counts.tolist())))


def _op(dev, s, dtype, cull=0, ray_depth=False, attrs=False):
    nv = s["verts"].shape[0]
    col, nrm = (torch.from_numpy(a).to(dev) for a in U.attributes(nv)) if attrs else (None, None)
    return _host(ops.mesh_raster(torch.from_numpy(np.array(s["verts"], np.float64)).to(dev), _dev_tris(s["tris"], dev, dtype), s["K"], s["c2w"], s["H"], s["W"],
                                 near=s["near"], cull=cull, ray_depth=ray_depth, vertex_colors=col, vertex_normals=nrm))


@pytest.mark.parametrize("size", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_every_fixture_equals_the_twin(dev, dtype, size):
    """the hand cases, the icosphere, the soups and the extreme mesh; the three cull modes; both depth modes and with / without vertex colours and normals
    alternate with the cull mode and the index width, so that every value of each occurs at every size"""
    H, W = size
    for name, s0 in U.scenes().items():
        s = U.resized(s0, H, W)
        for cull in (0, 1, 2):
            ray_depth, attrs = bool((cull + (dtype == torch.int64)) % 2), cull != 1
            want = U.twin(name, H, W, cull, ray_depth, attrs)
            U.assert_equal_results(_raw(dev, s, dtype, cull, ray_depth, attrs), want, (name, cull))
            U.assert_equal_results(_op(dev, s, dtype, cull, ray_depth, attrs), want, (name, cull, "op"))
        if (H, W) == (s0["H"], s0["W"]) and s0["expect"] is not None:
            assert U.image_of(_op(dev, s, dtype)["face"]) == s0["expect"], name


@pytest.mark.parametrize("name", ["icosphere", "grid_soup", "hand_crossing"])
def test_every_option_combination(dev, name):
    s = U.scenes()[name]
    for dtype in (torch.int32, torch.int64):
        for cull in (0, 1, 2):
            for ray_depth in (False, True):
                for attrs in (False, True):
                    U.assert_equal_results(_raw(dev, s, dtype, cull, ray_depth, attrs), U.twin(name, None, None, cull, ray_depth, attrs), (name, cull, ray_depth, attrs))


@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev)
    assert S["hf"].shape[0] > 100
    dv, dt, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=2)
    return dict(S, dv=dv.cpu().numpy(), df=dt.cpu().numpy())


def _scene_fixture(v_idx, f, R, view):
    K, c2ws = U.orbit_camera(48, 64)[0], surface.orbit_c2w(4, 25.0, 1.6)
    return dict(verts=np.asarray(v_idx, np.float64) / (R - 1.0) * 2.0 - 1.0, tris=np.asarray(f, np.int64), K=K, c2w=c2ws[view], H=48, W=64, near=0.05)


def test_the_stored_scene_before_and_after_clustering(scene):
    """whatever the images are, they are the twin's"""
    dev = scene["plain"][0].device
    for k, (v, f) in enumerate(((scene["hv"], scene["hf"]), (scene["dv"], scene["df"]))):
        for view in (0, 2):
            s = _scene_fixture(v, f, scene["R"], view)
            col, nrm = U.attributes(v.shape[0])
            want = raster.rasterize(s["verts"], s["tris"], s["K"], s["c2w"], 48, 64, near=0.05, ray_depth=bool(view), vertex_colors=col, vertex_normals=nrm)
            got = _op(dev, s, (torch.int32, torch.int64)[k], ray_depth=bool(view), attrs=True)
            U.assert_equal_results(got, want, (k, view))
            assert want["info"]["pixels"] > 100 and want["info"]["pairs"] >= want["info"]["binned"] > 100          # more than a tile of pixels, and of faces


def test_two_runs_and_a_second_stream_give_identical_bytes(dev, scene):
    side = torch.cuda.Stream(device=dev)
    for s in (_scene_fixture(scene["dv"], scene["df"], scene["R"], 1), U.scenes()["soup"], U.scenes()["hand_fan"]):
        runs = [_raw(dev, s, torch.int64, ray_depth=True, attrs=True, stream=st) for st in (None, None, side)]
        key = lambda r: tuple(sorted(r["info"].items())) + tuple(r[k].tobytes() for k in U.ARRAYS)
        assert key(runs[0]) == key(runs[1]) == key(runs[2])


GUARDED = ("hand_triangle", "hand_fan", "hand_crossing", "hand_skips", "hand_empty", "hand_no_vertices", "icosphere", "soup", "extreme")


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_kernel_writes_outside_its_buffers(dev, dtype):
    g = Guard(dev)
    expected = 0
    for name in GUARDED:
        for H, W in ((None, None), (29, 37)):
            s = U.resized(U.scenes()[name], H or U.scenes()[name]["H"], W or U.scenes()[name]["W"])
            got = _raw(dev, s, dtype, g=g)
            bad = g.damaged()
            assert not bad, bad
            U.assert_equal_results(got, U.twin(name, s["H"], s["W"]), name)
            expected += 8 + (got["info"]["pairs"] > 0)
    assert len(g.live) == expected


def test_every_refusal_is_a_status(dev):
    s = U.scenes()["hand_triangle"]
    verts, tris = torch.from_numpy(np.array(s["verts"])).to(dev), _dev_tris(s["tris"], dev, torch.int32)
    cam, n = _camera_args(s), 64
    wsb = _lib.call("o2345_mesh_raster_workspace_bytes", 3, 1, 8, 8)
    ws, counts = torch.zeros(wsb, dtype=torch.uint8, device=dev), torch.zeros(NC, dtype=torch.int64, device=dev)
    face, depth, bary = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev), torch.zeros(3 * n, device=dev)
    kind, rgb, nrm, lists = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(3 * n, device=dev), torch.zeros(3 * n, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    for sizes in ((-1, 1, 8, 8), (1 << 30, 1, 8, 8), (3, -1, 8, 8), (3, (1 << 31) // 3 + 1, 8, 8), (3, 1, 0, 8), (3, 1, 8, 0), (3, 1, 1 << 16, 1 << 15)):
        assert _lib.call("o2345_mesh_raster_workspace_bytes", *sizes) == 0, sizes
    assert _lib.call("o2345_mesh_raster_workspace_bytes", 0, 0, 1, 1) > 0

    def count(verts=verts, tris=tris, ib=4, nv=3, nt=1, cam=cam, H=8, W=8, near=0.125, cull=0, ws=ws, wsb=wsb, counts=counts):
        _lib.call("o2345_mesh_raster_count", verts, tris, ib, nv, nt, *cam, H, W, near, cull, ws, wsb, counts)

    def emit(nv=3, nt=1, cam=cam, H=8, W=8, near=0.125, cull=0, ray_depth=0, ws=ws, wsb=wsb, n_pairs=1, lists=lists, face=face, depth=depth, bary=bary, counts=counts):
        _lib.call("o2345_mesh_raster_emit", nv, nt, *cam, H, W, near, cull, ray_depth, ws, wsb, n_pairs, lists, face, depth, bary, counts)

    def shade(verts=verts, tris=tris, ib=4, nv=3, nt=1, face=face, bary=bary, H=8, W=8, kind=kind, rgb=rgb, nrm=nrm):
        _lib.call("o2345_mesh_raster_shade", verts, tris, ib, nv, nt, face, bary, H, W, None, None, kind, rgb, nrm)
    count(); emit(); shade()
    outs = (ws, counts, face, depth, bary, kind, rgb, nrm, lists)
    for o in outs:
        o.view(torch.uint8).fill_(0xA5)

    def changed(which, at, x):
        """the camera with entry ``at`` of K (which = 0) or of c2w (which = 1) replaced"""
        new = [a.copy() for a in cam]
        new[which][at] = x
        return tuple(new)
    cameras = [(changed(0, (0, 0), 0.0), "fx and fy"), (changed(0, (1, 1), -4.0), "fx and fy"), (changed(0, (0, 2), float("nan")), "finite"),
               (changed(1, (0, 3), float("inf")), "finite"), (changed(1, (0, 1), 1e-3), "rotation"), (changed(1, (0, 0), 2.0), "rotation"),
               ((None, cam[1]), "null pointer"), ((cam[0], None), "null pointer"), (changed(0, (0, 1), 0.5), "without skew"), (changed(0, (2, 2), 2.0), "without skew")]
    bad = [(count, dict(cam=c), m) for c, m in cameras] + [(emit, dict(cam=c), m) for c, m in cameras]
    for fn in (count, emit):
        bad += [(fn, dict(H=0), "image size"), (fn, dict(W=-1), "image size"), (fn, dict(H=1 << 16, W=1 << 15), "image size"), (fn, dict(near=0.0), "near"),
                (fn, dict(near=-1.0), "near"), (fn, dict(near=float("inf")), "near"), (fn, dict(near=float("nan")), "near"), (fn, dict(cull=3), "cull"),
                (fn, dict(cull=-1), "cull"), (fn, dict(wsb=wsb - 1), "workspace too small"), (fn, dict(ws=None), "null pointer"), (fn, dict(counts=None), "null pointer"),
                (fn, dict(nv=1 << 30), "bad sizes"), (fn, dict(nt=(1 << 31) // 3 + 1), "bad sizes"), (fn, dict(H=64, W=64), "workspace too small")]
    bad += [(count, dict(ib=2), "index_bytes"), (count, dict(verts=None), "null pointer"), (count, dict(tris=None), "null pointer"),
            (emit, dict(face=None), "null pointer"), (emit, dict(depth=None), "null pointer"), (emit, dict(bary=None), "null pointer"), (emit, dict(lists=None), "null pointer"),
            (emit, dict(n_pairs=-1), "pair count"), (emit, dict(n_pairs=1 << 31), "pair count"), (emit, dict(nt=0, n_pairs=1), "pair count"),
            (shade, dict(ib=3), "index_bytes"), (shade, dict(H=0), "image size"), (shade, dict(face=None), "null pointer"), (shade, dict(kind=None), "null pointer"),
            (shade, dict(tris=None), "null pointer"), (shade, dict(verts=None), "null pointer"), (shade, dict(nv=1 << 30), "bad sizes")]
    for fn, kw, message in bad:
        with pytest.raises(RuntimeError, match=message):
            fn(**kw)
    torch.cuda.synchronize()
    assert all(bool((o.view(torch.uint8) == 0xA5).all()) for o in outs)          # nothing was launched, not even a memset
    # the Python side refuses before anything is launched
    for kw in (dict(cull=3), dict(near=0.0), dict(H=0), dict(K=np.array([[4, 0.5, 0], [0, 4, 0], [0, 0, 1]], np.float32)), dict(c2w=2.0 * np.eye(4, dtype=np.float32)),
               dict(vertex_colors=torch.zeros(3, 3, dtype=torch.float64, device=dev)), dict(verts=verts.float())):
        a = {**dict(verts=verts, tris=tris, K=s["K"], c2w=s["c2w"], H=8, W=8, near=0.125), **kw}
        with pytest.raises(ValueError):
            ops.mesh_raster(**a)
    # a stale or foreign pair count is clamped, not trusted: fewer pairs than counted drop faces, they write nothing outside the lists
    g = Guard(dev)
    s = U.scenes()["icosphere"]
    v, t = torch.from_numpy(np.array(s["verts"])).to(dev), _dev_tris(s["tris"], dev, torch.int64)
    wsb2 = _lib.call("o2345_mesh_raster_workspace_bytes", v.shape[0], t.shape[0], 29, 37)
    ws2, n2 = g.buf(wsb2, "ws"), 29 * 37
    c2, f2, d2, b2 = g.buf(8 * NC, "counts").view(torch.int64), g.buf(4 * n2, "face").view(torch.int32), g.buf(4 * n2, "depth").view(torch.float32), g.buf(12 * n2, "bary").view(torch.float32)
    _lib.call("o2345_mesh_raster_count", v, t, 8, v.shape[0], t.shape[0], *_camera_args(s), 29, 37, s["near"], 0, ws2, wsb2, c2)
    short = g.buf(4 * 7, "lists").view(torch.int32)
    _lib.call("o2345_mesh_raster_emit", v.shape[0], t.shape[0], *_camera_args(s), 29, 37, s["near"], 0, 0, ws2, wsb2, 7, short, f2, d2, b2, c2)
    assert not g.damaged() and int(f2.max()) < t.shape[0] and int(f2.min()) >= -1


def test_reconstruct_folder_writes_mesh_previews(tmp_path, dev, monkeypatch):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    assert config.MESH_PREVIEW_VIEWS == 0                                  # the environment of the test run leaves it unset
    kw = dict(D=48, resolution=64, simplify_faces=600)
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), mesh_preview_views=2, preview_views=2, **kw)
    assert len(out["mesh_previews"]) == 2
    m = out["mesh_preview_mesh"]
    assert m["verts"].shape[0] == out["vertices"] and m["tris"].shape[0] == out["triangles"] and float(m["verts"].abs().max()) <= 1.0
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    K = s["query_intrinsic"].numpy()[:3, :3]
    for k, (p, q) in enumerate(zip(out["mesh_previews"], out["previews"])):
        assert p["path"] == str(tmp_path / f"mesh_preview_{k:03d}.png") and p["c2w"].tobytes() == q["c2w"].tobytes()          # the surface previews' cameras
        img = mio.read_png(p["path"])
        want = pipeline.render_mesh((m["verts"], m["tris"]), K, p["c2w"], 256, 256, vertex_colors=m["vertex_colors"])
        assert img.dtype == np.uint8 and img.shape == (256, 256, 4) and img.tobytes() == want["color"].cpu().numpy().tobytes() == p["color"].tobytes()
        assert p["normal"].tobytes() == want["normal"].cpu().numpy().tobytes() and p["depth"].tobytes() == want["depth"].cpu().numpy().tobytes()
        assert np.array_equal(p["face"], want["face"].cpu().numpy()) and p["info"] == want["info"] and p["info"]["pixels"] > 1000
        assert ((p["color"][..., 3] == 255) == (p["face"] >= 0)).all()
        # the chain changed the mesh, and only the mesh preview shows it; both show the same object from the same camera
        both = (p["face"] >= 0) & (q["depth"] > 0)
        assert p["color"].tobytes() != q["color"].tobytes() and both.sum() > 0.8 * max((p["face"] >= 0).sum(), (q["depth"] > 0).sum())
    assert out["mesh_previews"][0]["c2w"].tobytes() == s["query_c2w"].numpy().astype(np.float32).tobytes()
    # off: the new op is not reached, the result has no new key, and the PLY keeps its bytes
    monkeypatch.setattr(ops, "mesh_raster", lambda *a, **k: pytest.fail("mesh_preview_views = 0 must not reach ops.mesh_raster"))
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), **kw)
    off = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "c.ply"), mesh_preview_views=0, **kw)
    assert set(plain) == set(off) == set(out) - {"mesh_previews", "mesh_preview_mesh", "previews"}
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read() == open(tmp_path / "c.ply", "rb").read()
    assert not (tmp_path / "mesh_preview_002.png").exists()


def test_render_mesh_and_the_turntable(dev):
    s = U.scenes()["icosphere"]
    col, nrm = U.attributes(s["verts"].shape[0])
    want = raster.render(s["verts"], s["tris"], s["K"], s["c2w"], 29, 37, background=(9, 8, 7, 6), near=1e-3, ray_depth=True, vertex_colors=col, vertex_normals=nrm)
    got = pipeline.render_mesh((s["verts"], s["tris"].astype(np.int32)), s["K"], s["c2w"], 29, 37, vertex_colors=col, vertex_normals=torch.from_numpy(nrm).to(dev),
                               background=(9, 8, 7, 6))
    for k in ("color", "normal", "depth", "face"):
        assert got[k].is_cuda and got[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert got["info"] == want["info"]
    views, c2ws = pipeline.render_mesh_turntable((s["verts"], s["tris"]), s["K"], 29, 37, 3, elevation_deg=30.0, radius=2.2, vertex_colors=col)
    assert len(views) == 3 and c2ws.tobytes() == surface.orbit_c2w(3, 30.0, 2.2).tobytes()
    one = pipeline.render_mesh((s["verts"], s["tris"]), s["K"], c2ws[1], 29, 37, vertex_colors=col)
    assert torch.equal(views[1]["color"], one["color"]) and torch.equal(views[1]["depth"], one["depth"]) and views[1]["info"]["pixels"] > 0


def test_against_the_surface_renderer(dev):
    """once on the GPU, with the set-up whose two twins tests/test_mesh_raster.py checks: the spheres-and-specks lattice, its raw marching-cubes mesh (the
    device's), one orbit camera at 64 x 64, both device renderers"""
    from mesh_components_util import spheres_field
    u = spheres_field(32)
    du = torch.from_numpy(np.array(u)).to(dev)
    v_idx, tris = ops.marching_cubes(du, 0.0)
    K, c2w = U.orbit_camera(64, 64, view=1, n=5, elevation=25.0, radius=2.6)
    mesh = _host(ops.mesh_raster((v_idx / 31.0 * 2.0 - 1.0).contiguous(), tris, K, c2w, 64, 64, near=0.05, ray_depth=True))
    o, d = ops.camera_rays(K, c2w, 64, 64, dev)
    tr = ops.surface_trace(du, o, d, 0.0, 1.0e6, image_hw=(64, 64))
    got = cross_check(u, v_idx.cpu().numpy(), tris.cpu().numpy(), K, c2w, 64, 64, mesh, (tr["depth"].cpu().numpy(), tr["kind"].cpu().numpy()))
    print(got)
    assert got["differ_inside"] == 0, got
    assert got["max_gap"] <= 2.0 * 3.0 ** 0.5, got
    assert 2 * got["qualifying"] >= got["hits"] > 200, got
