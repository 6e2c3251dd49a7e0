"""CPU: the host twin of the textured shading stage (one-2-3-45_amd/raster.py: shade_textured, rasterize_textured, render_textured, asset_camera) against
hand cases and properties of the bake, never against itself: a hand triangle over an affine atlas, the bake round trip through texture_corners' corner
order and TEXCOORD rounding, the registration of the asset under asset_camera with the welded mesh under the reconstruction-frame camera, the normal
map through the file's tangent frames, the headlight formula, and the refusals."""
import importlib

import numpy as np
import pytest

import mesh_normal_map_util as NU
import mesh_raster_textured_util as TU
import mesh_raster_util as RU

raster = importlib.import_module("one-2-3-45_amd.raster")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
surface = importlib.import_module("one-2-3-45_amd.surface")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)))


# ---------------------------------------------------------------------------------------------------------- 1. the hand triangle
def test_hand_triangle_over_an_affine_atlas():
    pos, img = np.array(RU.TRIANGLE, np.float32), TU.hand_image()
    r = raster.rasterize_textured(pos, TU.HAND_UV, img, RU.HAND_K, RU.HAND_C2W, 8, 8)
    assert RU.image_of(r["face"]) == RU.TRIANGLE_IMAGE and r["info"]["pixels"] == 10 and r["tex_info"] == dict(bad_uv=0, flat_frame=0, back_lit=10)
    at = np.flatnonzero(r["face"].reshape(-1) == 0)
    # the triangle's corners sit on the screen points (1,1), (6,1), (1,6) at one depth: the barycentrics are those of the screen
    py, px = np.divmod(at, 8)
    b = np.stack([1.0 - (px - 1) / 5.0 - (py - 1) / 5.0, (px - 1) / 5.0, (py - 1) / 5.0], 1)
    assert np.abs(r["bary"].reshape(-1, 3)[at] - b).max() <= 1e-6
    bb = r["bary"].reshape(-1, 3)[at].astype(np.float64)
    u, v = bb @ TU.HAND_UV[:, 0].astype(np.float64), bb @ TU.HAND_UV[:, 1].astype(np.float64)
    want = TU.hand_value(u, v)
    got, taps = raster.fetch_texture(img, u, v)
    assert np.abs(got[:, :3] - want).max() <= 1e-9 * 255.0
    assert np.abs(sum(w for _, _, w in taps) - 1.0).max() <= 1e-15
    rgb = r["rgb"][at]
    assert (np.abs(rgb.astype(np.float64) - want / 255.0) <= ulp32(want / 255.0)).all()
    assert r["kind"].sum() == 10 and not r["rgb"][r["kind"] == 0].any() and not r["lit"][r["kind"] == 0].any() and not r["nrm"][r["kind"] == 0].any()
    # the flat normal of k_rs_shade, unnormalised
    e1, e2 = pos[1].astype(np.float64) - pos[0], pos[2].astype(np.float64) - pos[0]
    assert np.array_equal(r["nrm"][at], np.broadcast_to(np.cross(e1, e2).astype(np.float32), (10, 3)))
    # a back face under the headlight: the ambient term alone
    assert np.array_equal(r["lit"][at], (rgb.astype(np.float64) * 0.25).astype(np.float32))
    # the same fetch as the viewer's (mesh_io.sample_texture), tap for tap
    ref, touched = mio.sample_texture(img, np.stack([u, v], 1))
    assert np.array_equal(ref, got)
    for (xi, yi, w), (xj, yj, wj) in zip(taps, touched):
        assert np.array_equal(xi, xj) and np.array_equal(yi, yj) and np.array_equal(w, wj)


def test_uv_at_the_edges_outside_and_not_finite():
    c, img = TU.edge_case(), TU.hand_image()
    kind, rgb, nrm, lit, counts = raster.shade_textured(c["verts"], c["tris"], c["face"], c["bary"], c["uv"], img, RU.HAND_K, RU.HAND_C2W, ambient=1.0)
    assert kind.tolist() == [1] * 20 + [0, 0] and counts["bad_uv"] == 5 and counts["flat_frame"] == 0
    px = lambda j, i: img[j, i, :3].astype(np.float64) / 255.0
    # triangle 0: uv exactly (0,0), (1,1), (0,1): the corner texels, untouched by their neighbours
    for k, (j, i) in enumerate([(0, 0), (7, 7), (7, 0)]):
        assert np.array_equal(rgb[k], px(j, i).astype(np.float32))
    assert (np.abs(rgb[3].astype(np.float64) - TU.hand_value(0.5, 0.5)[None] / 255.0) <= ulp32(rgb[3])).all()          # (b0 + b1) / 2: the image's middle
    # triangle 1: outside, by a little and by 1e30: clamped to the border texels
    for k, (j, i) in enumerate([(7, 0), (0, 7), (0, 7)]):
        assert np.array_equal(rgb[5 + k], px(j, i).astype(np.float32))
    assert np.isfinite(rgb).all()
    # triangle 2: a NaN and an infinity among the coordinates: every pixel bad, rgb and lit 0, the flat normal, still a hit
    assert not rgb[10:15].any() and not lit[10:15].any() and nrm[10:15].any(1).all()
    # ambient 1: lit is the albedo
    assert np.array_equal(lit, rgb)
    # u = 1e300 reaches no index arithmetic: the clamp comes first
    got, taps = raster.fetch_texture(img, np.array([1e300, -1e300, 0.0, 1.0]), np.array([-1e300, 1e300, 1.0, 0.0]))
    assert np.array_equal(got[:, :3], np.stack([img[0, 7, :3], img[7, 0, :3], img[7, 0, :3], img[0, 7, :3]]).astype(np.float64))
    assert all(xi.min() >= 0 and xi.max() <= 7 and yi.min() >= 0 and yi.max() <= 7 for xi, yi, _ in taps)


# ---------------------------------------------------------------------------------------------------------- 2. the bake round trip
@pytest.mark.parametrize("texel,odd", [(4, False), (4, True), (5, True), (8, False)])
def test_bake_round_trip(texel, odd):
    """colours = an affine f of the texel's world point -> pack_texture -> texture_corners -> the textured render under asset_camera: at every hit pixel
    |rgb - f(p)| <= 1 / 255 + 1e-6 with p from the render's own face and bary on the welded vertices, corners reversed.  Derived: the truncating
    quantisation loses less than 1 / 255 per texel, a bilinear sample of an affine function is exact and a convex combination, the rest is float32 rounding."""
    a, r = TU.asset(texel, odd), TU.twin(texel, odd)
    assert (a["f"].shape[0] % 2 == 1) == odd and r["info"]["pixels"] > 300 and r["tex_info"]["bad_uv"] == 0
    at, p = TU.surface_points(a, r)
    err = np.abs(r["rgb"][at].astype(np.float64) - TU.colour_of(p))
    assert err.max() <= 1.0 / 255.0 + 1e-6, err.max()
    assert (r["rgb"][at].astype(np.float64) <= TU.colour_of(p) + 1e-6).all()                     # truncation only ever loses


@pytest.mark.parametrize("texel,odd", [(4, False), (4, True), (5, True), (8, False)])
def test_nothing_bleeds(texel, odd):
    """every triangle's own texels in a colour of its own, unused cells poisoned: a hit pixel shows its triangle's colour and nothing else"""
    a, r = TU.asset(texel, odd, paint="owners"), TU.twin(texel, odd, paint="owners")
    face = r["face"].reshape(-1)
    at = np.flatnonzero(face >= 0)
    want = TU.owner_bytes(a["f"].shape[0])[face[at]].astype(np.float64) / 255.0
    assert len(set(face[at].tolist())) > 50
    assert np.abs(r["rgb"][at].astype(np.float64) - want).max() <= 1e-6
    assert np.array_equal(r["face"], TU.twin(texel, odd)["face"])


# ---------------------------------------------------------------------------------------------------------- 3. registration
def exact_scene():
    """Welded triangles on integer index coordinates of a 9^3 lattice over [-1, 1]^3 (world coordinates are multiples of 0.25) under a camera whose rotation
    has entries 0, +-1 only and whose position is a multiple of 0.25: every product and sum of the projection is exact in both frames.  Every face is
    stored with its smallest index LAST: the asset's corner 0 (the welded corner 2) is then the first corner of the computation in both meshes, and the
    two windings, which are each other's reverse on the same screen points, run through the same sequence of operations."""
    rng = np.random.default_rng(12)
    v = rng.integers(1, 8, (40, 3)).astype(np.float64)
    f = rng.integers(0, 40, (60, 3))
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    k = np.argmin(f, 1)
    f = np.stack([f[np.arange(f.shape[0]), (k + 1) % 3], f[np.arange(f.shape[0]), (k + 2) % 3], f[np.arange(f.shape[0]), k]], 1).astype(np.int64)
    c2w = np.array([[1, 0, 0, 0.25], [0, -1, 0, -0.5], [0, 0, -1, 3.0], [0, 0, 0, 1]], np.float32)       # looks along -z; right x down = forward
    K = np.array([[16, 0, 11.5], [0, 16, 9.0], [0, 0, 1]], np.float32)
    return v, f, K, c2w


@pytest.mark.parametrize("cull", [0, 1, 2])
def test_registration_with_the_welded_mesh(cull):
    v, f, K, c2w = exact_scene()
    H, W, texel = 19, 24, 4
    pos, uv, _, _ = mio.texture_corners(v, f, texel, 9)
    world = v / 8.0 * 2.0 - 1.0
    assert np.array_equal(pos.astype(np.float64)[:, [0, 2, 1]], world[f[:, ::-1].reshape(-1)])
    M, s, mirrored = raster.asset_camera(c2w)
    assert s == 1.0 and mirrored and abs(np.linalg.det(M[:, :3].astype(np.float64)) + 1.0) < 1e-12
    assert np.array_equal(M, np.array([[1, 0, 0, 0.25], [0, 0, -1, 3.0], [0, -1, 0, -0.5]], np.float32))
    raster.camera(K, M, 1e-3, cull)                                                  # a reflection passes: R^T R is all that is tested
    image = np.full((mio.texture_layout(f.shape[0], texel)["height"], mio.texture_layout(f.shape[0], texel)["width"], 4), 200, np.uint8)
    welded = raster.rasterize(world, f, K, c2w, H, W, cull=cull)
    asset = raster.rasterize_textured(pos, uv, image, K, M, H, W, cull=cull)
    assert welded["info"]["pixels"] > 40 and np.array_equal(asset["face"], welded["face"])
    assert asset["depth"].tobytes() == welded["depth"].tobytes()
    assert asset["bary"].tobytes() == np.ascontiguousarray(welded["bary"][..., ::-1]).tobytes()
    if cull:
        both = raster.rasterize(world, f, K, c2w, H, W, cull=0)
        assert (welded["face"] != both["face"]).any()                                # the culling removes something
        assert asset["info"]["culled"] == welded["info"]["culled"] > 0


# ---------------------------------------------------------------------------------------------------------- 4. the normal map and the headlight
def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.sqrt((np.cross(a, b) ** 2).sum(-1)), (a * b).sum(-1))


@pytest.mark.parametrize("texel,odd", [(4, True), (5, False)])
def test_normal_map_through_the_files_frames(texel, odd):
    a, r = TU.asset(texel, odd, normal_map=True), TU.twin(texel, odd, normal_map=True)
    want = mio.frame_normals(TU.GRADIENT[None], a["trans_mat"])[0]
    at = np.flatnonzero(r["face"].reshape(-1) >= 0)
    assert at.shape[0] > 300 and r["tex_info"]["flat_frame"] == 0 and not mio.frame_is_degenerate(a["tan"]).any()
    ang = _angle(r["nrm"][at], want[None])
    assert ang.max() <= NU.DECODE_BOUND, ang.max()
    assert np.abs(np.sqrt((r["nrm"][at].astype(np.float64) ** 2).sum(1)) - 1.0).max() <= 2e-7
    # without the map the same pixels carry the flat normal, whose direction is the frame's N
    flat = TU.twin(texel, odd)
    assert np.array_equal(flat["face"], r["face"]) and np.array_equal(flat["rgb"], r["rgb"])
    assert _angle(flat["nrm"][at], a["nrm"][3 * r["face"].reshape(-1)[at]]).max() <= 1e-6


def test_a_degenerate_frame_gives_the_flat_normal_and_is_counted():
    a, r = TU.asset(5, False, normal_map=True), TU.twin(5, False, normal_map=True)
    face = r["face"].reshape(-1)
    t = int(np.bincount(face[face >= 0]).argmax())
    nrm, tan = a["nrm"].copy(), a["tan"].copy()
    nrm[3 * t:3 * t + 3], tan[3 * t:3 * t + 3] = (0.0, 1.0, 0.0), (1.0, -0.0, 0.0, 1.0)
    assert mio.frame_is_degenerate(tan).sum() == 3
    K, _, M, near = TU.camera(a, 29, 37)
    got = raster.rasterize_textured(a["pos"], a["uv"], a["image"], K, M, 29, 37, near=near, normals=nrm, tangents=tan, normal_image=a["nimage"])
    mine = face == t
    assert got["tex_info"]["flat_frame"] == mine.sum() > 0
    assert np.array_equal(got["nrm"][mine], np.broadcast_to(np.array([0, 1, 0], np.float32), (mine.sum(), 3)))
    assert np.array_equal(got["nrm"][~mine], r["nrm"][~mine]) and np.array_equal(got["rgb"], r["rgb"])


@pytest.mark.parametrize("ambient", [0.0, 0.25, 1.0])
def test_lit_is_the_headlight_formula(ambient):
    a = TU.asset(5, False, normal_map=True)
    r = TU.twin(5, False, normal_map=True, ambient=ambient)
    K, _, M, _ = TU.camera(a, 29, 37)
    at = np.flatnonzero(r["face"].reshape(-1) >= 0)
    py, px = np.divmod(at, 37)
    Kd, Md = K.astype(np.float64), M.astype(np.float64)
    d = np.stack([(px - Kd[0, 2]) / Kd[0, 0], (py - Kd[1, 2]) / Kd[1, 1], np.ones(at.shape[0])], 1) @ Md[:, :3].T
    d /= np.linalg.norm(d, axis=1)[:, None]
    n = r["nrm"][at].astype(np.float64)
    n /= np.linalg.norm(n, axis=1)[:, None]
    c = (n * d).sum(1)
    want = r["rgb"][at].astype(np.float64) * (ambient + (1.0 - ambient) * np.maximum(0.0, -c))[:, None]
    assert np.abs(r["lit"][at].astype(np.float64) - want).max() <= 2.0 ** -23                    # values in [0, 1]: a float32 rounding and the order of the sums
    assert r["tex_info"]["back_lit"] == int((c > 0).sum()) or abs(r["tex_info"]["back_lit"] - int((c > 0).sum())) <= int((np.abs(c) < 1e-12).sum())
    if ambient == 1.0:
        assert np.array_equal(r["lit"], r["rgb"])
    if ambient == 0.0:
        assert not r["lit"][at][c > 1e-9].any() and r["lit"][at][c < -0.1].any()
    # the handedness of the camera matrix does not enter: the reconstruction-frame view of the same surface is lit alike where the normal faces the camera
    assert (c < 0).mean() > 0.3


def test_render_textured_packs_the_three_images():
    a, r = TU.asset(5, False, normal_map=True), TU.twin(5, False, normal_map=True)
    K, _, M, near = TU.camera(a, 29, 37)
    out = raster.render_textured(a["pos"], a["uv"], a["image"], K, M, 29, 37, background=(1, 2, 3, 4), near=near, normals=a["nrm"], tangents=a["tan"],
                                 normal_image=a["nimage"])
    color, normal, depth = surface.pack_images(r["kind"], r["depth"].reshape(-1), r["rgb"], r["nrm"], 29, 37, (1, 2, 3, 4))
    lit = surface.pack_images(r["kind"], r["depth"].reshape(-1), r["lit"], r["nrm"], 29, 37, (1, 2, 3, 4))[0]
    assert set(out) == {"color", "lit", "normal", "depth", "face", "info", "tex_info"}
    assert np.array_equal(out["color"], color) and np.array_equal(out["lit"], lit) and np.array_equal(out["normal"], normal) and np.array_equal(out["depth"], depth)
    assert (out["color"][r["face"] < 0] == (1, 2, 3, 4)).all() and (out["lit"][r["face"] < 0] == (1, 2, 3, 4)).all()


# ---------------------------------------------------------------------------------------------------------- 5. refusals and asset_camera
def test_asset_camera_refusals_and_depth_scale():
    _, c2w = RU.orbit_camera(29, 37)
    sheared = NU.rotation().copy()
    sheared[0, 0, 1] += 0.01
    with pytest.raises(ValueError, match="orthogonal"):
        raster.asset_camera(c2w, None, sheared)
    for bad in (np.diag([2.0, 2.0, 3.0, 1.0]), np.diag([-1.0, -1.0, -1.0, 1.0]), np.diag([0.0, 0.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="scale"):
            raster.asset_camera(c2w, bad.astype(np.float32), None)
    with pytest.raises(ValueError):
        raster.asset_camera(np.eye(3, dtype=np.float32))
    # a reflecting trans_mat undoes the mirror
    flip = np.diag([1.0, 1.0, -1.0, 1.0]).astype(np.float32)
    assert not raster.asset_camera(c2w, None, flip)[2] and raster.asset_camera(c2w)[2]
    # the scaled and moved asset shows the pixels of the plain one, its depths multiplied by s
    plain, framed = TU.twin(5, False, framed=False), TU.twin(5, False)
    s = float(TU.SCALE_MAT[0, 0])
    assert raster.asset_camera(c2w, TU.SCALE_MAT, NU.rotation())[1] == s
    same = plain["face"] == framed["face"]
    assert same.mean() > 0.98 and (plain["face"] >= 0).sum() > 300                   # float32 positions move an edge across a sample here and there
    hit = same & (plain["face"] >= 0)
    assert np.abs(framed["depth"][hit] / plain["depth"][hit] - s).max() <= 1e-5
    ray = TU.twin(5, False, ray_depth=True)
    assert (ray["depth"][hit] >= framed["depth"][hit]).all() and np.array_equal(ray["face"], framed["face"])


def test_refusals_of_the_textured_stage():
    a = TU.asset(5, False, normal_map=True)
    K, _, M, near = TU.camera(a, 8, 8)
    go = lambda **kw: raster.rasterize_textured(**{**dict(positions=a["pos"], uv=a["uv"], image=a["image"], K=K, c2w=M, H=8, W=8, near=near), **kw})
    for kw in (dict(ambient=-0.1), dict(ambient=1.5), dict(ambient=float("nan")), dict(normal_image=a["nimage"]), dict(normals=a["nrm"], tangents=a["tan"]),
               dict(normals=a["nrm"], normal_image=a["nimage"]), dict(normals=a["nrm"], tangents=a["tan"], normal_image=a["nimage"][:-1]),
               dict(uv=a["uv"][:-3]), dict(image=a["image"][..., :3]), dict(image=a["image"].astype(np.float32)), dict(positions=a["pos"][:-1]),
               dict(positions=a["pos"].astype(np.float64)), dict(normals=a["nrm"][:-3], tangents=a["tan"], normal_image=a["nimage"]),
               dict(image=np.zeros((1, raster.TEX_MAX_SIDE + 1, 4), np.uint8)), dict(cull=3), dict(near=0.0)):
        with pytest.raises(ValueError):
            go(**kw)
    assert go()["tex_info"] == dict(bad_uv=0, flat_frame=0, back_lit=go()["tex_info"]["back_lit"])


# ---------------------------------------------------------------------------------------------------------- the file and the tool
def test_a_glb_read_from_disk_renders_like_its_buffers(tmp_path):
    a, r = TU.asset(5, False, normal_map=True), TU.twin(5, False, normal_map=True)
    path = str(tmp_path / "mesh.glb")
    mio.write_textured(path, a["pos"], a["uv"], a["nrm"], a["image"], tangents=a["tan"], normal_image=a["nimage"])
    b = mio.read_textured_glb(path)
    assert set(b) == {"pos", "uv", "image", "nrm", "tan", "nimage"}
    for k in b:
        assert b[k].dtype == a[k].dtype and b[k].tobytes() == a[k].tobytes(), k
    assert mio.frame_is_degenerate(b["tan"]).sum() == mio.frame_is_degenerate(a["tan"]).sum()
    K, _, M, near = TU.camera(a, 29, 37)
    got = raster.rasterize_textured(b["pos"], b["uv"], b["image"], K, M, 29, 37, near=near, normals=b["nrm"], tangents=b["tan"], normal_image=b["nimage"])
    for k in ("face", "depth", "bary", "kind", "rgb", "nrm", "lit"):
        assert got[k].tobytes() == r[k].tobytes(), k
    assert got["tex_info"] == r["tex_info"] and got["info"] == r["info"]
    plain = str(tmp_path / "plain.glb")
    mio.write_glb(plain, a["pos"], np.arange(a["pos"].shape[0], dtype=np.int32).reshape(-1, 3))
    with pytest.raises(ValueError, match="no texture"):
        mio.read_textured_glb(plain)


def test_the_tool_renders_a_textured_glb_on_the_host(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import mesh_render
    a = TU.asset(5, False, normal_map=True)
    path, out = str(tmp_path / "mesh.glb"), str(tmp_path / "out.png")
    mio.write_textured(path, a["pos"], a["uv"], a["nrm"], a["image"], tangents=a["tan"], normal_image=a["nimage"])
    rep = mesh_render.main([path, out, "--textured", "--lit", "--host", "--size", "24x32", "--cull", "1"])
    K, c2ws, half = mesh_render.fit_cameras(a["pos"].astype(np.float64), 1, 24, 32, 20.0)
    want = raster.render_textured(a["pos"], a["uv"], a["image"], K, c2ws[0], 24, 32, near=1e-3 * half, cull=1, normals=a["nrm"], tangents=a["tan"],
                                  normal_image=a["nimage"])
    assert np.array_equal(mio.read_png(out), want["lit"]) and rep[0]["pixels"] == want["info"]["pixels"] > 100 and rep[0]["back_lit"] == want["tex_info"]["back_lit"]
    assert want["info"]["culled"] > 0 and (want["lit"][..., :3].astype(int).sum(-1) > 0).sum() > 100
    # a proper camera in the asset's frame: cull 1 drops the far side, so nothing that is seen is lit from behind by more than the map's tilt
    assert want["tex_info"]["back_lit"] < 0.1 * want["info"]["pixels"]
    mesh_render.main([path, str(tmp_path / "albedo.png"), "--textured", "--host", "--size", "24x32"])
    assert np.array_equal(mio.read_png(str(tmp_path / "albedo.png")),
                          raster.render_textured(a["pos"], a["uv"], a["image"], K, c2ws[0], 24, 32, near=1e-3 * half, normals=a["nrm"], tangents=a["tan"],
                                                 normal_image=a["nimage"])["color"])
