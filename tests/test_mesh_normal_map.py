"""Tangent-space normal map on the CPU: the host twins of mesh_io (texture_frames / pack_normal_map / decode_normal_map), which are the definition the
device path (tests/test_gpu_mesh_normal_map.py) is compared against, and the files that carry the map.

The definition, restated (include/o2345.h): per triangle of the FILE -- float32 positions and uv, promoted to float64 -- N = unit(e1 x e2), T = unit(Pu -
N (N . Pu)) with Pu the derivative of the position along u, w = +1 iff (N x T) . (-Pv) >= 0; per texel n = the gradient normalised, rotated, renormalised,
y and z exchanged, and the channels are clamp(floor((n . {T, w N x T, N} 127.5 + 127.5) + 0.5), 0, 255).  Expected values come from that definition
(tests/mesh_normal_map_util.py spells it in plain Python floats), never from the code under test."""
import importlib
import json
import struct

import numpy as np
import pytest

import mesh_normal_map_util as U

mio = importlib.import_module("one-2-3-45_amd.mesh_io")


@pytest.fixture(scope="module")
def ball():
    return U.ellipsoid(24)


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("c", [4, 5])
def test_frames_and_decode_on_the_ellipsoid(ball, c, rot):
    v, f, grad_at = ball
    T = U.rotation() if rot else None
    nt = f.shape[0]
    pos, uv, _, _ = mio.texture_corners(v, f, c, 24, trans_mat=T)
    N, TW, degenerate = mio.texture_frames(pos, uv)
    assert N.dtype == TW.dtype == np.float32 and N.shape == (3 * nt, 3) and TW.shape == (3 * nt, 4) and degenerate == 0
    assert not mio.frame_is_degenerate(TW).any()
    for k in (1, 2):                                                          # flat: the three corners of a triangle carry one frame
        assert np.array_equal(N[0::3], N[k::3]) and np.array_equal(TW[0::3], TW[k::3])
    # the front face of the file's winding looks along the field's gradient, on every triangle
    centre = v[f].mean(1) / 23.0 * 2.0 - 1.0
    n_field = mio.frame_normals(grad_at(centre), T).astype(np.float64)
    Nd, Td, w = N[0::3].astype(np.float64), TW[0::3, :3].astype(np.float64), TW[0::3, 3].astype(np.float64)
    assert ((Nd * n_field).sum(1) > 0.0).all()
    assert (w == 1.0).all()                                                   # the layout is regular: no mirrored cell
    B = w[:, None] * np.cross(Nd, Td)
    for a, b, want in ((Nd, Nd, 1.0), (Td, Td, 1.0), (B, B, 1.0), (Nd, Td, 0.0), (Nd, B, 0.0), (Td, B, 0.0)):
        assert np.abs((a * b).sum(1) - want).max() < 1e-6
    # T follows increasing u and B decreasing v: against the derivatives of the position, solved from the corners' differences by LAPACK
    P, t = pos.reshape(nt, 3, 3).astype(np.float64), uv.reshape(nt, 3, 2).astype(np.float64)
    d = np.linalg.solve(np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]], 1), np.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], 1))      # rows: dP/du, dP/dv
    assert ((d[:, 0] * Td).sum(1) > 0.0).all() and ((d[:, 1] * B).sum(1) < 0.0).all()
    # decode: back in the asset frame every texel is the field's normal to within the quantisation
    _, world = mio.texture_points(v, f, c, 24)
    grad = grad_at(world)
    image, counts = mio.pack_normal_map(grad, N, TW, nt, c, T)
    L = mio.texture_layout(nt, c)
    assert image.shape == (L["height"], L["width"], 4) and image.dtype == np.uint8 and counts == {"bad_gradient": 0, "back_facing": 0}
    angles = U.decode_angles(image, N, TW, nt, c, mio.frame_normals(grad, T))
    print(f"normal map decode, c = {c}, rotation = {rot}: max angle {angles.max():.3e} rad, bound {U.DECODE_BOUND:.3e}")
    assert angles.max() <= U.DECODE_BOUND
    used, rest = U.to_cells(image, nt, c)
    assert (rest == U.FLAT).all() and (used[:, 3] == 255).all() and not (used == U.FLAT).all()
    assert mio.pack_normal_map(grad, N, TW, nt, c, None if T is None else T[0, :3, :3])[0].tobytes() == image.tobytes()       # the 3x3 alone
    # the face normal itself as the gradient (y and z back, the rotation back): z is 255; x and y are a rounding error around 0, which is the border
    # between 127 and 128 (the exact case: test_a_gradient_along_the_face_normal_is_the_flat_texel)
    g = N[3 * U.owners(nt, c)].astype(np.float64)[:, [0, 2, 1]]
    if rot:
        g = g @ T[0, :3, :3].astype(np.float64)
    flat = U.to_cells(mio.pack_normal_map(g.astype(np.float32), N, TW, nt, c, T)[0], nt, c)[0]
    assert (flat[:, 2:] == [255, 255]).all() and np.isin(flat[:, :2], (127, 128)).all() and (flat[:, :2] == 128).mean() > 0.4


@pytest.mark.parametrize("rot", [False, True])
def test_a_gradient_along_the_face_normal_is_the_flat_texel(rot):
    """n == N to the last bit needs a gradient that the normalisation leaves an exact unit vector: axis-aligned triangles, one for each of the six
    directions, with the flat (0, 1, 0) frame among them, which is no degenerate triangle"""
    T = None
    if rot:                                                                   # a quarter turn about z: exact in float32
        T = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    pos = []
    c, nt = 4, 6
    for n in axes:                                                            # a triangle with N = n: e1 x e2 = n
        e1 = np.roll(n, 1) if n.sum() > 0 else np.roll(-n, 2)
        e2 = np.cross(n, e1)
        pos += [np.zeros(3), e1, e2]
    pos = np.array(pos, np.float32)
    uv = mio.texture_corners(np.zeros((3, 3)), np.tile(np.arange(3), (nt, 1)), c, 8)[1]
    N, TW, degenerate = mio.texture_frames(pos, uv)
    assert degenerate == 0 and np.array_equal(N[0::3], axes.astype(np.float32))
    own = U.owners(nt, c)
    n_asset = N[3 * own].astype(np.float64)                                   # asset frame -> the gradient's frame: y and z back, then the rotation back
    g = n_asset[:, [0, 2, 1]]
    if rot:
        g = g @ T[:3, :3].astype(np.float64)                                  # R^T g, row-wise
    image, counts = mio.pack_normal_map((g * 7.0).astype(np.float32), N, TW, nt, c, T)
    assert (U.to_cells(image, nt, c)[0] == U.FLAT).all() and counts == {"bad_gradient": 0, "back_facing": 0}
    back, counts = mio.pack_normal_map((g * -7.0).astype(np.float32), N, TW, nt, c, T)
    assert (U.to_cells(back, nt, c)[0] == np.array([128, 128, 0, 255], np.uint8)).all() and counts == {"bad_gradient": 0, "back_facing": 6 // 2 * c * c}


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("nt, c", [(1, 4), (1, 5), (2, 4), (2, 5), (3, 4), (5, 4), (5, 5), (33, 4), (33, 5), (86, 4)])
def test_the_twin_equals_the_definition_texel_by_texel(nt, c, rot):
    case = U.strip(nt, c, seed=nt * 100 + c, rot=U.rotation() if rot else None)
    N, TW, degenerate = mio.texture_frames(case["pos"], case["uv"])
    image, counts = mio.pack_normal_map(case["grad"], N, TW, nt, c, case["rot"])
    rN, rTW, rimage, rcounts = U.reference(case)
    assert N.tobytes() == rN.tobytes() and TW.tobytes() == rTW.tobytes()          # bytes: the sign of the marking zero included
    assert image.tobytes() == rimage.tobytes()
    assert dict(counts, degenerate=degenerate) == rcounts
    # and the injected inputs did what they were put there for
    assert degenerate == len(case["degenerate"]) and counts["bad_gradient"] == len(case["bad"]) and counts["back_facing"] >= len(case["back"])
    used = U.to_cells(image, nt, c)[0]
    own = U.owners(nt, c)
    for t in case["degenerate"]:
        assert np.array_equal(N[3 * t:3 * t + 3], np.tile(np.float32([0, 1, 0]), (3, 1))) and np.array_equal(TW[3 * t:3 * t + 3], np.tile(np.float32([1, 0, 0, 1]), (3, 1)))
        assert mio.frame_is_degenerate(TW[3 * t:3 * t + 3]).all() and (used[own == t] == U.FLAT).all() and (own == t).any()
    assert (used[case["bad"]] == U.FLAT).all()
    for s in case["back"]:
        assert used[s, 2] == 0 and abs(int(used[s, 0]) - 128) <= 1 and abs(int(used[s, 1]) - 128) <= 1
    if nt % 2:                                                                # an odd count: the B half of the last cell is the last triangle's
        assert (own.reshape(-1, c * c)[-1] == nt - 1).all()
        last = used.reshape(-1, c * c, 4)[-1]
        assert not (last[np.arange(c * c) % c + np.arange(c * c) // c >= c] == U.FLAT).all() or nt - 1 in case["degenerate"] or nt == 1


def test_degenerate_frames():
    c = 4
    uv = mio.texture_corners(np.zeros((3, 3)), np.tile(np.arange(3), (6, 1)), c, 8)[1].copy()
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    pos = np.tile(tri, (6, 1))
    pos[3:6] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]                              # collinear: no area
    uv[6:9] = uv[6]                                                           # one uv for three corners: det == 0
    pos[9] = np.nan                                                           # a NaN coordinate
    pos[13, 0] = np.inf                                                       # an infinite one
    N, TW, degenerate = mio.texture_frames(pos, uv)
    assert degenerate == 4 and mio.frame_is_degenerate(TW[0::3]).tolist() == [False, True, True, True, True, False]
    assert np.array_equal(N[0], np.float32([0, 0, 1])) and np.array_equal(N[15], N[0]) and np.array_equal(TW[15], -TW[0] * np.float32([1, 1, 1, -1]))      # B's uv corners mirror A's
    assert np.array_equal(N[3:15], np.tile(np.float32([0, 1, 0]), (12, 1))) and np.array_equal(TW[3:15], np.tile(np.float32([1, 0, 0, 1]), (12, 1)))
    assert not np.signbit(N[[0, 15]]).any() and not np.signbit(TW[[0, 15]][TW[[0, 15]] == 0]).any()           # sound frames never carry the mark
    with pytest.raises(ValueError):
        mio.texture_frames(pos[:3], uv)
    with pytest.raises(ValueError):
        mio.pack_normal_map(np.zeros((5, 3), np.float32), N, TW, 6, c)
    with pytest.raises(ValueError):
        mio.pack_normal_map(np.zeros((3 * c * c, 3), np.float32), N[:3], TW, 6, c)


def test_decode():
    img = np.array([[[0, 255, 128, 7], [51, 102, 204, 255]]], np.uint8)
    assert np.array_equal(mio.decode_normal_map(img), np.array([[[-1.0, 1.0, 128 / 255 * 2 - 1], [51 / 255 * 2 - 1, 102 / 255 * 2 - 1, 204 / 255 * 2 - 1]]]))
    assert mio.NORMAL_MAP_FLAT == (128, 128, 255, 255)


# ------------------------------------------------------------------------------------------------------------------ files
@pytest.fixture(scope="module")
def asset(ball):
    v, f, grad_at = ball
    v, f = v, f[:41]
    c = 4
    pos, uv, vn, bounds = mio.texture_corners(v, f, c, 24, grad=grad_at(v / 23.0 * 2.0 - 1.0))
    pts, world = mio.texture_points(v, f, c, 24)
    N, TW, _ = mio.texture_frames(pos, uv)
    nimage, _ = mio.pack_normal_map(grad_at(world), N, TW, 41, c)
    image = mio.pack_texture(np.random.default_rng(0).uniform(0, 1, (world.shape[0], 3)).astype(np.float32), 41, c)
    return dict(pos=pos, uv=uv, vn=vn, N=N, TW=TW, image=image, nimage=nimage, bounds=bounds)


def test_glb_round_trip(asset, tmp_path):
    a = asset
    path = str(tmp_path / "m.glb")
    mio.write_textured(path, a["pos"], a["uv"], a["N"], a["image"], a["bounds"], tangents=a["TW"], normal_image=a["nimage"])
    p, faces, colors, normals = mio.read_glb(path)
    uv, image, sampler = mio.read_glb_texture(path)
    tangents, nimage = mio.read_glb_normal_map(path)
    assert np.array_equal(p, a["pos"]) and np.array_equal(uv, a["uv"]) and np.array_equal(normals, a["N"]) and colors is None
    assert tangents.tobytes() == a["TW"].tobytes() and np.array_equal(image, a["image"]) and np.array_equal(nimage, a["nimage"])
    assert np.array_equal(faces, np.arange(3 * 41).reshape(-1, 3))
    raw = open(path, "rb").read()
    jlen, = struct.unpack_from("<I", raw, 12)
    doc = json.loads(raw[20:20 + jlen])
    at = doc["meshes"][0]["primitives"][0]["attributes"]
    assert list(at) == ["POSITION", "NORMAL", "TANGENT", "TEXCOORD_0"]                  # TANGENT directly behind NORMAL
    tan = doc["accessors"][at["TANGENT"]]
    assert (tan["type"], tan["componentType"], tan["count"]) == ("VEC4", 5126, 3 * 41)
    assert doc["materials"][0]["normalTexture"] == {"index": 1} and doc["materials"][0]["pbrMetallicRoughness"]["baseColorTexture"] == {"index": 0}
    assert doc["textures"] == [{"sampler": 0, "source": 0}, {"sampler": 0, "source": 1}] and len(doc["images"]) == 2
    v0, v1 = (doc["bufferViews"][i["bufferView"]] for i in doc["images"])
    assert v1["byteOffset"] == v0["byteOffset"] + (v0["byteLength"] + 3) // 4 * 4 and "target" not in v1             # the second PNG behind the first
    assert doc["buffers"][0]["byteLength"] == v1["byteOffset"] + (v1["byteLength"] + 3) // 4 * 4 == len(raw) - 28 - jlen


def test_without_a_normal_map_the_bytes_are_the_parents(asset, tmp_path):
    """the parent's writers, spelled out: the JSON document key by key and the buffer order, for the textured file without a normal map"""
    a = asset
    for normals in (None, a["vn"]):
        path = str(tmp_path / "m.glb")
        mio.write_textured(path, a["pos"], a["uv"], normals, a["image"], a["bounds"])
        assert mio.read_glb_normal_map(path) is None
        n, m, png = 3 * 41, 41, mio.png_bytes(a["image"], 1)
        views, accessors, off = [], [], 0
        for nbytes, target, acc in ([(12 * m, 34963, {"componentType": 5125, "count": 3 * m, "type": "SCALAR"}),
                                     (12 * n, 34962, {"componentType": 5126, "count": n, "type": "VEC3", "min": [float(x) + 0.0 for x in a["bounds"][0]],
                                                      "max": [float(x) + 0.0 for x in a["bounds"][1]]})]
                                    + ([(12 * n, 34962, {"componentType": 5126, "count": n, "type": "VEC3"})] if normals is not None else [])
                                    + [(8 * n, 34962, {"componentType": 5126, "count": n, "type": "VEC2"})]):
            views.append({"buffer": 0, "byteOffset": off, "byteLength": nbytes, "target": target})
            accessors.append(dict({"bufferView": len(views) - 1, "byteOffset": 0}, **acc))
            off += nbytes
        views.append({"buffer": 0, "byteOffset": off, "byteLength": len(png)})
        off += (len(png) + 3) // 4 * 4
        attrs = {"POSITION": 1, **({"NORMAL": 2} if normals is not None else {}), "TEXCOORD_0": len(accessors) - 1}
        doc = {"asset": {"version": "2.0", "generator": "o2345-hip"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
               "meshes": [{"primitives": [{"attributes": attrs, "indices": 0, "mode": 4, "material": 0}]}], "accessors": accessors, "bufferViews": views,
               "buffers": [{"byteLength": off}],
               "materials": [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}],
               "textures": [{"sampler": 0, "source": 0}], "images": [{"bufferView": len(views) - 1, "mimeType": "image/png"}],
               "samplers": [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]}
        js = json.dumps(doc, separators=(",", ":")).encode("ascii")
        js += b" " * (-len(js) % 4)
        assert mio.glb_json(n, m, False, normals is not None, a["bounds"][0], a["bounds"][1], True, len(png)) == js
        body = (np.arange(n, dtype=np.uint32).tobytes() + a["pos"].tobytes() + (b"" if normals is None else normals.tobytes()) + a["uv"].tobytes()
                + png + b"\0" * (-len(png) % 4))
        want = struct.pack("<III", 0x46546C67, 2, 28 + len(js) + len(body)) + struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(body), 0x004E4942) + body
        assert open(path, "rb").read() == want
    obj = str(tmp_path / "plain.obj")
    mio.write_textured(obj, a["pos"], a["uv"], a["vn"], a["image"], a["bounds"])
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("plain")) == ["plain.mtl", "plain.obj", "plain.png"]
    assert b"map_Bump" not in open(str(tmp_path / "plain.mtl"), "rb").read() and mio.read_obj_normal_map(obj) is None
    assert np.array_equal(mio.read_obj_texture(obj)[4], a["image"])


def test_obj_triple_round_trip(asset, tmp_path):
    a = asset
    path = str(tmp_path / "m.obj")
    mio.write_textured(path, a["pos"], a["uv"], a["N"], a["image"], a["bounds"], tangents=a["TW"], normal_image=a["nimage"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["m.mtl", "m.obj", "m.png", "m_normal.png"]
    p, uv, vn, faces, image = mio.read_obj_texture(path)                      # keeps working, and the vn records carry the flat normals
    assert np.abs(p - a["pos"]).max() <= 0.5e-8 and np.abs(uv - a["uv"]).max() <= 1e-7 and np.abs(vn - a["N"]).max() <= 0.5e-8
    assert np.array_equal(image, a["image"]) and np.array_equal(faces, np.arange(3 * 41).reshape(-1, 3))
    assert np.array_equal(mio.read_obj_normal_map(path), a["nimage"]) and np.array_equal(mio.read_png(mio.obj_normal_map_name(path)), a["nimage"])
    mtl = open(str(tmp_path / "m.mtl")).read().split("\n")
    assert mtl[-4:] == ["map_Kd m.png", "map_Bump m_normal.png", "norm m_normal.png", ""]


def test_the_writers_refuse_half_a_normal_map(asset, tmp_path):
    a = asset
    for kw in (dict(tangents=a["TW"]), dict(normal_image=a["nimage"])):
        with pytest.raises(ValueError):
            mio.write_textured(str(tmp_path / "x.glb"), a["pos"], a["uv"], a["N"], a["image"], a["bounds"], **kw)
    with pytest.raises(ValueError):                                           # glTF needs NORMAL beside TANGENT
        mio.write_textured(str(tmp_path / "x.glb"), a["pos"], a["uv"], None, a["image"], a["bounds"], tangents=a["TW"], normal_image=a["nimage"])
    with pytest.raises(ValueError):
        mio.write_textured(str(tmp_path / "x.ply"), a["pos"], a["uv"], a["N"], a["image"], a["bounds"], tangents=a["TW"], normal_image=a["nimage"])
    with pytest.raises(ValueError):
        mio.glb_json(3, 1, False, True, [0, 0, 0], [1, 1, 1], True, 100, tangents=True)
    with pytest.raises(ValueError):
        mio.glb_json(3, 1, False, True, [0, 0, 0], [1, 1, 1], False, 0, tangents=True, normal_image_bytes=10)


def test_config_and_pipeline_refusals(monkeypatch):
    config = importlib.import_module("one-2-3-45_amd.config")
    pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
    assert config.MESH_NORMAL_MAP is False and config.mesh_normal_map() is False and config.mesh_normal_map(1) is True and config.mesh_normal_map(False) is False
    monkeypatch.setattr(config, "MESH_NORMAL_MAP", True)
    assert config.mesh_normal_map() is True and config.mesh_normal_map(0) is False
    opts = config.mesh_options(texture_texel=0)
    with pytest.raises(ValueError, match="texture_texel"):                    # before any device work: nothing else of the arguments is touched
        pipeline._mesh_fields(None, None, None, None, 16, opts, normal_map=True)
    assert pipeline._texture_block(None) is None
    lay = mio.texture_layout(5, 4)
    assert pipeline._texture_block(dict(layout=lay)) == {"width": 8, "height": 8, "texel": 4, "texels": 48}
    assert pipeline._texture_block(dict(layout=lay, grad=object()))["normal_map"] is True
