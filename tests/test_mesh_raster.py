"""CPU: the rasterizer's host twin (one-2-3-45_amd/raster.py), which defines the device's result, against hand cases whose images are written out in
mesh_raster_util.py, properties of the definition (order independence, a closed convex mesh under the three cull modes, ray depths on the faces' planes)
and the surface renderer's twin on the same lattice."""
import importlib

import numpy as np
import pytest

import mesh_raster_util as U

raster = importlib.import_module("one-2-3-45_amd.raster")
surface = importlib.import_module("one-2-3-45_amd.surface")
config = importlib.import_module("one-2-3-45_amd.config")


def test_the_hand_images():
    for name, s in U.scenes().items():
        if s["expect"] is None:
            continue
        r = U.twin(name)
        assert U.image_of(r["face"]) == s["expect"], (name, U.image_of(r["face"]))
        assert {k: r["info"][k] for k in s["info"]} == s["info"], (name, r["info"])
        hit = r["face"] >= 0
        assert np.array_equal(r["kind"].reshape(hit.shape) == 1, hit) and ((r["depth"] > 0) == hit).all() and (r["bary"][~hit] == 0).all()
        assert np.allclose(r["bary"][hit].sum(1), 1.0, atol=1e-6) and (r["rgb"][r["kind"] == 1] == 0.5).all()
        assert sum(r["info"][k] for k in raster.CLASSES[1:]) + r["info"]["binned"] == s["tris"].shape[0]


def test_the_hand_triangle_passes_through_samples():
    """its corner (1, 1), its top and left edges and its hypotenuse x + y = 7 run through pixel samples: the tie rule keeps the hypotenuse (d_y > 0) and
    drops the two others; depth is the plane's z = 1 and the barycentrics are the screen's"""
    r = U.twin("hand_triangle")
    assert r["face"][1, 1] == -1 and (r["face"][1, :] == -1).all() and (r["face"][:, 1] == -1).all()
    assert [r["face"][7 - x, x] for x in range(2, 6)] == [0, 0, 0, 0]
    assert (r["depth"][r["face"] == 0] == 1.0).all()
    assert r["bary"][2, 5].tolist() == [0.0, np.float32(0.8), np.float32(0.2)] and r["bary"][3, 3].tolist() == [np.float32(0.2), np.float32(0.4), np.float32(0.4)]


def test_a_shared_edge_through_samples_belongs_to_one_face():
    for name in ("hand_quad", "hand_quad_opposed"):
        s = U.scenes()[name]
        cam = raster.camera(s["K"], s["c2w"], s["near"], 0)
        S = raster.face_setup(s["verts"], s["tris"], cam, 8, 8)
        d = np.arange(1, 7)
        cov = [raster.pixel_terms(S, f, d, d)[1] for f in (0, 1)]                   # the diagonal's samples, corners included
        assert (cov[0].astype(int) + cov[1].astype(int))[1:5].tolist() == [1, 1, 1, 1], name
        assert U.image_of(U.twin(name)["face"]) == U.QUAD_IMAGE


def test_the_fan_vertex_has_one_owner():
    s = U.scenes()["hand_fan"]
    cam = raster.camera(s["K"], s["c2w"], s["near"], 0)
    S = raster.face_setup(s["verts"], s["tris"], cam, 16, 16)
    assert (S["cls"] == 0).all()
    py, px = (a.reshape(-1) for a in np.mgrid[0:16, 0:16])
    count = np.zeros(256, int)
    for f in range(6):
        x0, y0, x1, y1 = S["box"][f]
        inbox = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        count[inbox] += raster.pixel_terms(S, f, px[inbox], py[inbox])[1]
    count = count.reshape(16, 16)
    assert count.max() == 1 and count[8, 8] == 1                                    # no pixel twice: the spokes through samples, the hub
    assert count[8, 3:14].tolist() == [1] * 11                                      # the two horizontal spokes, between the rim vertices
    r = U.twin("hand_fan")
    assert np.array_equal(r["face"] >= 0, count == 1) and r["info"]["pixels"] == count.sum()
    # the hexagon's inside by its six half-planes in exact integers, for the samples off its boundary
    rim = [(14, 8), (11, 14), (5, 14), (2, 8), (5, 2), (11, 2)]
    edge = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for (ax, ay), (bx, by) in zip(rim, rim[1:] + rim[:1])]
    inside, outside = np.all([e > 0 for e in edge], 0).reshape(16, 16), np.any([e < 0 for e in edge], 0).reshape(16, 16)
    assert (count[inside] == 1).all() and (count[outside] == 0).all()


def test_identical_faces_and_crossing_faces():
    assert set(np.unique(U.twin("hand_identical")["face"])) == {-1, 0}
    r = U.twin("hand_crossing")
    assert (r["depth"][:, :4] < 2.0).all() and np.allclose(r["depth"][:, 4:], 2.0, rtol=1e-12)
    v, f = U.scenes()["hand_crossing"]["verts"], U.scenes()["hand_crossing"]["tris"]
    swapped = raster.rasterize(v, f[::-1].copy(), U.CENTRE_K, U.HAND_C2W, 8, 8, near=0.125)
    assert np.array_equal(swapped["face"], 1 - r["face"]) and swapped["depth"].tobytes() == r["depth"].tobytes()


def test_one_triangle_from_both_sides_under_each_cull():
    """seen from the origin its (P1 - P0) x (P2 - P0) points away from the camera: a back face; from behind it is a front face"""
    s = U.scenes()["hand_triangle"]
    P = s["verts"]
    n = np.cross(P[1] - P[0], P[2] - P[0])
    for name, c2w in (("hand_triangle", U.HAND_C2W), ("hand_triangle_back", U.BACK_C2W)):
        front = float(np.dot(n, c2w[:3, 3].astype(np.float64) - P[0])) > 0.0
        assert front == (name == "hand_triangle_back")
        hits = [int(U.twin(name, cull=c)["info"]["pixels"]) for c in (0, 1, 2)]
        culled = [int(U.twin(name, cull=c)["info"]["culled"]) for c in (0, 1, 2)]
        assert hits[0] > 0 and hits == ([hits[0], hits[0], 0] if front else [hits[0], 0, hits[0]]), (name, hits)
        assert culled == ([0, 0, 1] if front else [0, 1, 0])
    assert U.twin("hand_triangle_back")["info"]["pixels"] == 10


def test_refusals():
    s = U.scenes()["hand_triangle"]
    ok = lambda **kw: raster.rasterize(**{**dict(verts=s["verts"], tris=s["tris"], K=s["K"], c2w=s["c2w"], H=8, W=8, near=0.125), **kw})
    ok()
    skew, neg, shear = np.array(s["K"]), np.array(s["K"]), np.array(s["c2w"])
    skew[0, 1], neg[0, 0], shear[0, 1] = 0.1, -4.0, 1e-3
    for kw in (dict(K=skew), dict(K=neg), dict(c2w=shear), dict(c2w=2.0 * np.eye(4, dtype=np.float32)), dict(near=0.0), dict(near=np.inf), dict(near=np.nan),
               dict(cull=3), dict(cull=-1), dict(cull=True), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(verts=s["verts"].astype(np.float32)),
               dict(tris=s["tris"].astype(np.int16)), dict(vertex_colors=np.zeros((3, 3))), dict(vertex_normals=np.zeros((2, 3), np.float32))):
        with pytest.raises(ValueError):
            ok(**kw)


def _permuted(s, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(s["tris"].shape[0])
    rot = rng.integers(0, 3, perm.shape[0])
    tris = np.stack([np.roll(s["tris"][t], -int(k)) for t, k in zip(perm, rot)]) if perm.shape[0] else s["tris"].copy()
    return tris, perm, rot


@pytest.mark.parametrize("name", ["icosphere", "soup", "hand_fan", "hand_identical"])
def test_face_order_and_corner_rotation_only_permute(name):
    """face t of the new mesh is face perm[t] of the old with its corners rolled by rot[t]: face ids map through perm, bary rolls, depth keeps its bytes --
    up to the tie of two coincident faces, which goes to the smaller index of whichever order"""
    s, want = U.scenes()[name], U.twin(name)
    tris, perm, rot = _permuted(s, 5)
    got = raster.rasterize(s["verts"], tris, s["K"], s["c2w"], s["H"], s["W"], near=s["near"])
    assert got["depth"].tobytes() == want["depth"].tobytes() and got["info"] == want["info"]
    hit = got["face"] >= 0
    assert np.array_equal(hit, want["face"] >= 0)
    if name != "hand_identical":
        assert np.array_equal(perm[got["face"][hit]], want["face"][hit])
    k = rot[got["face"][hit]]
    rolled = np.stack([got["bary"][hit][np.arange(k.shape[0]), (j - k) % 3] for j in range(3)], 1)
    assert rolled.tobytes() == want["bary"][hit].tobytes()


def test_a_closed_convex_mesh_under_the_three_cull_modes():
    none, front, back = (U.twin("icosphere", cull=c) for c in (0, 1, 2))
    assert none["info"]["binned"] + none["info"]["offscreen"] + none["info"]["degenerate"] == 320 and none["info"]["binned"] > 100
    assert front["info"]["culled"] + back["info"]["culled"] + none["info"]["degenerate"] == 320            # every face with an area is one or the other
    a, b, c = (r["face"] >= 0 for r in (front, back, none))
    assert a.any() and np.array_equal(a, b) and np.array_equal(a | b, c)
    assert (front["depth"][a] <= back["depth"][a]).all() and (front["depth"][a] < back["depth"][a]).any()
    assert none["depth"].tobytes() == front["depth"].tobytes() and np.array_equal(none["face"], front["face"])


def test_ray_depth_lands_on_the_face():
    """The rasterizer interpolates over the SNAPPED screen triangle, so for an arbitrary mesh its depth is the plane's only to 1/512 pixel times the
    depth's slope.  The soup here has every corner on the 1/256-pixel grid (its projection is exact), so the snap moves nothing and what is left is the
    float32 rounding of the depth and of the ray's direction, 6e-8 relative each: the ray's point lies on the face's plane to 1e-6 of the depth."""
    s = U.scenes()["grid_soup"]
    r, plain = U.twin("grid_soup", ray_depth=True), U.twin("grid_soup")
    o, d = surface.camera_rays(s["K"], s["c2w"], s["H"], s["W"])
    hit = (r["face"] >= 0).reshape(-1)
    assert hit.sum() > 100 and np.array_equal(r["face"], plain["face"]) and r["bary"].tobytes() == plain["bary"].tobytes()
    t = r["depth"].reshape(-1)[hit].astype(np.float64)
    assert (t >= plain["depth"].reshape(-1)[hit]).all() and (t > plain["depth"].reshape(-1)[hit]).any()
    p = o[hit].astype(np.float64) + t[:, None] * d[hit].astype(np.float64)
    P = s["verts"][s["tris"][r["face"].reshape(-1)[hit]]]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    n /= np.linalg.norm(n, axis=1)[:, None]
    off = np.abs(((p - P[:, 0]) * n).sum(1)) / t
    assert (off <= 1e-6).all(), off.max()
    # and on the barycentric point, to the float32 rounding of the barycentrics times the face's size
    q = (r["bary"].reshape(-1, 3)[hit, :, None].astype(np.float64) * P).sum(1)
    assert (np.linalg.norm(q - p, axis=1) <= 1e-6 * (t + np.abs(P).max((1, 2)))).all()


def test_config_and_packer():
    assert config.MESH_PREVIEW_VIEWS == 0                                           # the environment of the test run leaves it unset
    assert config.mesh_preview_views() == 0 and config.mesh_preview_views(3) == 3 and config.mesh_preview_views(0) == 0
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            config.mesh_preview_views(bad)
    s = U.scenes()["icosphere"]
    col, nrm = U.attributes(s["verts"].shape[0])
    img = raster.render(s["verts"], s["tris"], s["K"], s["c2w"], s["H"], s["W"], background=(1, 2, 3, 4), near=s["near"], vertex_colors=col, vertex_normals=nrm)
    r = U.twin("icosphere", attrs=True)
    hit = r["face"] >= 0
    assert np.array_equal(img["face"], r["face"]) and (img["color"][~hit] == (1, 2, 3, 4)).all() and (img["color"][hit][:, 3] == 255).all()
    assert (img["normal"][~hit] == 0).all() and img["depth"].tobytes() == r["depth"].tobytes()
    assert 0.0 <= r["rgb"].min() and r["rgb"].max() <= 1.0 and np.array_equal(img["color"][hit][:, :3], surface._colour_u8(r["rgb"].reshape(29, 37, 3)[hit]))


# ---- the surface renderer on the same lattice ---------------------------------------------------------------------------------------------------------------
def cross_check(u, verts_idx, tris, K, c2w, H, W, mesh, trace):
    """The two conditions that follow from geometry (both surfaces separate the same lattice sign pattern, so inside a cell they are less than a cell
    diagonal apart) -> the figures.  mesh: rasterize's result with ray_depth; trace: (t f32 [H W], kind u8 [H W]) of the surface renderer."""
    R = u.shape[0]
    spacing = 2.0 / (R - 1)
    t_mesh, hit_mesh = mesh["depth"].astype(np.float64), mesh["face"] >= 0
    t_surf, hit_surf = trace[0].reshape(H, W).astype(np.float64), trace[1].reshape(H, W) != 0

    def eight_neighbours(m):
        """all eight neighbours are hits (a pixel on the image's border has a neighbour outside it: a miss)"""
        p = np.pad(m, 1, constant_values=False)
        return np.all([p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)], 0)
    surrounded = eight_neighbours(hit_mesh) & eight_neighbours(hit_surf)
    interior = surrounded & hit_mesh & hit_surf
    differ = hit_mesh != hit_surf
    _, d = surface.camera_rays(K, c2w, H, W)
    world = verts_idx / (R - 1.0) * 2.0 - 1.0
    P = world[tris[np.where(hit_mesh, mesh["face"], 0)]]
    n = np.cross(P[..., 1, :] - P[..., 0, :], P[..., 2, :] - P[..., 0, :])
    n /= np.maximum(np.linalg.norm(n, axis=-1), 1e-300)[..., None]
    facing = np.abs((n * d.reshape(H, W, 3)).sum(-1)) >= 0.5
    q = interior & facing
    gap = np.abs(t_mesh - t_surf)[q] / spacing
    return dict(differ_inside=int((differ & surrounded).sum()), differ=int(differ.sum()), qualifying=int(q.sum()), hits=int((hit_mesh | hit_surf).sum()),
                max_gap=float(gap.max()) if gap.size else 0.0)


def test_against_the_surface_twin():
    """the spheres-and-specks lattice, its raw marching-cubes mesh, one orbit camera at 64 x 64"""
    from mesh_components_util import spheres_field
    from oracle import mc as omc
    u = spheres_field(32)
    v, f = omc.marching_cubes(u, 0.0)
    K, c2w = U.orbit_camera(64, 64, view=1, n=5, elevation=25.0, radius=2.6)
    mesh = raster.rasterize(v / 31.0 * 2.0 - 1.0, f, K, c2w, 64, 64, near=0.05, ray_depth=True)
    o, d = surface.camera_rays(K, c2w, 64, 64)
    depth, kind, _, _ = surface.trace_rays(u, o, d, 0.0, 1.0e6)
    got = cross_check(u, v, f, K, c2w, 64, 64, mesh, (depth, kind))
    print(got)
    assert got["differ_inside"] == 0, got                                           # coverage differs only next to a miss of either image
    assert got["max_gap"] <= 2.0 * 3.0 ** 0.5, got
    assert 2 * got["qualifying"] >= got["hits"] > 200, got


def test_the_tool_renders_a_file_on_the_host(tmp_path, capsys):
    import json
    import os
    import sys
    mio = importlib.import_module("one-2-3-45_amd.mesh_io")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    tool = importlib.import_module("mesh_render")
    v, f = U.icosphere()
    colours = (U.attributes(v.shape[0])[0] * 255).astype(np.uint8)
    mio.write_ply_numpy(str(tmp_path / "ball.ply"), v, f, colours)
    mio.write_obj_numpy(str(tmp_path / "ball.obj"), v, f, colours)
    one = tool.main([str(tmp_path / "ball.ply"), str(tmp_path / "a.png"), "--host", "--size", "40x56", "--json"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == one and one[0]["path"] == str(tmp_path / "a.png")
    img = mio.read_png(one[0]["path"])
    hit = img[..., 3] == 255
    # the ball (radius 0.5) at 2.5 half diagonals of its box (2.165) under a focal length of 0.95 * 20 * sqrt(2.5^2 - 1) = 43.5: a disc of radius 10.3 pixels
    assert img.shape == (40, 56, 4) and 380 > one[0]["pixels"] == hit.sum() > 290 and one[0]["binned"] > 100
    assert not hit[0].any() and not hit[-1].any() and not hit[:, 0].any() and not hit[:, -1].any()           # the whole mesh is inside the image
    assert 19 <= hit.any(1).sum() <= 22 and 19 <= hit.any(0).sum() <= 22
    three = tool.main([str(tmp_path / "ball.obj"), str(tmp_path / "b.png"), "--host", "--size", "40x56", "--views", "3", "--normals", "--cull", "1"])
    assert [r["path"] for r in three] == [str(tmp_path / f"b_{k:03d}.png") for k in range(3)] and all(r["culled"] > 100 for r in three)
    assert mio.read_png(three[1]["path"]).shape == (40, 56, 4)
