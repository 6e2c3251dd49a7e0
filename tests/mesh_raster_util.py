"""What the rasterizer's tests share: the fixtures (hand cases with their expected images written out, an icosphere, a soup, an extreme mesh), the
cameras, and the twin's results, each computed once (one-2-3-45_amd/raster.py is the definition; expected values never come from the device).

The hand camera sits at the origin and looks along +z with x right and y down: K = [[4, 0, 0], [0, 4, 0], [0, 0, 1]], so a vertex (X z / 4, Y z / 4, z)
lands on the screen point (X, Y) exactly for the z used here.  An expected image is a list of rows, '.' for no hit, a digit for the face index."""
import functools
import importlib

import numpy as np

raster = importlib.import_module("one-2-3-45_amd.raster")
surface = importlib.import_module("one-2-3-45_amd.surface")

HAND_K = np.array([[4, 0, 0], [0, 4, 0], [0, 0, 1]], np.float32)
HAND_C2W = np.eye(4, dtype=np.float32)
# the same scene from behind: at (0, 0, 2), looking along -z (right = -x, so that right x down = forward)
BACK_C2W = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 2], [0, 0, 0, 1]], np.float32)
BACK_K = np.array([[4, 0, 7], [0, 4, 0], [0, 0, 1]], np.float32)             # the screen point (X, Y) of the hand camera appears at (7 - X, Y)
CENTRE_K = np.array([[4, 0, 3.5], [0, 4, 3.5], [0, 0, 1]], np.float32)       # for the faces that fill the screen


def at(X, Y, z=1.0, K=HAND_K):
    """the world point that the hand camera sees at screen (X, Y) and depth z"""
    return [(X - float(K[0, 2])) * z / float(K[0, 0]), (Y - float(K[1, 2])) * z / float(K[1, 1]), z]


def _scene(verts, tris, K=HAND_K, c2w=HAND_C2W, H=8, W=8, near=0.125, expect=None, info=None):
    return dict(verts=np.array(verts, np.float64).reshape(-1, 3), tris=np.array(tris, np.int64).reshape(-1, 3), K=K, c2w=c2w, H=H, W=W, near=near,
                expect=expect, info=info)


def icosphere(level=2, radius=0.5):
    """a closed convex mesh, outward oriented: 20 * 4^level faces"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
         (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v) * radius, np.array(f, np.int64)


def orbit_camera(H, W, view=1, n=5, elevation=25.0, radius=2.0):
    """an orbit camera that looks at the origin, the principal point in the image's middle"""
    focal = 0.9 * max(H, W)
    K = np.array([[focal, 0, (W - 1) / 2.0], [0, focal, (H - 1) / 2.0], [0, 0, 1]], np.float32)
    return K, surface.orbit_c2w(n, elevation, radius)[view]


TRIANGLE = [at(1, 1), at(6, 1), at(1, 6)]                  # A2 > 0: its (P1 - P0) x (P2 - P0) points along +z, away from the hand camera -- a BACK face
TRIANGLE_IMAGE = ["........", "........", "..0000..", "..000...", "..00....", "..0.....", "........", "........"]
QUAD = [at(1, 1), at(6, 1), at(6, 6), at(1, 6)]            # its diagonal (1,1) - (6,6) runs through four pixel samples
QUAD_IMAGE = ["........", "........", "..10000.", "..11000.", "..11100.", "..11110.", "..11111.", "........"]
BIG = [(-20, -20), (40, -20), (-20, 40)]                   # a screen triangle that holds the whole 8 x 8 image
EMPTY_IMAGE = ["........"] * 8


def _fan():
    """six faces around a vertex on the pixel sample (8, 8) of a 16 x 16 image; the rim vertices sit on samples too, and the spokes to (14, 8) and (2, 8)
    run through samples"""
    rim = [(14, 8), (11, 14), (5, 14), (2, 8), (5, 2), (11, 2)]
    v = [at(8, 8)] + [at(x, y) for x, y in rim]
    return v, [(0, 1 + k, 1 + (k + 1) % 6) for k in range(6)]


def _crossing():
    """face 0 at z = 2 everywhere; face 1 over the same screen triangle with 1 / z linear in X and z = 2 at X = 3.5: nearer for the columns 0 .. 3"""
    slope = (0.5 - 0.625) / 23.5
    inv = lambda X: 0.625 + slope * (X + 20.0)
    v = [at(X, Y, 2.0, CENTRE_K) for X, Y in BIG] + [at(X, Y, 1.0 / inv(X), CENTRE_K) for X, Y in BIG]
    return v, [(0, 1, 2), (3, 4, 5)]


def _skips():
    """one face per skip class around one visible triangle (face 0)"""
    v = TRIANGLE + [at(2, 2, 1.0), at(5, 2, 1.0), at(2, 5, 0.0625),               # 3..5: straddles near = 0.125
                    at(2, 2, -1.0), at(5, 2, -1.0), at(2, 5, -1.0),                # 6..8: behind the camera
                    at(1, 1), at(3, 3), at(5, 5),                                  # 9..11: a zero-area sliver
                    at(20, 1), at(30, 1), at(20, 9),                               # 12..14: off the screen
                    [np.nan, 0.0, 1.0],                                            # 15
                    at(1.0e7, 1), at(2, 2.5), at(2.5, 2.5), at(2.2, 2.8)]          # 16: beyond 2^21 pixels; 17..19: a face between the samples
    f = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (0, 1, 15), (0, 1, 20), (0, -1, 2), (0, 1, 16), (17, 18, 19)]
    return v, f


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(verts, tris, K, c2w, H, W, near, expect: the face image under cull = 0 or None, info: the expected counts that are asserted or None)"""
    S = {}
    S["hand_triangle"] = _scene(TRIANGLE, [(0, 1, 2)], expect=TRIANGLE_IMAGE, info=dict(binned=1, pairs=1, pixels=10))
    S["hand_triangle_back"] = _scene(TRIANGLE, [(0, 1, 2)], K=BACK_K, c2w=BACK_C2W,
                                     expect=["........", "........", "...0000.", "....000.", ".....00.", "......0.", "........", "........"], info=dict(binned=1, pixels=10))
    S["hand_quad"] = _scene(QUAD, [(0, 1, 2), (0, 2, 3)], expect=QUAD_IMAGE, info=dict(binned=2, pairs=2, pixels=25))
    S["hand_quad_opposed"] = _scene(QUAD, [(0, 1, 2), (0, 3, 2)], expect=QUAD_IMAGE, info=dict(binned=2, pairs=2, pixels=25))
    v, f = _fan()
    S["hand_fan"] = _scene(v, f, H=16, W=16)
    S["hand_identical"] = _scene(TRIANGLE, [(0, 1, 2), (0, 1, 2)], expect=TRIANGLE_IMAGE, info=dict(binned=2, pixels=10))
    v, f = _crossing()
    S["hand_crossing"] = _scene(v, f, K=CENTRE_K, expect=["11110000"] * 8, info=dict(binned=2, pairs=2, pixels=64))
    S["hand_fullscreen"] = _scene(_crossing()[0][:3], [(0, 1, 2)], K=CENTRE_K, expect=["00000000"] * 8, info=dict(binned=1, pairs=1, pixels=64))
    v, f = _skips()
    S["hand_skips"] = _scene(v, f, expect=TRIANGLE_IMAGE,
                             info=dict(bad_index=2, nonfinite=1, near=2, range=1, degenerate=1, culled=0, offscreen=2, binned=1, pairs=1, pixels=10))
    S["hand_empty"] = _scene(TRIANGLE, np.zeros((0, 3), np.int64), expect=EMPTY_IMAGE, info={k: 0 for k in raster.COUNTS})
    S["hand_no_vertices"] = _scene(np.zeros((0, 3)), [(0, 1, 2)], expect=EMPTY_IMAGE, info=dict(bad_index=1, binned=0, pixels=0))
    v, f = icosphere()
    K, c2w = orbit_camera(29, 37)
    S["icosphere"] = _scene(v, f, K=K, c2w=c2w, H=29, W=37)
    rng = np.random.default_rng(7)
    v = rng.normal(0.0, 0.45, (90, 3))
    S["soup"] = _scene(v, rng.integers(0, 90, (150, 3)), K=K, c2w=c2w, H=29, W=37)            # faces through each other, some through the camera's near plane
    v, f = extreme_mesh()
    S["extreme"] = _scene(v, f, K=K, c2w=c2w, H=29, W=37)
    # every corner on the 1/256-pixel grid of the hand camera, at a depth of a few bits: the projection and the snap are exact
    X, Y, z = rng.integers(-2 * 256, 18 * 256, 60) / 256.0, rng.integers(-2 * 256, 18 * 256, 60) / 256.0, rng.integers(8, 49, 60) / 16.0
    S["grid_soup"] = _scene([at(a, b, c) for a, b, c in zip(X, Y, z)], rng.integers(0, 60, (80, 3)), H=16, W=16)
    for s in S.values():
        for a in (s["verts"], s["tris"], s["K"], s["c2w"]):
            a.setflags(write=False)
    return S


def extreme_mesh():
    """ordinary triangles next to ones whose arithmetic leaves the ordinary range (coordinates at +-1e160 and 1e-170), a corner exactly at z_c = near, a
    corner at 2^21 pixels exactly and one past it -- for the hand camera with near = 0.125; under another camera they are merely odd"""
    rng = np.random.default_rng(3)
    big, tiny = 1e160, 1e-170
    v = np.concatenate([rng.normal(0.0, 0.4, (30, 3)) + [0, 0, 1.5],
                        [[big, 0, big], [0, big, big], [-big, -big, big], [big, big, -big], [tiny, tiny, big], [0.3 * big, 0.3 * big, 0.3]],
                        [[tiny, 0, 1], [0, tiny, 1], [tiny, tiny, 1], [0.2 * tiny, 0.2 * tiny, tiny], [1, 1, tiny], [tiny, 1, 2]],
                        [at(1, 1, 0.125), at(6, 2, 0.125), at(2, 6, 1.0)],                              # 42..44: corners exactly at near
                        [at(2.0 ** 21, 1), at(1, 2), at(1, -2.0 ** 21)],                                # 45..47: exactly at the bound
                        [at(2.0 ** 21 + 1, 1), at(1, 2), at(3, 5)]])                                    # 48..50: one past it
    f = np.concatenate([rng.integers(0, 30, (40, 3)), np.arange(30, 51).reshape(-1, 3), [[0, 30, 36], [1, 42, 45], [2, 37, 44]]])
    return v, f.astype(np.int64)


def image_of(face):
    """face int32 [H,W] -> rows of '.' and digits"""
    return ["".join("." if t < 0 else str(int(t)) for t in row) for row in np.asarray(face)]


def attributes(nv, seed=11):
    """vertex colours in [0, 1] and vertex normals (not normalised: the packer does that), float32 [nv,3]"""
    rng = np.random.default_rng(seed + nv)
    return rng.random((nv, 3)).astype(np.float32), rng.normal(0.0, 1.0, (nv, 3)).astype(np.float32)


def resized(s, H, W):
    """scene s on an H x W image: the hand scenes keep their camera (the image shows more or less of the same screen), the others get the orbit camera of
    that size"""
    if (H, W) == (s["H"], s["W"]):
        return s
    if s["K"] is HAND_K or s["K"] is CENTRE_K or s["K"] is BACK_K:
        return dict(s, H=H, W=W, expect=None, info=None)
    K, c2w = orbit_camera(H, W)
    return dict(s, K=K, c2w=c2w, H=H, W=W, expect=None, info=None)


@functools.lru_cache(maxsize=None)
def twin(name, H=None, W=None, cull=0, ray_depth=False, attrs=False):
    """the twin's result for a named scene (at its own size, or H x W), computed once; read-only"""
    s = scenes()[name]
    s = resized(s, H or s["H"], W or s["W"])
    col, nrm = attributes(s["verts"].shape[0]) if attrs else (None, None)
    r = raster.rasterize(s["verts"], s["tris"], s["K"], s["c2w"], s["H"], s["W"], near=s["near"], cull=cull, ray_depth=ray_depth, vertex_colors=col,
                         vertex_normals=nrm)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


ARRAYS = ("face", "depth", "bary", "kind", "rgb", "nrm")


def assert_equal_results(got, want, what=""):
    """byte for byte, and the counts"""
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    for k in ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.reshape(-1).shape == b.reshape(-1).shape, (what, k, a.dtype, a.shape, b.dtype, b.shape)
        assert a.tobytes() == b.tobytes(), (what, k, int((a.reshape(-1) != b.reshape(-1)).sum()))
