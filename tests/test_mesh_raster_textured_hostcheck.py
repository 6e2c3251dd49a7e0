"""CPU: csrc/mesh_raster_tex_math.h compiled for the host (tests/hostcheck/mesh_raster_tex_check.hip, a stand-alone program) against the numpy twin in
raster.py: per pixel the uv, the four taps and weights, the fetched value, the albedo, the decoded normal and the lit colour, all equal to the bit, over
the bake scenes, the normal-map scenes and the edge uvs of the twin's own tests.  This is the source the GPU executes; it pins the shared arithmetic
before any GPU time is spent."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import mesh_raster_textured_util as TU
import mesh_raster_util as RU

raster = importlib.import_module("one-2-3-45_amd.raster")
surface = importlib.import_module("one-2-3-45_amd.surface")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(HERE, "hostcheck", "mesh_raster_tex_check")
    src = os.path.join(HERE, "hostcheck", "mesh_raster_tex_check.hip")
    csrc = os.path.join(os.path.dirname(HERE), "one-2-3-45_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def run(exe, tmp_path, K, M, ambient, image, nimage, px, py, bary, uv6, N, T):
    n = px.shape[0]
    Kd, Md = surface._pinhole(K, M)
    camera = np.concatenate([Md[:, :3].reshape(-1), [Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2], float(np.float32(ambient))]]).astype(np.float64)
    qd = np.concatenate([np.stack([px, py], 1).astype(np.float64), bary.astype(np.float64)], 1)
    qf = np.concatenate([uv6.reshape(n, 6), N, T], 1).astype(np.float32)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([n, image.shape[0], image.shape[1], int(nimage is not None)], np.int64).tobytes() + camera.tobytes() + np.ascontiguousarray(image).tobytes()
                 + (b"" if nimage is None else np.ascontiguousarray(nimage).tobytes()) + np.ascontiguousarray(qd).tobytes() + np.ascontiguousarray(qf).tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    assert len(raw) == n * (16 * 8 + 8 * 8 + 9 * 4)
    od = np.frombuffer(raw, np.float64, 16 * n, 0).reshape(n, 16)
    oi = np.frombuffer(raw, np.int64, 8 * n, 128 * n).reshape(n, 8)
    of = np.frombuffer(raw, np.float32, 9 * n, 192 * n).reshape(n, 9)
    return od, oi, of


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check(exe, tmp_path, K, M, ambient, image, nimage, W, at, t, bary32, uv, normals, tangents, flat):
    """the pixels ``at`` (raster order on a W-wide image) of triangles ``t`` -> the number of bad pixels"""
    py, px = np.divmod(at, W)
    c = uv.reshape(-1, 3, 2)[t]
    mapped = nimage is not None
    N = normals[3 * t] if mapped else flat
    T = tangents[3 * t] if mapped else np.zeros((at.shape[0], 4), np.float32)
    od, oi, of = run(exe, tmp_path, K, M, ambient, image, nimage, px, py, bary32, c, N, T)
    u, v, good = raster.texture_uv(bary32.astype(np.float64), c.astype(np.float64))
    assert np.array_equal(od[:, 0], good.astype(np.float64)) and same(od[:, 1], u) and same(od[:, 2], v)
    g = np.flatnonzero(good)
    value, taps = raster.fetch_texture(image, u[g], v[g])
    for k, (xi, yi, w) in enumerate(taps):
        assert np.array_equal(oi[g, k], xi) and np.array_equal(oi[g, 4 + k], yi) and same(od[g, 3 + k], w), k
    assert same(od[g, 7:10], value[:, :3])
    albedo = (value[:, :3] / 255.0).astype(np.float32)
    assert same(of[g, 0:3], albedo)
    if mapped:
        s = raster.fetch_texture(nimage, u[g], v[g])[0][:, :3]
        nrm, ok = raster.tangent_normal(s, N[g], T[g])
        assert same(od[g, 10:13], s) and np.array_equal(od[g, 15], ok.astype(np.float64))
    else:
        nrm = N[g]
    assert same(of[g, 3:6], nrm)
    Kd, Md = surface._pinhole(K, M)
    factor, cosine = raster.headlight(Kd, Md, px[g], py[g], nrm, float(np.float32(ambient)))
    assert same(od[g, 13], factor) and np.array_equal(od[g, 14], (cosine > 0.0).astype(np.float64))
    assert same(of[g, 6:9], (albedo.astype(np.float64) * factor[:, None]).astype(np.float32))
    assert not od[~good, 3:].any() and not of[~good].any()
    return int((~good).sum())


@pytest.mark.parametrize("texel,odd,normal_map,ambient", [(4, False, False, 0.25), (4, True, False, 0.0), (5, True, False, 1.0), (8, False, False, 0.25),
                                                          (4, True, True, 0.25), (5, False, True, 0.7)])
def test_the_scenes_of_the_twins_tests(program, tmp_path, texel, odd, normal_map, ambient):
    a, r = TU.asset(texel, odd, normal_map), TU.twin(texel, odd, normal_map)
    K, _, M, _ = TU.camera(a, 29, 37)
    face = r["face"].reshape(-1)
    at = np.flatnonzero(face >= 0)
    nrm, tan = (a["nrm"], a["tan"].copy()) if normal_map else (None, None)
    if normal_map:                                                              # one visible triangle with the degenerate mark
        t = int(np.bincount(face[at]).argmax())
        tan[3 * t:3 * t + 3] = (1.0, -0.0, 0.0, 1.0)
    bad = check(program, tmp_path, K, M, ambient, a["image"], a.get("nimage"), 37, at, face[at], r["bary"].reshape(-1, 3)[at], a["uv"], nrm, tan, r["nrm"][at])
    assert bad == 0 and at.shape[0] > 300


def test_the_edge_uvs(program, tmp_path):
    c, img = TU.edge_case(), TU.hand_image()
    face = c["face"].reshape(-1)
    at = np.flatnonzero((face >= 0) & (face < 4))
    flat = np.random.default_rng(1).normal(0.0, 1.0, (at.shape[0], 3)).astype(np.float32)
    flat[3] = 0.0                                                               # a normal without a length
    flat[4] = (np.inf, 0.0, 1.0)
    assert check(program, tmp_path, RU.HAND_K, RU.HAND_C2W, 0.25, img, None, at.shape[0], at, face[at], c["bary"].reshape(-1, 3)[at], c["uv"], None, None, flat) == 5
    # the same uvs on an image that is not square, with a map whose texels are arbitrary bytes and frames that are arbitrary floats
    rng = np.random.default_rng(4)
    img, nimg = rng.integers(0, 256, (5, 11, 4)).astype(np.uint8), rng.integers(0, 256, (5, 11, 4)).astype(np.uint8)
    nimg[0, 10, :3] = (128, 128, 128)                                           # decodes to a vector of length ~0.007, still usable; and an exact zero:
    N, T = rng.normal(0.0, 1.0, (12, 3)).astype(np.float32), rng.normal(0.0, 1.0, (12, 4)).astype(np.float32)
    T[3:6, :3] = N[3:6]                                                         # T parallel to N: m = x T + z N may vanish, B = 0
    assert check(program, tmp_path, RU.HAND_K, RU.HAND_C2W, 0.5, img, nimg, at.shape[0], at, face[at], c["bary"].reshape(-1, 3)[at], c["uv"], N, T, None) == 5
