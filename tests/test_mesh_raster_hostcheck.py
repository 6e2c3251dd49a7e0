"""CPU: csrc/mesh_raster_math.h compiled for the host (tests/hostcheck/mesh_raster_check.hip, a stand-alone program) against the numpy twin in raster.py:
the class, the snapped corners, the corner order, the pixel box and the corner depths of every face, and per (face, pixel) the three edge functions,
the coverage flag, z and the barycentrics, all equal to the bit.  This is the source the GPU executes; it pins the shared arithmetic before any GPU
time is spent."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import mesh_raster_util as U

raster = importlib.import_module("one-2-3-45_amd.raster")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(HERE, "hostcheck", "mesh_raster_check")
    src = os.path.join(HERE, "hostcheck", "mesh_raster_check.hip")
    csrc = os.path.join(os.path.dirname(HERE), "one-2-3-45_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def queries_of(setup, limit=64):
    """every pixel of the box of every face that takes part (at most ``limit`` per face, evenly spread) -> int64 [n,3] = (face, px, py)"""
    out = []
    for f in np.flatnonzero(setup["cls"] == 0):
        x0, y0, x1, y1 = (int(v) for v in setup["box"][f])
        py, px = (a.reshape(-1) for a in np.mgrid[y0:y1 + 1, x0:x1 + 1])
        keep = np.unique(np.linspace(0, px.shape[0] - 1, min(limit, px.shape[0])).astype(np.int64))
        out.append(np.stack([np.full(keep.shape[0], f), px[keep], py[keep]], 1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 3), np.int64)


def run(exe, tmp_path, s, cull, cam, queries):
    v, f = np.ascontiguousarray(s["verts"], np.float64), np.ascontiguousarray(s["tris"], np.int64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    camera = np.concatenate([cam["R"].reshape(-1), cam["t"], [cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["near"]]]).astype(np.float64)
    with open(src, "wb") as fh:
        fh.write(np.array([v.shape[0], f.shape[0], s["H"], s["W"], cull, queries.shape[0]], np.int64).tobytes() + camera.tobytes() + v.tobytes() + f.tobytes()
                 + np.ascontiguousarray(queries, np.int64).tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    nt, nq = f.shape[0], queries.shape[0]
    assert len(raw) == 8 * (17 * nt + 8 * nq)
    at, out = 0, []
    for dt, n, shape in ((np.int64, 14 * nt, (nt, 14)), (np.float64, 3 * nt, (nt, 3)), (np.int64, 4 * nq, (nq, 4)), (np.float64, 4 * nq, (nq, 4))):
        out.append(np.frombuffer(raw, dt, n, at).reshape(shape))
        at += 8 * n
    return out


def check(exe, tmp_path, s, cull):
    cam = raster.camera(s["K"], s["c2w"], s["near"], cull)
    S = raster.face_setup(s["verts"], s["tris"], cam, s["H"], s["W"])
    q = queries_of(S)
    fi, fz, qi, qz = run(exe, tmp_path, s, cull, cam, q)
    want = np.concatenate([S["cls"][:, None], S["sx"], S["sy"], S["corner"], S["box"]], 1)
    assert np.array_equal(fi, want), np.flatnonzero((fi != want).any(1))[:5]
    assert fz.tobytes() == np.ascontiguousarray(S["z"]).tobytes()
    for f in np.unique(q[:, 0]):
        rows = np.flatnonzero(q[:, 0] == f)
        w, covered, z, b = raster.pixel_terms(S, f, q[rows, 1], q[rows, 2])
        assert np.array_equal(qi[rows, :3], w) and np.array_equal(qi[rows, 3], covered.astype(np.int64)), f
        inside = rows[covered]
        assert qz[inside, 0].tobytes() == np.ascontiguousarray(z[covered]).tobytes() and qz[inside, 1:].tobytes() == np.ascontiguousarray(b[covered]).tobytes(), f
    return S, q, qi


def test_the_arithmetic_equals_the_twin(program, tmp_path):
    scenes = U.scenes()
    seen = set()
    for name, s in scenes.items():
        for cull in (0, 1, 2):
            S, q, qi = check(program, tmp_path, s, cull)
            seen |= set(S["cls"].tolist())
    assert seen == set(range(len(raster.CLASSES)))                             # every class occurs


def test_the_extreme_mesh(program, tmp_path):
    """under the hand camera, whose near plane and 2^21-pixel bound the mesh's corners sit on"""
    v, f = U.extreme_mesh()
    s = dict(verts=v, tris=f, K=U.HAND_K, c2w=U.HAND_C2W, H=16, W=16, near=0.125)
    S, q, qi = check(program, tmp_path, s, 0)
    nt = f.shape[0]
    cls = dict(zip(range(nt), S["cls"]))
    assert cls[nt - 3 - 3] in (raster.CLASSES.index("ok"), raster.CLASSES.index("offscreen"))                        # corners exactly at near: not dropped for it
    assert cls[nt - 3 - 2] not in (raster.CLASSES.index("range"), raster.CLASSES.index("near"))                      # exactly at 2^21 pixels: inside the bound
    assert int(np.abs(S["sx"][nt - 3 - 2]).max()) == 2 ** 29 and int(np.abs(S["sy"][nt - 3 - 2]).max()) == 2 ** 29
    assert cls[nt - 3 - 1] == raster.CLASSES.index("range")                                                          # one past it
    assert {raster.CLASSES.index(k) for k in ("near", "range", "ok")} <= set(S["cls"].tolist())
    assert qi[:, 3].any() and not qi[:, 3].all()
