"""CPU: csrc/mesh_raycast_math.h compiled for the host (tests/hostcheck/mesh_raycast_check.hip, a stand-alone program) against the numpy twin in
mesh_io: the hit parameters, the face normals, the frames and the ray ends equal to the bit, the hit flags and the nearest hits equal.  This is the
source the GPU executes; it pins the shared arithmetic before any GPU time is spent."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import mesh_raycast_util as R
from test_mesh_intersect_hostcheck import extreme_mesh

mio = importlib.import_module("one-2-3-45_amd.mesh_io")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(HERE, "hostcheck", "mesh_raycast_check")
    src = os.path.join(HERE, "hostcheck", "mesh_raycast_check.hip")
    csrc = os.path.join(os.path.dirname(HERE), "one-2-3-45_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def run(exe, tmp_path, v, f, P, Q, dirs, points, table, L, bias):
    c = lambda a, dt: np.ascontiguousarray(a, dt)
    v, f, P, Q, dirs, points, table = c(v, np.float64), c(f, np.int64), c(P, np.float64), c(Q, np.float64), c(dirs, np.float64), c(points, np.float64), c(table, np.float64)
    nt, ns, nd, S = f.shape[0], P.shape[0], dirs.shape[0], table.shape[0]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([v.shape[0], nt, ns, nd, S], np.int64).tobytes() + np.array([L, bias], np.float64).tobytes())
        for a in (v, f, P, Q, dirs, points, table):
            fh.write(a.tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    out, off = {}, 0
    for name, dt, shape in (("t", np.float64, (ns, nt)), ("hit", np.int64, (ns, nt)), ("best", np.float64, (ns,)), ("best_tri", np.int64, (ns,)),
                            ("normal", np.float64, (nt, 3)), ("frame", np.float64, (nd, 9)), ("ok", np.int64, (nd,)), ("rays", np.float64, (nd, S, 6))):
        n = int(np.prod(shape))
        out[name] = np.frombuffer(raw, dt, n, off).reshape(shape)
        off += 8 * n
    assert off == len(raw)
    return out


def twin(v, f, P, Q, dirs, points, table, L, bias):
    A, B, C = (v[f[:, k]][None] for k in range(3))
    Ps, Qs = P[:, None, :], Q[:, None, :]
    bc = lambda x: np.broadcast_to(x, (P.shape[0], f.shape[0], 3))
    sP, sQ = mio.intersect_orient(bc(A), bc(B), bc(C), bc(Ps)), mio.intersect_orient(bc(A), bc(B), bc(C), bc(Qs))
    with np.errstate(all="ignore"):
        t = sP / (sP - sQ)
        e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        normal = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    hit = mio.segment_crosses_triangle(bc(Ps), bc(Qs), bc(A), bc(B), bc(C))
    best, best_tri = mio.segment_hits(P, Q, v, f)
    T, Bf, N, ok = mio.ray_frame(dirs)
    rays = np.zeros((dirs.shape[0], table.shape[0], 6))
    p0, q = mio.occlusion_rays(points[ok], T[ok], Bf[ok], N[ok], table, L, bias)
    rays[ok] = np.concatenate([np.broadcast_to(p0[:, None, :], q.shape), q], 2)
    frame = np.where(ok[:, None], np.concatenate([T, Bf, N], 1), 0.0)
    return dict(t=t, hit=hit.astype(np.int64), best=best, best_tri=best_tri.astype(np.int64), normal=normal, frame=frame, ok=ok.astype(np.int64), rays=rays)


def directions(rng, n):
    d = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    special = [[0, 0, 1.0], [0, 0, -1.0], [0, 0, -0.0], [0, 0, 0.0], [1, 0, 0.0], [1, 0, -0.0], [1e-300, 0, -1e-300], [1e200, 1e200, 0], [np.nan, 0, 1], [np.inf, 0, 0],
               [1e-170, 1e-170, 1e-170], [3e-162, 0, 4e-162], [1e154, 1e154, 1e154]]
    return np.concatenate([d, special])


def assert_same(got, want):
    for k, x in want.items():
        x = np.ascontiguousarray(x)
        assert got[k].dtype == x.dtype and got[k].shape == x.shape, k
        if x.dtype == np.float64 and k == "frame":                      # NaN payloads of the refused frames are zeroed on both sides
            assert got[k].tobytes() == x.tobytes(), k
        elif x.dtype == np.float64:
            same = (got[k].view(np.int64) == x.view(np.int64)) | (np.isnan(got[k]) & np.isnan(x))       # a NaN is a NaN: its sign and payload are not defined
            assert same.all(), (k, np.argwhere(~same)[:5])
        else:
            assert np.array_equal(got[k], x), k


def test_the_arithmetic_equals_the_twin(program, tmp_path):
    rng = np.random.default_rng(11)
    table = mio.occlusion_directions(16)
    cases = []
    v, f = R.meshes()["soup"]
    P, Q = R.segments(v, [0.06, 4.0], n=300, seed=3)
    cases.append((v, f, P, Q, 2.0, 1e-3))
    v, f = R.cube()
    P, Q = R.segments(v, [0.25], n=200, seed=4)
    cases.append((v, f, P, Q, 0.5, 0.0))
    v, f = extreme_mesh()                                                  # coordinates whose products overflow or underflow, and a needle
    ends = np.concatenate([v[rng.integers(0, v.shape[0], (150, 2))], np.stack([rng.normal(0, 2, (100, 3)), rng.normal(0, 2, (100, 3))], 1)])
    ends[:100] = ends[:100] * rng.uniform(0.5, 1.5, (100, 2, 3))
    cases.append((v, f, ends[:, 0], ends[:, 1], 1e160, 1e-170))
    for v, f, P, Q, L, bias in cases:
        dirs = directions(rng, 200)
        points = rng.normal(size=dirs.shape) * np.abs(v).max()
        got = run(program, tmp_path, v, f, P, Q, dirs, points, table, L, bias)
        want = twin(v, f, P, Q, dirs, points, table, L, bias)
        assert_same(got, want)
    # the soup decides both ways, the extreme mesh leaves the ordinary range, and some frames are refused
    assert 0 < want["ok"].sum() < want["ok"].size and want["ok"][-13:].tolist() == [1, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0]
    assert np.isnan(want["t"]).any() and np.isinf(want["t"]).any() and np.abs(want["rays"]).max() > 1e159
    soup = twin(*cases[0][:4], directions(rng, 1), np.zeros((14, 3)), table, 1.0, 0.0)
    assert 0 < soup["hit"].sum() < soup["hit"].size and (soup["best_tri"] >= 0).sum() > 50 and (soup["best_tri"] < 0).sum() > 50
