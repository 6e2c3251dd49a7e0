"""CPU: csrc/mesh_normalmap_math.h compiled for the host (tests/hostcheck/mesh_normalmap_check.hip, a stand-alone program) against the numpy twin in
mesh_io: the tangent frame of a triangle and the normal-map texel equal to the bit, the degenerate and bad inputs included.  This is the source the GPU
executes; it pins the shared arithmetic before any GPU time is spent."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import mesh_normal_map_util as U

mio = importlib.import_module("one-2-3-45_amd.mesh_io")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(HERE, "hostcheck", "mesh_normalmap_check")
    src = os.path.join(HERE, "hostcheck", "mesh_normalmap_check.hip")
    csrc = os.path.join(os.path.dirname(HERE), "one-2-3-45_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def run(exe, tmp_path, pos, uv, grad, owner, rot):
    nt, ne = pos.shape[0] // 3, grad.shape[0]
    R = np.zeros(9, np.float32) if rot is None else np.ascontiguousarray(np.asarray(rot, np.float32).reshape(-1, 4, 4)[0, :3, :3]).reshape(9)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([nt, ne, rot is not None], np.int64).tobytes() + np.ascontiguousarray(pos, np.float32).tobytes() + np.ascontiguousarray(uv, np.float32).tobytes()
                 + np.ascontiguousarray(grad, np.float32).tobytes() + R.tobytes() + np.ascontiguousarray(owner, np.int64).tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    assert len(raw) == 12 * nt + 16 * nt + 8 * nt + 4 * ne + 8 * ne
    N = np.frombuffer(raw, np.float32, 3 * nt).reshape(nt, 3)
    TW = np.frombuffer(raw, np.float32, 4 * nt, 12 * nt).reshape(nt, 4)
    ok = np.frombuffer(raw, np.int64, nt, 28 * nt)
    rgba = np.frombuffer(raw, np.uint8, 4 * ne, 36 * nt).reshape(ne, 4)
    flags = np.frombuffer(raw, np.int64, ne, 36 * nt + 4 * ne)
    return N, TW, ok, rgba, flags


def check(program, tmp_path, pos, uv, grad, nt, c, rot):
    own = U.owners(nt, c)
    N, TW, ok, rgba, flags = run(program, tmp_path, pos, uv, grad, own, rot)
    tN, tTW, degenerate = mio.texture_frames(pos, uv)
    image, counts = mio.pack_normal_map(grad, tN, tTW, nt, c, rot)
    assert N.tobytes() == tN[0::3].tobytes() and TW.tobytes() == tTW[0::3].tobytes()          # bytes: the sign of the marking zero included
    assert int((ok == 0).sum()) == degenerate
    assert rgba.tobytes() == np.ascontiguousarray(U.to_cells(image, nt, c)[0]).tobytes()
    assert int((flags & 1).sum()) == counts["bad_gradient"] and int(((flags & 2) != 0).sum()) == counts["back_facing"]
    return degenerate, counts


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("nt, c", [(1, 4), (2, 5), (3, 4), (33, 5), (86, 4), (171, 4)])
def test_strips_with_degenerate_and_bad_inputs_equal_the_twin(program, tmp_path, nt, c, rot):
    case = U.strip(nt, c, seed=nt * 100 + c, rot=U.rotation() if rot else None)
    degenerate, counts = check(program, tmp_path, case["pos"], case["uv"], case["grad"], nt, c, case["rot"])
    assert degenerate == len(case["degenerate"]) and counts["bad_gradient"] == len(case["bad"]) and counts["back_facing"] >= len(case["back"])


@pytest.mark.parametrize("rot", [False, True])
def test_the_ellipsoid_equals_the_twin(program, tmp_path, rot):
    v, f, grad_at = U.ellipsoid(24)
    T = U.rotation() if rot else None
    for c in (4, 5):
        pos, uv, _, _ = mio.texture_corners(v, f, c, 24, trans_mat=T)
        grad = grad_at(mio.texture_points(v, f, c, 24)[1])
        assert check(program, tmp_path, pos, uv, grad, f.shape[0], c, T) == (0, {"bad_gradient": 0, "back_facing": 0})


def test_extreme_frames_equal_the_twin(program, tmp_path):
    """no area, one uv for three corners, NaN and infinite coordinates, coordinates at both ends of the float32 range, a needle; and a rotation that is
    singular, so that the second normalisation is the one that fails"""
    c, nt = 4, 8
    uv = mio.texture_corners(np.zeros((3, 3)), np.tile(np.arange(3), (nt, 1)), c, 8)[1].copy()
    pos = np.tile(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), (nt, 1))
    pos[3:6] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]
    uv[6:9] = uv[6]
    pos[9] = np.nan
    pos[13, 0] = np.inf
    pos[15:18] *= np.float32(3e38)
    pos[18:21] *= np.float32(1e-38)
    pos[21:24] = [[0, 0, 0], [1, 0, 0], [0.5, 1e-7, 0]]
    grad = np.random.default_rng(5).normal(0, 1, (mio.texture_layout(nt, c)["texels"], 3)).astype(np.float32)
    degenerate, _ = check(program, tmp_path, pos, uv, grad, nt, c, None)
    assert degenerate == 4
    singular = np.zeros((4, 4), np.float32)
    singular[0, 0] = singular[3, 3] = 1.0
    grad[7] = [0.0, 2.0, 1.0]                                                 # through diag(1, 0, 0): nothing is left of it
    _, counts = check(program, tmp_path, pos, uv, grad, nt, c, singular)
    assert counts["bad_gradient"] == 1
