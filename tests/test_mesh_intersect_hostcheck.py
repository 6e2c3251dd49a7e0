"""CPU: csrc/mesh_intersect_math.h compiled for the host (tests/hostcheck/mesh_intersect_check.hip, a stand-alone program) against the numpy twin in
mesh_io: the orientation determinants equal to the bit, the crossing flags, the box overlap, the shared indices and the pair results equal.  This is
the source the GPU executes; it pins the shared arithmetic before any GPU time is spent."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import mesh_intersect_util as U

mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(HERE, "hostcheck", "mesh_intersect_check")
    src = os.path.join(HERE, "hostcheck", "mesh_intersect_check.hip")
    csrc = os.path.join(os.path.dirname(HERE), "one-2-3-45_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def run(exe, tmp_path, v, f, pairs):
    v, f, pairs = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64), np.ascontiguousarray(pairs, np.int64).reshape(-1, 2)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([v.shape[0], f.shape[0], pairs.shape[0]], np.int64).tobytes() + v.tobytes() + f.tobytes() + pairs.tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    n = pairs.shape[0]
    assert len(raw) == 8 * 15 * n
    return np.frombuffer(raw, np.float64, 6 * n).reshape(n, 6), np.frombuffer(raw, np.int64, 9 * n, 8 * 6 * n).reshape(n, 9)


def twin(v, f, pairs):
    """the same 6 + 9 columns from mesh_io"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    ft, fu = f[pairs[:, 0]], f[pairs[:, 1]]
    T, W = v[ft], v[fu]                                                    # [n,3,3]
    val = np.stack([mesh_io.intersect_orient(T[:, 0], T[:, 1], T[:, 2], W[:, k]) for k in range(3)]
                   + [mesh_io.intersect_orient(W[:, 0], W[:, 1], W[:, 2], T[:, k]) for k in range(3)], 1)
    flags = [mesh_io.segment_crosses_triangle(T[:, i], T[:, (i + 1) % 3], W[:, 0], W[:, 1], W[:, 2]) for i in range(3)]
    flags += [mesh_io.segment_crosses_triangle(W[:, i], W[:, (i + 1) % 3], T[:, 0], T[:, 1], T[:, 2]) for i in range(3)]
    flags.append(((T.min(1) <= W.max(1)) & (W.min(1) <= T.max(1))).all(1))
    flags.append((ft[:, :, None] == fu[:, None, :]).any(2).sum(1))
    flags.append(mesh_io.triangles_intersect(v, ft, fu))
    return val, np.stack([np.asarray(x).astype(np.int64) for x in flags], 1)


def extreme_mesh():
    """ordinary triangles next to ones whose arithmetic leaves the ordinary range: coordinates whose products overflow (inf, and inf - inf = NaN), ones
    whose products underflow to zero (a zero determinant: no crossing), and a needle"""
    rng = np.random.default_rng(3)
    big, tiny = 1e160, 1e-170
    v = np.concatenate([rng.normal(0.0, 2.0, (30, 3)),
                        [[big, 0, 0], [0, big, 0], [0, 0, big], [big, big, -big], [-big, big, big], [0.3 * big, 0.3 * big, 0.3 * big]],
                        [[tiny, 0, 0], [0, tiny, 0], [0, 0, tiny], [0.2 * tiny, 0.2 * tiny, -tiny], [0.2 * tiny, 0.2 * tiny, tiny], [tiny, tiny, 0]],
                        [[0.0, 0, 0], [1, 0, 0], [0.5, 1e-9, 0]]])
    f = np.concatenate([rng.integers(0, 30, (40, 3)), np.arange(30, 45).reshape(-1, 3)])
    return v, f.astype(np.int64)


def test_the_arithmetic_equals_the_twin(program, tmp_path):
    M = U.meshes()
    cases = [extreme_mesh(), M["soup"], M["field_filled"]] + [M[k] for k in sorted(M) if k.startswith("hand_")]
    for v, f in cases:
        nt = f.shape[0]
        pairs = np.stack(np.meshgrid(np.arange(nt), np.arange(nt), indexing="ij"), -1).reshape(-1, 2)
        if pairs.shape[0] > 20000:
            pairs = pairs[np.random.default_rng(nt).permutation(pairs.shape[0])[:20000]]
        val, flags = run(program, tmp_path, v, f, pairs)
        want_val, want_flags = twin(v, f, pairs)
        assert val.tobytes() == np.ascontiguousarray(want_val).tobytes()
        assert np.array_equal(flags, want_flags)
    # the extreme mesh does leave the ordinary range, and the soup does decide both ways
    v, f = extreme_mesh()
    val, flags = twin(v, f, [(a, b) for a in range(40, 45) for b in range(40, 45)])
    assert np.isnan(val).any() and np.isinf(val).any() and (val == 0.0).any()
    _, flags = twin(*M["soup"], [(a, b) for a in range(60) for b in range(60, 120)])
    assert 0 < flags[:, 8].sum() < flags.shape[0] and flags[:, :6].any(0).all()


def test_the_hand_cases(program, tmp_path):
    M = U.meshes()
    for name, want in U.EXPECTED.items():
        if not name.startswith("hand_") or want["faces"] != 2:
            continue
        _, flags = run(program, tmp_path, *M[name], [(0, 1)])
        assert flags[0, 6] == 1 and int(flags[0, 7] <= 1) == want["candidates"], name
        assert want["candidates"] == 0 or flags[0, 8] == want["pairs"], name
