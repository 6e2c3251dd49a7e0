"""CPU: csrc/mesh_audit_math.h compiled for the host (tests/hostcheck/mesh_audit_check.hip, a stand-alone program) against the numpy twin in mesh_io:
normal, area, volume term, squared edge lengths, quality, histogram bin and the crease test equal to the bit.  This is the source the GPU executes; it
pins the shared arithmetic before any GPU time is spent."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import mesh_audit_util as U

mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program():
    exe = os.path.join(HERE, "hostcheck", "mesh_audit_check")
    src = os.path.join(HERE, "hostcheck", "mesh_audit_check.hip")
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
    nt, npairs = f.shape[0], pairs.shape[0]
    assert len(raw) == 8 * (11 * nt + nt + npairs)
    val = np.frombuffer(raw, np.float64, 11 * nt).reshape(nt, 11)
    rest = np.frombuffer(raw, np.int64, nt + npairs, 8 * 11 * nt)
    return val, rest[:nt], rest[nt:]


def extreme_mesh():
    """ordinary triangles of every shape next to ones whose arithmetic leaves the ordinary range: no area, a needle, coordinates whose products overflow
    (the quality is inf / inf: no bin), coordinates whose products underflow to zero (s == 0: quality 0)"""
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.normal(0.0, 2.0, (40, 3)), [[1.0, 1, 1], [2, 2, 2], [3, 3, 3]], [[0.0, 0, 0], [1, 0, 0], [0.5, 1e-9, 0]],
                        [[1e160, 0, 0], [0, 1e160, 0], [0, 0, 1e160]], [[0.0, 0, 0], [1e-170, 0, 0], [0, 1e-170, 0]]])
    f = np.concatenate([rng.integers(0, 40, (60, 3)), np.arange(40, 52).reshape(-1, 3)])
    return v, f.astype(np.int64)


def test_triangle_arithmetic_equals_the_twin(program, tmp_path):
    for v, f in (extreme_mesh(), U.meshes()["sphere20"], U.meshes()["fan300"], U.meshes()["tetrahedron"]):
        rng = np.random.default_rng(f.shape[0])
        pairs = rng.integers(0, f.shape[0], (200, 2))
        val, bins, creased = run(program, tmp_path, v, f, pairs)
        T = mesh_io.audit_triangles(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
        want = np.concatenate([T["n"], T["nn"][:, None], T["area"][:, None], T["vol"][:, None], T["l"], T["s"][:, None], T["q"][:, None]], 1)
        assert val.tobytes() == np.ascontiguousarray(want).tobytes()
        assert np.array_equal(bins, mesh_io.audit_bins(T["q"]))
        a, b = pairs[:, 0], pairs[:, 1]
        with np.errstate(invalid="ignore", over="ignore"):
            want_c = (T["nn"][a] > 0.0) & (T["nn"][b] > 0.0) & (mesh_io._dot3(T["n"][a], T["n"][b]) < 0.0)
        assert np.array_equal(creased, want_c.astype(np.int64))
    v, f = extreme_mesh()
    T = mesh_io.audit_triangles(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert mesh_io.audit_bins(T["q"])[-4:].tolist() == [0, 0, -1, 0] and T["nn"][-4] == 0.0 and T["s"][-1] == 0.0 and np.isnan(T["q"][-2])


def test_the_bins_of_the_definition():
    q = np.array([0.0, 0.0999999, 0.1, 0.95, 1.0, 1.0000000000000002, 7.0, np.inf, -0.0, -1e-300, np.nan])
    assert mesh_io.audit_bins(q).tolist() == [0, 0, 1, 9, 9, 9, 9, 9, 0, -1, -1]


def test_the_right_angle_is_not_creased(program, tmp_path):
    """the unit right tetrahedron: the three edges at the right-angled corner have n . n' == 0 exactly, the other three are acute"""
    v, f = U.meshes()["tetrahedron"]
    pairs = [(a, b) for a in range(4) for b in range(4) if a != b]
    _, _, creased = run(program, tmp_path, v, f, pairs)
    assert creased.tolist() == [int(3 in p) for p in pairs]
