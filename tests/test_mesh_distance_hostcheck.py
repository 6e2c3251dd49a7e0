"""CPU: csrc/mesh_distance_math.h compiled for the host (tests/hostcheck/mesh_distance_check.hip) against the numpy twin in mesh_io: levels, sample points,
weights, d2, nearest and region equal to the bit.  This is the source the GPU executes; it pins the shared math before any GPU time is spent."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import mesh_distance_util as U

mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hc():
    so = os.path.join(HERE, "hostcheck", "libmesh_distance_check.so")
    src = os.path.join(HERE, "hostcheck", "mesh_distance_check.hip")
    csrc = os.path.join(os.path.dirname(HERE), "one-2-3-45_amd", "csrc")
    newest = max([os.path.getmtime(src)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                               "-fPIC", "-shared", src, "-o", so], stderr=subprocess.DEVNULL)
    L = ctypes.CDLL(so)
    L.mdc_samples.restype = ctypes.c_longlong
    L.mdc_levels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p]
    L.mdc_samples.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mdc_closest.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mdc_cell_index.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    return L


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def hand_mesh():
    """one triangle that hits the k = 64 cap at spacing 0.2, one without an area, one with a repeated index, and a few ordinary ones"""
    v = np.array([[0.0, 0, 0], [40, 0, 0], [0, 30, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [0.3, 0.1, 0.7], [1.1, 0.2, 0.9], [0.4, 1.3, 0.2]])
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 6, 7], [6, 7, 8], [8, 7, 6]], np.int64)
    return v, f


@pytest.mark.parametrize("spacing", [None, 0.75, 0.2])
def test_levels_and_samples_equal_the_twin(hc, spacing):
    (va, fa), _ = U.spheres()
    for v, f in ((va, fa), hand_mesh()):
        v, f = np.ascontiguousarray(v), np.ascontiguousarray(f)
        k = np.zeros(len(f), np.int32)
        hc.mdc_levels(P(v), P(f), len(f), 0.0 if spacing is None else spacing, P(k))
        assert np.array_equal(k, mesh_io.sample_levels(v, f, spacing))
        pts, w, tri = mesh_io.surface_samples(v, f, spacing)
        got_p, got_w = np.zeros_like(pts), np.zeros_like(w)
        assert hc.mdc_samples(P(v), P(f), len(f), P(k), P(got_p), P(got_w)) == len(w)
        assert bits(got_p, pts) and bits(got_w, w)
    if spacing == 0.2:
        assert k.tolist() == [64, 18, 5, 8, 8]


def test_closest_triangle_equals_the_twin_on_every_query_set(hc):
    _, (vb, fb) = U.spheres()
    q = U.all_queries()
    d2, nearest, region, _ = U.twin_answers()
    got_d2, got_n, got_r = np.zeros(len(q)), np.zeros(len(q), np.int32), np.zeros(len(q), np.uint8)
    hc.mdc_closest(P(q), len(q), P(vb), P(fb), len(fb), P(got_d2), P(got_n), P(got_r))
    assert bits(got_d2, d2) and bits(got_n, nearest) and bits(got_r, region)


def test_degenerate_targets_and_the_cell_index(hc):
    v, f = hand_mesh()
    q = np.ascontiguousarray(np.random.default_rng(0).uniform(-5, 45, (300, 3)))
    d2, nearest, region, _, deg = mesh_io.closest_triangles(q, v, f)
    got_d2, got_n, got_r = np.zeros(len(q)), np.zeros(len(q), np.int32), np.zeros(len(q), np.uint8)
    hc.mdc_closest(P(q), len(q), P(v), P(f), len(f), P(got_d2), P(got_n), P(got_r))
    assert deg == 2 and bits(got_d2, d2) and bits(got_n, nearest) and bits(got_r, region) and set(nearest.tolist()) <= {0, 3, 4}
    # one monotone function places triangles and queries: clamped at both ends, a border coordinate belongs to the upper cell, a NaN to cell 0
    idx = [hc.mdc_cell_index(x, 3.0, 1.0, 8) for x in (-1e300, 2.9, 3.0, 3.999999, 4.0, 10.0, 10.999, 11.0, 1e300, float("nan"))]
    assert idx == [0, 0, 0, 0, 1, 7, 7, 7, 7, 0]
    xs = np.sort(np.random.default_rng(1).uniform(-3, 9, 2000))
    cells = [hc.mdc_cell_index(float(x), -1.11, 0.37, 20) for x in xs]
    assert cells == sorted(cells) and cells[0] == 0 and cells[-1] == 19
