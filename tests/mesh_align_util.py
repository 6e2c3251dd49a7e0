"""What the mesh alignment tests share (test_mesh_align.py, test_mesh_align_hostcheck.py, test_gpu_mesh_align.py): a 320-face blob without a rigid
symmetry, its two moved copies, and the host twin's runs on them, each computed once per process and never written to."""
import functools
import importlib

import numpy as np

mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")

SHIFT = (0.3, -0.2, 0.1)
MOVES = {"small": dict(angle=20.0, axis=(1.0, 2.0, 3.0), scale=1.15), "large": dict(angle=170.0, axis=(0.0, 0.0, 1.0), scale=0.8)}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def icosphere(subdivisions=2):
    """unit vertices and faces of an icosahedron subdivided ``subdivisions`` times: 162 vertices and 320 faces at 2"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.sqrt(1.0 + g * g) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.sqrt(p @ p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v), np.array(f, np.int64)


@functools.lru_cache(maxsize=None)
def blob():
    """-> (verts float64 [162,3], faces int64 [320,3]): unit vertex v goes to v r (1, 0.7, 0.45), r = 1 + 0.45 v_x + 0.35 v_y^2 + 0.3 v_x v_z + 0.6
    exp(-8 |v - (0.6, 0.64, 0.48)|^2): no rigid symmetry"""
    v, f = icosphere(2)
    bump = v - np.array([0.6, 0.64, 0.48])
    r = 1.0 + 0.45 * v[:, 0] + 0.35 * v[:, 1] ** 2 + 0.3 * v[:, 0] * v[:, 2] + 0.6 * np.exp(-8.0 * (bump * bump).sum(1))
    return _frozen(np.ascontiguousarray(v * r[:, None] * np.array([1.0, 0.7, 0.45])), f)


def diameter(verts=None):
    """the diagonal of the bounding box"""
    v = blob()[0] if verts is None else verts
    return float(np.sqrt(((v.max(0) - v.min(0)) ** 2).sum()))


@functools.lru_cache(maxsize=None)
def move(name):
    """-> the 4 x 4 similarity of MOVES[name]: the rotation about the axis through the origin, the scale, then SHIFT"""
    m = MOVES[name]
    axis = np.array(m["axis"]) / np.sqrt(np.dot(m["axis"], m["axis"]))
    T = np.eye(4)
    T[:3, :3] = m["scale"] * mesh_io.rodrigues(axis * np.deg2rad(m["angle"]))
    T[:3, 3] = SHIFT
    return _frozen(T)[0]


@functools.lru_cache(maxsize=None)
def moved(name):
    """-> the blob's vertices under move(name) (the same tessellation: mesh B of the tests; A is the blob)"""
    T = move(name)
    return _frozen(np.ascontiguousarray(blob()[0] @ T[:3, :3].T + T[:3, 3]))[0]


def worst_vertex(transform, name):
    """the largest distance of a vertex of A under ``transform`` from its true image, in diameters of B"""
    got = mesh_io.transform_vertices(blob()[0], transform)
    return float(np.sqrt(((got - moved(name)) ** 2).sum(1)).max()) / diameter(moved(name))


@functools.lru_cache(maxsize=None)
def twin_run(name, azimuths):
    """mesh_io.align_meshes of the blob onto moved(name): the identity alone (azimuths = 0) or that many azimuth candidates"""
    cand = mesh_io.rotation_candidates(azimuths) if azimuths else None
    return mesh_io.align_meshes(*blob(), moved(name), blob()[1], candidates=cand)
