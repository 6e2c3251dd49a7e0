"""Meshes and fields for the adjacency / smoothing tests (tests/test_mesh_smooth.py on the host, tests/test_gpu_mesh_smooth.py on the device): built once
per process and never modified."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def grid_patch(n=20):
    """n x n vertices on the unit lattice, every cell split along the same diagonal: 2 (n - 1)^2 triangles, an open patch with 4 n - 4 boundary vertices
    and interior valence 6.  -> (verts float64 [n*n, 3] with z = 0, faces int64, boundary mask bool [n*n])"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i.ravel(), j.ravel(), np.zeros(n * n)], 1).astype(np.float64)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).ravel().astype(np.int64)
    f = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)])
    rim = ((i == 0) | (j == 0) | (i == n - 1) | (j == n - 1)).ravel()
    for x in (v, f, rim):
        x.setflags(write=False)
    return v, f, rim


@functools.lru_cache(maxsize=None)
def icosphere(subdivisions=4):
    """Unit icosphere: 10 * 4^s + 2 vertices (2,562 at s = 4), closed.  -> (verts float64 [N,3], faces int64 [M,3])"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def noisy_icosphere():
    """icosphere(4) with every radius scaled by 1 + 0.02 N(0, 1), seed 7"""
    v, f = icosphere(4)
    out = v * (1.0 + 0.02 * np.random.default_rng(7).standard_normal(v.shape[0]))[:, None]
    out.setflags(write=False)
    return out, f


@functools.lru_cache(maxsize=None)
def bipyramid(nt):
    """A ring of nt vertices (2 .. nt + 1) joined to two apices (0 and 1): 2 nt triangles, closed (every edge has two triangles), both apex rows have nt
    neighbours.  nt = 1, 2 give degenerate but legal index meshes (a triangle with two equal corners contributes two of its six pairs twice)."""
    i = np.arange(nt, dtype=np.int64)
    r0, r1 = 2 + i, 2 + (i + 1) % max(nt, 1)
    f = np.concatenate([np.stack([np.zeros(nt, np.int64), r0, r1], 1), np.stack([np.ones(nt, np.int64), r1, r0], 1)])
    f.setflags(write=False)
    return f, nt + 2


@functools.lru_cache(maxsize=None)
def cut_sphere_field(n=24):
    """float32 [n,n,n] on linspace(-1, 1, n)^3, negative inside a sphere of radius 0.4 centred at x = 0.9: the volume's face x = n - 1 cuts it open, so
    marching cubes gives a surface whose rim lies on that plane."""
    ax = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    u = (np.sqrt((x - 0.9) ** 2 + y ** 2 + z ** 2) - 0.4).astype(np.float32)
    u.setflags(write=False)
    return u


def radial(v):
    r = np.linalg.norm(np.asarray(v, np.float64), axis=1)
    return float(r.mean()), float(r.std())
