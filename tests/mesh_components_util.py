"""Index meshes for the component tests (tests/test_mesh_components.py on the host, tests/test_gpu_mesh_components.py on the device): built once per
process and never modified."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def strip(n_quads=100_000, permuted=True):
    """A strip of n_quads quads = 2 n_quads triangles over 2 n_quads + 2 vertices (diameter ~ n_quads edges): ONE component.  ``permuted``: the vertex ids
    are shuffled with default_rng(1), so that neighbouring vertices have unrelated indices; otherwise natural order (the deepest parent chains).
    -> (faces int64 [2 n_quads, 3], n_vertices)"""
    i = np.arange(n_quads, dtype=np.int64)
    a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3
    f = np.empty((2 * n_quads, 3), np.int64)
    f[0::2] = np.stack([a, b, c], 1)
    f[1::2] = np.stack([b, d, c], 1)
    nv = 2 * n_quads + 2
    if permuted:
        f = np.random.default_rng(1).permutation(nv)[f]
    f.setflags(write=False)
    return f, nv


@functools.lru_cache(maxsize=None)
def fan(nt, extra=5):
    """nt triangles around vertex 3 (one component when nt > 0), with `extra` unreferenced vertices in front of, between and behind the referenced ones."""
    i = np.arange(nt, dtype=np.int64)
    f = np.stack([np.full(nt, 3, np.int64), 7 + i, 8 + i], 1)
    f.setflags(write=False)
    return f, 7 + nt + 1 + extra


@functools.lru_cache(maxsize=None)
def disjoint(nt):
    """nt triangles that share no vertex: nt components of one face; every fourth vertex slot is unreferenced, and the vertex order inside a triangle
    rotates (the label is the smallest index, not the first one)."""
    i = np.arange(nt, dtype=np.int64)
    base = 4 * i + 1
    f = np.stack([base + (i % 3), base + ((i + 1) % 3), base + ((i + 2) % 3)], 1)
    f.setflags(write=False)
    return f, 4 * nt + 2


@functools.lru_cache(maxsize=None)
def spheres_field(n=40):
    """float32 [n,n,n] on linspace(-1, 1, n)^3, negative inside: three spheres (one large, two equal small ones) plus a dozen one-node specks away from
    them -- marching cubes gives three closed surfaces and one 8-face octahedron per speck."""
    ax = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    u = np.full((n, n, n), np.inf)
    for (cx, cy, cz), r in (((-0.4, 0.0, 0.0), 0.45), ((0.5, 0.3, 0.0), 0.25), ((0.5, -0.45, 0.1), 0.25)):
        u = np.minimum(u, np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r)
    u = np.minimum(u, 0.5).astype(np.float32)
    rng = np.random.default_rng(5)
    placed = []
    while len(placed) < 12:
        p = tuple(int(t) for t in rng.integers(2, n - 2, 3))
        if u[p] < 0.2 or any(max(abs(p[k] - q[k]) for k in range(3)) < 3 for q in placed):      # clear of the spheres and of the other specks
            continue
        placed.append(p)
        u[p] = -0.3
    u.setflags(write=False)
    return u


def partition_equal(a, b):
    """Two labelings describe the same partition."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))
