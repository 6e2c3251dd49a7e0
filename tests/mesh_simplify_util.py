"""Meshes for the simplification tests (host twin: mesh_io.simplify_mesh; device: csrc/mesh_simplify.hip), and the checks both suites share."""
import functools

import numpy as np


def cube(g, offset=(0.0, 0.0, 0.0), sphere=False):
    """The welded surface of the cube [0, g]^3 with g x g quads per face, two triangles each, outward -> (verts float64 [6 g^2 + 2, 3], faces int64
    [12 g^2, 3]); ``sphere``: the vertices projected onto the sphere of radius g / 2 around the centre"""
    index, verts, faces = {}, [], []

    def vid(q):
        if q not in index:
            index[q] = len(verts)
            verts.append(q)
        return index[q]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, g):
            for i in range(g):
                for j in range(g):
                    def at(di, dj):
                        q = [0, 0, 0]
                        q[axis], q[u], q[w] = side, i + di, j + dj
                        return vid(tuple(q))
                    a, b, c, d = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
                    quad = [(a, b, c), (a, c, d)] if side else [(a, c, b), (a, d, c)]           # e_u x e_w = +e_axis: outward on the far side
                    faces += quad
    v = np.array(verts, np.float64)
    if sphere:
        d = v - g / 2.0
        v = d / np.linalg.norm(d, axis=1, keepdims=True) * (g / 2.0) + g / 2.0
    return v + np.asarray(offset, np.float64), np.array(faces, np.int64)


@functools.lru_cache(maxsize=None)
def cube10():
    """the welded 10 x 10 x 6 cube: 602 vertices, 1,200 faces, unit grid, at a non-integer offset"""
    v, f = cube(10, (0.37, -1.21, 2.93))
    v.setflags(write=False); f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def sphere20():
    """the cube-projected sphere: 2,402 vertices, 4,800 faces"""
    v, f = cube(20, (-3.3, 0.41, 1.7), sphere=True)
    v.setflags(write=False); f.setflags(write=False)
    return v, f


def corners(v, g=10):
    """indices of the 8 cube corners of cube(g, offset)"""
    lo, hi = v.min(0), v.max(0)
    at = (np.abs(v - lo) < 1e-9) | (np.abs(v - hi) < 1e-9)
    return np.flatnonzero(at.all(1))


def grid(nx, ny, z=0.25, jitter=None):
    """an open planar grid of nx x ny quads -> (verts, faces)"""
    x, y = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), indexing="ij")
    v = np.stack([x.reshape(-1) + 0.13, y.reshape(-1) - 0.71, np.full(x.size, z)], 1)
    if jitter is not None:
        v[:, 2] += jitter.uniform(-0.05, 0.05, v.shape[0])
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).reshape(-1)
    b, c, d = a + ny + 1, a + ny + 2, a + 1
    return v, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int64)


def fan(k, closed=True):
    """a double cone over a k-gon: the two apexes (vertices 0 and 1) have valence k -> (verts, faces): closed and manifold"""
    ang = 2 * np.pi * np.arange(k) / k
    ring = np.stack([3.0 * np.cos(ang) + 0.11, 3.0 * np.sin(ang) - 0.23, 0.05 * np.cos(3 * ang)], 1)
    v = np.concatenate([[[0.11, -0.23, 1.5], [0.11, -0.23, -1.5]], ring])
    i = np.arange(k)
    r0, r1 = 2 + i, 2 + (i + 1) % k
    f = np.concatenate([np.stack([np.zeros(k, np.int64), r0, r1], 1), np.stack([np.ones(k, np.int64), r1, r0], 1)])
    return v, f.astype(np.int64)


def edge_counts(f):
    """-> the number of faces on every undirected edge"""
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def signed_volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def check_outputs(v, f, out):
    """what every result must satisfy against its input, whatever produced it"""
    wv, wf, _, source, merged, info = out
    n = v.shape[0]
    assert wv.dtype == np.float64 and source.dtype == np.int32 and merged.dtype == np.int32 and wf.dtype == f.dtype
    assert wv.tobytes() == np.ascontiguousarray(v[source]).tobytes() and (np.diff(source) > 0).all()                  # bit copies, in the old order
    assert info["vertices"] == wv.shape[0] == source.size and info["triangles"] == wf.shape[0] and info["rounds"] == len(info["collapses"])
    assert wf.shape[0] == f.shape[0] - 2 * sum(info["collapses"])
    assert merged.shape == (n,) and merged.max(initial=-1) < source.size and np.array_equal(merged[source], np.arange(source.size))
    if wf.size:
        assert wf.min() >= 0 and wf.max() < source.size and np.array_equal(np.unique(wf), np.arange(source.size))   # kept iff referenced
