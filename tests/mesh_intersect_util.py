"""Meshes for the self-intersection tests (host twin: mesh_io.mesh_intersections; device: csrc/mesh_intersect.hip) and the facts about them.  The
numbers in EXPECTED come from a separate numpy statement of the definition (orient as a plain determinant over all pairs), never from the code under
test; the hand cases are known from their construction."""
import functools
import importlib

import numpy as np

import mesh_audit_util as A

# name -> the facts that are asserted (a subset of the report)
EXPECTED = {
    "torus": {"candidates": 1081, "pairs": 0}, "fan40": {"pairs": 0}, "fan300": {"candidates": 135791, "pairs": 0},
    "sphere20": {"candidates": 22992, "pairs": 0}, "tetrahedron": {"pairs": 0}, "tetrahedron_one_reversed": {"pairs": 0}, "two_tetrahedra": {"pairs": 0},
    "grid_nt0": {"pairs": 0, "faces": 0}, "grid_nt1": {"pairs": 0}, "grid_nt255": {"pairs": 0}, "grid_nt256": {"pairs": 0}, "grid_nt257": {"pairs": 0},
    "defects": {"pairs": 0, "skipped": 2, "faces": 8},
    "two_spheres": {"faces": 9600, "candidates": 71744, "pairs": 367},
    "soup": {"faces": 120, "candidates": 4917, "pairs": 1791},
    "field": {"faces": 210, "pairs": 0},
    "field_filled": {"faces": 242, "pairs": 8},
    "hand_crossing": {"faces": 2, "candidates": 1, "pairs": 1},
    "hand_touching_vertex": {"faces": 2, "candidates": 1, "pairs": 0},
    "hand_coplanar": {"faces": 2, "candidates": 1, "pairs": 0},
    "hand_shared_index_crossing": {"faces": 2, "candidates": 1, "pairs": 1},
    "hand_shared_index_apart": {"faces": 2, "candidates": 1, "pairs": 0},
    "hand_shared_edge": {"faces": 2, "candidates": 0, "pairs": 0},
    "hand_repeated": {"faces": 1, "skipped": 1, "candidates": 0, "pairs": 0},
    "hand_zero_area": {"faces": 1, "skipped": 1, "candidates": 0, "pairs": 0},
}

_BASE = [[0.0, 0, 0], [2, 0, 0], [0, 2, 0]]


def hand_cases():
    """two triangles each; the first is the right triangle with legs of 2 in the plane z = 0"""
    through = [[0.5, 0.5, -1], [0.5, 0.5, 1]]                             # a segment through the first triangle's inside
    away = [[-1.0, 0, 1], [0, -1, 1]]
    two = np.array([[0, 1, 2], [3, 4, 5]])
    return {
        "hand_crossing": (_BASE + through + [[3.0, 3, 0]], two),
        "hand_touching_vertex": (_BASE + [[0.0, 0, 0]] + away, two),              # vertex 3 has the bits of vertex 0 and another index
        "hand_coplanar": (_BASE + [[0.5, 0.5, 0], [2.5, 0.5, 0], [0.5, 2.5, 0]], two),
        "hand_shared_index_crossing": (_BASE + through, np.array([[0, 1, 2], [0, 3, 4]])),
        "hand_shared_index_apart": (_BASE + away, np.array([[0, 1, 2], [0, 3, 4]])),
        "hand_shared_edge": (_BASE + [[1.0, 1, -1]], np.array([[0, 1, 2], [1, 0, 3]])),      # folded over the shared edge: the audit's business
        "hand_repeated": (_BASE + through + [[3.0, 3, 0]], np.array([[0, 1, 2], [3, 4, 4]])),
        "hand_zero_area": (_BASE + [[0.5, 0.5, -1], [0.5, 0.5, 0], [0.5, 0.5, 1]], two),       # three collinear corners, through the first triangle
    }


def two_spheres():
    v, f = A.meshes()["sphere20"]
    return np.concatenate([v, v + [0.5, 0.1, 0.05]]), np.concatenate([f, f + v.shape[0]])


def soup():
    return np.random.default_rng(1).random((360, 3)), np.arange(360).reshape(-1, 3)


def height_field():
    """a 13 x 13 height field with an L-shaped hole: no face crosses another; the centroid fan that fills the hole folds over itself"""
    i, j = np.meshgrid(np.arange(13), np.arange(13), indexing="ij")
    v = np.stack([i, j, 1.5 * np.sin(0.9 * i) * np.cos(0.7 * j)], -1).reshape(-1, 3).astype(np.float64)
    at = lambda a, b: a * 13 + b
    f = []
    for a in range(12):
        for b in range(12):
            if (2 <= a < 10 and 2 <= b < 5) or (2 <= a < 5 and 2 <= b < 10):
                continue
            f += [(at(a, b), at(a + 1, b), at(a + 1, b + 1)), (at(a, b), at(a + 1, b + 1), at(a, b + 1))]
    return v, np.array(f, np.int64)


def sphere_and_blade():
    """sphere20 plus one triangle far larger than a grid cell through its middle, as the LAST face: it is the larger index of every pair it is in"""
    v, f = A.meshes()["sphere20"]
    c = 0.5 * (v.min(0) + v.max(0))
    blade = c + np.array([[-40.0, -35, 0.3], [45, -30, 0.2], [1, 50, -0.4]])
    return np.concatenate([v, blade]), np.concatenate([f, [[v.shape[0], v.shape[0] + 1, v.shape[0] + 2]]])


@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (verts float64, faces int64): every mesh of the two suites; shared, so read-only by agreement"""
    mio = importlib.import_module("one-2-3-45_amd.mesh_io")
    out = {k: m for k, m in A.meshes().items()}
    out.update(hand_cases())
    out["two_spheres"], out["soup"], out["field"], out["blade"] = two_spheres(), soup(), height_field(), sphere_and_blade()
    out["field_filled"] = mio.fill_holes(*out["field"], 40)[:2]
    bv, bf = out["blade"]
    out["blade_first"] = (bv, np.concatenate([bf[-1:], bf[:-1]]))          # the blade as face 0: one row of the pair list holds every pair
    out = {k: (np.ascontiguousarray(v, np.float64).reshape(-1, 3), np.ascontiguousarray(f, np.int64).reshape(-1, 3)) for k, (v, f) in out.items()}
    return out


_twins = {}


def twin(name, v=None, f=None):
    """mesh_io.mesh_intersections(..., return_pairs=True) of a named mesh, computed once"""
    if name not in _twins:
        mio = importlib.import_module("one-2-3-45_amd.mesh_io")
        _twins[name] = mio.mesh_intersections(*(meshes()[name] if v is None else (v, f)), return_pairs=True)
    return _twins[name]


def assert_equal_reports(got, want):
    """every count equal; pairs and per-face hits equal to the byte"""
    assert set(got) == set(want), set(got) ^ set(want)
    for k, x in want.items():
        if isinstance(x, np.ndarray):
            assert got[k].dtype == x.dtype and got[k].shape == x.shape and got[k].tobytes() == x.tobytes(), k
        else:
            assert got[k] == x and type(got[k]) is type(x), (k, got[k], x)
