"""GPU: csrc/mesh_align.hip against its host twin (mesh_io.align_terms / align_meshes) -- moved points, d2 and nearest to the bit (and equal to the distance
query's), the counts exactly, every sum to 1e-12 of the sum of the terms' magnitudes -- at the seams of the kernel's tiling, plus guard bands around
every buffer, the twin's trajectories, ops.mesh_align end to end and the distance report with and without an alignment."""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import mesh_align_util as A
import mesh_distance_util as U
from guard_util import Guard
from mesh_scene_util import dev, ops, pipeline          # noqa: F401  (dev is a fixture)

mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
_lib = importlib.import_module("one-2-3-45_amd._lib")
pytestmark = pytest.mark.gpu

TAU = 0.12          # rejects a part of the samples under the transforms below, keeps the rest


def up(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a)).to(dev)
    return (t if dtype is None else t.to(dtype)).contiguous()


def same(t, a):
    """device tensor == host array, bit for bit"""
    h = t.cpu().numpy()
    return h.dtype == a.dtype and h.shape == a.shape and h.tobytes() == np.ascontiguousarray(a).tobytes()


@functools.lru_cache(maxsize=None)
def cloud():
    """4,097 weighted samples of the blob (the first n of them are the points of a test), and three transforms near the small move: the move itself, the
    start that moment matching gives, and one a few degrees off"""
    v, f = A.blob()
    pts, w, _ = mesh_io.surface_samples(v, f, 0.04)
    assert len(w) >= 4097
    pick = np.random.default_rng(3).permutation(len(w))[:4097]
    w = w[pick].copy()
    w[::17] = 0.0
    T = A.move("small")[:3]
    off = np.concatenate([1.1 * mesh_io.rodrigues([0.05, -0.08, 0.3]) @ T[:, :3], T[:, 3:] + 0.05], 1)
    start = mesh_io.align_meshes(v, f, A.moved("small"), f, iterations=0)["transform"][:3]
    pts, Ts = np.ascontiguousarray(pts[pick]), np.ascontiguousarray(np.stack([off, T, start]).reshape(3, 12))
    for a in (pts, w, Ts):
        a.setflags(write=False)
    return pts, w, Ts


def targets():
    v, f = A.moved("small"), A.blob()[1]
    degenerate = np.array([[0, 0, 1], [5, 5, 5], [2, 1, 2]])
    return {"blob": (v, f), "blob+degenerate": (v, np.concatenate([degenerate, f[:100], degenerate, f[100:]])), "all degenerate": (v, np.tile(degenerate, (30, 1)))}


def check_rows(rows, terms, what=""):
    """every sum column within 1e-12 of sum |term| of math.fsum of the twin's terms; the counts exact; the last two zero"""
    rows = rows.cpu().numpy() if torch.is_tensor(rows) else rows
    assert rows.shape == terms.shape[::2]
    for k in range(rows.shape[0]):
        for col in range(43):
            ref, mag = math.fsum(terms[k, :, col]), math.fsum(np.abs(terms[k, :, col]))
            assert abs(rows[k, col] - ref) <= 1e-12 * mag, (what, k, col, rows[k, col], ref, mag)
        assert [rows[k, c] for c in (43, 44, 45)] == [terms[k, :, c].sum() for c in (43, 44, 45)] and (rows[k, 46:] == 0).all(), (what, k, rows[k, 43:])


# ---- the step against the twin -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 256, 257, 4096, 4097])
def test_step_equals_the_twin_at_the_tile_edges(dev, n, K):
    """a block's edge (256 threads of 16 samples: n = 4,096 fills one block, 4,097 starts a second row of partials), a thread's edge (n = 256, 257: sixteen
    full threads and one sample more), one sample; grid, exhaustive and no target; weights given and not; no truncation and one that rejects; both
    index widths"""
    pts, w, Ts = cloud()
    pts, w, Ts = pts[:n], w[:n], Ts[:K]
    v, f = targets()["blob"]
    c = v.mean(0)
    tp, tw, tT, tv = up(pts, dev), up(w, dev), up(Ts, dev), up(v, dev)
    grid = ops.mesh_distance_grid(tv, up(f, dev))
    seen = {}
    combos = (("grid", True, None, torch.int32), ("all", False, TAU, torch.int64), ("none", True, None, None), ("grid", False, TAU, torch.int64),
              ("all", True, None, torch.int32), ("none", False, TAU, None))
    for mode, weights, tau, dtype in combos[:3 if n >= 4096 else 6]:          # the twin is brute force: the large sizes take each mode once
        want = mesh_io.align_terms(pts, w if weights else None, Ts, *((v, f) if mode != "none" else (None, None)), tau, c)
        target = None if mode == "none" else (tv, up(f, dev, dtype))
        runs = [ops.mesh_align_step(tp, tw if weights else None, tT, target, grid if mode == "grid" else None, tau, c, want=("moved", "d2", "nearest"))
                for _ in range(2)]
        rows, extra = runs[0]
        assert rows.cpu().numpy().tobytes() == runs[1][0].cpu().numpy().tobytes()                      # the same bytes on every run
        assert same(extra["moved"], want["moved"]) and same(extra["d2"], want["d2"]) and same(extra["nearest"], want["nearest"]), (mode, weights, tau)
        check_rows(rows, want["terms"], (mode, weights, tau))
        if mode != "none":
            q = ops.mesh_closest_triangle(extra["moved"].view(-1, 3), *target, grid if mode == "grid" else None)          # the distance query's own bits
            assert torch.equal(q[0].view(torch.int64), extra["d2"].view(-1).view(torch.int64)) and torch.equal(q[1], extra["nearest"].view(-1))
        bare = ops.mesh_align_step(tp, tw if weights else None, tT, target, grid if mode == "grid" else None, tau, c)          # without the optional outputs
        assert bare[1] == {} and bare[0].cpu().numpy().tobytes() == rows.cpu().numpy().tobytes()
        seen[(mode, weights, tau)] = rows.cpu().numpy()
        if tau and mode != "none" and n >= 256:
            assert seen[(mode, weights, tau)][0, 44] > 0 and seen[(mode, weights, tau)][0, 43] > 0      # the first transform: some rejected, some kept
    assert (seen[("none", True, None)][:, :35] == 0).all() and (seen[("none", True, None)][:, 36] == 0).all()


def test_grid_and_exhaustive_rows_are_the_same_bytes_and_degenerate_triangles_take_no_part(dev):
    pts, w, Ts = cloud()
    pts, w = pts[:700], w[:700]
    tp, tw, tT = up(pts, dev), up(w, dev), up(Ts, dev)
    v, f = targets()["blob+degenerate"]
    tv, tf = up(v, dev), up(f, dev)
    grid = ops.mesh_distance_grid(tv, tf, 0.2)
    assert grid.degenerate == 6
    want = mesh_io.align_terms(pts, w, Ts, v, f, TAU, (0.1, 0.2, 0.3))
    got = [ops.mesh_align_step(tp, tw, tT, (tv, tf), g, TAU, (0.1, 0.2, 0.3), want=("d2", "nearest")) for g in (grid, None)]
    assert got[0][0].cpu().numpy().tobytes() == got[1][0].cpu().numpy().tobytes()
    for rows, extra in got:
        assert same(extra["d2"], want["d2"]) and same(extra["nearest"], want["nearest"])
        check_rows(rows, want["terms"])
    assert not np.isin(want["nearest"], [0, 1, 2, 103, 104, 105]).any() and (want["nearest"] > 105).any()
    # a target of degenerate triangles alone: every pair is unmatched, nothing is summed
    v, f = targets()["all degenerate"]
    rows, extra = ops.mesh_align_step(tp, tw, tT, (up(v, dev), up(f, dev)), None, None, (0.0, 0.0, 0.0), want=("d2", "nearest"))
    rows = rows.cpu().numpy()
    assert (rows[:, :45] == 0).all() and (rows[:, 45] == 700).all() and bool(torch.isinf(extra["d2"]).all()) and bool((extra["nearest"] == -1).all())
    check_rows(rows, mesh_io.align_terms(pts, w, Ts, v, f)["terms"])


def test_bad_target_input_is_skipped_as_the_query_skips_it(dev):
    """an index out of range and a non-finite coordinate (the twin refuses both; the exhaustive query leaves such triangles out): d2 and nearest are the
    query's, and what is left of the target gives the rows of the clean target"""
    pts, w, Ts = cloud()
    pts, w, Ts = pts[:300], w[:300], Ts[:2]
    v, f = targets()["blob"]
    v2 = np.concatenate([v, [[np.nan, 0.0, 0.0]]])
    f2 = np.concatenate([f, [[0, 1, len(v2)], [-1, 2, 3], [0, 1, len(v)]]])             # behind the good ones: their indices stay
    tp, tw, tT = up(pts, dev), up(w, dev), up(Ts, dev)
    rows, extra = ops.mesh_align_step(tp, tw, tT, (up(v2, dev), up(f2, dev)), None, None, (0.0, 0.0, 0.0), want=("moved", "d2", "nearest"))
    q = ops.mesh_closest_triangle(extra["moved"].view(-1, 3), up(v2, dev), up(f2, dev))
    assert torch.equal(q[0].view(torch.int64), extra["d2"].view(-1).view(torch.int64)) and torch.equal(q[1], extra["nearest"].view(-1))
    clean = ops.mesh_align_step(tp, tw, tT, (up(v, dev), up(f, dev)), None, None, (0.0, 0.0, 0.0))[0]
    assert rows.cpu().numpy().tobytes() == clean.cpu().numpy().tobytes() and int(extra["nearest"].max()) < len(f)


def test_refusals(dev):
    pts, w, Ts = cloud()
    tp, tT = up(pts[:10], dev), up(Ts, dev)
    bad = Ts.copy()
    bad[1, 7] = np.inf
    with pytest.raises(RuntimeError, match="transform 1 has a non-finite entry"):
        ops.mesh_align_step(tp, None, up(bad, dev))
    with pytest.raises(ValueError, match="transforms"):
        ops.mesh_align_step(tp, None, up(np.tile(Ts[:1], (65, 1)), dev))
    with pytest.raises(ValueError, match="max_distance"):
        ops.mesh_align_step(tp, None, tT, max_distance=-1.0)
    with pytest.raises(RuntimeError, match="n < 2\\^28"):
        _lib.call("o2345_mesh_align_step", tp, None, 2 ** 28, tT, 3, None, None, 4, 0, 0, None, 0, 0, 0.0, 0.0, 0.0, 0.0, tp, 4096, tp, None, None, None)
    with pytest.raises(RuntimeError, match="pivot"):
        ops.mesh_align_step(tp, None, tT, pivot=(0.0, float("nan"), 0.0))
    v, f = A.blob()
    with pytest.raises(ValueError, match="iterations"):
        ops.mesh_align(up(v, dev), up(f, dev), up(v, dev), up(f, dev), iterations=-1)


def test_transform_equals_the_twin(dev):
    v = A.blob()[0]
    for name in ("small", "large"):
        assert same(ops.mesh_transform(up(v, dev), A.move(name)), mesh_io.transform_vertices(v, A.move(name)))
    assert same(ops.mesh_transform(up(v, dev), np.eye(3, 4)), v)


# ---- guard bands -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, K, ib, np_idx, outputs", [(4097, 3, 4, np.int32, True), (257, 1, 8, np.int64, False), (4096, 2, 8, np.int64, True)])
def test_the_step_stays_inside_its_buffers(dev, n, K, ib, np_idx, outputs):
    L = _lib.lib()
    pts, w, Ts = cloud()
    v, f = targets()["blob+degenerate"]
    G = Guard(dev)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gp, gw, gT = G.buf(np.ascontiguousarray(pts[:n]), "points"), G.buf(np.ascontiguousarray(w[:n]), "weights"), G.buf(np.ascontiguousarray(Ts[:K]), "transforms")
    gv, gf = G.buf(np.ascontiguousarray(v), "verts"), G.buf(f.astype(np_idx), "tris")
    nv, nt, max_cells = len(v), len(f), 4096
    gwb = L.o2345_mesh_distance_grid_workspace_bytes(nt, max_cells)
    gws = G.buf(gwb, "grid workspace")
    ne = ctypes.c_longlong()
    _lib.check(L.o2345_mesh_distance_grid_count(P(gv), P(gf), ib, nv, nt, 0.0, max_cells, P(gws), gwb, ctypes.byref(ne), None, None, None, stream), "grid count")
    gb = L.o2345_mesh_distance_grid_bytes(max_cells, ne.value)
    grid = G.buf(gb, "grid")
    _lib.check(L.o2345_mesh_distance_grid_emit(P(gv), P(gf), ib, nv, nt, max_cells, P(gws), ne.value, P(grid), gb, stream), "grid emit")
    wsb = L.o2345_mesh_align_workspace_bytes(n, K)
    assert wsb == 384 * K * -(-n // 4096)
    ws = G.buf(wsb, "workspace")
    results = []
    for g, gbytes, cells, tris in ((grid, gb, max_cells, gf), (None, 0, 0, gf), (None, 0, 0, None)):
        moments = G.buf(8 * 48 * K, "moments")                        # the row at its exact size
        moved, d2, nearest = (G.buf(24 * K * n, "moved"), G.buf(8 * K * n, "d2"), G.buf(4 * K * n, "nearest")) if outputs else (None, None, None)
        _lib.check(L.o2345_mesh_align_step(P(gp), P(gw), n, P(gT), K, P(gv), P(tris), ib, nv, nt, P(g), gbytes, cells, TAU, 0.1, 0.2, 0.3, P(ws), wsb, P(moments),
                                           P(moved), P(d2), P(nearest), stream), "step")
        results.append((moments.cpu().numpy().view(np.float64).reshape(K, 48), d2, nearest))
    assert G.damaged() == []
    assert results[0][0].tobytes() == results[1][0].tobytes() and (results[0][0][:, 43] > 0).all() and (results[2][0][:, 43] == n).all()
    if outputs:
        assert torch.equal(results[0][1], results[1][1]) and torch.equal(results[0][2], results[1][2])
    check_rows(results[0][0], mesh_io.align_terms(pts[:n], w[:n], Ts[:K], v, f, TAU, (0.1, 0.2, 0.3))["terms"])


# ---- the twin's trajectories ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, azimuths", [("small", 0), ("large", 8)])
def test_every_transform_of_the_twins_history(dev, name, azimuths):
    """all transforms of the kept candidate's history as the K transforms of ONE step: each row meets the bound, and the inlier counts are the twin's"""
    v, f = A.blob()
    b = A.moved(name)
    run = A.twin_run(name, azimuths)
    Ts = np.ascontiguousarray(np.stack([h["transform"] for h in run["history"]]).reshape(-1, 12))
    assert 2 <= len(Ts) <= 64
    pts, w, _ = mesh_io.surface_samples(v, f)
    tv, tf = up(b, dev), up(f, dev)
    rows = ops.mesh_align_step(up(pts, dev), up(w, dev), up(Ts, dev), (tv, tf), ops.mesh_distance_grid(tv, tf), None, run["pivot"])[0].cpu().numpy()
    check_rows(rows, mesh_io.align_terms(pts, w, Ts, b, f, None, run["pivot"])["terms"], name)
    assert [int(r[43]) for r in rows] == [h["inliers"] for h in run["history"]] and [int(r[45]) for r in rows] == [h["unmatched"] for h in run["history"]]
    for r, h in zip(rows, run["history"]):
        assert abs(r[38] / r[37] - h["score"]) <= 4e-12 * h["score"] + 1e-300


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, azimuths", [("small", 0), ("large", 8)])
def test_mesh_align_end_to_end(dev, name, azimuths):
    v, f = A.blob()
    twin = A.twin_run(name, azimuths)
    cand = mesh_io.rotation_candidates(azimuths) if azimuths else None
    got = ops.mesh_align(up(v, dev), up(f, dev, torch.int32), up(A.moved(name), dev), up(f, dev), candidates=cand)
    print(name, "device: iterations", got["iterations"], "worst vertex", A.worst_vertex(got["transform"], name), "twin: iterations", twin["iterations"])
    assert set(got) == set(twin) and got["candidate"] == twin["candidate"] == (4 if azimuths else 0) and got["converged"]
    assert A.worst_vertex(got["transform"], name) <= 1e-9
    assert len(got["candidate_scores"]) == max(1, azimuths) and got["inlier_fraction"] == 1.0
    via_pipeline = pipeline.mesh_align((v, f), (up(A.moved(name), dev), f), candidates=cand)          # host arrays and device tensors mixed
    assert np.array_equal(via_pipeline["transform"], got["transform"]) and via_pipeline["iterations"] == got["iterations"]


def test_distance_with_and_without_alignment(dev):
    v, f = A.blob()
    b = A.moved("large")
    a_mesh, b_mesh = (up(v, dev), up(f, dev)), (up(b, dev), up(f, dev))
    plain = pipeline.mesh_distance(a_mesh, b_mesh, thresholds=(0.01,))
    assert set(plain) == {"a_to_b", "b_to_a", "chamfer", "hausdorff", "thresholds", "precision", "recall", "fscore", "degenerate_targets"}
    assert plain == pipeline.mesh_distance(a_mesh, b_mesh, thresholds=(0.01,), align=None) == ops.mesh_distance(*a_mesh, *b_mesh, thresholds=(0.01,))
    assert plain["chamfer"] > 0.05 * A.diameter(b)
    got = pipeline.mesh_distance(a_mesh, b_mesh, thresholds=(0.01,), align=True)
    print("chamfer", plain["chamfer"], "->", got["chamfer"])
    assert set(got) == set(plain) | {"alignment"} and got["alignment"]["candidate"] == 4 and got["alignment"]["converged"]
    assert got["chamfer"] <= 1e-9 * A.diameter(b) and got["fscore"] == [1.0]
    alone = pipeline.mesh_distance(a_mesh, b_mesh, align={"candidates": None})
    assert alone["chamfer"] > 1e-3 * A.diameter(b) and len(alone["alignment"]["candidate_scores"]) == 1
