"""GPU: csrc/mesh_distance.hip against its host twin (mesh_io.surface_samples / closest_triangles / mesh_distance) -- samples, d2 and nearest to the bit, the
grid query against the exhaustive one to the bit, the summary's integers exactly and its sums to 1e-12 -- plus guard bands around every buffer and the
pipeline's report."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import mesh_distance_util as U
from guard_util import Guard
from mesh_scene_util import args, dev, ops, pipeline, stored_scene          # noqa: F401  (dev is a fixture)

mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
_lib = importlib.import_module("one-2-3-45_amd._lib")
STATS = "O2345DistanceStats"
STATS_BYTES = ctypes.sizeof(_lib.STRUCTS[STATS])        # the block at its exact size: one byte more written and a guard band shows it
pytestmark = pytest.mark.gpu


def up(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a)).to(dev)
    return (t if dtype is None else t.to(dtype)).contiguous()


def same(t, a):
    """device tensor == host array, bit for bit"""
    h = t.cpu().numpy()
    return h.dtype == a.dtype and h.shape == a.shape and h.tobytes() == np.ascontiguousarray(a).tobytes()


def hand_mesh():
    """one triangle that hits the k = 64 cap at spacing 0.2, one without an area, one with a repeated index, and two ordinary ones"""
    v = np.array([[0.0, 0, 0], [40, 0, 0], [0, 30, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [0.3, 0.1, 0.7], [1.1, 0.2, 0.9], [0.4, 1.3, 0.2]])
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 6, 7], [6, 7, 8], [8, 7, 6]], np.int64)
    return v, f


# ---- samples ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("mesh, spacing", [("sphere", None), ("sphere", 0.75), ("sphere", 0.2), ("hand", 0.2), ("hand", None), ("one", 0.3), ("none", 0.3)])
def test_samples_equal_the_twin(dev, mesh, spacing, dtype):
    v, f = {"sphere": U.spheres()[0], "hand": hand_mesh(), "one": (hand_mesh()[0], hand_mesh()[1][3:4]), "none": (hand_mesh()[0], np.zeros((0, 3), np.int64))}[mesh]
    pts, w, tri = mesh_io.surface_samples(v, f, spacing)
    got = ops.mesh_surface_samples(up(v, dev), up(f, dev, dtype).view(-1, 3), spacing)
    assert same(got[0], pts) and same(got[1], w) and same(got[2], tri)
    if mesh == "hand" and spacing == 0.2:
        assert len(w) == 64 * 64 + 18 * 18 + 25 + 64 + 64 and (w[4096:4096 + 324 + 25] == 0).all()
    if mesh == "none":
        assert got[0].shape == (0, 3)


@pytest.mark.parametrize("what, mesh", [("non-finite", lambda v, f: (np.where(np.arange(len(v))[:, None] == 7, np.inf, v), f)),
                                        ("index outside", lambda v, f: (v, np.concatenate([f, [[0, 1, len(v)]], [[-1, 0, 1]]])))])
def test_samples_refuse_bad_input_without_touching_it(dev, what, mesh):
    v, f = mesh(*hand_mesh())
    with pytest.raises(RuntimeError, match=what):
        ops.mesh_surface_samples(up(v, dev), up(f, dev), 0.5)
    with pytest.raises(RuntimeError, match=what):
        ops.mesh_distance_grid(up(v, dev), up(f, dev))
    with pytest.raises(ValueError, match="spacing"):
        ops.mesh_surface_samples(up(v, dev), up(f, dev), 0.0)


# ---- queries ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B(dev):
    _, (vb, fb) = U.spheres()
    return dict(v=up(vb, dev), f=up(fb, dev), q=up(U.all_queries(), dev))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_exhaustive_query_equals_the_twin(dev, B, dtype):
    d2, nearest, _, _ = U.twin_answers()
    got_d2, got_n = ops.mesh_closest_triangle(B["q"], B["v"], B["f"].to(dtype))
    assert same(got_d2, d2) and same(got_n, nearest)


def _targets():
    (va, fa), (vb, fb) = U.spheres()
    box = (np.array([[-1.0, -2.0, -1.5], [25.0, 24.0, 1.0], [3.0, 26.0, 25.5]]), np.array([[0, 1, 2]]))          # one triangle through the whole box
    return {"sphere": (vb, fb), "sphere+span": U.joined((vb, fb), box), "sphere+far": U.joined((vb, fb), U.octahedron((51.9, 11.8, 11.7))),
            "single": (box[0], box[1].astype(np.int64))}


def _grid_origin(grid):
    return grid.buffer[:24].cpu().numpy().view(np.float64)


@pytest.mark.parametrize("target", ["sphere", "sphere+span", "sphere+far", "single"])
@pytest.mark.parametrize("cell", [None, 1.0, 0.37, 50.0])
def test_grid_query_equals_the_exhaustive_query(dev, B, target, cell):
    v, f = _targets()[target]
    tv, tf = up(v, dev), up(f, dev, torch.int32 if cell == 0.37 else torch.int64).view(-1, 3)
    grid = ops.mesh_distance_grid(tv, tf, cell)
    origin, dims = _grid_origin(grid), np.array(grid.dims)
    assert grid.entries >= len(f) and grid.degenerate == 0 and (dims >= 1).all() and (dims <= 256).all() and int(dims.prod()) <= grid.max_cells
    if cell is not None:
        assert grid.cell == cell                                      # nothing had to be enlarged
        assert np.array_equal(origin, np.floor(v.min(0) / cell) * cell)
    if cell == 1.0:
        assert np.array_equal(origin, np.round(origin))              # a marching-cubes vertex has two integer coordinates: exactly on cell borders
        assert np.array_equal(dims, np.floor((v.max(0) - origin) / cell) + 1)
    if cell == 50.0 and target == "sphere":
        assert grid.dims == (1, 1, 1)                                # a single cell
    rng = np.random.default_rng(5)
    far = np.array([[sx * 1e3, sy * 1e3, sz * 1e3] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) + 11.0
    axis = np.concatenate([np.eye(3) * 1e3, -np.eye(3) * 1e3]) + rng.uniform(5, 18, (6, 3))
    ijk = rng.integers(0, dims + 1, (400, 3))
    corners = origin + ijk * grid.cell                                # exactly on cell corners, the outer faces of the grid included
    extra = up(np.concatenate([far, axis, corners, rng.uniform(-6, 60, (300, 3))]), dev)
    q = torch.cat([B["q"][::3], extra]).contiguous()
    want_d2, want_n = ops.mesh_closest_triangle(q, tv, tf)
    got_d2, got_n = ops.mesh_closest_triangle(q, tv, tf, grid)
    assert torch.equal(got_d2.view(torch.int64), want_d2.view(torch.int64)) and torch.equal(got_n, want_n)
    assert bool((want_n >= 0).all()) and bool(torch.isfinite(want_d2).all())


def test_grid_lists_are_ascending_and_complete(dev):
    v, f = _targets()["sphere+span"]
    tv, tf = up(v, dev), up(f, dev)
    for cell in (2.0, 50.0):                                          # short rows in registers; one row of 2,001 triangles by the block sort
        grid = ops.mesh_distance_grid(tv, tf, cell, max_cells=4096)
        raw = grid.buffer.cpu().numpy()
        n_cells = int(np.prod(grid.dims))
        start = raw[128:128 + 4 * (n_cells + 1)].view(np.int32)
        entries = raw[128 + (4 * (4096 + 1) + 15) // 16 * 16:].view(np.int32)[:grid.entries]
        assert start[0] == 0 and start[-1] == grid.entries and (np.diff(start) >= 0).all()
        origin = raw[:24].view(np.float64)
        P = v[f]
        lo = np.clip(np.floor((P.min(1) - origin) / grid.cell), 0, np.array(grid.dims) - 1).astype(int)
        hi = np.clip(np.floor((P.max(1) - origin) / grid.cell), 0, np.array(grid.dims) - 1).astype(int)
        assert int((hi - lo + 1).prod(1).sum()) == grid.entries
        for c in range(n_cells):
            row = entries[start[c]:start[c + 1]]
            assert (np.diff(row) > 0).all()
            x, y, z = c % grid.dims[0], c // grid.dims[0] % grid.dims[1], c // (grid.dims[0] * grid.dims[1])
            inside = ((lo <= (x, y, z)) & ((x, y, z) <= hi)).all(1)
            assert np.array_equal(row, np.nonzero(inside)[0])


ROW_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 34, 65]          # around 4, 16 and 32 (the register sorts of 4, 16 and 32 entries); 33, 34 and 65: long rows


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_cell_lists_around_the_register_sort_limits(dev, dtype):
    """258 small triangles with an area in 13 groups of ROW_SIZES; those of group k lie strictly inside the cell at x in (2k + 0.25, 2k + 0.75), y and z in
    (0.25, 0.75) of a grid of edge 1.  The triangle indices are shuffled, so the members of a cell come from all over the index range and reach its list
    in any order.  Every occupied cell's list is its group, ascending; every other cell is empty."""
    rng = np.random.default_rng(17)
    owner = rng.permutation(np.repeat(np.arange(len(ROW_SIZES)), ROW_SIZES))
    nt = owner.size
    assert nt == 258
    corner = rng.uniform(0.3, 0.6, (nt, 1, 3)) + np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.02], [0.0, 0.1, 0.03]])          # three corners per triangle
    assert (corner > 0.25).all() and (corner < 0.75).all()
    corner[:, :, 0] += 2.0 * owner[:, None]
    v, f = corner.reshape(-1, 3), np.arange(3 * nt, dtype=np.int64).reshape(nt, 3)
    grid = ops.mesh_distance_grid(up(v, dev), up(f, dev, dtype).view(-1, 3), 1.0, max_cells=4096)
    assert grid.cell == 1.0 and grid.dims == (2 * len(ROW_SIZES) - 1, 1, 1) and grid.entries == nt
    raw = grid.buffer.cpu().numpy()
    n_cells = grid.dims[0]
    assert (raw[:24].view(np.float64) == 0.0).all()                  # the origin: cell c is x in [c, c + 1)
    start = raw[128:128 + 4 * (n_cells + 1)].view(np.int32)
    entries = raw[128 + (4 * (4096 + 1) + 15) // 16 * 16:].view(np.int32)[:grid.entries]
    assert start[0] == 0 and start[-1] == nt
    for c in range(n_cells):
        row = entries[start[c]:start[c + 1]]
        want = np.flatnonzero(owner == c // 2) if c % 2 == 0 else np.zeros(0, np.int64)
        assert np.array_equal(row, want), (c, row, want)


def test_degenerate_targets_take_no_part(dev):
    v, f = U.square(0.0)
    f2 = np.concatenate([[[0, 0, 1], [0, 1, 2]], f, [[3, 3, 3]]])
    f2 = np.concatenate([f2] * 3)                                     # 105 triangles: over the exhaustive threshold of ops.mesh_distance
    q = up(np.random.default_rng(2).uniform(-1, 2, (500, 3)), dev)
    d2, nearest, _, _, deg = mesh_io.closest_triangles(q.cpu().numpy(), v, f2)
    grid = ops.mesh_distance_grid(up(v, dev), up(f2, dev))
    for g in (None, grid):
        got = ops.mesh_closest_triangle(q, up(v, dev), up(f2, dev), g)
        assert same(got[0], d2) and same(got[1], nearest)
    assert deg == 9 and grid.degenerate == 9
    r = ops.mesh_distance(up(v, dev), up(f, dev), up(v, dev), up(f2, dev), 0.3)
    assert r["degenerate_targets"] == {"a": 0, "b": 9} and r["hausdorff"] < 1e-15
    none = up(np.array([[0, 0, 1], [2, 2, 2]] * 40), dev)
    with pytest.raises(RuntimeError, match="no triangle with an area"):
        ops.mesh_distance(up(v, dev), up(f, dev), up(v, dev), none)
    with pytest.raises(RuntimeError, match="no triangle with an area"):
        ops.mesh_distance(up(v, dev), up(f, dev), up(v, dev), none[:2].contiguous())          # the exhaustive path says so too
    got = ops.mesh_closest_triangle(q, up(v, dev), none[:2].contiguous())
    assert bool(torch.isinf(got[0]).all()) and bool((got[1] == -1).all())


# ---- summary ---------------------------------------------------------------------------------------------------------------------------------------
def test_summary_integers_exact_sums_to_1e_12_and_bytes_repeat(dev, B):
    d2, nearest, _, _ = U.twin_answers()
    n = len(d2)
    assert n > 3 * 4096                                              # several blocks and a ragged last one
    w = np.random.default_rng(7).uniform(0.0, 2.0, n)
    w[::11] = 0.0
    d2 = d2.copy(); nearest = nearest.copy()
    d2[5], nearest[5] = np.inf, -1                                    # left out and counted
    nearest[4097] = -1
    th = (0.0, 0.05, 0.3, 0.31, 1.0, 14.0, 14.6, 100.0)
    keep = nearest >= 0
    d = np.sqrt(d2[keep])
    td2, tn, tw = up(d2, dev), up(nearest, dev), up(w, dev)
    runs = [ops.mesh_distance_stats(td2, tn, tw, th, target=(B["v"], B["f"])).cpu().numpy() for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()
    st = _lib.read_struct(STATS, runs[0])
    assert runs[0].nbytes == STATS_BYTES and [st.max_d2_bits, st.n, st.n_unmatched, st.n_degenerate, st.n_bad] == [int(d2[keep].max().view(np.uint64)), n, 2, 0, 0]
    want = [math.fsum(w[keep]), math.fsum(w[keep] * d), math.fsum(w[keep] * d2[keep])] + [math.fsum(w[keep][d <= t]) for t in th]
    for got, ref in zip([st.sum_w, st.sum_wd, st.sum_wd2] + list(st.within), want, strict=True):
        assert abs(got - ref) <= 1e-12 * ref, (got, ref)
    assert 0 < want[3] < want[5] < want[10] == want[0]               # some at distance 0, some within 0.3, the pushed-out ones beyond, all within 100
    # without weights and without nearest: every sample counts 1
    st = _lib.read_struct(STATS, ops.mesh_distance_stats(td2[:4096].contiguous(), None, None, (0.3,)).cpu().numpy())
    assert st.sum_w == 4095.0 and [st.n, st.n_unmatched, st.n_degenerate, st.n_bad] == [4096, 1, 0, 0]
    with pytest.raises(ValueError, match="thresholds"):
        ops.mesh_distance_stats(td2, tn, tw, [0.1] * 9)


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ib, np_idx", [(4, np.int32), (8, np.int64)])
def test_every_entry_stays_inside_its_buffers(dev, ib, np_idx):
    L = _lib.lib()
    (va, fa), _ = U.spheres()
    v, f = U.joined((va, fa), (hand_mesh()[0], hand_mesh()[1][3:]))
    nv, nt = len(v), len(f)
    G = Guard(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gv, gf = G.buf(v, "verts"), G.buf(f.astype(np_idx), "tris")
    # samples
    wsb = L.o2345_mesh_samples_workspace_bytes(nt)
    ws = G.buf(wsb, "samples workspace")
    n = ctypes.c_longlong()
    _lib.check(L.o2345_mesh_samples_count(P(gv), P(gf), ib, nv, nt, 0.75, P(ws), wsb, ctypes.byref(n), stream), "count")
    n = n.value
    assert n == len(mesh_io.surface_samples(v, f, 0.75)[1])
    pts, w, tri = G.buf(24 * n, "points"), G.buf(8 * n, "weights"), G.buf(4 * n, "triangle")
    _lib.check(L.o2345_mesh_samples_emit(P(gv), P(gf), ib, nv, nt, P(ws), n, P(pts), P(w), P(tri), stream), "emit")
    # grid: the smallest max_cells the default edge fits
    max_cells = 4096
    gwb = L.o2345_mesh_distance_grid_workspace_bytes(nt, max_cells)
    gws = G.buf(gwb, "grid workspace")
    ne, dims = ctypes.c_longlong(), (ctypes.c_int * 3)()
    _lib.check(L.o2345_mesh_distance_grid_count(P(gv), P(gf), ib, nv, nt, 0.0, max_cells, P(gws), gwb, ctypes.byref(ne), None, dims, None, stream), "grid count")
    gb = L.o2345_mesh_distance_grid_bytes(max_cells, ne.value)
    grid = G.buf(gb, "grid")
    _lib.check(L.o2345_mesh_distance_grid_emit(P(gv), P(gf), ib, nv, nt, max_cells, P(gws), ne.value, P(grid), gb, stream), "grid emit")
    assert 1 < dims[0] * dims[1] * dims[2] <= max_cells
    # queries
    out = [(G.buf(8 * n, "d2"), G.buf(4 * n, "nearest")) for _ in range(2)]
    _lib.check(L.o2345_mesh_distance_query(P(pts), n, P(gv), P(gf), ib, nv, nt, P(grid), gb, max_cells, P(out[0][0]), P(out[0][1]), stream), "grid query")
    _lib.check(L.o2345_mesh_distance_query(P(pts), n, P(gv), P(gf), ib, nv, nt, None, 0, 0, P(out[1][0]), P(out[1][1]), stream), "query")
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # summary
    rwb = L.o2345_mesh_distance_reduce_workspace_bytes(n)
    rws, stats = G.buf(rwb, "reduce workspace"), G.buf(STATS_BYTES, "stats")
    th = np.array([0.1, 0.2], np.float64)
    _lib.check(L.o2345_mesh_distance_reduce(P(out[0][0]), P(out[0][1]), P(w), n, th.ctypes.data_as(ctypes.c_void_p), 2, P(gv), P(gf), ib, nv, nt, P(rws), rwb,
                                            P(stats), stream), "reduce")
    assert G.damaged() == []
    assert _lib.read_struct(STATS, stats.cpu().numpy()).n == n and float(out[0][0].view(torch.float64).max()) < 1e-12 * 24 ** 2


# ---- the whole thing -------------------------------------------------------------------------------------------------------------------------------
def _close(a, b):
    return a == b or abs(a - b) <= 1e-12 * abs(b)


def _reports_agree(got, want):
    for side in ("a_to_b", "b_to_a"):
        assert got[side]["samples"] == want[side]["samples"] and got[side]["max"] == want[side]["max"]
        for k in ("mean", "rms", "area"):
            assert _close(got[side][k], want[side][k]), (side, k)
        assert len(got[side]["within"]) == len(want[side]["within"]) and all(_close(x, y) for x, y in zip(got[side]["within"], want[side]["within"]))
    assert got["hausdorff"] == want["hausdorff"] and _close(got["chamfer"], want["chamfer"]) and got["degenerate_targets"] == want["degenerate_targets"]
    assert got["thresholds"] == want["thresholds"] and set(got) - {"samples"} == set(want) - {"samples"}
    for k in ("precision", "recall", "fscore"):
        assert all(_close(x, y) for x, y in zip(got[k], want[k])), k


def test_spheres_through_ops_equal_the_twin(dev):
    (va, fa), (vb, fb) = U.spheres()
    th = (0.1, 0.3, 0.5, 1.0)
    want = mesh_io.mesh_distance(va, fa, vb, fb, 0.75, th, return_samples=True)
    got = ops.mesh_distance(up(va, dev), up(fa, dev), up(vb, dev), up(fb, dev, torch.int32), 0.75, th, return_samples=True)
    _reports_agree(got, want)
    for side in ("a", "b"):
        for k in ("points", "weight", "triangle", "d2", "nearest"):
            assert same(got["samples"][side][k], want["samples"][side][k]), (side, k)
    assert 0.2 < got["chamfer"] < 0.35 and got["precision"][0] < got["precision"][1] < got["precision"][3] == 1.0
    assert abs(got["hausdorff"] - math.sqrt(0.4 ** 2 + 0.3 ** 2 + 0.2 ** 2)) < 0.1          # the two spheres are one shift apart


@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev)
    S["dec"] = pipeline.extract_mesh(*args(S), return_index_verts=True, decimate_cell=2)
    return S


def test_pipeline_distance_of_the_decimated_small_scene_equals_the_twin(dev, scene):
    S = scene
    dv, df = S["dec"][0], S["dec"][1]
    assert 0 < df.shape[0] < S["hf"].shape[0]
    th = (0.25, 0.5, 1.0, 2.0)
    want = mesh_io.mesh_distance(dv.cpu().numpy(), df.cpu().numpy(), S["hv"], S["hf"], None, th, return_samples=True)
    got = pipeline.mesh_distance((dv, df), (S["hv"], S["hf"]), thresholds=th, return_samples=True)          # device tensors and host arrays mixed
    _reports_agree(got, want)
    for side in ("a", "b"):
        assert same(got["samples"][side]["d2"], want["samples"][side]["d2"]) and same(got["samples"][side]["nearest"], want["samples"][side]["nearest"])
    assert got["hausdorff"] > 0 and got["a_to_b"]["samples"] == df.shape[0] and got["b_to_a"]["samples"] == S["hf"].shape[0]


def test_reconstruct_folder_reports_the_mesh_error_only_when_asked(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    run = lambda name, **kw: pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / name), D=48, resolution=64, decimate_cell=2, **kw)
    never, off, on = run("a.ply"), run("b.ply", mesh_error=False), run("c.ply", mesh_error=True)
    assert set(never) == set(off) and "mesh_error" not in off and set(on) == set(off) | {"mesh_error"}
    raw = [open(r["ply"], "rb").read() for r in (never, off, on)]
    assert raw[0] == raw[1] == raw[2] and len(raw[0]) > 1000
    # the same scene once more through the pieces
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    T = lambda t: t.to(dev).contiguous().float()
    vol = pipeline.build_volume(wt, T(s["images"]), T(s["affine_mats"]), s["partial_vol_origin"].numpy(), 48, 2.0 / 47)
    proj, cam_pos = pipeline.camera_terms(T(s["intrinsics"]), T(s["w2cs"]))
    pv, pf, _, _ = pipeline.extract_mesh(wt, vol, proj, cam_pos, 64, return_index_verts=True)
    dv, df, _, _ = pipeline.extract_mesh(wt, vol, proj, cam_pos, 64, return_index_verts=True, decimate_cell=2)
    want = pipeline.mesh_distance((dv, df), (pv, pf), pipeline.MESH_ERROR_SPACING, pipeline.MESH_ERROR_THRESHOLDS)
    assert on["mesh_error"] == want and want["thresholds"] == [0.25, 0.5, 1.0, 2.0]
    assert want["hausdorff"] > 0 and want["a_to_b"]["samples"] > on["triangles"] and 0 < want["fscore"][0] <= want["fscore"][3] <= 1.0
