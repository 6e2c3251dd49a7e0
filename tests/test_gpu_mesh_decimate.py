"""GPU: decimation by vertex clustering (csrc/mesh_decimate.hip) against the host twin (mesh_io.decimate_mesh), which defines the result.  Integer and
topology work plus one sum in a defined order: every comparison is EXACT (torch.equal / bytes).  Expected values are the host twin applied to the same
inputs, or facts derived from the definition, never the code under test."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mesh_components_util as mcu
import mesh_smooth_util as msu
from guard_util import PRE, Guard
from mesh_scene_util import args as _args, bits as _bits, dev, dev_tris as _dev_tris, fields_at as _fields_at, golden_mirror, mc, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("one-2-3-45_amd")
ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

NVS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 4097)          # every block (256) and scan-tile (2048) boundary
INFO_KEYS = {"clusters", "vertices", "triangles", "degenerate", "duplicate"}


def _mc(dev, field, shift=0.0):
    m = mc(dev, field)
    hv, hf = m["hv"] + shift, m["hf"]
    hv.setflags(write=False)
    hf.setflags(write=False)
    return dict(hv=hv, hf=hf)


@pytest.fixture(scope="module")
def closed_mesh(dev):
    """HIP marching cubes of the three-spheres-and-specks field; the twin says that cell 2 exercises every path: degenerate and duplicate triangles, dropped
    clusters (the specks collapse into one cell each) and clusters of 8 members and more"""
    m = _mc(dev, mcu.spheres_field(40))
    _, _, _, cluster, info = mio.decimate_mesh(m["hv"], m["hf"], 2.0)
    assert info["degenerate"] > 0 and info["duplicate"] > 0 and info["vertices"] < info["clusters"] and np.bincount(cluster[cluster >= 0]).max() >= 8, info
    return m


@pytest.fixture(scope="module")
def cut_mesh(dev):
    return _mc(dev, msu.cut_sphere_field(24))


def _check(hv, hf, dev, dtype, cell, want=None):
    """ops.mesh_decimate == the twin, exactly; the inputs are only read -> (the device outputs, the twin's info)"""
    hv = np.array(hv, np.float64).reshape(-1, 3)                          # a copy: the shared meshes are read-only
    verts, tris = torch.from_numpy(hv).to(dev), _dev_tris(hf, dev, dtype)
    tris0 = tris.clone()
    v, t, cluster, info = ops.mesh_decimate(verts, tris, cell)
    wv, wf, _, wcluster, winfo = mio.decimate_mesh(hv, np.asarray(hf).reshape(-1, 3), cell) if want is None else want
    assert set(info) == INFO_KEYS and info == winfo, (info, winfo)
    assert v.dtype == torch.float64 and v.shape == (winfo["vertices"], 3) and v.cpu().numpy().tobytes() == np.ascontiguousarray(wv).tobytes()
    assert t.dtype == dtype and t.shape == (winfo["triangles"], 3) and np.array_equal(t.cpu().numpy(), wf)
    assert cluster.dtype == torch.int32 and np.array_equal(cluster.cpu().numpy(), wcluster)
    assert verts.cpu().numpy().tobytes() == hv.tobytes() and torch.equal(tris, tris0)
    return (v, t, cluster), winfo


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("cell", [0.5, 2.0, 3.0])
def test_marching_cubes_mesh(dev, closed_mesh, cell, dtype):
    _, info = _check(closed_mesh["hv"], closed_mesh["hf"], dev, dtype, cell)
    assert 0 < info["vertices"] < closed_mesh["hv"].shape[0]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("shift", [0.0, -11.3])
def test_cut_mesh_and_negative_coordinates(dev, cut_mesh, shift, dtype):
    _, info = _check(cut_mesh["hv"] + shift, cut_mesh["hf"], dev, dtype, 2.0)
    assert info["clusters"] == (65 if shift == 0.0 else 52)          # the twin on this mesh; the shift moves the lattice through the surface


def _chain(nv):
    """triangles (i, i + 1, i + 2): over vertices in cells of their own all are kept"""
    i = np.arange(max(nv - 2, 0), dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1)


def _layout(kind, nv, cell, rng):
    inside = rng.uniform(0.05, 0.95, (nv, 3)) * cell
    i = np.arange(nv)
    if kind == "line":              # keys differ in their high bits only: a weak hash shows as long probe chains
        return inside + np.stack([i, 0 * i, 0 * i], 1) * cell, _chain(nv)
    if kind == "lattice":
        return inside + np.stack([i % 16, (i // 16) % 16, i // 256], 1) * cell - 3 * cell, _chain(nv)
    if kind == "one_cell":          # the long row; every triangle collapses
        return inside, _chain(nv)
    assert kind == "one_cell_alive"  # all but the last two vertices in one cell; every triangle maps to the same three clusters: nv - 3 duplicates
    p = inside.copy()
    if nv >= 3:
        p[-2] += [5 * cell, 0, 0]
        p[-1] += [0, 5 * cell, 0]
        return p, np.stack([i[:-2], np.full(nv - 2, nv - 2), np.full(nv - 2, nv - 1)], 1).astype(np.int64)
    return p, np.zeros((0, 3), np.int64)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("kind", ["line", "lattice", "one_cell", "one_cell_alive"])
def test_every_block_and_tile_boundary(dev, dtype, kind):
    rng = np.random.default_rng(11)
    cell = 0.37
    for nv in NVS:
        hv, hf = _layout(kind, nv, cell, rng)
        _, info = _check(hv, hf, dev, dtype, cell)
        nt = hf.shape[0]
        if kind in ("line", "lattice"):
            assert info == {"clusters": nv, "vertices": nv if nt else 0, "triangles": nt, "degenerate": 0, "duplicate": 0}
        elif kind == "one_cell":
            assert info == {"clusters": min(nv, 1), "vertices": 0, "triangles": 0, "degenerate": nt, "duplicate": 0}
        elif nv >= 3:
            assert info == {"clusters": 3, "vertices": 3, "triangles": 1, "degenerate": 0, "duplicate": nt - 1}


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_strip_and_fans(dev, dtype):
    rng = np.random.default_rng(12)
    f, nv = mcu.strip(3000, True)
    hv = rng.uniform(-6.0, 6.0, (nv, 3))
    for cell in (0.05, 1.0, 4.0):
        _check(hv, f, dev, dtype, cell)
    for nt in NVS:                                                       # triangle counts at the same boundaries; unreferenced vertices in between
        f, nv = mcu.fan(nt)
        _check(rng.uniform(-2.0, 2.0, (nv, 3)), f, dev, dtype, 0.8)
    # no triangle at all: every cluster is dropped
    _, info = _check(rng.uniform(-2.0, 2.0, (300, 3)), np.zeros((0, 3), np.int64), dev, dtype, 0.8)
    assert info["clusters"] > 1 and info["vertices"] == 0


ROW_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 34, 65]    # around the register networks of 4, 16 and 32 members, and the first rows of the block sort


def _sequential_sum(x):
    acc = np.float64(0.0)
    for v in x:
        acc = acc + v
    return acc


@pytest.fixture(scope="module")
def row_mesh():
    """258 vertices in 13 clusters of ROW_SIZES members, cluster k in the cell at x = 2k; the vertex indices are shuffled, so the members of a
    cluster lie all over the index range and reach their row in any order; the offsets inside a cell have random mantissas over four binades, so a cluster's fp64 sum depends on the order of its
    members; one triangle over every three consecutive clusters keeps all of them.  -> (vertices, triangles, the twin's result)"""
    rng = np.random.default_rng(13)
    owner = rng.permutation(np.repeat(np.arange(len(ROW_SIZES)), ROW_SIZES))
    hv = rng.uniform(0.5, 1.0, (owner.size, 3)) * 2.0 ** -rng.integers(0, 4, (owner.size, 3))
    hv[:, 0] += 2.0 * owner
    first = np.array([np.flatnonzero(owner == k)[0] for k in range(len(ROW_SIZES))], np.int64)
    hf = np.stack([first[:-2], first[1:-1], first[2:]], 1)
    rows = [np.flatnonzero(owner == k) for k in range(len(ROW_SIZES)) if ROW_SIZES[k] >= 15]
    assert any(_sequential_sum(hv[r, d]) != _sequential_sum(hv[r[::-1], d]) for r in rows for d in range(3))       # the order is visible in the result
    return hv, hf, mio.decimate_mesh(hv, hf, 1.0)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_member_rows_around_the_register_sort_limits(dev, row_mesh, dtype):
    hv, hf, twin = row_mesh
    cluster, info = twin[3], twin[4]
    assert np.sort(np.bincount(cluster[cluster >= 0])).tolist() == ROW_SIZES and (cluster >= 0).all()
    assert info == {"clusters": len(ROW_SIZES), "vertices": len(ROW_SIZES), "triangles": len(ROW_SIZES) - 2, "degenerate": 0, "duplicate": 0}
    _check(hv, hf, dev, dtype, 1.0, want=twin)


def test_two_runs_and_a_second_stream_give_identical_bytes(dev, closed_mesh):
    verts, tris = torch.from_numpy(closed_mesh["hv"].copy()).to(dev), _dev_tris(closed_mesh["hf"], dev, torch.int64)
    torch.cuda.synchronize()
    runs = []
    side = torch.cuda.Stream(device=dev)
    for stream in (None, None, side):
        with torch.cuda.stream(stream):
            v, t, c, info = ops.mesh_decimate(verts, tris, 2.0)
            runs.append([x.cpu().numpy().tobytes() for x in (v, t, c)] + [info])
    assert runs[0] == runs[1] == runs[2]


def test_off_launches_nothing(dev, closed_mesh, monkeypatch):
    verts, tris = torch.from_numpy(closed_mesh["hv"].copy()).to(dev), _dev_tris(closed_mesh["hf"], dev, torch.int64)

    class Dead:
        def __getattr__(self, name):
            pytest.fail(f"cell = 0 must not reach the library ({name})")
    monkeypatch.setattr(_lib, "_LIB", Dead())
    assert config.MESH_DECIMATE_CELL == 0.0                               # the environment of the test run leaves it unset
    for cell in (0, 0.0, None):
        out = ops.mesh_decimate(verts, tris, cell)
        assert out[0] is verts and out[1] is tris and out[2] is None and out[3] is None


def test_errors_are_statuses_not_faults(dev):
    """each refusal on a mesh of a few vertices: counted on the device, raised on the host, and the next call works"""
    good = torch.tensor([[0.1, 0.2, 0.3], [1.5, 0.2, 0.3], [0.1, 1.7, 0.3], [0.1, 0.2, 2.9]], dtype=torch.float64, device=dev)
    tris = torch.tensor([[0, 1, 2], [1, 2, 3]], device=dev)
    for bad in (float("nan"), float("inf"), float("-inf")):
        v = good.clone()
        v[2, 1] = bad
        with pytest.raises(RuntimeError, match="non-finite"):
            ops.mesh_decimate(v, tris, 1.0)
    for bad in (4, -1, 2 ** 31 + 1):
        t = tris.clone()
        t[1, 2] = bad
        with pytest.raises(RuntimeError, match="index outside"):
            ops.mesh_decimate(good, t, 1.0)
    with pytest.raises(RuntimeError, match="index outside"):
        ops.mesh_decimate(good, torch.tensor([[0, 1, 7]], dtype=torch.int32, device=dev), 1.0)
    far = good.clone()
    far[3, 0] = 0.1 + 2.0 ** 21
    with pytest.raises(RuntimeError, match="2\\^21"):
        ops.mesh_decimate(far, tris, 1.0)
    far[3, 0] = 0.1 + 2.0 ** 21 - 1                                       # one cell less is legal
    _check(far.cpu().numpy(), tris.cpu().numpy(), dev, torch.int64, 1.0)
    with pytest.raises(RuntimeError, match="2\\^21"):
        ops.mesh_decimate(good * 1e300, tris, 1e-300)                     # p / cell overflows to infinity
    for cell in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.mesh_decimate(good, tris, cell)
    with pytest.raises(ValueError):
        ops.mesh_decimate(good, tris.float(), 1.0)
    with pytest.raises(ValueError):
        ops.mesh_decimate(good.float(), tris, 1.0)
    _check(good.cpu().numpy(), tris.cpu().numpy(), dev, torch.int64, 1.0)


# ---- guard bands (tests/guard_util.py): every output and the workspace at their EXACT sizes ---------------------------------------------------------
def _guarded_run(g, dev, hv, hf, dtype, cell):
    """The two-call protocol through the C ABI itself, every buffer carved at its exact size -> (verts, tris, cluster, info) as numpy"""
    L = _lib.lib()
    nv, nt = hv.shape[0], hf.shape[0]
    ib = 8 if dtype == torch.int64 else 4
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    hv = np.array(hv, np.float64)
    tris, verts = _dev_tris(hf, dev, dtype), torch.from_numpy(hv).to(dev)
    wsb = L.o2345_mesh_decimate_workspace_bytes(nv, nt)
    assert wsb > 0 and PRE % 16 == 0
    ws = g.buf(wsb, ("workspace", nv, nt))
    out = [ctypes.c_longlong() for _ in range(5)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.o2345_mesh_decimate_count(P(verts), P(tris), ib, nv, nt, cell, ctypes.c_void_p(ws.data_ptr()), wsb, *[ctypes.byref(x) for x in out], s),
               "mesh_decimate_count")
    ncl, nvo, nto, ndeg, ndup = (x.value for x in out)
    vo, to, cl = g.buf(24 * nvo, ("verts_out", nv, nt)), g.buf(3 * ib * nto, ("tris_out", nv, nt)), g.buf(4 * nv, ("cluster", nv, nt))
    _lib.check(L.o2345_mesh_decimate_emit(P(verts), P(tris), ib, nv, nt, ctypes.c_void_p(ws.data_ptr()), P(vo), P(to), P(cl), s), "mesh_decimate_emit")
    h = lambda t, dt: t.cpu().numpy().view(dt)
    assert verts.cpu().numpy().tobytes() == hv.tobytes() and np.array_equal(tris.cpu().numpy(), hf)
    return (h(vo, np.float64).reshape(-1, 3), h(to, np.int64 if ib == 8 else np.int32).reshape(-1, 3), h(cl, np.int32),
            {"clusters": ncl, "vertices": nvo, "triangles": nto, "degenerate": ndeg, "duplicate": ndup})


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_kernel_writes_outside_its_buffers(dev, closed_mesh, cut_mesh, dtype):
    g = Guard(dev)
    cases = [(closed_mesh["hv"], closed_mesh["hf"], c) for c in (0.5, 2.0, 3.0, 100.0)] + [(cut_mesh["hv"] - 11.3, cut_mesh["hf"], 2.0)]
    rng = np.random.default_rng(13)
    for nv in NVS:
        for kind in ("line", "lattice", "one_cell", "one_cell_alive"):
            hv, hf = _layout(kind, nv, 0.37, rng)
            cases.append((hv, hf, 0.37))
        f, n = mcu.fan(nv)
        cases.append((rng.uniform(-2.0, 2.0, (n, 3)), f, 0.8))
    for hv, hf, cell in cases:
        v, t, cl, info = _guarded_run(g, dev, hv, hf, dtype, cell)
        bad = g.damaged()
        assert not bad, bad
        wv, wf, _, wcl, winfo = mio.decimate_mesh(hv, hf, cell)
        assert info == winfo and v.tobytes() == np.ascontiguousarray(wv).tobytes() and np.array_equal(t, wf) and np.array_equal(cl, wcl), (hv.shape, hf.shape, cell)
    assert len(g.live) == 4 * len(cases)


# ---- the pipeline on the stored small scene (D = 20, R = 64) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev)
    assert S["hf"].shape[0] > 100
    twin = mio.decimate_mesh(S["hv"], S["hf"], 2.0)
    assert 0 < twin[4]["vertices"] < S["hv"].shape[0] // 2
    return dict(S, twin=twin)


def test_extract_mesh_with_decimation(scene):
    S = scene
    dev = S["plain"][0].device
    wv, wf, _, _, winfo = S["twin"]
    v, t, rgb, u = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=2)
    assert v.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(t.cpu().numpy(), wf) and t.dtype == S["plain"][1].dtype and _bits(u, S["plain"][3])
    # gradient and colours are taken at the NEW vertices
    fields = pipeline._mesh_fields(*_args(S), config.mesh_options(decimate_cell=2.0))
    info = fields.info
    want_rgb, want_g = _fields_at(S, torch.from_numpy(wv).to(dev))
    assert _bits(rgb, want_rgb) and _bits(fields[3], want_rgb) and _bits(fields[5], want_g)
    assert info["decimate"] == winfo and info["components"] is None
    assert torch.equal(fields[0], v / (S["R"] - 1.0) * 2.0 - 1.0)
    # with the component filter and smoothing: filter, then twin, then smooth_vertices of the twin's mesh
    v, t, rgb, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, keep_largest=True, decimate_cell=2, smooth_iterations=3)
    fv, ff, _, _, _, _ = mio.filter_components(S["hv"], S["hf"], keep_largest=True)
    dv, df, _, _, _ = mio.decimate_mesh(fv, ff, 2.0)
    assert v.cpu().numpy().tobytes() == mio.smooth_vertices(dv, df, 3).tobytes() and np.array_equal(t.cpu().numpy(), df)
    assert _bits(rgb, _fields_at(S, torch.from_numpy(dv).to(dev))[0])           # coloured after decimation, before smoothing


def test_exports_with_decimation_equal_the_export_of_the_twins_mesh(scene, tmp_path):
    S = scene
    dev = S["plain"][0].device
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 0.9; scale[:3, 3] = [0.01, 0.02, -0.03]
    B = lambda p: open(p, "rb").read()
    wv, wf = torch.from_numpy(S["twin"][0]).to(dev), torch.from_numpy(S["twin"][1]).to(dev)
    rgb = _fields_at(S, wv)[0]
    got, want = str(tmp_path / "g.ply"), str(tmp_path / "w.ply")
    n = pipeline.export_mesh_ply(got, *_args(S), scale_mat=scale[None], decimate_cell=2.0)
    assert n == (S["twin"][4]["vertices"], S["twin"][4]["triangles"])
    assert n == mio.export_mesh(want, wv, wf, S["R"], scale_mat=scale[None], vertex_colors=rgb) and B(got) == B(want)
    for ext in (".glb", ".obj"):
        got, want = str(tmp_path / ("g" + ext)), str(tmp_path / ("w" + ext))
        assert pipeline.export_mesh_asset(got, *_args(S), scale_mat=scale[None], decimate_cell=2.0) == n
        mio.export_asset(want, wv, wf, S["R"], scale_mat=scale[None], vertex_colors=rgb)
        assert B(got) == B(want), ext


def test_a_mesh_that_collapses_takes_the_empty_mesh_path(scene, tmp_path):
    S = scene
    v, t, rgb, u = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=1000.0)
    assert v.shape == (0, 3) and t.shape == (0, 3) and rgb.shape == (0, 3) and _bits(u, S["plain"][3])
    assert pipeline.export_mesh_ply(str(tmp_path / "e.ply"), *_args(S), decimate_cell=1000.0) == (0, 0)


def test_decimation_off_is_todays_output(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    assert config.MESH_DECIMATE_CELL == 0.0                               # the environment of the test run leaves it unset
    monkeypatch.setattr(ops, "mesh_decimate", lambda *a, **k: pytest.fail("decimation must not run when it is off"))
    for kw in (dict(decimate_cell=0), dict(decimate_cell=None), dict()):
        off = pipeline.extract_mesh(*_args(S), return_index_verts=True, **kw)
        for a, b in zip(S["plain"], off):
            assert _bits(a, b)
        info = pipeline._mesh_fields(*_args(S), config.mesh_options(**kw)).info
        assert info["decimate"] is None
        for ext in (".ply", ".glb", ".obj"):
            p0, p1 = str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))
            fn = pipeline.export_mesh_ply if ext == ".ply" else pipeline.export_mesh_asset
            want = (mio.export_mesh if ext == ".ply" else mio.export_asset)(p0, S["plain"][0], S["plain"][1], S["R"], vertex_colors=S["plain"][2])
            assert fn(p1, *_args(S), **kw) == want
            assert B(p0) == B(p1)


def test_config_default_reaches_the_pipeline(scene, monkeypatch):
    S = scene
    monkeypatch.setattr(config, "MESH_DECIMATE_CELL", 2.0)
    v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True)
    assert v.cpu().numpy().tobytes() == S["twin"][0].tobytes() and np.array_equal(t.cpu().numpy(), S["twin"][1])
    v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=3.0)          # an explicit cell wins
    w = mio.decimate_mesh(S["hv"], S["hf"], 3.0)
    assert v.cpu().numpy().tobytes() == w[0].tobytes() and np.array_equal(t.cpu().numpy(), w[1])
    off = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=0)                    # and so does an explicit 0
    for a, b in zip(S["plain"], off):
        assert _bits(a, b)


def test_reconstruct_folder_reports_the_cell_and_the_counts(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64)
    assert plain["decimate_cell"] == 0.0 and plain["decimate"] is None and plain["triangles"] > 0
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64, decimate_cell=2)
    # the twin on the plain mesh: the same scene once more through the pieces
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    T = lambda t: t.to(dev).contiguous().float()
    vol = pipeline.build_volume(wt, T(s["images"]), T(s["affine_mats"]), s["partial_vol_origin"].numpy(), 48, 2.0 / 47)
    proj, cam_pos = pipeline.camera_terms(T(s["intrinsics"]), T(s["w2cs"]))
    v, t, _, _ = pipeline.extract_mesh(wt, vol, proj, cam_pos, 64, return_index_verts=True)
    winfo = mio.decimate_mesh(v.cpu().numpy(), t.cpu().numpy(), 2.0)[4]
    assert out["decimate_cell"] == 2.0 and out["decimate"] == winfo
    assert (out["vertices"], out["triangles"]) == (winfo["vertices"], winfo["triangles"]) and 0 < out["triangles"] < plain["triangles"]
    assert (mio.read_ply(out["ply"])[0].shape[0], mio.read_ply(out["ply"])[1].shape[0]) == (winfo["vertices"], winfo["triangles"])


# ---- the drop-in mirror ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_extract_geometry_applies_the_configured_decimation(dev, monkeypatch):
    ren, sdf, dense = golden_mirror(dev)
    R = 48
    call = lambda: ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=R, threshold=0, device=dev,
                                        conditional_volume=dense, lod=0)
    v0, t0, u0 = call()
    assert t0.shape[0] > 0
    # the mirror decimates INDEX coordinates and maps them to world units afterwards: the twin on marching cubes of the u it returns
    vi, ti = ops.marching_cubes(torch.from_numpy(u0).to(dev).contiguous(), 0.0)
    hv, hf = vi.cpu().numpy(), ti.cpu().numpy()
    assert np.array_equal(hf, t0)
    monkeypatch.setattr(config, "MESH_DECIMATE_CELL", 2.0)
    v, t, u = call()
    wv, wf, _, _, winfo = mio.decimate_mesh(hv, hf, 2.0)
    assert 0 < winfo["vertices"] < hv.shape[0]
    assert v.dtype == np.float64 and v.tobytes() == (wv / (R - 1) * 2.0 + -1.0).tobytes() and np.array_equal(t, wf) and u.tobytes() == u0.tobytes()
