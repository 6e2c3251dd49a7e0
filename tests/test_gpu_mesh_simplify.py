"""GPU: simplification by quadric-error edge collapse (csrc/mesh_simplify.hip) against the host twin (mesh_io.simplify_mesh), which defines the result.
Integer and topology work plus fp64 arithmetic in a defined order: every comparison is EXACT (bytes).  Expected values are the host twin applied to the
same inputs, or facts derived from the definition, never the code under test.  A twin result is computed once per (mesh, arguments) and shared."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mesh_components_util as mcu
import mesh_simplify_util as U
import mesh_smooth_util as msu
from guard_util import PRE, Guard
from mesh_scene_util import args as _args, bits as _bits, dev, dev_tris as _dev_tris, fields_at as _fields_at, golden_mirror, mc, sdf_field, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

STATS_BYTES = ctypes.sizeof(_lib.STRUCTS["O2345SimplifyStats"])         # behind it: 8 bytes per round
INFO_KEYS = {"rounds", "vertices", "triangles", "collapses", "max_cost", "stopped"}
SCAN_TILE = 2048                                                        # csrc/mesh_common.h
SIZES = (0, 1, 255, 256, 257, SCAN_TILE - 1, SCAN_TILE + 1)             # every block, wave and scan-tile boundary
INF = float("inf")
_twins = {}


def _twin(key, hv, hf, target, max_error=INF, max_rounds=256):
    k = (key, target, max_error, max_rounds)
    if k not in _twins:
        _twins[k] = mio.simplify_mesh(hv, np.asarray(hf).reshape(-1, 3).astype(np.int64), target, max_error, max_rounds)
    return _twins[k]


def _check(key, hv, hf, dev, dtype, target, max_error=INF, max_rounds=256):
    """ops.mesh_simplify == the twin, exactly; the inputs are only read -> the twin's info"""
    hv = np.array(hv, np.float64).reshape(-1, 3)                          # a copy: the shared meshes are read-only
    verts, tris = torch.from_numpy(hv).to(dev), _dev_tris(hf, dev, dtype)
    tris0 = tris.clone()
    v, t, source, merged, info = ops.mesh_simplify(verts, tris, target, max_error, max_rounds)
    wv, wf, _, wsource, wmerged, winfo = _twin(key, hv, hf, target, max_error, max_rounds)
    assert set(info) == INFO_KEYS and info == winfo, (info, winfo)
    assert v.dtype == torch.float64 and v.shape == (winfo["vertices"], 3) and v.cpu().numpy().tobytes() == np.ascontiguousarray(wv).tobytes()
    assert t.dtype == dtype and t.shape == (winfo["triangles"], 3) and np.array_equal(t.cpu().numpy(), wf)
    assert source.dtype == torch.int32 and np.array_equal(source.cpu().numpy(), wsource)
    assert merged.dtype == torch.int32 and np.array_equal(merged.cpu().numpy(), wmerged)
    assert verts.cpu().numpy().tobytes() == hv.tobytes() and torch.equal(tris, tris0)
    return winfo


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_cube_and_sphere(dev, dtype):
    v, f = U.cube10()
    nt = f.shape[0]
    assert _check("cube", v, f, dev, dtype, nt)["rounds"] == 0            # the target is met: zero rounds
    assert _check("cube", v, f, dev, dtype, nt // 5)["stopped"] == "target"
    info = _check("cube", v, f, dev, dtype, 0, 1e-9)
    assert info["stopped"] == "blocked" and info["triangles"] <= 300
    v, f = U.sphere20()
    nt = f.shape[0]
    assert _check("sphere", v, f, dev, dtype, nt + 7)["rounds"] == 0
    assert _check("sphere", v, f, dev, dtype, nt // 5)["triangles"] <= nt // 5
    info = _check("sphere", v, f, dev, dtype, 0, 1e-3)
    assert info["stopped"] == "blocked" and 0 < info["rounds"] and info["max_cost"] <= 1e-3
    assert _check("sphere", v, f, dev, dtype, nt // 20, INF, 5)["stopped"] == "rounds"


@pytest.fixture(scope="module")
def closed_mesh(dev):
    """HIP marching cubes of the three-spheres-and-specks field: closed surfaces, and octahedra of 8 faces"""
    return mc(dev, mcu.spheres_field(32))


@pytest.fixture(scope="module")
def cut_mesh(dev):
    m = mc(dev, msu.cut_sphere_field(24))
    assert 1 in U.edge_counts(m["hf"])                                    # the rim on the box
    return m


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_marching_cubes_meshes(dev, closed_mesh, cut_mesh, dtype):
    hv, hf = closed_mesh["hv"], closed_mesh["hf"]
    info = _check("closed", hv, hf, dev, dtype, hf.shape[0] // 5)
    assert info["stopped"] == "target" and info["rounds"] > 3
    assert _check("closed", hv, hf, dev, dtype, 0, 0.02)["max_cost"] <= 0.02
    hv, hf = cut_mesh["hv"], cut_mesh["hf"]
    rim = np.flatnonzero(mio.vertex_adjacency(hf, hv.shape[0])[2])
    for shift in (0.0, -11.3):
        info = _check(("cut", shift), hv + shift, hf, dev, dtype, hf.shape[0] // 5)
        assert info["rounds"] > 0 and np.isin(rim, _twin(("cut", shift), hv + shift, hf, hf.shape[0] // 5)[3]).all()


def _sized(nv=None, nt=None):
    """an open grid of two rows of quads (its middle row can go) with exactly nv vertices, or exactly nt triangles: the rest are unreferenced vertices,
    or single triangles over vertices of their own"""
    rng = np.random.default_rng(17)
    if nv is not None:
        nx = max(nv // 3 - 1, 0)
        v, f = U.grid(nx, 2, jitter=rng) if nx else (np.zeros((0, 3)), np.zeros((0, 3), np.int64))
        extra = nv - v.shape[0]
        return np.concatenate([v, rng.uniform(-3.0, 3.0, (extra, 3))]), f
    nx, loose = nt // 4, nt % 4
    v, f = U.grid(nx, 2, jitter=rng) if nx else (np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    n0 = v.shape[0]
    return (np.concatenate([v, rng.uniform(-3.0, 3.0, (3 * loose, 3))]),
            np.concatenate([f, n0 + np.arange(3 * loose, dtype=np.int64).reshape(-1, 3)]))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_every_block_and_tile_boundary(dev, dtype):
    for n in SIZES:
        v, f = _sized(nv=n)
        assert v.shape[0] == n
        _check(("nv", n), v, f, dev, dtype, f.shape[0] // 3 if n > 9 else 1)
        v, f = _sized(nt=n)
        assert f.shape[0] == n
        info = _check(("nt", n), v, f, dev, dtype, n // 3 if n > 12 else 1)
        assert info["rounds"] > 0 or n < 12


ROWS = (3, 8, 15, 16, 17, 31, 32, 33, 40, 65)                           # triangles at an apex: around the register sorts of 16 and 32 and into the block sort


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_fans_around_the_row_limits(dev, dtype):
    """a double cone over a k-gon: both apexes have k triangles (their quadric is a sum of k terms whose order shows in its bits) and k neighbours
    (2 k raw entries: the block path of the adjacency from k = 17, of the triangle rows from k = 33); the fan of valence 40 is among them"""
    for k in ROWS:
        v, f = U.fan(k)
        perm = np.random.default_rng(k).permutation(f.shape[0])           # the apex's triangles all over the face order
        info = _check(("fan", k), v, f[perm], dev, dtype, 8)
        assert info["rounds"] > 0 or k == 3
    _check(("fan", 40, "e"), *U.fan(40), dev, dtype, 0, 0.05)


def test_two_runs_and_a_second_stream_give_identical_bytes(dev, closed_mesh):
    verts, tris = torch.from_numpy(closed_mesh["hv"].copy()).to(dev), _dev_tris(closed_mesh["hf"], dev, torch.int64)
    torch.cuda.synchronize()
    runs = []
    side = torch.cuda.Stream(device=dev)
    for stream in (None, None, side):
        with torch.cuda.stream(stream):
            out = ops.mesh_simplify(verts, tris, tris.shape[0] // 5)
            runs.append([x.cpu().numpy().tobytes() for x in out[:4]] + [out[4]])
    assert runs[0] == runs[1] == runs[2]


def test_off_launches_nothing(dev, monkeypatch):
    v, f = U.cube10()
    verts, tris = torch.from_numpy(v.copy()).to(dev), _dev_tris(f, dev, torch.int64)

    class Dead:
        def __getattr__(self, name):
            pytest.fail(f"a target of 0 must not reach the library ({name})")
    monkeypatch.setattr(_lib, "_LIB", Dead())
    assert config.MESH_SIMPLIFY_FACES == 0 and config.MESH_SIMPLIFY_MAX_ERROR == INF         # the environment of the test run leaves them unset
    for target in (0, None):
        out = ops.mesh_simplify(verts, tris, target)
        assert out[0] is verts and out[1] is tris and out[2:] == (None, None, None)
    opts = config.mesh_options()
    assert opts.simplify_faces == 0
    cv, ct, info = ops.mesh_cleanup(verts, tris, opts, None, None, 64)
    assert cv is verts and ct is tris and info == {"components": None, "components_kept": None, "decimate": None, "simplify": None, "project": None}


def test_errors_are_statuses_not_faults(dev):
    """each refusal on a mesh of a few vertices: counted on the device, raised on the host, and the next call works"""
    v, f = U.fan(5)
    good, tris = torch.from_numpy(v).to(dev), _dev_tris(f, dev, torch.int64)
    for bad in (float("nan"), float("inf"), float("-inf")):
        w = good.clone()
        w[2, 1] = bad
        with pytest.raises(RuntimeError, match="non-finite"):
            ops.mesh_simplify(w, tris, 4)
    for bad in (v.shape[0], -1, 2 ** 31 + 1):
        t = tris.clone()
        t[1, 2] = bad
        with pytest.raises(RuntimeError, match="index outside"):
            ops.mesh_simplify(good, t, 4)
    t = tris.clone()
    t[3, 0] = t[3, 1]
    with pytest.raises(RuntimeError, match="repeat"):
        ops.mesh_simplify(good, t.to(torch.int32), 4)
    for kw in (dict(target_faces=-1), dict(target_faces=2.5), dict(target_faces=4, max_error=-1.0), dict(target_faces=4, max_error=float("nan")),
               dict(target_faces=4, max_rounds=-1)):
        with pytest.raises(ValueError):
            ops.mesh_simplify(good, tris, **kw)
    with pytest.raises(ValueError):
        ops.mesh_simplify(good, tris.float(), 4)
    with pytest.raises(ValueError):
        ops.mesh_simplify(good.float(), tris, 4)
    # the C ABI itself: null pointers, a short workspace, bad sizes
    L = _lib.lib()
    nv, nt = v.shape[0], f.shape[0]
    wsb = L.o2345_mesh_simplify_workspace_bytes(nv, nt)
    assert wsb > 0 and L.o2345_mesh_simplify_workspace_bytes(2 ** 30, 0) == 0 and L.o2345_mesh_simplify_workspace_bytes(-1, 0) == 0
    assert L.o2345_mesh_simplify_workspace_bytes(0, 2 ** 31 // 6 + 1) == 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stats = torch.empty(STATS_BYTES + 8 * 16, dtype=torch.uint8, device=dev)
    count = lambda *a: _lib.call("o2345_mesh_simplify_count", *a)
    for a, what in (((None, tris, 8, nv, nt, 4, INF, 16, ws, wsb, stats), "null pointer"), ((good, None, 8, nv, nt, 4, INF, 16, ws, wsb, stats), "null pointer"),
                    ((good, tris, 8, nv, nt, 4, INF, 16, None, wsb, stats), "null pointer"), ((good, tris, 8, nv, nt, 4, INF, 16, ws, wsb, None), "null pointer"),
                    ((good, tris, 8, nv, nt, 4, INF, 16, ws, wsb - 1, stats), "workspace too small"), ((good, tris, 2, nv, nt, 4, INF, 16, ws, wsb, stats), "index_bytes"),
                    ((good, tris, 8, nv, nt, -1, INF, 16, ws, wsb, stats), "target_faces"), ((good, tris, 8, nv, nt, 4, -1.0, 16, ws, wsb, stats), "max_error"),
                    ((good, tris, 8, 2 ** 30, nt, 4, INF, 16, ws, wsb, stats), "bad sizes")):
        with pytest.raises(RuntimeError, match=what):
            count(*a)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("o2345_mesh_simplify_emit", good, 8, nv, nt, None, None, None, None, None)
    _check(("fan", 5), v, f, dev, torch.int64, 4)


# ---- guard bands (tests/guard_util.py): every output, the stats block and the workspace at their EXACT sizes -----------------------------------------
def _guarded_run(g, dev, hv, hf, dtype, target, max_error, max_rounds):
    """The two-call protocol through the C ABI itself, every buffer carved at its exact size -> (verts, tris, source, merged, info) as numpy"""
    L = _lib.lib()
    nv, nt = hv.shape[0], hf.shape[0]
    ib = 8 if dtype == torch.int64 else 4
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    hv = np.array(hv, np.float64)
    tris, verts = _dev_tris(hf, dev, dtype), torch.from_numpy(hv).to(dev)
    wsb = L.o2345_mesh_simplify_workspace_bytes(nv, nt)
    assert wsb > 0 and PRE % 16 == 0
    ws = g.buf(wsb, ("workspace", nv, nt))
    stats = g.buf(STATS_BYTES + 8 * max_rounds, ("stats", nv, nt))
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.o2345_mesh_simplify_count(P(verts), P(tris), ib, nv, nt, target, max_error, max_rounds, ctypes.c_void_p(ws.data_ptr()), wsb,
                                           ctypes.c_void_p(stats.data_ptr()), s), "mesh_simplify_count")
    host = stats.cpu().numpy()
    assert list(_lib.read_struct("O2345SimplifyStats", host).reserved) == [0, 0, 0]
    info = ops.simplify_info(host)
    nvo, nto = info["vertices"], info["triangles"]
    vo, to = g.buf(24 * nvo, ("verts_out", nv, nt)), g.buf(3 * ib * nto, ("tris_out", nv, nt))
    so, me = g.buf(4 * nvo, ("source", nv, nt)), g.buf(4 * nv, ("merged", nv, nt))
    _lib.check(L.o2345_mesh_simplify_emit(P(verts), ib, nv, nt, ctypes.c_void_p(ws.data_ptr()), P(vo), P(to), P(so), P(me), s), "mesh_simplify_emit")
    h = lambda t, dt: t.cpu().numpy().view(dt)
    assert verts.cpu().numpy().tobytes() == hv.tobytes() and np.array_equal(tris.cpu().numpy(), hf)
    return h(vo, np.float64).reshape(-1, 3), h(to, np.int64 if ib == 8 else np.int32).reshape(-1, 3), h(so, np.int32), h(me, np.int32), info


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_kernel_writes_outside_its_buffers(dev, cut_mesh, dtype):
    g = Guard(dev)
    cv, cf = U.cube10()
    cases = [("cube", cv, cf, 240, INF, 256), ("cube", cv, cf, 0, 1e-9, 256), (("cut", 0.0), cut_mesh["hv"], cut_mesh["hf"], cut_mesh["hf"].shape[0] // 5, INF, 256),
             (("fan", 40, "e"), *U.fan(40), 0, 0.05, 256), ("sphere", *U.sphere20(), U.sphere20()[1].shape[0] // 20, INF, 5)]
    for n in SIZES:
        v, f = _sized(nv=n)
        cases.append((("nv", n), v, f, f.shape[0] // 3 if n > 9 else 1, INF, 256))
        v, f = _sized(nt=n)
        cases.append((("nt", n), v, f, n // 3 if n > 12 else 1, INF, 256))
    for key, hv, hf, target, max_error, max_rounds in cases:
        v, t, so, me, info = _guarded_run(g, dev, hv, hf, dtype, target, max_error, max_rounds)
        bad = g.damaged()
        assert not bad, bad
        wv, wf, _, wso, wme, winfo = _twin(key, hv, hf, target, max_error, max_rounds)
        assert info == winfo and v.tobytes() == np.ascontiguousarray(wv).tobytes() and np.array_equal(t, wf) and np.array_equal(so, wso) and np.array_equal(me, wme), key
    assert len(g.live) == 6 * len(cases)


# ---- the pipeline on the stored small scene (D = 20, R = 64) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev)
    nt = S["hf"].shape[0]
    assert nt > 100
    target = nt // 4
    twin = mio.simplify_mesh(S["hv"], S["hf"], target)
    assert 0 < twin[5]["triangles"] <= target and twin[5]["rounds"] > 0
    return dict(S, twin=twin, target=target)


def test_extract_mesh_with_simplification(scene):
    S = scene
    dev = S["plain"][0].device
    wv, wf, _, _, _, winfo = S["twin"]
    v, t, rgb, u = pipeline.extract_mesh(*_args(S), return_index_verts=True, simplify_faces=S["target"])
    assert v.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(t.cpu().numpy(), wf) and t.dtype == S["plain"][1].dtype and _bits(u, S["plain"][3])
    fields = pipeline._mesh_fields(*_args(S), config.mesh_options(simplify_faces=S["target"]))
    want_rgb, want_g = _fields_at(S, torch.from_numpy(wv).to(dev))          # gradient and colours are taken at the kept vertices
    assert _bits(rgb, want_rgb) and _bits(fields[3], want_rgb) and _bits(fields[5], want_g)
    assert fields.info["simplify"] == winfo and fields.info["decimate"] is None and fields.info["components"] is None


def test_exports_with_simplification_equal_the_export_of_the_twins_mesh(scene, tmp_path):
    S = scene
    dev = S["plain"][0].device
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 0.9; scale[:3, 3] = [0.01, 0.02, -0.03]
    B = lambda p: open(p, "rb").read()
    wv, wf = torch.from_numpy(S["twin"][0]).to(dev), torch.from_numpy(S["twin"][1]).to(dev)
    rgb = _fields_at(S, wv)[0]
    got, want = str(tmp_path / "g.ply"), str(tmp_path / "w.ply")
    n = pipeline.export_mesh_ply(got, *_args(S), scale_mat=scale[None], simplify_faces=S["target"])
    assert n == (S["twin"][5]["vertices"], S["twin"][5]["triangles"])
    assert n == mio.export_mesh(want, wv, wf, S["R"], scale_mat=scale[None], vertex_colors=rgb) and B(got) == B(want)
    for ext in (".glb", ".obj"):
        got, want = str(tmp_path / ("g" + ext)), str(tmp_path / ("w" + ext))
        assert pipeline.export_mesh_asset(got, *_args(S), scale_mat=scale[None], simplify_faces=S["target"]) == n
        mio.export_asset(want, wv, wf, S["R"], scale_mat=scale[None], vertex_colors=rgb)
        assert B(got) == B(want), ext


def test_simplification_off_is_todays_output(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    assert config.MESH_SIMPLIFY_FACES == 0                                # the environment of the test run leaves it unset
    monkeypatch.setattr(ops, "mesh_simplify", lambda *a, **k: pytest.fail("simplification must not run when it is off"))
    real = _lib.call
    monkeypatch.setattr(ops, "call", lambda name, *a: pytest.fail("the simplify entry was reached") if "simplify" in name else real(name, *a))
    for kw in (dict(simplify_faces=0), dict(simplify_faces=None), dict()):
        off = pipeline.extract_mesh(*_args(S), return_index_verts=True, **kw)
        for a, b in zip(S["plain"], off):
            assert _bits(a, b)
        assert pipeline._mesh_fields(*_args(S), config.mesh_options(**kw)).info["simplify"] is None
        for ext in (".ply", ".glb", ".obj"):
            p0, p1 = str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))
            fn = pipeline.export_mesh_ply if ext == ".ply" else pipeline.export_mesh_asset
            want = (mio.export_mesh if ext == ".ply" else mio.export_asset)(p0, S["plain"][0], S["plain"][1], S["R"], vertex_colors=S["plain"][2])
            assert fn(p1, *_args(S), **kw) == want
            assert B(p0) == B(p1)


def test_config_default_reaches_the_pipeline(scene, monkeypatch):
    S = scene
    monkeypatch.setattr(config, "MESH_SIMPLIFY_FACES", S["target"])
    v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True)
    assert v.cpu().numpy().tobytes() == S["twin"][0].tobytes() and np.array_equal(t.cpu().numpy(), S["twin"][1])
    off = pipeline.extract_mesh(*_args(S), return_index_verts=True, simplify_faces=0)                   # an explicit 0 wins
    for a, b in zip(S["plain"], off):
        assert _bits(a, b)
    monkeypatch.setattr(config, "MESH_SIMPLIFY_MAX_ROUNDS", 2)                                          # and so do the limits
    v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True)
    w = mio.simplify_mesh(S["hv"], S["hf"], S["target"], max_rounds=2)
    assert w[5]["stopped"] == "rounds" and v.cpu().numpy().tobytes() == w[0].tobytes() and np.array_equal(t.cpu().numpy(), w[1])


def test_reconstruct_folder_reports_the_target_and_the_counts(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64)
    assert plain["simplify_faces"] == 0 and plain["simplify"] is None and plain["triangles"] > 0
    target = plain["triangles"] // 4
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64, simplify_faces=target)
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    T = lambda t: t.to(dev).contiguous().float()
    vol = pipeline.build_volume(wt, T(s["images"]), T(s["affine_mats"]), s["partial_vol_origin"].numpy(), 48, 2.0 / 47)
    proj, cam_pos = pipeline.camera_terms(T(s["intrinsics"]), T(s["w2cs"]))
    v, t, _, _ = pipeline.extract_mesh(wt, vol, proj, cam_pos, 64, return_index_verts=True)
    winfo = mio.simplify_mesh(v.cpu().numpy(), t.cpu().numpy(), target)[5]
    assert out["simplify_faces"] == target and out["simplify"] == winfo
    assert (out["vertices"], out["triangles"]) == (winfo["vertices"], winfo["triangles"]) and 0 < out["triangles"] <= target
    assert (mio.read_ply(out["ply"])[0].shape[0], mio.read_ply(out["ply"])[1].shape[0]) == (winfo["vertices"], winfo["triangles"])


# ---- the drop-in mirror: the configured value alone, and every option at once ------------------------------------------------------------------------
def test_mirror_extract_geometry_applies_the_configured_simplification(dev, monkeypatch):
    ren, sdf, dense = golden_mirror(dev)
    R = 48
    call = lambda: ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=R, threshold=0, device=dev,
                                        conditional_volume=dense, lod=0)
    v0, t0, u0 = call()
    assert t0.shape[0] > 0
    vi, ti = ops.marching_cubes(torch.from_numpy(u0).to(dev).contiguous(), 0.0)
    hv, hf = vi.cpu().numpy(), ti.cpu().numpy()
    assert np.array_equal(hf, t0)
    target = hf.shape[0] // 4
    monkeypatch.setattr(config, "MESH_SIMPLIFY_FACES", target)
    v, t, u = call()
    wv, wf, _, _, _, winfo = mio.simplify_mesh(hv, hf, target)
    assert 0 < winfo["triangles"] <= target
    assert v.dtype == np.float64 and v.tobytes() == (wv / (R - 1) * 2.0 + -1.0).tobytes() and np.array_equal(t, wf) and u.tobytes() == u0.tobytes()
    # every option on at once: filter -> clustering -> collapse -> projection -> smoothing, the twins composed in that order
    monkeypatch.setattr(config, "MESH_KEEP_LARGEST", True)
    monkeypatch.setattr(config, "MESH_DECIMATE_CELL", 1.5)
    monkeypatch.setattr(config, "MESH_PROJECT_ITERATIONS", 4)
    monkeypatch.setattr(config, "MESH_SMOOTH_ITERATIONS", 3)
    assert config.MESH_PROJECT_MAX_MOVE is None
    fv, ff, _, _, _, _ = mio.filter_components(hv, hf, keep_largest=True)
    dv, df, _, _, dinfo = mio.decimate_mesh(fv, ff, 1.5)
    target = dinfo["triangles"] // 3
    monkeypatch.setattr(config, "MESH_SIMPLIFY_FACES", target)
    v, t, u = call()
    cv, cf, _, _, _, cinfo = mio.simplify_mesh(dv, df, target)
    field = sdf_field(sdf.sdf_layer.blob(), dense[0].permute(1, 2, 3, 0).contiguous(), None)
    pv, pinfo = mio.project_vertices(cv, field, R, 4, level=-0.0, max_move=1.5)
    sv = mio.smooth_vertices(pv, cf, 3)
    assert cinfo["rounds"] > 0 and 0 < cinfo["triangles"] < dinfo["triangles"] and pv.tobytes() != np.ascontiguousarray(cv).tobytes()
    want = sv / (R - 1) * 2.0 + -1.0
    assert v.dtype == np.float64 and v.shape == want.shape and v.tobytes() == want.tobytes() and np.array_equal(t, cf)
