"""GPU: the vertex adjacency table and Taubin smoothing (csrc/mesh_smooth.hip) against the host twin (mesh_io.vertex_adjacency / smooth_vertices), which
defines the result.  The table is integer work and the smoothing step a sum in a defined order: every comparison is EXACT (torch.equal / bytes).  Expected
values are the host twin applied to the same inputs, never the code under test."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mesh_components_util as mcu
import mesh_smooth_util as msu
from guard_util import Guard
from mesh_scene_util import args as _args, bits as _bits, dev, dev_tris as _dev_tris, golden_mirror, mc, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("one-2-3-45_amd")
ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

NTS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 4097)          # every block (256) and scan-tile (2048) boundary; from 17 triangles on a fan's centre is a long row


def _mc(dev, field):
    m = mc(dev, field)
    return dict(m, adj=mio.vertex_adjacency(m["hf"], m["hv"].shape[0]))


@pytest.fixture(scope="module")
def closed_mesh(dev):
    """HIP marching cubes of the three-spheres-and-specks field: closed surfaces, the 8-face octahedra included"""
    m = _mc(dev, mcu.spheres_field(40))
    deg = np.diff(m["adj"][0])
    assert m["hv"].shape[0] > 2000 and int(m["adj"][2].sum()) == 0 and 4 <= deg.min() and deg.max() <= 12, (m["hv"].shape, deg.min(), deg.max())
    return m


@pytest.fixture(scope="module")
def cut_mesh(dev):
    """HIP marching cubes of a sphere that the volume's face x = 23 cuts open: the rim is boundary"""
    m = _mc(dev, msu.cut_sphere_field(24))
    bnd = m["adj"][2].astype(bool)
    assert 0 < bnd.sum() < bnd.size and (m["hv"][bnd, 0] == 23.0).all(), (bnd.sum(), bnd.size)
    return m


def _check_adjacency(f, nv, dev, dtype, want=None):
    got = ops.mesh_vertex_adjacency(_dev_tris(f, dev, dtype), nv)
    want = mio.vertex_adjacency(f, nv) if want is None else want
    assert [g.dtype for g in got] == [torch.int32, torch.int32, torch.uint8]
    for g, w, what in zip(got, want, ("offsets", "neighbours", "boundary")):
        assert g.shape == w.shape, (what, g.shape, w.shape)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), what
    return got


def _check_smooth(hv, f, dev, dtype, iterations, **kw):
    verts = torch.from_numpy(np.ascontiguousarray(hv, np.float64)).to(dev)
    got = ops.mesh_smooth(verts, _dev_tris(f, dev, dtype), iterations, **kw)
    want = mio.smooth_vertices(hv, f, iterations, **{k: v for k, v in kw.items() if v is not None})
    assert got.dtype == torch.float64 and got.shape == verts.shape and got is not verts
    assert got.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes(), (iterations, kw)
    assert verts.cpu().numpy().tobytes() == np.ascontiguousarray(hv, np.float64).tobytes()          # the input is only read
    return got


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("which", ["closed", "cut"])
def test_marching_cubes_meshes(dev, closed_mesh, cut_mesh, which, dtype):
    m = closed_mesh if which == "closed" else cut_mesh
    _check_adjacency(m["hf"], m["hv"].shape[0], dev, dtype, m["adj"])
    for it in (1, 2, 5):
        moved = _check_smooth(m["hv"], m["hf"], dev, dtype, it)
        assert not torch.equal(moved, m["verts"])
    if which == "cut":
        _check_smooth(m["hv"], m["hf"], dev, dtype, 2, pin_boundary=False)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("kind", ["fan", "disjoint", "bipyramid"])
def test_every_block_and_tile_boundary_and_the_long_rows(dev, dtype, kind):
    rng = np.random.default_rng(6)
    for nt in NTS:
        f, nv = {"fan": mcu.fan, "disjoint": mcu.disjoint, "bipyramid": msu.bipyramid}[kind](nt)
        off, _, bnd = _check_adjacency(f, nv, dev, dtype)
        hv = rng.normal(size=(nv, 3))
        if kind == "fan":               # pinned, a fan does not move at all; unpinned, the centre's row of nt + 1 neighbours is summed in order
            assert nt == 0 or int(off[4] - off[3]) == nt + 1
            _check_smooth(hv, f, dev, dtype, 2, pin_boundary=False)
        elif kind == "bipyramid":       # closed: nothing is pinned, both apex rows are long
            assert int(bnd.sum()) == 0 and (nt < 3 or (int(off[1] - off[0]) == nt and int(off[2] - off[1]) == nt))
            _check_smooth(hv, f, dev, dtype, 2)
        else:
            _check_smooth(hv, f, dev, dtype, 1, pin_boundary=False)


def test_rows_around_the_register_sort_limit(dev):
    """fans whose centre has 16, 17, 32, 33, 34 raw entries (8 .. 17 triangles): both register networks, the last short row and the first long ones"""
    for nt in (7, 8, 9, 15, 16, 17, 33):
        f, nv = mcu.fan(nt)
        _check_adjacency(f, nv, dev, torch.int64)
        f2, nv2 = msu.bipyramid(nt)
        _check_adjacency(f2, nv2, dev, torch.int32)


@pytest.mark.parametrize("pin", [True, False])
def test_strip(dev, pin):
    f, nv = mcu.strip(100_000, True)
    hv = np.random.default_rng(8).normal(size=(nv, 3))
    _check_adjacency(f, nv, dev, torch.int64)
    _check_smooth(hv, f, dev, torch.int64, 3, pin_boundary=pin)


def test_step_parity_and_factors(dev, cut_mesh):
    """mu = 0 makes one launch per iteration: odd and even step counts end in verts_out all the same; lam = 1 moves a vertex onto its neighbours' mean"""
    m = cut_mesh
    for it in (1, 2, 3, 4):
        _check_smooth(m["hv"], m["hf"], dev, torch.int32, it, mu=0.0)
    for it in (1, 2):
        _check_smooth(m["hv"], m["hf"], dev, torch.int64, it, lam=1.0)
        _check_smooth(m["hv"], m["hf"], dev, torch.int64, it, lam=1.0, mu=0.0, pin_boundary=False)
    _check_smooth(m["hv"], m["hf"], dev, torch.int64, 3, lam=0.33, mu=-0.34)


def test_two_runs_give_identical_bytes(dev, closed_mesh):
    m = closed_mesh
    runs = []
    for _ in range(2):
        adj = ops.mesh_vertex_adjacency(m["tris"], m["hv"].shape[0])
        out = ops.mesh_smooth(m["verts"], m["tris"], 4)
        runs.append([x.cpu().numpy().tobytes() for x in (*adj, out)])
    assert runs[0] == runs[1]


def test_zero_iterations_launch_nothing(dev, closed_mesh, monkeypatch):
    m = closed_mesh

    class Dead:
        def __getattr__(self, name):
            pytest.fail(f"iterations = 0 must not reach the library ({name})")
    monkeypatch.setattr(_lib, "_LIB", Dead())
    assert ops.mesh_smooth(m["verts"], m["tris"], 0) is m["verts"]
    monkeypatch.setattr(config, "MESH_SMOOTH_ITERATIONS", 0)
    assert ops.mesh_smooth(m["verts"], m["tris"], None) is m["verts"]


def test_bad_arguments(dev, closed_mesh):
    tris = torch.tensor([[0, 1, 2], [1, 2, 9]], device=dev)
    with pytest.raises(RuntimeError, match="index outside"):
        ops.mesh_vertex_adjacency(tris, 4)
    with pytest.raises(RuntimeError, match="index outside"):
        ops.mesh_smooth(torch.zeros(4, 3, dtype=torch.float64, device=dev), tris, 1)
    m = closed_mesh
    for kw in (dict(iterations=-1), dict(iterations=1, lam=0.0), dict(iterations=1, mu=0.2), dict(iterations=1.5)):
        with pytest.raises(ValueError):
            ops.mesh_smooth(m["verts"], m["tris"], **kw)
    with pytest.raises(ValueError):
        ops.mesh_vertex_adjacency(m["tris"].float(), 4)


# ---- guard bands (tests/guard_util.py): every output and the workspace at their EXACT sizes ---------------------------------------------------------
def _guarded_run(g, dev, hv, hf, dtype, iterations, mu, pin):
    """Both protocols through the C ABI itself, every buffer carved at its exact size -> (offsets, neighbours, boundary, verts_out) as numpy"""
    L = _lib.lib()
    nv, nt = hv.shape[0], hf.shape[0]
    ib = 8 if dtype == torch.int64 else 4
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    tris, verts = _dev_tris(hf, dev, dtype), torch.from_numpy(np.ascontiguousarray(hv, np.float64)).to(dev)
    wsb = L.o2345_mesh_adjacency_workspace_bytes(nv, nt)
    ws = g.buf(wsb, ("workspace", nv, nt))
    ne = ctypes.c_longlong()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.o2345_mesh_adjacency_count(P(tris), ib, nv, nt, ctypes.c_void_p(ws.data_ptr()), wsb, ctypes.byref(ne), s), "mesh_adjacency_count")
    off, nbr, bnd = g.buf(4 * (nv + 1), ("offsets", nv, nt)), g.buf(4 * ne.value, ("neighbours", nv, nt)), g.buf(nv, ("boundary", nv, nt))
    _lib.check(L.o2345_mesh_adjacency_emit(ctypes.c_void_p(ws.data_ptr()), nv, P(off), P(nbr), P(bnd), s), "mesh_adjacency_emit")
    tmp, out = g.buf(24 * nv, ("verts_tmp", nv, nt)), g.buf(24 * nv, ("verts_out", nv, nt))
    _lib.check(L.o2345_mesh_smooth(P(verts), nv, P(off), P(nbr), P(bnd) if pin else None, iterations, 0.5, mu, P(tmp), P(out), s), "mesh_smooth")
    h = lambda t, dt: t.cpu().numpy().view(dt)
    assert verts.cpu().numpy().tobytes() == np.ascontiguousarray(hv, np.float64).tobytes()
    return h(off, np.int32), h(nbr, np.int32), h(bnd, np.uint8), h(out, np.float64).reshape(-1, 3)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_kernel_writes_outside_its_buffers(dev, closed_mesh, cut_mesh, dtype):
    g = Guard(dev)
    cases = [(m["hv"], m["hf"], kw) for m in (closed_mesh, cut_mesh) for kw in ((1, -0.53, True), (2, 0.0, True), (3, 0.0, False), (0, -0.53, True))]
    rng = np.random.default_rng(3)
    for nt in NTS:
        for make, kw in ((mcu.fan, (1, -0.53, False)), (mcu.disjoint, (1, 0.0, False)), (msu.bipyramid, (2, -0.53, True))):
            f, nv = make(nt)
            cases.append((rng.normal(size=(nv, 3)), f, kw))
    for hv, hf, (iterations, mu, pin) in cases:
        off, nbr, bnd, out = _guarded_run(g, dev, hv, hf, dtype, iterations, mu, pin)
        bad = g.damaged()
        assert not bad, bad
        woff, wnbr, wbnd = mio.vertex_adjacency(hf, hv.shape[0])
        assert np.array_equal(off, woff) and np.array_equal(nbr, wnbr) and np.array_equal(bnd, wbnd)
        want = mio.smooth_vertices(hv, hf, iterations, mu=mu, pin_boundary=pin)
        assert out.tobytes() == np.ascontiguousarray(want, np.float64).tobytes(), (hv.shape, iterations, mu, pin)
    assert len(g.live) == 6 * len(cases)


# ---- the pipeline on the stored small scene (D = 20, R = 64) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev)
    assert S["hf"].shape[0] > 100
    return S


def test_extract_mesh_with_smoothing(scene):
    S = scene
    pv, pt, prgb, pu = S["plain"]
    v, t, rgb, u = pipeline.extract_mesh(*_args(S), return_index_verts=True, smooth_iterations=3)
    assert _bits(t, pt) and _bits(rgb, prgb) and _bits(u, pu)          # colours are taken at the unsmoothed vertices
    want = mio.smooth_vertices(S["hv"], S["hf"], 3)
    assert v.cpu().numpy().tobytes() == want.tobytes() and not torch.equal(v, pv)
    # world-frame vertices: the same elementwise expression on the smoothed index coordinates
    vw = pipeline.extract_mesh(*_args(S), smooth_iterations=3)[0]
    assert torch.equal(vw, v / (S["R"] - 1.0) * 2.0 - 1.0)
    # with the component filter: filter, then twin
    v, t, rgb, u = pipeline.extract_mesh(*_args(S), return_index_verts=True, keep_largest=True, smooth_iterations=3)
    fv, ff, _, _, kept, _ = mio.filter_components(S["hv"], S["hf"], keep_largest=True)
    assert v.cpu().numpy().tobytes() == mio.smooth_vertices(fv, ff, 3).tobytes() and np.array_equal(t.cpu().numpy(), ff)
    assert _bits(rgb, prgb[torch.from_numpy(kept).to(prgb.device).long()])


def test_exports_with_smoothing_equal_the_export_of_the_twins_vertices(scene, tmp_path):
    S = scene
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 0.9; scale[:3, 3] = [0.01, 0.02, -0.03]
    B = lambda p: open(p, "rb").read()
    pv, pt, prgb, _ = S["plain"]
    sv = torch.from_numpy(mio.smooth_vertices(S["hv"], S["hf"], 3)).to(pv.device)
    got, want = str(tmp_path / "g.ply"), str(tmp_path / "w.ply")
    n = pipeline.export_mesh_ply(got, *_args(S), scale_mat=scale[None], smooth_iterations=3)
    assert n == mio.export_mesh(want, sv, pt, S["R"], scale_mat=scale[None], vertex_colors=prgb) and B(got) == B(want)
    plain = str(tmp_path / "p.ply")
    pipeline.export_mesh_ply(plain, *_args(S), scale_mat=scale[None])
    assert B(plain) != B(got)
    for ext in (".glb", ".obj"):
        got, want = str(tmp_path / ("g" + ext)), str(tmp_path / ("w" + ext))
        assert pipeline.export_mesh_asset(got, *_args(S), scale_mat=scale[None], smooth_iterations=3) == n
        mio.export_asset(want, sv, pt, S["R"], scale_mat=scale[None], vertex_colors=prgb)
        assert B(got) == B(want), ext


def test_smoothing_off_is_todays_output(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    assert config.MESH_SMOOTH_ITERATIONS == 0                            # the environment of the test run leaves it unset
    monkeypatch.setattr(ops, "mesh_smooth", lambda *a, **k: pytest.fail("smoothing must not run when it is off"))
    monkeypatch.setattr(ops, "mesh_vertex_adjacency", lambda *a, **k: pytest.fail("no adjacency is built when smoothing is off"))
    for kw in (dict(smooth_iterations=0), dict(smooth_iterations=None), dict()):
        off = pipeline.extract_mesh(*_args(S), return_index_verts=True, **kw)
        for a, b in zip(S["plain"], off):
            assert _bits(a, b)
        for ext in (".ply", ".glb", ".obj"):
            p0, p1 = str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))
            fn = pipeline.export_mesh_ply if ext == ".ply" else pipeline.export_mesh_asset
            want = (mio.export_mesh if ext == ".ply" else mio.export_asset)(p0, S["plain"][0], S["plain"][1], S["R"], vertex_colors=S["plain"][2])
            assert fn(p1, *_args(S), **kw) == want
            assert B(p0) == B(p1)


def test_config_default_reaches_the_pipeline(scene, monkeypatch):
    S = scene
    monkeypatch.setattr(config, "MESH_SMOOTH_ITERATIONS", 2)
    v, t, rgb, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True)
    assert v.cpu().numpy().tobytes() == mio.smooth_vertices(S["hv"], S["hf"], 2).tobytes() and _bits(t, S["plain"][1]) and _bits(rgb, S["plain"][2])
    # lambda, mu and pinning come from config as well
    monkeypatch.setattr(config, "MESH_SMOOTH_LAMBDA", 0.4)
    monkeypatch.setattr(config, "MESH_SMOOTH_MU", 0.0)
    monkeypatch.setattr(config, "MESH_SMOOTH_PIN_BOUNDARY", False)
    v = pipeline.extract_mesh(*_args(S), return_index_verts=True)[0]
    assert v.cpu().numpy().tobytes() == mio.smooth_vertices(S["hv"], S["hf"], 2, lam=0.4, mu=0.0, pin_boundary=False).tobytes()
    # an explicit 0 wins over the configured default
    v0 = pipeline.extract_mesh(*_args(S), return_index_verts=True, smooth_iterations=0)[0]
    assert _bits(v0, S["plain"][0])


def test_reconstruct_folder_reports_the_count_and_writes_the_twins_file(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64)
    assert plain["smooth_iterations"] == 0
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64, smooth_iterations=2)
    assert out["smooth_iterations"] == 2 and (out["vertices"], out["triangles"]) == (plain["vertices"], plain["triangles"]) and out["triangles"] > 0
    # the file of the twin's vertices: the same scene once more through the pieces, smoothed on the host in between
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    T = lambda t: t.to(dev).contiguous().float()
    vol = pipeline.build_volume(wt, T(s["images"]), T(s["affine_mats"]), s["partial_vol_origin"].numpy(), 48, 2.0 / 47)
    proj, cam_pos = pipeline.camera_terms(T(s["intrinsics"]), T(s["w2cs"]))
    v, t, rgb, _ = pipeline.extract_mesh(wt, vol, proj, cam_pos, 64, return_index_verts=True)
    sv = torch.from_numpy(mio.smooth_vertices(v.cpu().numpy(), t.cpu().numpy(), 2)).to(dev)
    want = str(tmp_path / "want.ply")
    mio.export_mesh(want, sv, t, 64, scale_mat=s["scale_mat"], trans_mat=s["trans_mat"], vertex_colors=rgb)
    B = lambda p: open(p, "rb").read()
    assert B(out["ply"]) == B(want) != B(plain["ply"])


# ---- the drop-in mirror ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_extract_geometry_applies_the_configured_smoothing(dev, monkeypatch):
    ren, sdf, dense = golden_mirror(dev)
    R = 48
    call = lambda: ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=R, threshold=0, device=dev,
                                        conditional_volume=dense, lod=0)
    v0, t0, u0 = call()
    assert t0.shape[0] > 0
    # the mirror smooths INDEX coordinates and maps them to world units afterwards: the twin on its own unsmoothed output, taken back to index coordinates
    # by the step it can observe (marching cubes alone), mapped forward by the expression of the reference (sparse_neus_renderer.py:936)
    vi, ti = ops.marching_cubes(torch.from_numpy(u0).to(dev).contiguous(), 0.0)
    hv, hf = vi.cpu().numpy(), ti.cpu().numpy()
    assert np.array_equal(hf, t0) and (hv / (R - 1) * 2.0 + -1.0).tobytes() == v0.tobytes()
    for it in (1, 4):
        monkeypatch.setattr(config, "MESH_SMOOTH_ITERATIONS", it)
        v, t, u = call()
        want = mio.smooth_vertices(hv, hf, it) / (R - 1) * 2.0 + -1.0
        assert v.dtype == np.float64 and v.tobytes() == want.tobytes() and np.array_equal(t, t0) and u.tobytes() == u0.tobytes()
        assert v.tobytes() != v0.tobytes()
