"""GPU: connected components of a mesh and the component filter (csrc/mesh_components.hip) against the host twin (mesh_io.component_labels /
filter_components), which defines the result.  Integer / topology work: every comparison is EXACT (torch.equal / bytes).  Expected values are the host
twin applied to the same HIP marching-cubes output, never the code under test."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import mesh_components_util as mcu
from guard_util import Guard
from mesh_scene_util import args as _args, dev, dev_tris as _dev_tris, golden_mirror, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("one-2-3-45_amd")
ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

NTS = (0, 1, 255, 256, 257, 2047, 2048, 2049, 4097)          # every block (256) and scan-tile (2048) boundary of the kernels


@pytest.fixture(scope="module")
def field_mesh(dev):
    """(a): HIP marching cubes of the three-spheres-and-specks field -> device tensors, host copies and the host twin's labels."""
    u = torch.from_numpy(np.array(mcu.spheres_field(40))).to(dev)
    verts, tris = ops.marching_cubes(u, 0.0)
    hv, hf = verts.cpu().numpy(), tris.cpu().numpy()
    lab = mio.component_labels(hf, hv.shape[0])
    sizes = np.sort(np.bincount(lab[hf[:, 0]], minlength=hv.shape[0])[np.unique(lab)])[::-1]
    assert len(sizes) >= 10 and sizes[0] > sizes[1] > 100 and sizes[-1] == 8, sizes          # not vacuous: three big surfaces, a dozen octahedra
    return dict(verts=verts, tris=tris, hv=hv, hf=hf, lab=lab, sizes=sizes)


def _check_labels(f, nv, dev, dtype, want=None):
    got = ops.mesh_component_labels(_dev_tris(f, dev, dtype), nv)
    want = mio.component_labels(f, nv) if want is None else want
    assert got.dtype == torch.int32 and got.shape == (nv,)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    return got


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_labels_on_a_marching_cubes_mesh(dev, field_mesh, dtype):
    m = field_mesh
    _check_labels(m["hf"], m["hv"].shape[0], dev, dtype, m["lab"])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("permuted", [True, False])
def test_labels_on_the_strip(dev, dtype, permuted):
    """200,000 triangles in a row: natural order builds the deepest parent chains (a find that does not terminate, or a hook that loses an edge, shows
    here), the permuted ids make every union meet unrelated indices."""
    f, nv = mcu.strip(100_000, permuted)
    got = _check_labels(f, nv, dev, dtype, np.zeros(nv, np.int32))
    assert not got.any()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("kind", ["fan", "disjoint"])
def test_labels_at_every_block_and_tile_boundary(dev, dtype, kind):
    for nt in NTS:
        f, nv = (mcu.fan if kind == "fan" else mcu.disjoint)(nt)
        _check_labels(f, nv, dev, dtype)


def _filter_both(verts, tris, hv, hf, **kw):
    """device filter and host twin on the same mesh; asserts equality of everything and returns the device outputs"""
    v, t, kept, info = ops.mesh_filter_components(verts, tris, **kw)
    wv, wf, _, _, wkept, winfo = mio.filter_components(hv, hf, **kw)
    assert v.dtype == torch.float64 and t.dtype == tris.dtype and kept.dtype == torch.int32
    assert v.shape == wv.shape and t.shape == wf.shape and kept.shape == wkept.shape, (v.shape, wv.shape, t.shape, wf.shape)
    assert v.cpu().numpy().tobytes() == np.ascontiguousarray(wv).tobytes()
    assert torch.equal(t.cpu().to(torch.int64), torch.from_numpy(np.ascontiguousarray(wf)).to(torch.int64))
    assert torch.equal(kept.cpu(), torch.from_numpy(wkept))
    assert info == winfo, (info, winfo)
    return v, t, kept, info


@pytest.mark.parametrize("keep_largest", [False, True])
@pytest.mark.parametrize("min_faces", [1, 9, 100, 10 ** 9])
def test_filter_equals_the_host_twin(dev, field_mesh, min_faces, keep_largest):
    m = field_mesh
    v, t, kept, info = _filter_both(m["verts"], m["tris"], m["hv"], m["hf"], min_faces=min_faces, keep_largest=keep_largest)
    n_big = int((m["sizes"] >= max(min_faces, 1)).sum())
    assert info["components"] == len(m["sizes"]) and info["components_kept"] == (min(n_big, 1) if keep_largest else n_big)
    assert t.shape[0] == (int(m["sizes"][0]) if keep_largest and n_big else int(m["sizes"][m["sizes"] >= max(min_faces, 1)].sum()))
    t32 = m["tris"].to(torch.int32)
    _filter_both(m["verts"], t32, m["hv"], m["hf"].astype(np.int32), min_faces=min_faces, keep_largest=keep_largest)


def test_tie_for_largest_goes_to_the_smaller_label(dev, field_mesh):
    """The largest surface twice: once where marching cubes put it, once appended with shifted indices.  Two components of equal size: the original
    (smaller label) must win, on the device as on the host."""
    m = field_mesh
    nv, lab, hf, hv = m["hv"].shape[0], m["lab"], m["hf"], m["hv"]
    big = np.bincount(lab[hf[:, 0]], minlength=nv).argmax()
    dup_f = hf[lab[hf[:, 0]] == big] + nv                                       # indices into a second copy of the whole vertex array
    hv2, hf2 = np.concatenate([hv, hv + 100.0]), np.concatenate([dup_f[:7], hf, dup_f[7:]])       # the copy's faces come FIRST and last in face order
    verts2, tris2 = torch.from_numpy(hv2).to(dev), torch.from_numpy(hf2).to(dev)
    for kw in (dict(min_faces=100, keep_largest=True), dict(keep_largest=True)):
        v, t, kept, info = _filter_both(verts2, tris2, hv2, hf2, **kw)
        assert info["components_kept"] == 1 and t.shape[0] == m["sizes"][0] and int(kept.max()) < nv and int(kept.min()) == big
    # without keep_largest both copies survive the threshold
    v, t, kept, info = _filter_both(verts2, tris2, hv2, hf2, min_faces=int(m["sizes"][0]))
    assert info["components_kept"] == 2 and int(kept.max()) >= nv


def test_nothing_selected_returns_the_inputs(dev, field_mesh):
    m = field_mesh
    v, t, kept, info = ops.mesh_filter_components(m["verts"], m["tris"])
    assert v is m["verts"] and t is m["tris"] and kept is None and info is None


def test_strip_twice_gives_identical_bytes(dev):
    f, nv = mcu.strip(100_000, True)
    tris = _dev_tris(f, dev, torch.int64)
    verts = torch.arange(3 * nv, dtype=torch.float64, device=dev).view(nv, 3)
    runs = []
    for _ in range(2):
        lab = ops.mesh_component_labels(tris, nv)
        v, t, kept, info = ops.mesh_filter_components(verts, tris, keep_largest=True)
        runs.append([x.cpu().numpy().tobytes() for x in (lab, v, t, kept)] + [info])
    assert runs[0] == runs[1]
    assert runs[0][4] == {"components": 1, "components_kept": 1} and runs[0][1] == verts.cpu().numpy().tobytes() and runs[0][2] == f.tobytes()


def test_out_of_range_triangle_is_an_error(dev):
    tris = torch.tensor([[0, 1, 2], [1, 2, 9]], device=dev)
    with pytest.raises(RuntimeError, match="index outside"):
        ops.mesh_component_labels(tris, 4)


# ---- guard bands (tests/guard_util.py): every output and the workspace at their EXACT sizes ---------------------------------------------------------
def _guarded_run(g, dev, hv, hf, dtype, min_faces, keep_largest):
    """The two-call protocol through the C ABI itself, every buffer carved at its exact size -> (labels, verts, tris, kept) as numpy"""
    L = _lib.lib()
    nv, nt = hv.shape[0], hf.shape[0]
    ib = 8 if dtype == torch.int64 else 4
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    tris, verts = _dev_tris(hf, dev, dtype), torch.from_numpy(np.ascontiguousarray(hv, np.float64)).to(dev)
    wsb = L.o2345_mesh_components_workspace_bytes(nv, nt)
    ws, labels = g.buf(wsb, ("workspace", nv, nt)), g.buf(4 * nv, ("labels", nv, nt))
    out = [ctypes.c_longlong() for _ in range(4)]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.o2345_mesh_components_count(P(tris), ib, nv, nt, min_faces, int(keep_largest), ctypes.c_void_p(ws.data_ptr()), wsb, P(labels),
                                             *[ctypes.byref(o) for o in out], s), "mesh_components_count")
    nvk, ntk = out[2].value, out[3].value
    vo, to, ko = g.buf(24 * nvk, ("verts_out", nv, nt)), g.buf(3 * ib * ntk, ("tris_out", nv, nt)), g.buf(4 * nvk, ("kept_out", nv, nt))
    _lib.check(L.o2345_mesh_components_emit(P(verts), P(tris), ib, nv, nt, ctypes.c_void_p(ws.data_ptr()), P(vo), P(to), P(ko), s), "mesh_components_emit")
    h = lambda t, dt: t.cpu().numpy().view(dt)
    return h(labels, np.int32), h(vo, np.float64).reshape(-1, 3), h(to, np.int64 if ib == 8 else np.int32).reshape(-1, 3), h(ko, np.int32)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_component_kernel_writes_outside_its_buffers(dev, field_mesh, dtype):
    g = Guard(dev)
    cases = [(field_mesh["hv"], field_mesh["hf"], kw) for kw in ((0, False), (9, False), (1, True), (10 ** 9, True))]
    rng = np.random.default_rng(3)
    for nt in NTS:
        for make, kw in ((mcu.fan, (1, False)), (mcu.disjoint, (1, True)), (mcu.disjoint, (2, False))):
            f, nv = make(nt)
            cases.append((rng.normal(size=(nv, 3)), f, kw))
    for hv, hf, (min_faces, keep_largest) in cases:
        lab, v, t, kept = _guarded_run(g, dev, hv, hf, dtype, min_faces, keep_largest)
        bad = g.damaged()
        assert not bad, bad
        wv, wf, _, _, wkept, _ = mio.filter_components(hv, hf, min_faces=min_faces, keep_largest=keep_largest)
        assert np.array_equal(lab, mio.component_labels(hf, hv.shape[0])) and np.array_equal(kept, wkept)
        assert v.tobytes() == np.ascontiguousarray(wv, np.float64).tobytes() and np.array_equal(t, wf)
    assert len(g.live) == 5 * len(cases)


# ---- the pipeline on the stored small scene (D = 20, R = 64) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev)
    lab = mio.component_labels(S["hf"], S["hv"].shape[0])
    assert len(np.unique(lab)) >= 2, "the scene's mesh must have floaters for these tests to mean anything"
    return S


def test_extract_mesh_with_the_filter(scene):
    S = scene
    pv, pt, prgb, pu = S["plain"]
    for kw in (dict(keep_largest=True), dict(min_component_faces=100), dict(min_component_faces=10, keep_largest=True)):
        v, t, rgb, u = pipeline.extract_mesh(*_args(S), return_index_verts=True, **kw)
        wv, wf, _, _, kept, info = mio.filter_components(S["hv"], S["hf"], min_faces=kw.get("min_component_faces", 0), keep_largest=kw.get("keep_largest", False))
        assert 0 < wf.shape[0] < S["hf"].shape[0]
        assert v.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(t.cpu().numpy(), wf) and torch.equal(u, pu)
        # a vertex's colour does not depend on which other vertices are in the call
        assert rgb.shape == (len(kept), 3) and torch.equal(rgb.view(torch.int32), prgb[torch.from_numpy(kept).to(prgb.device).long()].view(torch.int32))
        # world-frame vertices: the same elementwise expression on the kept rows
        vw = pipeline.extract_mesh(*_args(S), **kw)[0]
        full = pipeline.extract_mesh(*_args(S))[0]
        assert torch.equal(vw, full[torch.from_numpy(kept).to(full.device).long()])


def test_exports_with_the_filter_equal_the_host_conversion(scene, tmp_path):
    S = scene
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 0.9; scale[:3, 3] = [0.01, 0.02, -0.03]
    B = lambda p: open(p, "rb").read()
    plain_ply = str(tmp_path / "plain.ply")
    pipeline.export_mesh_ply(plain_ply, *_args(S), scale_mat=scale[None])
    for i, kw in enumerate((dict(keep_largest=True), dict(min_component_faces=100))):
        host_kw = dict(min_faces=kw.get("min_component_faces", 0), keep_largest=kw.get("keep_largest", False))
        ply = str(tmp_path / f"f{i}.ply")
        nv, nt = pipeline.export_mesh_ply(ply, *_args(S), scale_mat=scale[None], **kw)
        rv, rf, rc = mio.read_ply(plain_ply)
        fv, ff, fc, _, kept, _ = mio.filter_components(rv, rf, rc, **host_kw)
        assert (nv, nt) == (fv.shape[0], ff.shape[0]) and 0 < nt < rf.shape[0]
        want = str(tmp_path / f"w{i}.ply")
        mio.write_ply(want, fv, ff, fc)
        assert B(ply) == B(want)
        for ext in (".glb", ".obj"):
            out, host = str(tmp_path / f"f{i}{ext}"), str(tmp_path / f"h{i}{ext}")
            assert pipeline.export_mesh_asset(out, *_args(S), scale_mat=scale[None], **kw) == (nv, nt)
            mio.convert_mesh(plain_ply, host, min_component_faces=host_kw["min_faces"], keep_largest=host_kw["keep_largest"])
            assert B(out) == B(host), (kw, ext)


def test_filter_off_is_todays_output(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    monkeypatch.setattr(ops, "mesh_filter_components", lambda *a, **k: pytest.fail("the filter must not run when nothing is selected"))
    off = pipeline.extract_mesh(*_args(S), return_index_verts=True, min_component_faces=0, keep_largest=False)
    for a, b in zip(S["plain"], off):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for ext in (".ply", ".glb", ".obj"):
        p0, p1 = str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))
        fn = pipeline.export_mesh_ply if ext == ".ply" else pipeline.export_mesh_asset
        assert fn(p0, *_args(S)) == fn(p1, *_args(S), min_component_faces=0, keep_largest=False)
        assert B(p0) == B(p1)


def test_config_defaults_reach_the_pipeline(scene, monkeypatch):
    S = scene
    monkeypatch.setattr(config, "MESH_KEEP_LARGEST", True)
    v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True)
    wv, wf, _, _, _, _ = mio.filter_components(S["hv"], S["hf"], keep_largest=True)
    assert v.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(t.cpu().numpy(), wf)
    # an explicit argument wins over the configured default
    v0, t0, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, keep_largest=False)
    assert torch.equal(v0, S["plain"][0]) and torch.equal(t0, S["plain"][1])


def test_reconstruct_folder_reports_the_components(tmp_path):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(torch.device("cuda:0"), seed=0)
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64)
    assert plain["components"] is None and plain["components_kept"] is None
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64, keep_largest=True)
    rv, rf, rc = mio.read_ply(plain["ply"])
    fv, ff, fc, _, _, info = mio.filter_components(rv, rf, rc, keep_largest=True)
    assert out["components"] == info["components"] >= 1 and out["components_kept"] == info["components_kept"] == 1
    assert (out["vertices"], out["triangles"]) == (fv.shape[0], ff.shape[0])
    want = str(tmp_path / "want.ply")
    mio.write_ply(want, fv, ff, fc)
    assert open(out["ply"], "rb").read() == open(want, "rb").read()


# ---- the drop-in mirror ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_extract_geometry_applies_the_configured_filter(dev, monkeypatch):
    ren, sdf, dense = golden_mirror(dev)
    call = lambda: ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=48, threshold=0, device=dev,
                                        conditional_volume=dense, lod=0)
    v0, t0, u0 = call()
    assert t0.shape[0] > 0
    lab = mio.component_labels(t0, v0.shape[0])
    sizes = np.sort(np.bincount(lab[t0[:, 0]], minlength=v0.shape[0])[np.unique(lab)])[::-1]
    for min_faces, keep_largest in ((0, True), (int(sizes[0]), False), (int(sizes[0]) + 1, False)):
        monkeypatch.setattr(config, "MESH_MIN_COMPONENT_FACES", min_faces)
        monkeypatch.setattr(config, "MESH_KEEP_LARGEST", keep_largest)
        v, t, u = call()
        wv, wf, _, _, _, _ = mio.filter_components(v0, t0, min_faces=min_faces, keep_largest=keep_largest)
        assert v.dtype == np.float64 and t.dtype == t0.dtype and v.tobytes() == wv.tobytes() and np.array_equal(t, wf)
        assert u.tobytes() == u0.tobytes()
        assert (t.shape[0] == 0) == (min_faces > sizes[0])
