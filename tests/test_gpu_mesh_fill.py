"""GPU: the hole filling (csrc/mesh_fill.hip) against the host twin (mesh_io.fill_holes), which defines the result: vertices, triangles, hole numbers and
the eight counts are compared EXACTLY (bytes).  Expected values are the twin applied to the same inputs, never the code under test; a twin result is
computed once per mesh (mesh_fill_util.twin) and left unchanged."""
import importlib

import numpy as np
import pytest
import torch

import mesh_fill_util as U
from guard_util import PRE, Guard
from mesh_scene_util import args as _args, bits as _bits, dev, dev_tris as _dev_tris, fields_at as _fields_at, golden_mirror, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")


def _equal(got, want, dtype):
    """(verts, tris, hole, info) of the device == the twin's, to the bit"""
    wv, wf, _, _, whole, winfo = want
    gv, gf, ghole, ginfo = got
    assert ginfo == winfo and all(type(x) is int for x in ginfo.values())
    assert gv.dtype == torch.float64 and gf.dtype == dtype and ghole.dtype == torch.int32
    assert gv.cpu().numpy().tobytes() == np.ascontiguousarray(wv, np.float64).tobytes()
    assert gf.cpu().numpy().tobytes() == np.ascontiguousarray(wf).astype(gf.cpu().numpy().dtype).tobytes()
    assert ghole.cpu().numpy().tobytes() == whole.tobytes()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_every_mesh_equals_the_twin(dev, dtype):
    """every case of mesh_fill_util: holes of 3, 4, 10, 40, 255, 256, 257, 300 and 1,402 edges (more than a block of threads, more than 1,024), twenty holes
    at once, a hole too long next to one that is filled, chains at a bow-tie, at a non-manifold edge and at a reversed triangle, no boundary at all,
    nt = 0, 1, 255, 256, 257; twice, with identical bytes; the inputs are only read; the audit of the result"""
    for name, (hv, hf, n) in U.cases().items():
        verts, tris = torch.from_numpy(hv.copy()).to(dev), _dev_tris(hf, dev, dtype)
        tris0 = tris.clone()
        got = ops.mesh_fill_holes(verts, tris, n)
        _equal(got, U.twin(name), dtype)
        again = ops.mesh_fill_holes(verts, tris, n)
        same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()      # empty ones too
        assert all(same(a, b) for a, b in zip(got[:3], again[:3])) and got[3] == again[3]
        assert verts.cpu().numpy().tobytes() == hv.tobytes() and torch.equal(tris, tris0)
        if name in U.TABLE:
            assert U.counts(got[3], hv.shape[0], hf.shape[0]) == U.TABLE[name]
        if got[3]["boundary"] == 0:
            assert got[0] is verts and got[1] is tris and got[2].shape == (0,)
        if hf.shape[0]:
            report = ops.mesh_audit(got[0], got[1])
            assert report["boundary_edges"] == got[3]["boundary"] - sum(3 if k == 1 else int(k) for k in np.bincount(U.twin(name)[4]))
            if name in U.MANIFOLD:
                assert report["boundary_edges"] == 0 and report["watertight"]


def test_off_launches_nothing(dev, monkeypatch):
    hv, hf, _ = U.cases()["cube_open"]
    verts, tris = torch.from_numpy(hv.copy()).to(dev), _dev_tris(hf, dev, torch.int64)
    monkeypatch.setattr(ops, "call", lambda name, *a: pytest.fail("an entry was reached with the stage off"))
    assert config.MESH_FILL_HOLES == 0
    for n in (None, 0):
        out = ops.mesh_fill_holes(verts, tris, n)
        assert out[0] is verts and out[1] is tris and out[2] is None and out[3] is None
    monkeypatch.undo()
    for bad in (1, 2, -1):
        with pytest.raises(ValueError):
            ops.mesh_fill_holes(verts, tris, bad)
    with pytest.raises(ValueError):
        ops.mesh_fill_holes(verts.float(), tris, 3)
    with pytest.raises(ValueError):
        ops.mesh_fill_holes(verts, tris.float(), 3)


def _raw(dev, hv, hf, n, dtype, g, outputs=(True, True, True)):
    """the two entries themselves, every buffer at its exact size inside guard bands -> (counts, verts_out, tris_out, hole) as numpy"""
    nv, nt = hv.shape[0], hf.shape[0]
    ib = 8 if dtype == torch.int64 else 4
    np_idx = np.int64 if ib == 8 else np.int32
    verts = g.buf(np.ascontiguousarray(hv, np.float64), ("verts", nv)).view(torch.float64)
    tris = g.buf(np.ascontiguousarray(hf, np_idx), ("tris", nt)).view(dtype)
    wsb = _lib.call("o2345_mesh_fill_workspace_bytes", nv, nt)
    assert wsb > 0 and PRE % 16 == 0
    ws = g.buf(wsb, ("workspace", nv, nt))
    counts = g.buf(64, ("counts", nv, nt)).view(torch.int64)
    torch.cuda.synchronize()
    _lib.call("o2345_mesh_fill_count", tris, ib, nv, nt, n, ws, wsb, counts)
    c = counts.tolist()
    vo = g.buf(24 * c[6], ("verts_out", nv)).view(torch.float64) if outputs[0] else None
    to = g.buf(3 * ib * c[7], ("tris_out", nt)).view(dtype) if outputs[1] else None
    ho = g.buf(4 * (c[7] - nt), ("hole", nt)).view(torch.int32) if outputs[2] else None
    torch.cuda.synchronize()
    _lib.call("o2345_mesh_fill_emit", verts, tris, ib, nv, nt, ws, vo, to, ho)
    torch.cuda.synchronize()
    assert verts.cpu().numpy().tobytes() == np.ascontiguousarray(hv, np.float64).tobytes() and tris.cpu().numpy().tobytes() == np.ascontiguousarray(hf, np_idx).tobytes()
    h = lambda t: None if t is None else t.cpu().numpy()
    return c, h(vo), h(to), h(ho)


GUARDED = ("tetrahedron_open", "cube_open", "cone255", "cone256", "cone257", "grid_700_1", "cube_pinholes", "sphere_small", "bowtie_grids", "defects", "torus",
           "grid_nt0", "grid_nt1", "grid_nt255", "grid_nt256", "grid_nt257")


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_kernel_writes_outside_its_buffers(dev, dtype):
    g = Guard(dev)
    for name in GUARDED:
        hv, hf, n = U.cases()[name]
        c, vo, to, ho = _raw(dev, hv, hf, n, dtype, g)
        bad = g.damaged()
        assert not bad, bad
        wv, wf, _, _, whole, winfo = U.twin(name)
        assert c == [winfo[k] for k in mio.FILL_COUNTS]
        assert vo.tobytes() == np.ascontiguousarray(wv, np.float64).tobytes() and to.tobytes() == np.ascontiguousarray(wf).astype(to.dtype).tobytes()
        assert ho.tobytes() == whole.tobytes()
    # any output may be null
    hv, hf, n = U.cases()["cube_open"]
    full = _raw(dev, hv, hf, n, dtype, g)
    for k in range(3):
        part = _raw(dev, hv, hf, n, dtype, g, outputs=tuple(i != k for i in range(3)))
        assert part[1 + k] is None and all(np.array_equal(a, b) for i, (a, b) in enumerate(zip(part, full)) if i != 1 + k)
    assert not g.damaged()


def test_a_bad_index_is_a_status_not_a_fault(dev):
    hv, hf, _ = U.cases()["cube_open"]
    verts, tris = torch.from_numpy(hv.copy()).to(dev), _dev_tris(hf, dev, torch.int64)
    for bad in (hv.shape[0], -1, 2 ** 31 + 1):
        for dtype in (torch.int64, torch.int32):
            if dtype == torch.int32 and bad > 2 ** 31:
                continue
            t = tris.clone()
            t[7, 1] = bad
            t = t.to(dtype)
            t0 = t.clone()
            with pytest.raises(RuntimeError, match="index outside"):
                ops.mesh_fill_holes(verts, t, 40)
            assert torch.equal(t, t0)
    _equal(ops.mesh_fill_holes(verts, tris, config.MESH_FILL_HOLES_ALL), U.twin("cube_open"), torch.int64)


@pytest.fixture(scope="module")
def scene(dev):
    """The stored small scene's mesh, and the number of holes of its host copy.  Where it has none of its own, the pipeline test cuts some by dropping
    the faces of one lattice slab, those whose centroid has R / 2 <= z < R / 2 + 1, which opens a rim on both sides of the slab."""
    S = stored_scene(dev)
    assert S["hf"].shape[0] > 100
    S["holes"] = mio.fill_holes(S["hv"], S["hf"])[5]["holes"]
    return S


def _cut(S, verts_idx, tris):
    z = verts_idx[tris.long()].mean(1)[:, 2]
    return tris[~((z >= S["R"] // 2) & (z < S["R"] // 2 + 1))].contiguous()


def test_pipeline_fills_after_the_cleanup_and_colours_the_caps(scene, monkeypatch):
    S = scene
    opts = config.mesh_options()
    if S["holes"] == 0:                                                  # cut the mesh open where marching cubes hands it to the clean-up chain
        real = ops.marching_cubes
        monkeypatch.setattr(ops, "marching_cubes", lambda u, iso=0.0, **kw: (lambda v, t: (v, _cut(S, v, t)))(*real(u, iso, **kw)))
    off = pipeline._mesh_fields(*_args(S), opts)
    hv, hf = off.verts_idx.cpu().numpy(), off.tris.cpu().numpy()
    want = mio.fill_holes(hv, hf)
    assert want[5]["holes"] >= 1 and want[5]["filled"] == want[5]["holes"]
    on = pipeline._mesh_fields(*_args(S), opts, fill_holes=config.MESH_FILL_HOLES_ALL)
    nv, nt = hv.shape[0], hf.shape[0]
    assert on.verts_idx.shape[0] == want[5]["vertices"] > nv and on.tris.shape[0] == want[5]["triangles"] > nt
    assert _bits(on.verts_idx[:nv], off.verts_idx) and _bits(on.tris[:nt], off.tris)
    assert on.verts_idx.cpu().numpy().tobytes() == want[0].tobytes() and on.tris.cpu().numpy().tobytes() == want[1].tobytes()
    assert on.info["fill"] == want[5] and "fill" not in off.info and {k: v for k, v in on.info.items() if k != "fill"} == off.info
    rgb, grad = _fields_at(S, on.verts_idx)
    assert _bits(on.rgb, rgb) and _bits(on.grad, grad)                   # the cap's vertices are coloured like any other
    assert ops.mesh_audit(on.verts_idx, on.tris)["boundary_edges"] == on.info["fill"]["open"]
    # the keyword reaches the public calls, and the config default reaches them
    v, t, c, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, fill_holes=config.MESH_FILL_HOLES_ALL)
    assert _bits(v, on.verts_idx) and _bits(t, on.tris) and _bits(c, on.rgb)
    monkeypatch.setattr(config, "MESH_FILL_HOLES", 3)
    few = pipeline._mesh_fields(*_args(S), opts, fill_holes=config.mesh_fill_holes()).info["fill"]
    assert few == mio.fill_holes(hv, hf, 3)[5]


def test_reconstruct_folder_reports_the_fill_when_on_and_keeps_its_keys_when_off(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    on = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64, fill_holes=config.MESH_FILL_HOLES_ALL)
    off = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64)
    zero = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "c.ply"), D=48, resolution=64, fill_holes=0)
    assert "fill_holes" not in off and set(off) == set(on) - {"fill_holes"} and {k: x for k, x in zero.items() if k != "ply"} == {k: x for k, x in off.items() if k != "ply"}
    assert open(off["ply"], "rb").read() == open(zero["ply"], "rb").read()
    fill = on["fill_holes"]
    assert list(fill) == list(mio.FILL_COUNTS) and (on["vertices"], on["triangles"]) == (fill["vertices"], fill["triangles"])
    assert fill["triangles"] - off["triangles"] >= fill["filled"] and fill["vertices"] - off["vertices"] <= fill["filled"]
    v, t, _ = mio.read_ply(on["ply"])
    assert mio.mesh_audit(v.astype(np.float64), t)["boundary_edges"] == fill["open"] and fill["too_long"] == 0


def test_mirror_extract_geometry_applies_the_configured_fill(dev, monkeypatch):
    """the drop-in mirror fills INDEX coordinates between its clean-up and its smoothing and maps them to world units afterwards: the twin on the
    marching cubes of the u it returns, cut open by one lattice slab as above"""
    ren, sdf, dense = golden_mirror(dev)
    R = 48
    real = ops.marching_cubes

    def cut(u, iso=0.0, **kw):
        v, t = real(u, iso, **kw)
        z = v[t.long()].mean(1)[:, 2]
        return v, t[~((z >= R // 2) & (z < R // 2 + 1))].contiguous()
    monkeypatch.setattr(ops, "marching_cubes", cut)
    call = lambda: ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=R, threshold=0, device=dev,
                                        conditional_volume=dense, lod=0)
    v0, t0, u0 = call()
    vi, ti = cut(torch.from_numpy(u0).to(dev).contiguous(), 0.0)
    hv, hf = vi.cpu().numpy(), ti.cpu().numpy()
    assert t0.shape[0] > 0 and np.array_equal(hf, t0)
    want = mio.fill_holes(hv, hf)
    assert want[5]["filled"] >= 1
    monkeypatch.setattr(config, "MESH_FILL_HOLES", config.MESH_FILL_HOLES_ALL)
    v, t, u = call()
    assert v.dtype == np.float64 and v.tobytes() == (want[0] / (R - 1) * 2.0 + -1.0).tobytes() and np.array_equal(t, want[1]) and u.tobytes() == u0.tobytes()


def test_files_keep_their_bytes_when_off_and_carry_the_caps_when_on(scene, tmp_path, monkeypatch):
    S = scene
    real = ops.marching_cubes
    monkeypatch.setattr(ops, "marching_cubes", lambda u, iso=0.0, **kw: (lambda v, t: (v, _cut(S, v, t)))(*real(u, iso, **kw)))
    real_call = _lib.call
    guard = lambda name, *a: pytest.fail("a fill entry was reached with the stage off") if "mesh_fill" in name else real_call(name, *a)
    for ext in (".ply", ".glb"):
        export = pipeline.export_mesh_ply if ext == ".ply" else pipeline.export_mesh_asset
        plain, off, on = (str(tmp_path / (k + ext)) for k in ("plain", "off", "on"))
        n_plain = export(plain, *_args(S))
        monkeypatch.setattr(ops, "call", guard)
        assert export(off, *_args(S), fill_holes=0) == n_plain and export(str(tmp_path / ("none" + ext)), *_args(S), fill_holes=None) == n_plain
        monkeypatch.setattr(ops, "call", real_call)
        assert open(plain, "rb").read() == open(off, "rb").read() == open(str(tmp_path / ("none" + ext)), "rb").read()
        n_on = export(on, *_args(S), fill_holes=config.MESH_FILL_HOLES_ALL)
        assert n_on[0] > n_plain[0] and n_on[1] > n_plain[1]
        if ext == ".glb":
            p, t = mio.read_glb(on)[:2]
            assert (p.shape[0], t.shape[0]) == n_on
            v, f = pipeline.extract_mesh(*_args(S), return_index_verts=True)[:2]
            info = mio.fill_holes(v.cpu().numpy(), f.cpu().numpy())[5]
            assert n_on == (info["vertices"], info["triangles"])
