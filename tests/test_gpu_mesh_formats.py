"""GPU: the device path of the asset export (csrc/mesh_export.hip behind ops.mesh_asset_pack / ops.obj_text / mesh_io.export_asset /
pipeline.export_mesh_asset) against the host layer of mesh_io, which defines the two files (tests/test_mesh_formats.py).

Orientation rule, restated: asset frame = PLY frame with y and z exchanged, (x, y, z) -> (x, z, y), every face reversed, (a, b, c) -> (c, b, a)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_guard import GuardedTorch

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")


def _ellipsoid(dev, R=96):
    """The field of tests/test_mesh_io.py::test_mesh_pack_matches_oracle."""
    g = np.linspace(-1, 1, R, dtype=np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    u = (0.8 - np.sqrt(X ** 2 + 1.3 * Y ** 2 + Z ** 2)).astype(np.float32)
    verts, tris = ops.marching_cubes(torch.from_numpy(u).to(dev), 0.0)
    assert verts.shape[0] > 1000
    return verts, tris


def _mats():
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 1.7321; scale[:3, 3] = [0.11, -0.23, 0.05]
    a = 0.6
    trans = np.array([[np.cos(a), -np.sin(a), 0, 0.3], [np.sin(a), np.cos(a), 0, -0.2], [0, 0, 1, 1.5], [0, 0, 0, 1]], np.float32)
    return scale[None], trans[None]                                   # the reference's sample dict carries a batch dimension


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("with_mats", [False, True])
def test_device_export_equals_host_conversion(tmp_path, with_mats, with_colors):
    """a.ply through the existing device path, a.glb / a.obj through export_asset; convert_mesh(a.ply) must reproduce both files byte for byte (both
    vertex kernels call one vertex function: equality holds with matrices too)."""
    dev = torch.device("cuda:0")
    R = 96
    verts, tris = _ellipsoid(dev, R)
    n = verts.shape[0]
    rgb = None
    if with_colors:
        rgb = torch.from_numpy(np.random.default_rng(1).uniform(0, 1, (n, 3)).astype(np.float32))
        rgb[:5] = torch.tensor([[0.0, 1.0, 0.999999], [1.0, 0.5, 0.0039215], [0.0039216, 0.25, 0.75], [1 / 255, 2 / 255, 254.999 / 255], [0.1, 0.2, 0.3]])
        rgb = rgb.to(dev)
    scale, trans = _mats() if with_mats else (None, None)
    bmin, bmax = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
    ply = str(tmp_path / "a.ply")
    assert mio.export_asset(ply, verts, tris, R, bmin, bmax, scale, trans, rgb) == (n, tris.shape[0])        # .ply delegates to export_mesh
    mio.export_mesh(str(tmp_path / "b.ply"), verts, tris, R, bmin, bmax, scale, trans, rgb)
    assert _bytes(ply) == _bytes(str(tmp_path / "b.ply"))
    pv, pf, pc = mio.read_ply(ply)
    for ext in (".glb", ".obj"):
        dev_file, host_file = str(tmp_path / ("a" + ext)), str(tmp_path / ("host" + ext))
        assert mio.export_asset(dev_file, verts, tris, R, bmin, bmax, scale, trans, rgb) == (n, tris.shape[0])
        mio.convert_mesh(ply, host_file)
        a, b = _bytes(dev_file), _bytes(host_file)
        assert len(a) == len(b)
        assert a == b, (ext, next(i for i in range(len(a)) if a[i] != b[i]))
    v, f, c, nr = mio.read_glb(str(tmp_path / "a.glb"))
    assert np.array_equal(v.view(np.uint32), np.ascontiguousarray(pv[:, [0, 2, 1]]).view(np.uint32)) and np.array_equal(f, pf[:, ::-1]) and nr is None
    assert (c is None and pc is None) if not with_colors else np.array_equal(c, pc)
    # int32 triangles give the same indices
    i64 = ops.mesh_asset_pack(verts, tris, R)[3]
    i32 = ops.mesh_asset_pack(verts, tris.to(torch.int32), R)[3]
    assert torch.equal(i64, i32) and np.array_equal(i64.cpu().numpy(), tris.cpu().numpy()[:, ::-1])


def _normals_numpy(g, trans):
    """fp64 normalize(g) -> 3x3 of trans_mat -> renormalise -> swap -> float32."""
    g = g.astype(np.float64)
    nrm = g / np.linalg.norm(g, axis=1, keepdims=True)
    if trans is not None:
        nrm = nrm @ trans.reshape(-1, 4, 4)[0][:3, :3].astype(np.float64).T
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return nrm[:, [0, 2, 1]].astype(np.float32)


@pytest.mark.parametrize("with_mats", [False, True])
def test_normals(tmp_path, with_mats):
    dev = torch.device("cuda:0")
    R = 96
    verts, tris = _ellipsoid(dev, R)
    n = verts.shape[0]
    rng = np.random.default_rng(2)
    g = (rng.normal(0, 1, (n, 3)) * rng.uniform(1e-3, 50, (n, 1))).astype(np.float32)
    g[:3] = [[1, 0, 0], [0, 0, -2], [0, 1e-20, 0]]
    zero_rows = [10, 11, 12]
    g[10] = 0
    g[11] = [np.nan, 1, 0]
    g[12] = [np.inf, 0, 0]
    scale, trans = _mats() if with_mats else (None, None)
    if with_mats:                                                      # not a pure rotation: renormalisation has something to do
        trans = trans.copy(); trans[0, :3, :3] = trans[0, :3, :3] @ np.diag([1.0, 1.5, 0.75]).astype(np.float32)
    rgb = torch.from_numpy(rng.uniform(0, 1, (n, 3)).astype(np.float32)).to(dev)
    pos, rgba, nrm, idx, bounds = ops.mesh_asset_pack(verts, tris, R, scale_mat=scale, trans_mat=trans, rgb=rgb, grad=torch.from_numpy(g).to(dev))
    got = nrm.cpu().numpy()
    keep = np.ones(n, bool); keep[zero_rows] = False
    with np.errstate(all="ignore"):
        want = _normals_numpy(g, trans)
    err = np.abs(got[keep] - want[keep]).max()
    unit = np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max()
    print(f"normals: max abs difference {err:.3e}, max | |n| - 1 | {unit:.3e}")
    assert err <= 1e-6
    assert unit <= 1e-6
    assert np.array_equal(got[zero_rows], np.array([[0, 1, 0]] * 3, np.float32))
    # bounds of the pass == column min / max of the positions it wrote
    p = pos.cpu().numpy()
    assert np.array_equal(bounds.cpu().numpy(), np.stack([p.min(0), p.max(0)]))
    # files with normals: GLB carries them bit for bit, the OBJ parses and its faces are a//a
    for ext in (".glb", ".obj"):
        f = str(tmp_path / ("n" + ext))
        mio.export_asset(f, verts, tris, R, scale_mat=scale, trans_mat=trans, vertex_colors=rgb, normals=torch.from_numpy(g).to(dev))
        host = str(tmp_path / ("h" + ext))
        (mio.write_glb if ext == ".glb" else mio.write_obj_numpy)(host, p, idx.cpu().numpy().view(np.uint32), rgba.cpu().numpy(), got)
        assert _bytes(f) == _bytes(host)
    v2, f2, c2, n2 = mio.read_glb(str(tmp_path / "n.glb"))
    assert np.array_equal(n2.view(np.uint32), got.view(np.uint32))
    v3, f3, c3, n3 = mio.read_obj(str(tmp_path / "n.obj"))
    assert n3.shape == (n, 3) and np.abs(n3 - got.astype(np.float64)).max() <= 0.5e-8 + 1e-15 and np.array_equal(f3, tris.cpu().numpy()[:, ::-1])
    face_lines = [l for l in open(str(tmp_path / "n.obj")).read().split("\n") if l.startswith("f ")]
    assert len(face_lines) == tris.shape[0] and len({len(l) for l in face_lines}) == 1
    for l in face_lines[:: max(1, len(face_lines) // 500)]:
        for t in l.split()[1:]:
            a, mid, b = t.split("/")
            assert mid == "" and a == b and 1 <= int(a) <= n


def _scene(dev):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    pipeline = bench.pipeline
    wt = pipeline.SceneWeights(dev, seed=0)
    inp = bench.make_inputs(dev, 4, 0, 1)
    D, R = 48, 64
    vol = pipeline.build_volume(wt, inp["imgs"], inp["aff"], inp["origin"], D, 2.0 / (D - 1))
    return pipeline, wt, inp, vol, R


def test_pipeline_asset_equals_ply_under_swap_and_reverse(tmp_path):
    dev = torch.device("cuda:0")
    pipeline, wt, inp, vol, R = _scene(dev)
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 0.9; scale[:3, 3] = [0.01, 0.02, -0.03]
    ply, glb, obj = (str(tmp_path / ("scene" + e)) for e in (".ply", ".glb", ".obj"))
    nv, nt = pipeline.export_mesh_ply(ply, wt, vol, inp["proj"], inp["cam_pos"], R, scale_mat=scale[None])
    assert pipeline.export_mesh_asset(glb, wt, vol, inp["proj"], inp["cam_pos"], R, scale_mat=scale[None]) == (nv, nt) and nv > 0
    pv, pf, pc = mio.read_ply(ply)
    v, f, c, nr = mio.read_glb(glb)
    assert np.array_equal(v.view(np.uint32), np.ascontiguousarray(pv[:, [0, 2, 1]]).view(np.uint32))
    assert np.array_equal(f, pf[:, ::-1]) and np.array_equal(c, pc) and nr is None
    assert _bytes(glb) == _bytes(mio.convert_mesh(ply, str(tmp_path / "host.glb")))
    pipeline.export_mesh_asset(obj, wt, vol, inp["proj"], inp["cam_pos"], R, scale_mat=scale[None])
    assert _bytes(obj) == _bytes(mio.convert_mesh(ply, str(tmp_path / "host.obj")))
    # with normals: unit vectors, positions unchanged
    pipeline.export_mesh_asset(glb, wt, vol, inp["proj"], inp["cam_pos"], R, scale_mat=scale[None], normals=True)
    v2, f2, c2, n2 = mio.read_glb(glb)
    assert np.array_equal(v2, v) and np.array_equal(c2, c) and np.abs(np.linalg.norm(n2.astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_reconstruct_folder_output_format(tmp_path):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(torch.device("cuda:0"), seed=0)
    os.makedirs(str(tmp_path / "a")); os.makedirs(str(tmp_path / "b"))
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a" / "mesh.ply"), D=48, resolution=64)
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b" / "mesh.ply"), D=48, resolution=64, output_format=".glb")
    assert out["ply"] == str(tmp_path / "b" / "mesh.ply") and out["asset"] == str(tmp_path / "b" / "mesh.glb")
    assert os.path.exists(out["ply"]) and os.path.exists(out["asset"]) and "asset" not in plain and not os.path.exists(str(tmp_path / "a" / "mesh.glb"))
    assert _bytes(out["ply"]) == _bytes(str(tmp_path / "a" / "mesh.ply"))
    assert out["vertices"] == plain["vertices"] > 0 and out["triangles"] == plain["triangles"] > 0
    pv, pf, pc = mio.read_ply(out["ply"])
    v, f, c, _ = mio.read_glb(out["asset"])
    assert np.array_equal(v, pv[:, [0, 2, 1]]) and np.array_equal(f, pf[:, ::-1]) and np.array_equal(c, pc)
    with pytest.raises(ValueError):
        pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b" / "mesh.ply"), D=48, resolution=64, output_format=".stl")


def test_extract_mesh_is_unchanged_by_an_asset_export(tmp_path):
    dev = torch.device("cuda:0")
    pipeline, wt, inp, vol, R = _scene(dev)
    before = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], R)
    assert len(before) == 4
    pipeline.export_mesh_asset(str(tmp_path / "s.obj"), wt, vol, inp["proj"], inp["cam_pos"], R, normals=True)
    after = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], R)
    assert len(after) == 4
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- guard bands (tests/test_gpu_guard.py::GuardedTorch stands in for ``torch`` inside ops) --------------------------------------------------------------
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
def test_no_export_kernel_writes_outside_its_buffers(monkeypatch, index_dtype):
    dev = torch.device("cuda:0")
    g = GuardedTorch()
    monkeypatch.setattr(ops, "torch", g)
    monkeypatch.setattr(ops, "_ws_cache", {})
    rng = np.random.default_rng(5)
    R = 33
    lens = set()
    for n, m, s in [(1, 1, 1.0), (63, 65, 1.0), (257, 1, 40.0), (1001, 777, 1.0), (300, 2049, 123456.0), (5000, 9999, 1.0)]:
        verts = torch.from_numpy(rng.uniform(0, R - 1, (n, 3))).to(dev)
        tris = torch.from_numpy(rng.integers(0, n, (m, 3))).to(dev).to(index_dtype)
        scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= s; scale[:3, 3] = [0.5, -0.25, 0.125]
        rgb = torch.from_numpy(rng.uniform(0, 1, (n, 3)).astype(np.float32)).to(dev)
        grad = torch.from_numpy(rng.normal(0, 1, (n, 3)).astype(np.float32)).to(dev)
        for use_rgb, use_grad in ((False, False), (True, False), (True, True)):
            live0 = len(g.live)
            pos, rgba, nrm, idx, bounds = ops.mesh_asset_pack(verts, tris, R, scale_mat=scale, rgb=rgb if use_rgb else None, grad=grad if use_grad else None)
            text = ops.obj_text(pos, idx, rgba, nrm, bounds=bounds)
            assert len(g.live) >= live0 + 4 + use_rgb + use_grad               # positions, indices, bounds, text [, rgba] [, normals] (+ the workspace when it grows)
            bad = g.check()
            assert not bad, (n, m, s, use_rgb, use_grad, bad)
            # and what they wrote inside is the host definition
            h = lambda t: None if t is None else t.cpu().numpy()
            K = mio.obj_coordinate_digits(h(bounds))
            want = mio.obj_text_numpy(h(pos), h(idx).view(np.uint32), h(rgba), h(nrm), K)
            assert bytes(h(text)) == want, (n, m, s, use_rgb, use_grad)
            dn = len(str(n))
            lens |= {1 + 3 * (K + 11) + (33 if use_rgb else 0) + 1, 1 + 3 * (1 + (2 * dn + 2 if use_grad else dn)) + 1} | ({39} if use_grad else set())
    assert sum(1 for l in lens if l % 16) >= 8, lens                            # record lengths that are not multiples of 16
