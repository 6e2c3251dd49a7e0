"""GPU: the ray cast and the ambient occlusion (csrc/mesh_raycast.hip) against the host twins (mesh_io.segment_hits / mesh_occlusion), which define the
result.  t is compared by its bytes, tri, hits and the counters as integers, through the grid at several cell edges and without a grid.  Expected values
are the twin applied to the same inputs, never the code under test; a twin result is computed once per mesh and shared."""
import importlib
import os

import numpy as np
import pytest
import torch

import mesh_raycast_util as R
from guard_util import PRE, Guard
from mesh_scene_util import args as _args, colours_at, dev, dev_tris as _dev_tris, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

MESHES = ("cube", "icosphere", "soup", "two_spheres")
CELLS = ("default", "fine", "single", "exhaustive")
SAMPLES = (1, 16, 64, 100, 1024)                  # rows of a wave: 64 points, 4 points, one, a row that straddles waves, a row of 16 waves
L_OCC, BIAS = 0.6, 1e-6


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def cases(dev):
    """per mesh: the device mesh, its grids, the segments (which need the default grid's cell edge) and the twin's answers"""
    out = {}
    for name in MESHES:
        v, f = R.meshes()[name]
        verts = _up(v, dev)
        tris = {dt: _dev_tris(f, dev, dt) for dt in (torch.int32, torch.int64)}
        cells = R.grid_cells(v)
        grids = {k: ops.mesh_distance_grid(verts, tris[torch.int32], c) for k, c in cells.items() if k != "single"}
        grids["single"] = ops.mesh_distance_grid(verts, tris[torch.int32], max_cells=1)           # the lattice is anchored at 0: an edge alone cannot force one cell
        assert grids["single"].dims == (1, 1, 1) and max(grids["fine"].dims) >= 17 and min(g.entries for g in grids.values()) >= f.shape[0]
        P, Q = R.segments(v, [grids["default"].cell, cells["fine"], cells["single"]], n=2000, seed=len(name))
        t, tri = mio.segment_hits(P, Q, v, f)
        assert 200 < (tri >= 0).sum() < tri.size - 200, name
        out[name] = dict(v=v, f=f, verts=verts, tris=tris, grids=dict(grids, exhaustive=None), P=P, Q=Q, t=t, tri=tri, dP=_up(P, dev), dQ=_up(Q, dev))
    return out


def _grid_args(G):
    return (G.buffer, G.buffer.numel(), G.max_cells) if G is not None else (None, 0, 0)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", MESHES)
def test_segments_equal_the_twin(cases, dev, name, cell):
    c = cases[name]
    n, nv, nt = c["P"].shape[0], c["v"].shape[0], c["f"].shape[0]
    for dt, ib in ((torch.int32, 4), (torch.int64, 8)):
        t = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        tri = torch.full((n,), -7, dtype=torch.int32, device=dev)
        flag = torch.full((n,), -7, dtype=torch.int32, device=dev)
        _lib.call("o2345_mesh_ray_cast", c["dP"], c["dQ"], n, c["verts"], c["tris"][dt], ib, nv, nt, *_grid_args(c["grids"][cell]), 0, t, tri)
        _lib.call("o2345_mesh_ray_cast", c["dP"], c["dQ"], n, c["verts"], c["tris"][dt], ib, nv, nt, *_grid_args(c["grids"][cell]), 1, None, flag)
        got_t, got_tri, got_flag = t.cpu().numpy(), tri.cpu().numpy(), flag.cpu().numpy()
        wrong = np.flatnonzero((got_tri != c["tri"]) | (got_t.view(np.int64) != c["t"].view(np.int64)))
        assert wrong.size == 0, (name, cell, dt, wrong[:8], got_t[wrong[:8]], c["t"][wrong[:8]], got_tri[wrong[:8]], c["tri"][wrong[:8]])
        assert got_t.tobytes() == c["t"].tobytes() and np.array_equal(got_tri, c["tri"]) and np.array_equal(got_flag, (c["tri"] >= 0).astype(np.int32))
    assert c["dP"].cpu().numpy().tobytes() == c["P"].tobytes() and c["verts"].cpu().numpy().tobytes() == c["v"].tobytes()      # inputs are only read


def test_ops_and_pipeline_calls(cases, dev):
    c = cases["icosphere"]
    o, d = c["P"][:300], (c["Q"] - c["P"])[:300] / 3.0
    want_d, want_tri = mio.ray_cast(o, d, c["v"], c["f"], 3.0)
    want_flags = mio.ray_cast(o, d, c["v"], c["f"], 3.0, any_hit=True)
    for grid in (None, False, c["grids"]["fine"]):
        dist, tri = ops.mesh_ray_cast(_up(o, dev), _up(d, dev), c["verts"], c["tris"][torch.int64], 3.0, grid=grid)
        assert dist.cpu().numpy().tobytes() == want_d.tobytes() and np.array_equal(tri.cpu().numpy(), want_tri)
        flags = ops.mesh_ray_cast(_up(o, dev), _up(d, dev), c["verts"], c["tris"][torch.int32], 3.0, grid=grid, any_hit=True)
        assert flags.dtype == torch.bool and np.array_equal(flags.cpu().numpy(), want_flags)
    dist, tri = pipeline.mesh_ray_cast((c["v"], c["f"]), o, d, 3.0)                       # host arrays are uploaded
    assert dist.cpu().numpy().tobytes() == want_d.tobytes() and np.array_equal(tri.cpu().numpy(), want_tri)
    with pytest.raises(ValueError, match="max_distance"):
        ops.mesh_ray_cast(_up(o, dev), _up(d, dev), c["verts"], c["tris"][torch.int32], 0.0)
    # the per-face occlusion of a mesh against itself: a convex mesh is open from outside and closed from inside
    out = pipeline.mesh_occlusion((c["v"], c["f"]), samples=16)
    hits, counts = mio.mesh_occlusion(mio.surface_samples(c["v"], c["f"])[0], c["v"], c["f"], owners=np.arange(320), samples=16)
    assert np.array_equal(out["hits"].cpu().numpy(), hits) and out["counts"] == counts and counts["rays"] == 16 * 320
    assert out["mean"] == 1.0 and out["exposure"].cpu().tolist() == [1.0] * 320
    inside = pipeline.mesh_occlusion((c["v"], c["f"]), samples=16, flip=True)
    assert inside["mean"] < 0.05 and inside["counts"] == counts
    # a mesh without a triangle that has an area: nothing is hit
    flat = torch.zeros(300, 3, dtype=torch.float64, device=dev)
    none = ops.mesh_ray_cast(_up(o, dev), _up(d, dev), flat, c["tris"][torch.int32], 3.0)
    assert none[1].cpu().tolist() == [-1] * 300 and bool(torch.isinf(none[0]).all())


@pytest.fixture(scope="module")
def occlusion(dev):
    """per mesh and form: the points and the twin's hits and counts for every sample count (1024 with one form, two_spheres with the small counts only)"""
    out = {}
    for name in MESHES:
        v, f = R.meshes()[name]
        pts = R.occlusion_points(v, f, n=24 if name != "two_spheres" else 12, seed=7)
        for form, keys in R.FORMS.items():
            for S in SAMPLES:
                if (S == 1024 and form != "both") or (S > 16 and name == "two_spheres"):          # 9,600 triangles: the twin is exhaustive
                    continue
                kw = {k: pts[k] for k in keys}
                out[name, form, S] = mio.mesh_occlusion(pts["points"], v, f, samples=S, max_distance=L_OCC, bias=BIAS, **kw)
        out[name] = pts
    return out


@pytest.mark.parametrize("cell", ("default", "fine", "exhaustive"))
@pytest.mark.parametrize("name", MESHES)
def test_occlusion_equals_the_twin(cases, occlusion, dev, name, cell):
    c, pts = cases[name], occlusion[name]
    G = c["grids"][cell]
    seen = 0
    for (m, form, S), (want_hits, want_counts) in ((k, x) for k, x in occlusion.items() if isinstance(k, tuple) and k[0] == name):
        kw = {k: _up(pts[k], dev) for k in R.FORMS[form]}
        dt = torch.int64 if S in (16, 100) else torch.int32
        hits, counts = ops.mesh_occlusion(_up(pts["points"], dev), c["verts"], c["tris"][dt], samples=S, max_distance=L_OCC, bias=BIAS, grid=G if G is not None else False,
                                          **kw)
        assert hits.dtype == torch.int32 and np.array_equal(hits.cpu().numpy(), want_hits), (name, cell, form, S, hits.cpu().numpy(), want_hits)
        assert counts == want_counts, (name, cell, form, S)
        assert want_counts["bad_points"] == 1 and want_counts["bad_frames"] == 2 and want_counts["rays"] == S * (want_hits.size - 3)
        seen += int(want_hits.sum() > 0 and (want_hits < S).any())
        v = ops.mesh_occlusion_values(hits, S)
        assert v.cpu().numpy().tobytes() == mio.occlusion_values(want_hits, S).tobytes()
    assert seen >= 6                                                      # the fixtures do occlude, and not everything


NT_EDGES = (0, 1, 255, 256, 257)


def test_guard_bands_at_exact_sizes(dev):
    """every output at its exact size between guard bands: n = 0, and nt = 0, 1, 255, 256, 257 triangles of the icosphere, both entries, grid and not"""
    v, f = R.meshes()["icosphere"]
    P, Q = R.segments(v, [0.3], n=333, seed=9)
    pts = R.occlusion_points(v, f[:255], n=13, seed=3)
    table = _up(mio.occlusion_directions(100), dev)
    g = Guard(dev)
    assert PRE % 16 == 0
    for nt in NT_EDGES:
        fk = f[:nt]
        verts, tris = _up(v, dev), _dev_tris(fk, dev, torch.int32)
        G = ops.mesh_distance_grid(verts, tris) if nt else None
        for n in (0, P.shape[0]):
            want_t, want_tri = mio.segment_hits(P[:n], Q[:n], v, fk)
            for grid in ((G, None) if G is not None else (None,)):
                t, tri, flag = g.buf(8 * n, ("t", nt, n)), g.buf(4 * n, ("tri", nt, n)), g.buf(4 * n, ("flag", nt, n))
                dP, dQ = g.buf(P[:n], ("P", nt, n)), g.buf(Q[:n], ("Q", nt, n))
                torch.cuda.synchronize()
                a = (dP.view(torch.float64), dQ.view(torch.float64), n, verts, tris, 4, v.shape[0], nt) + _grid_args(grid)
                _lib.call("o2345_mesh_ray_cast", *a, 0, t.view(torch.float64), tri.view(torch.int32))
                _lib.call("o2345_mesh_ray_cast", *a, 1, None, flag.view(torch.int32))
                assert t.cpu().numpy().tobytes() == want_t.tobytes() and np.array_equal(tri.cpu().numpy().view(np.int32), want_tri)
                assert np.array_equal(flag.cpu().numpy().view(np.int32), (want_tri >= 0).astype(np.int32))
        for n in (0, 13):
            want_hits, want_counts = mio.mesh_occlusion(pts["points"][:n], v, fk, normals=pts["normals"][:n], owners=pts["owners"][:n], samples=100,
                                                        max_distance=L_OCC, bias=BIAS)
            for grid in ((G, None) if G is not None else (None,)):
                hits, counters = g.buf(4 * n, ("hits", nt, n)), g.buf(32, ("counters", nt, n))
                dp, dn, do = g.buf(pts["points"][:n], "points"), g.buf(pts["normals"][:n], "normals"), g.buf(pts["owners"][:n], "owners")
                torch.cuda.synchronize()
                _lib.call("o2345_mesh_occlusion", dp.view(torch.float64), dn.view(torch.float64), do.view(torch.int32), n, table, 100, L_OCC, BIAS, verts, tris, 4,
                          v.shape[0], nt, *_grid_args(grid), hits.view(torch.int32), counters.view(torch.int64))
                assert np.array_equal(hits.cpu().numpy().view(np.int32), want_hits), (nt, n)
                got = counters.view(torch.int64).cpu().tolist()
                assert mio.occlusion_report(got) == want_counts and got[3] == 0, (nt, n, got, want_counts)
    assert g.damaged() == []


def test_refusals(cases, dev):
    c = cases["cube"]
    n, nv, nt = 4, 8, 12
    P, Q, t, tri = c["dP"][:n].contiguous(), c["dQ"][:n].contiguous(), torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    G = c["grids"]["default"]
    table, hits, counters = _up(mio.occlusion_directions(4), dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
    owners = torch.zeros(n, dtype=torch.int32, device=dev)
    many = 2 ** 16 + 1
    big = torch.zeros(many, 3, dtype=torch.int32, device=dev)
    for a, msg in (((P, Q, n, c["verts"], c["tris"][torch.int32], 3, nv, nt, None, 0, 0, 0, t, tri), "index_bytes"),
                   ((P, Q, -1, c["verts"], c["tris"][torch.int32], 4, nv, nt, None, 0, 0, 0, t, tri), "bad sizes"),
                   ((P, None, n, c["verts"], c["tris"][torch.int32], 4, nv, nt, None, 0, 0, 0, t, tri), "null pointer"),
                   ((P, Q, n, c["verts"], c["tris"][torch.int32], 4, nv, nt, None, 0, 0, 0, None, tri), "null pointer"),
                   ((P, Q, n, c["verts"], c["tris"][torch.int32], 4, nv, nt, G.buffer, 64, G.max_cells, 0, t, tri), "grid of 64 bytes"),
                   ((P, Q, n, c["verts"], c["tris"][torch.int32], 4, nv, nt, G.buffer, G.buffer.numel(), 0, 0, t, tri), "max_cells"),
                   ((P, Q, n, c["verts"], big, 4, nv, many, None, 0, 0, 0, t, tri), "without a grid")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("o2345_mesh_ray_cast", *a)
    mesh = (c["verts"], c["tris"][torch.int32], 4, nv, nt, None, 0, 0)
    for a, msg in (((P, None, None, n, table, 4, 1.0, 0.0) + mesh + (hits, counters), "direction or an owner"),
                   ((P, None, owners, n, table, 0, 1.0, 0.0) + mesh + (hits, counters), "n_samples"),
                   ((P, None, owners, n, table, 1025, 1.0, 0.0) + mesh + (hits, counters), "n_samples"),
                   ((P, None, owners, n, table, 4, 0.0, 0.0) + mesh + (hits, counters), "max_distance"),
                   ((P, None, owners, n, table, 4, float("inf"), 0.0) + mesh + (hits, counters), "max_distance"),
                   ((P, None, owners, n, table, 4, 1.0, -1.0) + mesh + (hits, counters), "bias"),
                   ((P, None, owners, n, None, 4, 1.0, 0.0) + mesh + (hits, counters), "null pointer"),
                   ((P, None, owners, n, table, 4, 1.0, 0.0) + mesh + (hits, None), "null pointer")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("o2345_mesh_occlusion", *a)
    with pytest.raises(ValueError, match="direction"):
        ops.mesh_occlusion(P, c["verts"], c["tris"][torch.int32])
    with pytest.raises(ValueError, match="samples"):
        ops.mesh_occlusion(P, c["verts"], c["tris"][torch.int32], owners=owners, samples=2000)


# ---- the pipeline on the stored small scene (D = 20, R = 64), the scene of tests/test_gpu_mesh_texture.py -------------------------------------------------
OCC_SAMPLES = 16


@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev, extract=False)
    v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=4)
    hv, hf = v.cpu().numpy(), t.cpu().numpy()
    nt = hf.shape[0]
    assert 50 < nt < 5000
    pts, world = mio.texture_points(hv, hf, 4, S["R"])
    dpts = ops.mesh_texture_points(v, t, 4, S["R"])[0]
    assert dpts.cpu().numpy().tobytes() == pts.tobytes()                  # the device-produced points are the twin's
    rgb, grad = colours_at(S, torch.from_numpy(world).to(dev))
    owners = mio._texel_owners(mio.texture_layout(nt, 4), nt).reshape(-1)
    hits, counts = mio.mesh_occlusion(dpts.cpu().numpy(), hv, hf, normals=grad.cpu().numpy().astype(np.float64), owners=owners, samples=OCC_SAMPLES,
                                      max_distance=S["R"] / 8.0, bias=1e-3, prefilter=True)
    pos, uv, _, bounds = mio.texture_corners(hv, hf, 4, S["R"])
    S.update(nt=nt, hits=hits, counts=counts, oimage=mio.pack_texture(mio.occlusion_values(hits, OCC_SAMPLES), nt, 4), pos=pos, uv=uv, bounds=bounds,
             image=mio.pack_texture(rgb.cpu().numpy(), nt, 4))
    return S


def test_baked_occlusion_end_to_end(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    assert config.MESH_OCCLUSION is False and config.MESH_OCCLUSION_SAMPLES == 64 and config.MESH_OCCLUSION_BIAS == 1e-3 and config.mesh_occlusion_distance(64) == 8.0
    monkeypatch.setattr(config, "MESH_OCCLUSION_SAMPLES", OCC_SAMPLES)
    nt = S["nt"]
    kw = dict(decimate_cell=4, texture_texel=4)
    path, obj = str(tmp_path / "o.glb"), str(tmp_path / "o.obj")
    assert pipeline.export_mesh_asset(path, *_args(S), ambient_occlusion=True, **kw) == (3 * nt, nt)
    got = mio.read_glb_occlusion(path)
    print(f"occlusion bake: {nt} triangles, {S['hits'].size} texels, counts {S['counts']}, mean exposure {1.0 - S['hits'].mean() / OCC_SAMPLES:.3f}")
    assert got.tobytes() == S["oimage"].tobytes()
    assert 0 < S["hits"].sum() and (S["hits"] == 0).any() and S["counts"]["bad_points"] == 0                    # concavities are shaded, open texels are not
    want = str(tmp_path / "want.glb")
    mio.write_textured(want, S["pos"], S["uv"], None, S["image"], S["bounds"], occlusion_image=S["oimage"])
    assert B(path) == B(want)
    pipeline.export_mesh_asset(obj, *_args(S), ambient_occlusion=True, **kw)
    assert np.array_equal(mio.read_obj_occlusion(obj), got) and B(tmp_path / "o_occlusion.png") == mio.png_bytes(got, 1)
    # next to a normal map: image 2
    both = str(tmp_path / "b.glb")
    pipeline.export_mesh_asset(both, *_args(S), ambient_occlusion=True, normal_map=True, **kw)
    assert mio.read_glb_occlusion(both).tobytes() == got.tobytes() and mio.read_glb_normal_map(both) is not None
    # off: nothing is launched, and the file is the parent's (the twin writers without the new arguments)
    for name in ("mesh_occlusion", "mesh_occlusion_values"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"ambient_occlusion off must not reach ops.{_n}"))
    plain = str(tmp_path / "want_plain.glb")
    mio.write_textured(plain, S["pos"], S["uv"], None, S["image"], S["bounds"])
    for k, flag in enumerate((None, False)):
        off = str(tmp_path / f"off{k}.glb")
        pipeline.export_mesh_asset(off, *_args(S), ambient_occlusion=flag, **kw)
        assert B(off) == B(plain) and mio.read_glb_occlusion(off) is None
    assert not [n for n in os.listdir(tmp_path) if n.startswith("off") and n.endswith("_occlusion.png")]
    with pytest.raises(ValueError, match="texture_texel"):
        pipeline.export_mesh_asset(str(tmp_path / "x.glb"), *_args(S), decimate_cell=4, ambient_occlusion=True)
