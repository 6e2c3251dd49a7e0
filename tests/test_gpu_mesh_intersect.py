"""GPU: the self-intersection report (csrc/mesh_intersect.hip) against the host twin (mesh_io.mesh_intersections), which defines the result.  Counts,
per-face hits and the pair list are compared EXACTLY (integers, bytes), through the grid at several cell edges and without a grid.  Expected values
are the twin applied to the same inputs, never the code under test; a twin result is computed once per mesh."""
import importlib

import numpy as np
import pytest
import torch

import mesh_intersect_util as U
from guard_util import PRE, Guard
from mesh_scene_util import args as _args, dev, dev_tris as _dev_tris, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

COUNTS = mio.INTERSECT_COUNTS


def _host(out):
    return {k: x.cpu().numpy() if torch.is_tensor(x) else x for k, x in out.items()}


def _grid_of(verts, tris, cell):
    """the mesh's grid, or None where it has no triangle with an area (the grid's refusal)"""
    try:
        return ops.mesh_distance_grid(verts, tris, cell)
    except RuntimeError as e:
        assert "no triangle with an area" in str(e)
        return None


def _raw(dev, hv, hf, dtype, grid=True, cell=None, g=None, face_hits=True, pairs=True, stream=None):
    """the two entries themselves, every buffer at its exact size (inside guard bands when ``g`` is given) -> the report of the twin's shape: counts,
    "face_hits" (None when not asked for), "pairs_list" (None when not asked for); through the mesh's grid when ``grid`` and the mesh has one"""
    nv, nt = hv.shape[0], hf.shape[0]
    ib = 8 if dtype == torch.int64 else 4
    verts, tris = torch.from_numpy(np.array(hv, np.float64)).to(dev), _dev_tris(hf, dev, dtype)
    G = _grid_of(verts, tris, cell) if grid and nt > 0 else None
    gp, gb, gm = (G.buffer, G.buffer.numel(), G.max_cells) if G is not None else (None, 0, 0)
    wsb = _lib.call("o2345_mesh_intersect_workspace_bytes", nv, nt)
    assert wsb > 0 and PRE % 16 == 0
    new = (lambda n, what: g.buf(n, (what, nv, nt))) if g else (lambda n, what: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev))
    ws, counts = new(wsb, "workspace"), new(8 * len(COUNTS), "counts")
    fh = new(4 * nt, "face_hits") if face_hits else None
    torch.cuda.synchronize()                                              # the buffers were filled on the current stream
    with torch.cuda.stream(stream):
        _lib.call("o2345_mesh_intersect_count", verts, tris, ib, nv, nt, gp, gb, gm, ws, wsb, counts.view(torch.int64), None if fh is None else fh.view(torch.int32))
        out = mio.intersect_report(counts.view(torch.int64).tolist())
        pl = None
        if pairs:
            pl = new(8 * out["pairs"], "pairs")
            torch.cuda.synchronize()
            _lib.call("o2345_mesh_intersect_emit", verts, tris, ib, nv, nt, gp, gb, gm, ws, out["pairs"], pl.view(torch.int32))
    torch.cuda.synchronize()
    assert verts.cpu().numpy().tobytes() == np.ascontiguousarray(hv, np.float64).tobytes() and np.array_equal(tris.cpu().numpy(), hf)
    out["face_hits"] = None if fh is None else fh.cpu().numpy().view(np.int32)
    out["pairs_list"] = None if pl is None else pl.cpu().numpy().view(np.int32).reshape(-1, 2)
    return out


@pytest.mark.parametrize("grid", [True, False], ids=["grid", "exhaustive"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_every_fixture_equals_the_twin(dev, dtype, grid):
    """the audit's meshes, the hand cases, the two spheres, the soup, the height field before and after its fill, the blade: the entries themselves
    through the mesh's own grid (also below the size at which ops builds one) or without a grid, and ops.mesh_intersections"""
    for name, (v, f) in U.meshes().items():
        want = U.twin(name)
        U.assert_equal_reports(_raw(dev, v, f, dtype, grid=grid), want)
        got = ops.mesh_intersections(torch.from_numpy(v.copy()).to(dev), _dev_tris(f, dev, dtype), return_pairs=True, grid=grid)
        assert got["pairs_list"].is_cuda and got["face_hits"].is_cuda
        U.assert_equal_reports(_host(got), want)
        plain = ops.mesh_intersections(torch.from_numpy(v.copy()).to(dev), _dev_tris(f, dev, dtype), grid=grid)
        assert plain == {k: want[k] for k in COUNTS}
        if name in U.EXPECTED:
            assert {k: want[k] for k in U.EXPECTED[name]} == U.EXPECTED[name]


@pytest.mark.parametrize("cell", [None, 0.05, 10.0])
@pytest.mark.parametrize("name", ["soup", "blade", "blade_first"])
def test_the_result_does_not_depend_on_the_cell(dev, name, cell):
    """cell = 0.05: faces span many cells (the home-cell rule drops every repeat); cell = 10: one cell for the soup, whose row of 120 is longer than
    ROW_SHORT; the blade spans the whole grid at every edge"""
    v, f = U.meshes()[name]
    verts, tris = torch.from_numpy(v.copy()).to(dev), _dev_tris(f, dev, torch.int64)
    G = ops.mesh_distance_grid(verts, tris, cell)
    if name == "soup":
        assert (cell != 10.0 or G.dims == (1, 1, 1)) and (cell != 0.05 or (G.entries > 50 * f.shape[0] and G.cell == 0.05))
    U.assert_equal_reports(_host(ops.mesh_intersections(verts, tris, return_pairs=True, cell=cell)), U.twin(name))
    U.assert_equal_reports(_raw(dev, v, f, torch.int32, cell=cell), U.twin(name))


@pytest.fixture(scope="module")
def scene(dev):
    S = stored_scene(dev)
    assert S["hf"].shape[0] > 100
    dv, dt, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=2)
    return dict(S, dv=dv.cpu().numpy(), df=dt.cpu().numpy())


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_the_stored_scene_before_and_after_clustering(scene, dtype):
    """whatever the numbers are, they are the twin's"""
    dev = scene["plain"][0].device
    for key, v, f in (("scene", scene["hv"], scene["hf"]), ("scene_decimated", scene["dv"], scene["df"])):
        want = U.twin(key, np.asarray(v, np.float64), f)
        got = ops.mesh_intersections(torch.from_numpy(np.array(v, np.float64)).to(dev), _dev_tris(f, dev, dtype), return_pairs=True)
        U.assert_equal_reports(_host(got), want)
        assert want["faces"] + want["skipped"] == f.shape[0]


GUARDED = ("defects", "hand_crossing", "hand_repeated", "soup", "field_filled", "fan300", "blade_first", "grid_nt0", "grid_nt1", "grid_nt255", "grid_nt256", "grid_nt257")


@pytest.mark.parametrize("grid", [True, False], ids=["grid", "exhaustive"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_no_kernel_writes_outside_its_buffers(dev, dtype, grid):
    g = Guard(dev)
    for name in GUARDED:
        v, f = U.meshes()[name]
        got = _raw(dev, v, f, dtype, grid=grid, g=g)
        bad = g.damaged()
        assert not bad, bad
        U.assert_equal_reports(got, U.twin(name))
    assert len(g.live) == 4 * len(GUARDED)


def test_two_runs_and_a_second_stream_give_identical_bytes(dev, scene):
    side = torch.cuda.Stream(device=dev)
    for hv, hf in ((scene["dv"], scene["df"]), U.meshes()["soup"], U.meshes()["two_spheres"], U.meshes()["blade_first"]):
        runs = [_raw(dev, np.asarray(hv, np.float64), hf, torch.int64, stream=s) for s in (None, None, side)]
        key = lambda r: tuple(r[k] for k in COUNTS) + (r["face_hits"].tobytes(), r["pairs_list"].tobytes())
        assert key(runs[0]) == key(runs[1]) == key(runs[2])


def test_every_optional_output_may_be_null(dev):
    v, f = U.meshes()["soup"]
    want = U.twin("soup")
    for grid in (True, False):
        got = _raw(dev, v, f, torch.int32, grid=grid, face_hits=False, pairs=False)
        assert got["face_hits"] is None and got["pairs_list"] is None and {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
        got = _raw(dev, v, f, torch.int32, grid=grid, face_hits=False)
        assert got["face_hits"] is None and got["pairs_list"].tobytes() == want["pairs_list"].tobytes()
    # no pair: emit takes a null list
    v, f = U.meshes()["torus"]
    verts, tris = torch.from_numpy(v.copy()).to(dev), _dev_tris(f, dev, torch.int64)
    ws = torch.empty(_lib.call("o2345_mesh_intersect_workspace_bytes", v.shape[0], f.shape[0]), dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    _lib.call("o2345_mesh_intersect_count", verts, tris, 8, v.shape[0], f.shape[0], None, 0, 0, ws, ws.numel(), counts, None)
    assert counts.tolist()[5] == 0
    _lib.call("o2345_mesh_intersect_emit", verts, tris, 8, v.shape[0], f.shape[0], None, 0, 0, ws, 0, None)


def test_refusals_are_statuses_not_faults(dev):
    """counted on the device, raised on the host after the one copy; the input is not written, and the next call works"""
    v, f = U.meshes()["fan40"]
    good, tris = torch.from_numpy(v.copy()).to(dev), _dev_tris(f, dev, torch.int64)
    for grid in (True, False):
        for bad in (float("nan"), float("inf"), float("-inf")):
            w = good.clone()
            w[2, 1] = bad
            w0 = w.clone()
            with pytest.raises(RuntimeError, match="non-finite"):
                ops.mesh_intersections(w, tris, grid=grid)
            assert torch.equal(w.view(torch.int64), w0.view(torch.int64))
        for bad in (v.shape[0], -1, 2 ** 31 + 1):
            for dtype in (torch.int64, torch.int32):
                if dtype == torch.int32 and bad > 2 ** 31:
                    continue
                t = tris.clone()
                t[1, 2] = bad
                t = t.to(dtype)
                t0 = t.clone()
                with pytest.raises(RuntimeError, match="index outside"):
                    ops.mesh_intersections(good, t, grid=grid)
                assert torch.equal(t, t0)
    # the entry counts them and leaves the faces out: fan40 has 80 faces, one of them bad
    t = tris.clone()
    t[1, 2] = -1
    ws = torch.empty(_lib.call("o2345_mesh_intersect_workspace_bytes", v.shape[0], f.shape[0]), dtype=torch.uint8, device=dev)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    _lib.call("o2345_mesh_intersect_count", good, t, 8, v.shape[0], f.shape[0], None, 0, 0, ws, ws.numel(), counts, None)
    assert counts.tolist()[:4] == [1, 0, 79, 0]
    with pytest.raises(ValueError):
        ops.mesh_intersections(good, tris.float())
    with pytest.raises(ValueError):
        ops.mesh_intersections(good.float(), tris)
    # the C ABI itself: null pointers, a short workspace, bad sizes, a grid that is too small, no grid above 2^16 triangles
    nv, nt = v.shape[0], f.shape[0]
    size = lambda a, b: _lib.call("o2345_mesh_intersect_workspace_bytes", a, b)
    wsb = size(nv, nt)
    assert wsb > 0 and size(2 ** 30, 0) == 0 and size(-1, 0) == 0 and size(0, -1) == 0 and size(0, 2 ** 31 // 3 + 1) == 0 and size(0, 0) > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    G = ops.mesh_distance_grid(good, tris)
    gp, gb, gm = G.buffer, G.buffer.numel(), G.max_cells
    many = 2 ** 16 + 1
    big_ws = torch.empty(size(nv, many), dtype=torch.uint8, device=dev)
    big_tris = torch.zeros(many, 3, dtype=torch.int32, device=dev)
    for a, what in (((None, tris, 8, nv, nt, gp, gb, gm, ws, wsb, counts, None), "null pointer"), ((good, None, 8, nv, nt, gp, gb, gm, ws, wsb, counts, None), "null pointer"),
                    ((good, tris, 8, nv, nt, gp, gb, gm, None, wsb, counts, None), "null pointer"), ((good, tris, 8, nv, nt, gp, gb, gm, ws, wsb, None, None), "null pointer"),
                    ((good, tris, 8, nv, nt, gp, gb, gm, ws, wsb - 1, counts, None), "workspace too small"), ((good, tris, 2, nv, nt, gp, gb, gm, ws, wsb, counts, None), "index_bytes"),
                    ((good, tris, 8, 2 ** 30, nt, gp, gb, gm, ws, wsb, counts, None), "bad sizes"), ((good, tris, 8, nv, nt, gp, 64, gm, ws, wsb, counts, None), "grid of 64 bytes"),
                    ((good, tris, 8, nv, nt, gp, gb, 0, ws, wsb, counts, None), "max_cells"), ((good, tris, 8, nv, nt, gp, gb, 2 ** 24 + 1, ws, wsb, counts, None), "max_cells"),
                    ((good, big_tris, 4, nv, many, None, 0, 0, big_ws, big_ws.numel(), counts, None), "without a grid")):
        with pytest.raises(RuntimeError, match=what):
            _lib.call("o2345_mesh_intersect_count", *a)
    pairs = torch.empty(4, 2, dtype=torch.int32, device=dev)
    for a, what in (((good, tris, 8, nv, nt, gp, gb, gm, None, 4, pairs), "null pointer"), ((good, tris, 8, nv, nt, gp, gb, gm, ws, 4, None), "null pointer"),
                    ((None, tris, 8, nv, nt, gp, gb, gm, ws, 4, pairs), "null pointer"), ((good, tris, 8, nv, nt, gp, gb, gm, ws, -1, pairs), "bad pair count"),
                    ((good, tris, 8, nv, nt, gp, gb, gm, ws, 2 ** 30, pairs), "bad pair count"), ((good, tris, 3, nv, nt, gp, gb, gm, ws, 4, pairs), "index_bytes"),
                    ((good, tris, 8, nv, -1, gp, gb, gm, ws, 4, pairs), "bad sizes"), ((good, tris, 8, nv, nt, gp, 64, gm, ws, 4, pairs), "grid of 64 bytes"),
                    ((good, big_tris, 4, nv, many, None, 0, 0, big_ws, 4, pairs), "without a grid")):
        with pytest.raises(RuntimeError, match=what):
            _lib.call("o2345_mesh_intersect_emit", *a)
    U.assert_equal_reports(_raw(dev, v, f, torch.int64), U.twin("fan40"))


def test_a_mesh_without_a_face_that_takes_part_gives_zeros(dev):
    """64 triangles and more go to the grid, which refuses a mesh without an area: ops turns that into the report"""
    v = np.zeros((5, 3))
    f = np.tile(np.array([[0, 1, 2]]), (100, 1))
    got = ops.mesh_intersections(torch.from_numpy(v).to(dev), _dev_tris(f, dev, torch.int64), return_pairs=True)
    U.assert_equal_reports(_host(got), mio.mesh_intersections(v, f, return_pairs=True))
    assert [got[k] for k in COUNTS] == [0, 0, 0, 100, 0, 0, 0, 0]


def test_pipeline_report_is_there_when_on_and_nothing_runs_when_off(tmp_path, dev, monkeypatch):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    on = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64, mesh_intersections=True)
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    T = lambda t: t.to(dev).contiguous().float()
    vol = pipeline.build_volume(wt, T(s["images"]), T(s["affine_mats"]), s["partial_vol_origin"].numpy(), 48, 2.0 / 47)
    proj, cam_pos = pipeline.camera_terms(T(s["intrinsics"]), T(s["w2cs"]))
    v, t, _, _ = pipeline.extract_mesh(wt, vol, proj, cam_pos, 64, return_index_verts=True)
    hv, hf = v.cpu().numpy(), t.cpu().numpy()
    want = mio.mesh_intersections(hv, hf, return_pairs=True)
    plain = {k: want[k] for k in COUNTS}
    assert on["triangles"] == plain["faces"] + plain["skipped"] > 0 and on["mesh_intersections"] == plain
    assert pipeline.mesh_intersections((v, t)) == plain
    U.assert_equal_reports(_host(pipeline.mesh_intersections((hv, hf.astype(np.int32)), return_pairs=True)), want)       # host arrays are uploaded
    # off, which is the default: no key, and the unit's entries are not reached
    assert config.MESH_INTERSECTIONS is False                             # the environment of the test run leaves it unset
    monkeypatch.setattr(ops, "mesh_intersections", lambda *a, **k: pytest.fail("the report must not run when it is off"))
    real = _lib.call
    monkeypatch.setattr(ops, "call", lambda name, *a: pytest.fail("the unit's entry was reached") if "intersect" in name else real(name, *a))
    for kw in (dict(), dict(mesh_intersections=None), dict(mesh_intersections=False)):
        off = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64, **kw)
        assert "mesh_intersections" not in off and set(off) == set(on) - {"mesh_intersections"} and all(off[k] == on[k] for k in off if k != "ply")
        assert open(off["ply"], "rb").read() == open(on["ply"], "rb").read()
