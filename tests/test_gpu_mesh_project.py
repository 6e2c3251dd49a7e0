"""GPU: projection of mesh vertices onto the SDF's zero set (csrc/mesh_project.hip) against the host twin (mesh_io.project_vertices), which defines the
result.  The twin's field is the device's own SDF kernel (ops.sdf_mlp, variant 2, the same precision), everything else is fp64 in a defined order: every
comparison is EXACT (bytes, whole info dicts).  Expected values are the host twin applied to the same inputs, or facts of the definition, never the code
under test."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from guard_util import PRE, Guard
from mesh_scene_util import args as _args, bits as _bits, dev, fields_at as _fields_at, golden_mirror, sdf_field as _field, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("one-2-3-45_amd")
ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")
STATS_BYTES = ctypes.sizeof(_lib.STRUCTS["O2345ProjectStats"])        # the block at its exact size: one byte more written and a guard band shows it

NVS = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2049)          # the 32-point tile of the SDF kernels, the 64-lane ballot, the 256-thread block
PRECISIONS = ("f16x3", "fp32")
INFO_KEYS = {"evaluated", "converged", "unconverged", "stalled", "clamped", "max_before", "max_after"}
TOL = 5e-5


@pytest.fixture(scope="module")
def scene(dev):
    """the stored small scene (D = 20), its marching-cubes mesh at R = 64 and the twin's cell-2 decimation of it"""
    S = stored_scene(dev)
    hv, hf = S["hv"], S["hf"]
    assert hv.shape[0] > 2049 and hf.shape[0] > 100
    dec = mio.decimate_mesh(hv, hf, 2.0)
    assert 100 < dec[4]["vertices"] < hv.shape[0] // 2
    hv.setflags(write=False)
    return dict(S, dec=dec, twins={})


def _twin(S, hv, prec, iterations, key=None, **kw):
    """mesh_io.project_vertices with the device's kernel as the field; computed once per key and shared"""
    if key is not None and (key, prec, iterations) in S["twins"]:
        return S["twins"][(key, prec, iterations)]
    out = mio.project_vertices(hv, _field(S["wt"].sdf_blob, S["vol"]["vol_cl"], prec), S["R"], iterations, **kw)
    out[0].setflags(write=False)
    if key is not None:
        S["twins"][(key, prec, iterations)] = out
    return out


def _check(S, hv, prec, iterations, key=None, **kw):
    """ops.mesh_project == the twin, exactly; the input is only read -> (device vertices, info)"""
    hv = np.array(hv, np.float64).reshape(-1, 3)
    dev = S["vol"]["vol_cl"].device
    verts = torch.from_numpy(hv).to(dev)
    v, info = ops.mesh_project(S["wt"].sdf_blob, S["vol"]["vol_cl"], verts, S["R"], iterations, precision=prec, **kw)
    wv, winfo = _twin(S, hv, prec, iterations, key, **kw)
    assert set(info) == INFO_KEYS and info == winfo, (info, winfo)
    assert type(info["max_before"]) is float and type(info["max_after"]) is float and len(info["evaluated"]) == iterations + 1
    assert v.dtype == torch.float64 and v.shape == hv.shape and v.cpu().numpy().tobytes() == wv.tobytes()
    assert verts.cpu().numpy().tobytes() == hv.tobytes() and v is not verts
    return v, info


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("iterations", [1, 4])
def test_device_equals_twin_at_every_tile_wave_and_block_boundary(scene, prec, iterations):
    for nv in NVS:
        _, info = _check(scene, scene["hv"][:nv], prec, iterations, key=("prefix", nv))
        assert info["evaluated"][0] == nv
    assert info["max_before"] > 1e-2 and info["evaluated"][1] < 2049                 # something to do, and some vertices leave after round 0


@pytest.mark.parametrize("prec", PRECISIONS)
def test_device_equals_twin_on_other_inputs(scene, prec):
    S = scene
    # the twin's decimation, whose cluster means may travel two spacings
    _, info = _check(S, S["dec"][0], prec, 4, key="dec2", max_move=2.0)
    assert info["max_before"] > 1e-2
    # another level set
    _, info = _check(S, S["hv"][:700], prec, 4, level=0.01)
    assert info["converged"] > 0
    # other limits: a step clamp that binds and a box that stops vertices
    _, info = _check(S, S["dec"][0], prec, 3, max_step=0.05, max_move=0.125, tol=1e-6)
    assert info["clamped"] > 0 and info["unconverged"] > 0
    # a vertex far outside the volume (its float32 world point overflows: the network returns no finite value there) and one that starts converged
    done = _twin(S, S["hv"], prec, 6, key="all")[0]
    hv = np.array(S["hv"][:100])
    hv[40] = 1e40
    hv[77] = done[77]
    v, info = _check(S, hv, prec, 4)
    assert info["stalled"] == 1 and v[40].cpu().numpy().tobytes() == hv[40].tobytes() and v[77].cpu().numpy().tobytes() == hv[77].tobytes()


@pytest.mark.parametrize("prec", PRECISIONS)
def test_quality_six_rounds_leave_every_vertex_within_tol(scene, prec):
    S = scene
    for hv, key, kw in ((S["hv"], "all", {}), (S["dec"][0], "dec2", dict(max_move=2.0))):
        v, info = _check(S, hv, prec, 6, key=key, **kw)
        print(prec, key, info)
        assert info["unconverged"] == 0
        pts = (v / (S["R"] - 1.0) * 2.0 - 1.0).to(torch.float32).contiguous()
        s = ops.sdf_mlp(S["wt"].sdf_blob, S["vol"]["vol_cl"], pts, variant=2, precision=prec)["sdf"]
        print(float(s.abs().max()))
        assert float(s.abs().max()) <= TOL                                           # the kernel the op uses: no cross-kernel rounding in between


def test_two_runs_and_a_second_stream_give_identical_bytes(scene, dev):
    S = scene
    verts = torch.from_numpy(np.array(S["hv"])).to(dev)
    torch.cuda.synchronize()
    runs = []
    side = torch.cuda.Stream(device=dev)
    for stream in (None, None, side):
        with torch.cuda.stream(stream):
            v, info = ops.mesh_project(S["wt"].sdf_blob, S["vol"]["vol_cl"], verts, S["R"], 4)
            runs.append((v.cpu().numpy().tobytes(), info))
    assert runs[0] == runs[1] == runs[2]


def test_off_launches_nothing(scene, dev, monkeypatch):
    S = scene
    verts = torch.from_numpy(np.array(S["hv"])).to(dev)

    class Dead:
        def __getattr__(self, name):
            pytest.fail(f"iterations = 0 must not reach the library ({name})")
    monkeypatch.setattr(_lib, "_LIB", Dead())
    assert config.MESH_PROJECT_ITERATIONS == 0                            # the environment of the test run leaves it unset
    for it in (0, None):
        out = ops.mesh_project(S["wt"].sdf_blob, S["vol"]["vol_cl"], verts, S["R"], it)
        assert out[0] is verts and out[1] is None


def test_errors_are_statuses_not_faults(scene, dev):
    """each refusal on a few vertices: counted on the device or refused on the host, raised, and the next call works"""
    S = scene
    blob, vol_cl, R = S["wt"].sdf_blob, S["vol"]["vol_cl"], S["R"]
    good = torch.from_numpy(np.array(S["hv"][:70])).to(dev)
    for bad in (float("nan"), float("inf"), float("-inf")):
        v = good.clone()
        v[37, 1] = bad
        with pytest.raises(RuntimeError, match="non-finite"):
            ops.mesh_project(blob, vol_cl, v, R, 2)
        _check(S, S["hv"][:70], "f16x3", 2)
    for kw in (dict(iterations=65), dict(iterations=-1), dict(tol=-1.0), dict(tol=float("nan")), dict(max_step=0.0), dict(max_step=float("inf")),
               dict(max_move=0.0), dict(max_move=float("nan")), dict(level=float("nan")), dict(bound_min=(1.0, -1.0, -1.0)), dict(resolution=1)):
        a = dict(resolution=R, iterations=2)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.mesh_project(blob, vol_cl, good, **a)
    with pytest.raises(ValueError):
        ops.mesh_project(blob, vol_cl, good.float(), R, 2)
    with pytest.raises(ValueError):
        ops.mesh_project(blob, vol_cl, good.view(-1), R, 2)
    # through the C ABI: a workspace that is too small, bad arguments, output = input
    L = _lib.lib()
    nv = good.shape[0]
    wsb = L.o2345_mesh_project_workspace_bytes(nv)
    assert wsb > 0 and L.o2345_mesh_project_workspace_bytes(-1) == 0 and L.o2345_mesh_project_workspace_bytes(2 ** 30) == 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out, stats = torch.empty(nv, 3, dtype=torch.float64, device=dev), torch.empty(STATS_BYTES, dtype=torch.uint8, device=dev)
    b0, b1 = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(wsb_=wsb, it=2, mode=2, tol=TOL, step=0.5, move=1.0, out_=out, bmax=b1):
        return L.o2345_mesh_project(P(blob), P(vol_cl), vol_cl.shape[0], mode, P(good), nv, R, H(b0), H(bmax), it, 0.0, tol, step, move, P(ws), wsb_, P(out_),
                                    P(stats), s)
    for kw, what in ((dict(wsb_=wsb - 1), "workspace too small"), (dict(it=65), "iterations"), (dict(it=0), "iterations"), (dict(mode=1), "sdf_mode"),
                     (dict(tol=-1.0), "tol"), (dict(step=0.0), "max_step"), (dict(move=float("nan")), "max_move"), (dict(out_=good), "verts_out"),
                     (dict(bmax=b0), "bound_max")):
        assert call(**kw) == -1 and what in L.o2345_last_error().decode(), kw
    assert call() == 0
    torch.cuda.synchronize()
    want = _twin(S, S["hv"][:70], "f16x3", 2)
    assert out.cpu().numpy().tobytes() == want[0].tobytes() and ops.project_info(stats.cpu().numpy(), 2) == want[1]


# ---- guard bands (tests/guard_util.py): the output, the stats block and the workspace at their EXACT sizes --------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_no_kernel_writes_outside_its_buffers(scene, dev, prec):
    S = scene
    L = _lib.lib()
    g = Guard(dev)
    blob, vol_cl, R = S["wt"].sdf_blob, S["vol"]["vol_cl"], S["R"]
    b0, b1 = np.full(3, -1.0, np.float32), np.full(3, 1.0, np.float32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    H = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert PRE % 16 == 0
    for nv in NVS:
        hv = np.array(S["hv"][:nv])
        verts = torch.from_numpy(hv).to(dev)
        wsb = L.o2345_mesh_project_workspace_bytes(nv)
        assert wsb > 0
        ws, out, stats = g.buf(wsb, ("workspace", nv)), g.buf(24 * nv, ("verts_out", nv)), g.buf(STATS_BYTES, ("stats", nv))
        _lib.check(L.o2345_mesh_project(P(blob), P(vol_cl), vol_cl.shape[0], 2 if prec == "f16x3" else 0, P(verts), nv, R, H(b0), H(b1), 4, 0.0, TOL, 0.5, 1.0,
                                        P(ws), wsb, P(out), P(stats), s), "mesh_project")
        bad = g.damaged()
        assert not bad, bad
        wv, winfo = _twin(S, hv, prec, 4, key=("prefix", nv))
        assert out.cpu().numpy().tobytes() == wv.tobytes() and ops.project_info(stats.cpu().numpy(), 4) == winfo, nv
        assert verts.cpu().numpy().tobytes() == hv.tobytes()
    assert len(g.live) == 3 * len(NVS)


# ---- the pipeline on the stored small scene (D = 20, R = 64) ------------------------------------------------------------------------------------
def _pipeline_twins(S):
    """(vertices, faces, info) the pipeline must produce with project_iterations = 4: without decimation, and after the twin's cell-2 decimation, where
    the move limit is max(1, cell) = 2"""
    prec = S["wt"].sdf_precision
    p0 = _twin(S, S["hv"], prec, 4, key="all")
    p2 = _twin(S, S["dec"][0], prec, 4, key="dec2", max_move=2.0)
    return (p0[0], S["hf"], p0[1]), (p2[0], S["dec"][1], p2[1])


def test_extract_mesh_with_projection(scene, dev):
    S = scene
    for (wv, wf, winfo), kw in zip(_pipeline_twins(S), (dict(), dict(decimate_cell=2))):
        unprojected = pipeline.extract_mesh(*_args(S), return_index_verts=True, **kw)
        v, t, rgb, u = pipeline.extract_mesh(*_args(S), return_index_verts=True, project_iterations=4, **kw)
        assert v.cpu().numpy().tobytes() == wv.tobytes() and _bits(t, unprojected[1]) and np.array_equal(t.cpu().numpy(), wf) and _bits(u, S["plain"][3])
        assert v.cpu().numpy().tobytes() != unprojected[0].cpu().numpy().tobytes()
        # gradient and colours are taken at the PROJECTED vertices
        fields = pipeline._mesh_fields(*_args(S), config.mesh_options(project_iterations=4, **kw))
        info = fields.info
        want_rgb, want_g = _fields_at(S, torch.from_numpy(np.array(wv)).to(dev))
        assert _bits(rgb, want_rgb) and _bits(fields[3], want_rgb) and _bits(fields[5], want_g)
        assert info["project"] == winfo and (info["decimate"] is None) == (not kw)
        assert torch.equal(fields[0], v / (S["R"] - 1.0) * 2.0 - 1.0) and _bits(fields[1], v)
        # smoothing runs last, on the projected mesh, and does not touch the colours
        vs, ts, rgbs, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, project_iterations=4, smooth_iterations=3, **kw)
        assert vs.cpu().numpy().tobytes() == mio.smooth_vertices(wv, wf, 3).tobytes() and _bits(ts, t) and _bits(rgbs, want_rgb)


def test_exports_with_projection_equal_the_export_of_the_twins_mesh(scene, dev, tmp_path):
    S = scene
    scale = np.eye(4, dtype=np.float32); scale[:3, :3] *= 0.9; scale[:3, 3] = [0.01, 0.02, -0.03]
    B = lambda p: open(p, "rb").read()
    for k, ((wv, wf, _), kw) in enumerate(zip(_pipeline_twins(S), (dict(), dict(decimate_cell=2.0)))):
        wv, wf = torch.from_numpy(np.array(wv)).to(dev), torch.from_numpy(np.array(wf)).to(dev)
        rgb = _fields_at(S, wv)[0]
        got, want = str(tmp_path / f"g{k}.ply"), str(tmp_path / f"w{k}.ply")
        n = pipeline.export_mesh_ply(got, *_args(S), scale_mat=scale[None], project_iterations=4, **kw)
        assert n == (wv.shape[0], wf.shape[0])
        assert n == mio.export_mesh(want, wv, wf, S["R"], scale_mat=scale[None], vertex_colors=rgb) and B(got) == B(want)
        for ext in (".glb", ".obj"):
            got, want = str(tmp_path / (f"g{k}" + ext)), str(tmp_path / (f"w{k}" + ext))
            assert pipeline.export_mesh_asset(got, *_args(S), scale_mat=scale[None], project_iterations=4, **kw) == n
            mio.export_asset(want, wv, wf, S["R"], scale_mat=scale[None], vertex_colors=rgb)
            assert B(got) == B(want), ext


def test_projection_off_is_todays_output(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    assert config.MESH_PROJECT_ITERATIONS == 0                            # the environment of the test run leaves it unset
    monkeypatch.setattr(ops, "mesh_project", lambda *a, **k: pytest.fail("projection must not run when it is off"))
    for kw in (dict(project_iterations=0), dict(project_iterations=None), dict()):
        off = pipeline.extract_mesh(*_args(S), return_index_verts=True, **kw)
        for a, b in zip(S["plain"], off):
            assert _bits(a, b)
        info = pipeline._mesh_fields(*_args(S), config.mesh_options(**kw)).info
        assert info["project"] is None
        for ext in (".ply", ".glb", ".obj"):
            p0, p1 = str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))
            fn = pipeline.export_mesh_ply if ext == ".ply" else pipeline.export_mesh_asset
            want = (mio.export_mesh if ext == ".ply" else mio.export_asset)(p0, S["plain"][0], S["plain"][1], S["R"], vertex_colors=S["plain"][2])
            assert fn(p1, *_args(S), **kw) == want
            assert B(p0) == B(p1)


def test_config_default_reaches_the_pipeline(scene, monkeypatch):
    S = scene
    (wv, wf, _), _ = _pipeline_twins(S)
    monkeypatch.setattr(config, "MESH_PROJECT_ITERATIONS", 4)
    v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True)
    assert v.cpu().numpy().tobytes() == wv.tobytes() and np.array_equal(t.cpu().numpy(), wf)
    v, _, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, project_iterations=1)          # an explicit count wins
    assert v.cpu().numpy().tobytes() == _twin(S, S["hv"], S["wt"].sdf_precision, 1, key="all")[0].tobytes()
    off = pipeline.extract_mesh(*_args(S), return_index_verts=True, project_iterations=0)                 # and so does an explicit 0
    for a, b in zip(S["plain"], off):
        assert _bits(a, b)


def test_reconstruct_folder_reports_the_iterations_and_the_info(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a.ply"), D=48, resolution=64)
    assert plain["project_iterations"] == 0 and plain["project"] is None and plain["triangles"] > 0
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b.ply"), D=48, resolution=64, project_iterations=3)
    # the twin on the plain mesh: the same scene once more through the pieces
    s = ds.SceneFolder(str(tmp_path), "export_mesh", specific_dataset_name="shape")[0]
    T = lambda t: t.to(dev).contiguous().float()
    vol = pipeline.build_volume(wt, T(s["images"]), T(s["affine_mats"]), s["partial_vol_origin"].numpy(), 48, 2.0 / 47)
    proj, cam_pos = pipeline.camera_terms(T(s["intrinsics"]), T(s["w2cs"]))
    v, t, _, _ = pipeline.extract_mesh(wt, vol, proj, cam_pos, 64, return_index_verts=True)
    winfo = mio.project_vertices(v.cpu().numpy(), _field(wt.sdf_blob, vol["vol_cl"], wt.sdf_precision), 64, 3)[1]
    assert out["project_iterations"] == 3 and out["project"] == winfo and winfo["evaluated"][0] == plain["vertices"]
    assert (out["vertices"], out["triangles"]) == (plain["vertices"], plain["triangles"])


# ---- the drop-in mirror ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_extract_geometry_applies_the_configured_projection(dev, monkeypatch):
    ren, sdf, dense = golden_mirror(dev)
    D = dense.shape[2]
    R = 48
    call = lambda threshold=0, **kw: ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=R, threshold=threshold, device=dev,
                                                          conditional_volume=dense, lod=0, **kw)
    field = _field(sdf.sdf_layer.blob(), dense[0].permute(1, 2, 3, 0).contiguous(), None)
    mask = torch.ones(D, D, D, device=dev)
    mask[: D // 2] = 0
    plain = {th: call(th) for th in (0, 0.01)}
    masked = call(0, occupancy_mask=mask)
    monkeypatch.setattr(config, "MESH_PROJECT_ITERATIONS", 4)
    for th, (v0, t0, u0) in plain.items():
        assert t0.shape[0] > 0
        # the mirror projects INDEX coordinates and maps them to world units afterwards: the twin on marching cubes of the u it returns
        vi, ti = ops.marching_cubes(torch.from_numpy(u0).to(dev).contiguous(), float(th))
        assert np.array_equal(ti.cpu().numpy(), t0)
        wv, winfo = mio.project_vertices(vi.cpu().numpy(), field, R, 4, level=-float(th))
        assert winfo["converged"] > 0 and winfo["max_before"] > 1e-3
        v, t, u = call(th)
        assert v.dtype == np.float64 and v.tobytes() == (wv / (R - 1) * 2.0 + -1.0).tobytes() and np.array_equal(t, t0) and u.tobytes() == u0.tobytes()
        # the converged vertices are where sdf = -threshold: the field itself at the float32 points says so
        s, _ = field(v.astype(np.float32))
        r = np.abs(s.astype(np.float64) + float(th))
        assert np.count_nonzero(r <= TOL) >= winfo["converged"] > v.shape[0] // 2
    # with an occupancy mask the vertices on the mask's walls are not on the level set: no projection
    v, t, u = call(0, occupancy_mask=mask)
    assert v.tobytes() == masked[0].tobytes() and np.array_equal(t, masked[1]) and u.tobytes() == masked[2].tobytes()
