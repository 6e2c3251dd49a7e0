"""GPU: the tangent-space normal map of the textured asset (csrc/mesh_texture.hip: k_tex_frames, k_tex_normal_pack) against the host twins
(mesh_io.texture_frames / pack_normal_map), which define the result.  Everything outside the two networks is fp64 in a defined order: every comparison is
EXACT (bytes, the counters included).  Expected values are the host twins applied to the same inputs, or the library's own network kernels at the twin's
points, never the code under test."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import mesh_normal_map_util as U
from guard_util import Guard
from mesh_scene_util import args as _args, colours_at, dev, stored_scene  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")

# 85 triangles are 255 corners, 86 are 258: the two straddle a 256-thread block of k_tex_frames; odd counts repeat the B half of the last cell
COUNTS = (1, 2, 3, 5, 33, 85, 86, 171)
TEXELS = (4, 5, 64)


def _B(t):
    return t.contiguous().cpu().numpy().tobytes()


def _counters(t):
    return ops.normal_map_counts(t.cpu().numpy())


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("c", TEXELS)
def test_frames_and_pack_equal_the_twins(dev, c, rot):
    T = U.rotation() if rot else None
    for nt in COUNTS:
        case = U.strip(nt, c, seed=nt * 100 + c, rot=T)
        wN, wTW, degenerate = mio.texture_frames(case["pos"], case["uv"])
        wimage, wcounts = mio.pack_normal_map(case["grad"], wN, wTW, nt, c, T)
        assert degenerate == len(case["degenerate"]) and wcounts["bad_gradient"] == 3 and wcounts["back_facing"] >= len(case["back"])
        verts, grad = torch.from_numpy(case["v"]).to(dev), torch.from_numpy(case["grad"]).to(dev)
        for dtype in (torch.int32, torch.int64):
            pos, uv, _, _, _ = ops.mesh_texture_corners(verts, torch.from_numpy(case["f"]).to(dev).to(dtype), c, 512, trans_mat=T)
            for t in case["degenerate"]:
                pos[3 * t + 1] = pos[3 * t]
                pos[3 * t + 2] = pos[3 * t]
            assert _B(pos) == case["pos"].tobytes() and _B(uv) == case["uv"].tobytes()
            nrm, tan, counters = ops.mesh_texture_frames(pos, uv)
            assert nrm.dtype == tan.dtype == torch.float32 and tuple(nrm.shape) == (3 * nt, 3) and tuple(tan.shape) == (3 * nt, 4)
            assert _B(nrm) == wN.tobytes() and _B(tan) == wTW.tobytes(), (nt, c)          # bytes: the sign of the marking zero included
            assert counters.cpu().tolist() == [degenerate, 0, 0, 0]
            image = ops.mesh_texture_normal_pack(grad, nrm, tan, nt, c, rotation=T, counters=counters)
            assert image.dtype == torch.uint8 and tuple(image.shape) == wimage.shape and _B(image) == wimage.tobytes(), (nt, c)
            assert _counters(counters) == dict(wcounts, degenerate=degenerate) and counters[3].item() == 0
            assert _B(pos) == case["pos"].tobytes() and _B(grad) == case["grad"].tobytes() and _B(nrm) == wN.tobytes()          # inputs are only read
        # the rotation as a device array, and without a block of the caller's
        if rot:
            r9 = torch.from_numpy(np.ascontiguousarray(T[0, :3, :3])).to(dev)
            assert _B(ops.mesh_texture_normal_pack(grad, nrm, tan, nt, c, rotation=r9)) == wimage.tobytes()


# ---- the pipeline on the stored small scene (D = 20, R = 64), the scene of tests/test_gpu_mesh_texture.py -------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    return dict(stored_scene(dev, extract=False), cache={})


def _expected(S, project, trans):
    """the twin chain: texture_corners -> texture_frames -> gradients and colours of the network kernels at the twin's (optionally projected) texel points
    -> pack_normal_map / pack_texture"""
    key = (project, trans is not None)
    if key not in S["cache"]:
        dev = S["vol"]["vol_cl"].device
        v, t, _, _ = pipeline.extract_mesh(*_args(S), return_index_verts=True, decimate_cell=2, project_iterations=project)
        hv, hf = v.cpu().numpy(), t.cpu().numpy()
        nt = hf.shape[0]
        assert 100 < nt < 20000
        pts, world = mio.texture_points(hv, hf, 4, S["R"])
        world = torch.from_numpy(world).to(dev)
        if project:
            p, _ = ops.mesh_project(S["wt"].sdf_blob, S["vol"]["vol_cl"], torch.from_numpy(pts).to(dev), S["R"], project, max_move=2.0, precision=S["wt"].sdf_precision)
            world = (p / (S["R"] - 1.0) * 2.0 - 1.0).to(torch.float32).contiguous()
        rgb, grad = colours_at(S, world)
        grad = grad.cpu().numpy()
        pos, uv, _, bounds = mio.texture_corners(hv, hf, 4, S["R"], trans_mat=trans)
        N, TW, degenerate = mio.texture_frames(pos, uv)
        nimage, counts = mio.pack_normal_map(grad, N, TW, nt, 4, trans)
        S["cache"][key] = dict(nt=nt, pos=pos, uv=uv, bounds=bounds, N=N, TW=TW, grad=grad, nimage=nimage, image=mio.pack_texture(rgb.cpu().numpy(), nt, 4),
                               counts=dict(counts, degenerate=degenerate))
    return S["cache"][key]


@pytest.mark.parametrize("project, rot", [(0, False), (2, True)])
def test_normal_mapped_glb_end_to_end(scene, tmp_path, project, rot):
    S = scene
    T = U.rotation() if rot else None
    E = _expected(S, project, T)
    nt = E["nt"]
    path, plain = str(tmp_path / "n.glb"), str(tmp_path / "t.glb")
    kw = dict(decimate_cell=2, project_iterations=project, texture_texel=4, trans_mat=T, normals=True)
    assert pipeline.export_mesh_asset(path, *_args(S), normal_map=True, **kw) == (3 * nt, nt)
    assert pipeline.export_mesh_asset(plain, *_args(S), **kw) == (3 * nt, nt)
    tangents, nimage = mio.read_glb_normal_map(path)
    p, f, col, nr = mio.read_glb(path)
    uv, img, _ = mio.read_glb_texture(path)
    assert nimage.tobytes() == E["nimage"].tobytes() and tangents.tobytes() == E["TW"].tobytes() and nr.tobytes() == E["N"].tobytes()      # NORMAL is the flat normal
    # the decode bound of the definition, on every texel of a used cell with a valid gradient (and a triangle that has a frame)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((E["grad"].astype(np.float64) ** 2).sum(1))
    valid = (length > 0) & np.isfinite(length) & ~mio.frame_is_degenerate(tangents[3 * U.owners(nt, 4)])
    assert int((~(length > 0) | ~np.isfinite(length)).sum()) == E["counts"]["bad_gradient"] and valid.sum() > 0.99 * valid.size
    angles = U.decode_angles(nimage, nr, tangents, nt, 4, mio.frame_normals(E["grad"], T))[valid]
    print(f"normal map decode, project = {project}, rotation = {rot}: max angle {angles.max():.3e} rad, bound {U.DECODE_BOUND:.3e}; counts {E['counts']}")
    assert angles.max() <= U.DECODE_BOUND
    used, rest = U.to_cells(nimage, nt, 4)
    assert (rest == U.FLAT).all() and not (used == U.FLAT).all() and len(np.unique(used, axis=0)) > 100          # not all flat: the coarse mesh lost detail
    # everything else is the file without the map: base colour, positions, uv, indices
    pp, pf, _, pn = mio.read_glb(plain)
    puv, pimg, _ = mio.read_glb_texture(plain)
    assert mio.read_glb_normal_map(plain) is None and pn.tobytes() != nr.tobytes()
    assert img.tobytes() == pimg.tobytes() == E["image"].tobytes() and p.tobytes() == pp.tobytes() == E["pos"].tobytes() and uv.tobytes() == puv.tobytes() == E["uv"].tobytes()
    assert np.array_equal(f, pf)
    # and the file is the twin writers' file
    want = str(tmp_path / "want.glb")
    mio.write_textured(want, E["pos"], E["uv"], E["N"], E["image"], E["bounds"], tangents=E["TW"], normal_image=E["nimage"])
    assert open(path, "rb").read() == open(want, "rb").read()


def test_two_runs_and_a_second_stream_give_identical_files_and_the_obj_agrees(scene, dev, tmp_path):
    S = scene
    B = lambda p: open(p, "rb").read()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    files = []
    for k, stream in enumerate((None, None, side)):
        with torch.cuda.stream(stream):
            d = tmp_path / f"run{k}"
            os.mkdir(d)
            for ext in (".glb", ".obj"):
                pipeline.export_mesh_asset(str(d / ("mesh" + ext)), *_args(S), decimate_cell=2, texture_texel=4, normal_map=True)
            assert sorted(os.listdir(d)) == ["mesh.glb", "mesh.mtl", "mesh.obj", "mesh.png", "mesh_normal.png"]
            files.append([B(d / n) for n in sorted(os.listdir(d))])
    assert files[0] == files[1] == files[2]
    d = tmp_path / "run0"
    E = _expected(S, 0, None)
    p, f, _, nr = mio.read_glb(str(d / "mesh.glb"))
    tangents, nimage = mio.read_glb_normal_map(str(d / "mesh.glb"))
    assert nimage.tobytes() == E["nimage"].tobytes()
    op, ouv, on, of, oimg = mio.read_obj_texture(str(d / "mesh.obj"))
    assert np.array_equal(mio.read_obj_normal_map(str(d / "mesh.obj")), nimage) and B(d / "mesh_normal.png") == mio.png_bytes(nimage, 1)
    assert np.array_equal(oimg, mio.read_glb_texture(str(d / "mesh.glb"))[1]) and np.array_equal(of, f)
    assert np.abs(op - p).max() <= 0.5e-8 and np.abs(on - nr).max() <= 0.5e-8             # the vn records carry the flat normals
    K = mio.obj_coordinate_digits(p)
    assert B(d / "mesh.obj") == mio.obj_texture_header(str(d / "mesh.obj")) + mio.obj_texture_text_numpy(p, mio.read_glb_texture(str(d / "mesh.glb"))[0], nr, K)
    # smoothing comes last: the gradients are the unsmoothed surface's, the frames follow the positions that are written
    sm = str(tmp_path / "s.glb")
    pipeline.export_mesh_asset(sm, *_args(S), decimate_cell=2, texture_texel=4, normal_map=True, smooth_iterations=2)
    sp, _, _, sn = mio.read_glb(sm)
    stan, simage = mio.read_glb_normal_map(sm)
    assert sp.tobytes() != p.tobytes()
    wN, wTW, _ = mio.texture_frames(sp, mio.read_glb_texture(sm)[0])
    assert sn.tobytes() == wN.tobytes() and stan.tobytes() == wTW.tobytes()
    assert simage.tobytes() == mio.pack_normal_map(E["grad"], wN, wTW, E["nt"], 4)[0].tobytes()


def test_off_is_todays_path(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    assert config.MESH_NORMAL_MAP is False                                # the environment of the test run leaves it unset
    E = _expected(S, 0, None)
    for name in ("mesh_texture_frames", "mesh_texture_normal_pack"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"normal_map off must not reach ops.{_n}"))
    for k, flag in enumerate((None, False, 0)):
        for ext in (".glb", ".obj"):
            pipeline.export_mesh_asset(str(tmp_path / f"off{k}{ext}"), *_args(S), decimate_cell=2, texture_texel=4, normal_map=flag)
    assert not [n for n in os.listdir(tmp_path) if n.endswith("_normal.png")]
    # the textured file of the parent: the twin writers without the new arguments (their bytes are pinned on the CPU, tests/test_mesh_normal_map.py)
    want = str(tmp_path / "want.glb")
    mio.write_textured(want, E["pos"], E["uv"], None, E["image"], E["bounds"])
    mio.write_textured(str(tmp_path / "want.obj"), E["pos"], E["uv"], None, E["image"], E["bounds"])
    for k in range(3):
        assert B(tmp_path / f"off{k}.glb") == B(want)
        for ext in (".obj", ".mtl"):                                      # the two name their neighbours
            assert B(tmp_path / f"off{k}{ext}").replace(f"off{k}".encode(), b"want") == B(tmp_path / ("want" + ext))
        assert B(tmp_path / f"off{k}.png") == B(tmp_path / "want.png")
    with pytest.raises(ValueError, match="texture_texel"):
        pipeline.export_mesh_asset(str(tmp_path / "x.glb"), *_args(S), decimate_cell=2, normal_map=True)
    with pytest.raises(ValueError, match="ply"):
        pipeline.export_mesh_asset(str(tmp_path / "x.ply"), *_args(S), decimate_cell=2, texture_texel=4, normal_map=True)
    assert not os.path.exists(tmp_path / "x.glb") and not os.path.exists(tmp_path / "x.ply")


def test_config_default_reaches_the_pipeline(scene, tmp_path, monkeypatch):
    S = scene
    B = lambda p: open(p, "rb").read()
    want, plain, got, off = (str(tmp_path / n) for n in ("want.glb", "plain.glb", "got.glb", "off.glb"))
    pipeline.export_mesh_asset(want, *_args(S), decimate_cell=2, texture_texel=4, normal_map=True)
    pipeline.export_mesh_asset(plain, *_args(S), decimate_cell=2, texture_texel=4)
    monkeypatch.setattr(config, "MESH_NORMAL_MAP", True)
    pipeline.export_mesh_asset(got, *_args(S), decimate_cell=2, texture_texel=4)
    pipeline.export_mesh_asset(off, *_args(S), decimate_cell=2, texture_texel=4, normal_map=False)          # an explicit off wins
    assert B(got) == B(want) != B(plain) and B(off) == B(plain)
    with pytest.raises(ValueError, match="texture_texel"):                # the default needs the atlas too: an error, not a no-op
        pipeline.export_mesh_asset(got, *_args(S), decimate_cell=2)


def test_reconstruct_folder_reports_the_normal_map(tmp_path, dev):
    ds = importlib.import_module("one-2-3-45_amd.dataset")
    ds.write_synthetic_folder(str(tmp_path), "shape", seed=1)
    wt = pipeline.SceneWeights(dev, seed=0)
    os.mkdir(tmp_path / "a")
    os.mkdir(tmp_path / "b")
    kw = dict(D=48, resolution=64, output_format=".glb", decimate_cell=2, texture_texel=4)
    plain = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "a" / "m.ply"), **kw)
    out = pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "b" / "m.ply"), normal_map=True, **kw)
    assert "normal_map" not in plain["texture"] and out["texture"] == dict(plain["texture"], normal_map=True)
    assert {k: v for k, v in out.items() if k not in ("texture", "ply", "asset")} == {k: v for k, v in plain.items() if k not in ("texture", "ply", "asset")}
    assert open(out["ply"], "rb").read() == open(plain["ply"], "rb").read()
    tangents, nimage = mio.read_glb_normal_map(out["asset"])
    L = mio.texture_layout(plain["triangles"], 4)
    assert nimage.shape == (L["height"], L["width"], 4) and tangents.shape == (3 * plain["triangles"], 4) and mio.read_glb_normal_map(plain["asset"]) is None
    assert np.array_equal(mio.read_glb_texture(out["asset"])[1], mio.read_glb_texture(plain["asset"])[1])
    with pytest.raises(ValueError, match="texture_texel"):
        pipeline.reconstruct_folder(str(tmp_path), "shape", wt, str(tmp_path / "c.ply"), D=48, resolution=64, output_format=".glb", normal_map=True)


def test_errors_are_statuses_not_faults(dev):
    case = U.strip(33, 4, seed=1)
    pos, uv, grad = (torch.from_numpy(case[k]).to(dev) for k in ("pos", "uv", "grad"))
    nrm, tan, counters = ops.mesh_texture_frames(pos, uv)
    with pytest.raises(ValueError, match="CUDA"):
        ops.mesh_texture_frames(pos.cpu(), uv.cpu())
    with pytest.raises(ValueError, match="CUDA"):
        ops.mesh_texture_normal_pack(grad.cpu(), nrm.cpu(), tan.cpu(), 33, 4)
    for call in (lambda: ops.mesh_texture_frames(pos, uv.cpu()), lambda: ops.mesh_texture_frames(pos[:98], uv[:98]), lambda: ops.mesh_texture_frames(pos, uv[:96]),
                 lambda: ops.mesh_texture_frames(pos.double(), uv), lambda: ops.mesh_texture_frames(pos[:0], uv[:0]),
                 lambda: ops.mesh_texture_normal_pack(grad[:5], nrm, tan, 33, 4), lambda: ops.mesh_texture_normal_pack(grad, nrm[:3], tan, 33, 4),
                 lambda: ops.mesh_texture_normal_pack(grad, nrm, tan[:, :3], 33, 4), lambda: ops.mesh_texture_normal_pack(grad, nrm, tan, 33, 3),
                 lambda: ops.mesh_texture_normal_pack(grad, nrm, tan, 33, 65), lambda: ops.mesh_texture_normal_pack(grad, nrm.cpu(), tan, 33, 4),
                 lambda: ops.mesh_texture_normal_pack(grad, nrm, tan, 33, 4, rotation=np.eye(2)), lambda: ops.mesh_texture_normal_pack(grad, nrm, tan, 33, 4, counters=counters[:3]),
                 lambda: ops.mesh_texture_normal_pack(grad, nrm, tan, 33, 4, counters=counters.int()),
                 lambda: ops.mesh_texture_normal_pack(grad, nrm, tan, 33, 4, rotation=torch.eye(3, dtype=torch.float64, device=dev))):
        with pytest.raises(ValueError):
            call()
    # through the C ABI: null pointers, refused layouts and misaligned counters are statuses with a message
    L = _lib.lib()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    image = torch.empty(16, 20, 4, dtype=torch.uint8, device=dev)
    odd = torch.zeros(5, dtype=torch.int64, device=dev).view(torch.uint8)[4:36]
    err = lambda: L.o2345_last_error().decode()
    assert L.o2345_mesh_texture_frames(None, P(uv), 33, P(nrm), P(tan), P(counters), s) == -1 and "null" in err()
    assert L.o2345_mesh_texture_frames(P(pos), P(uv), 33, P(nrm), P(tan), None, s) == -1 and "null" in err()
    assert L.o2345_mesh_texture_frames(P(pos), P(uv), 0, P(nrm), P(tan), P(counters), s) == -1 and "size" in err()
    assert L.o2345_mesh_texture_frames(P(pos), P(uv), 2 ** 30, P(nrm), P(tan), P(counters), s) == -1 and "size" in err()
    assert L.o2345_mesh_texture_frames(P(pos), P(uv), 33, P(nrm), P(tan), P(odd), s) == -1 and "aligned" in err()
    assert L.o2345_mesh_texture_frames(P(pos), P(uv), 33, P(nrm), ctypes.c_void_p(tan.data_ptr() + 4), P(counters), s) == -1 and "aligned" in err()
    assert L.o2345_mesh_texture_normal_pack(None, None, P(nrm), P(tan), 33, 4, P(image), P(counters), s) == -1 and "null" in err()
    assert L.o2345_mesh_texture_normal_pack(P(grad), None, P(nrm), P(tan), 33, 4, None, P(counters), s) == -1 and "null" in err()
    for nt, c in ((0, 4), (33, 3), (33, 65), (2 * 256 * 256 + 1, 64)):
        assert L.o2345_mesh_texture_normal_pack(P(grad), None, P(nrm), P(tan), nt, c, P(image), P(counters), s) == -1 and "layout" in err()
    assert L.o2345_mesh_texture_normal_pack(P(grad), None, P(nrm), P(tan), 33, 4, P(image), P(odd), s) == -1 and "aligned" in err()
    assert L.o2345_mesh_texture_normal_pack(P(grad), None, P(nrm), P(tan), 33, 4, ctypes.c_void_p(image.data_ptr() + 2), P(counters), s) == -1 and "aligned" in err()
    # and the next call works
    wN, wTW, degenerate = mio.texture_frames(case["pos"], case["uv"])
    got = ops.mesh_texture_normal_pack(grad, nrm, tan, 33, 4, counters=counters)
    assert _B(got) == mio.pack_normal_map(case["grad"], wN, wTW, 33, 4)[0].tobytes() and _counters(counters)["degenerate"] == degenerate == 1


# ---- guard bands (tests/guard_util.py): every output of both entries at its EXACT size ---------------------------------------------------------------------
@pytest.mark.parametrize("rot", [False, True])
def test_no_kernel_writes_outside_its_buffers(dev, rot):
    L = _lib.lib()
    g = Guard(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    T = U.rotation() if rot else None
    r9 = None if T is None else g.buf(np.ascontiguousarray(T[0, :3, :3]), "rotation")
    for nt, c in ((33, 4), (86, 5)):
        case = U.strip(nt, c, seed=nt, rot=T)
        lay = mio.texture_layout(nt, c)
        pos, uv, grad = g.buf(case["pos"], ("positions", nt)), g.buf(case["uv"], ("uv", nt)), g.buf(case["grad"], ("grad", nt))
        nrm, tan, counters = g.buf(36 * nt, ("normals", nt)), g.buf(48 * nt, ("tangents", nt)), g.buf(32, ("counters", nt))
        image = g.buf(4 * lay["width"] * lay["height"], ("image", nt))
        _lib.check(L.o2345_mesh_texture_frames(P(pos), P(uv), nt, P(nrm), P(tan), P(counters), s), "mesh_texture_frames")
        _lib.check(L.o2345_mesh_texture_normal_pack(P(grad), None if r9 is None else P(r9), P(nrm), P(tan), nt, c, P(image), P(counters), s), "mesh_texture_normal_pack")
        bad = g.damaged()
        assert not bad, bad
        wN, wTW, degenerate = mio.texture_frames(case["pos"], case["uv"])
        wimage, wcounts = mio.pack_normal_map(case["grad"], wN, wTW, nt, c, T)
        assert _B(nrm) == wN.tobytes() and _B(tan) == wTW.tobytes() and _B(image) == wimage.tobytes()
        assert np.frombuffer(_B(counters), np.int64).tolist() == [degenerate, wcounts["bad_gradient"], wcounts["back_facing"], 0]
        assert _B(pos) == case["pos"].tobytes() and _B(uv) == case["uv"].tobytes() and _B(grad) == case["grad"].tobytes()
    assert len(g.live) == 7 * 2 + rot
