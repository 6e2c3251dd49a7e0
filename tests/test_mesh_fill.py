"""CPU: the host twin of the hole filling (mesh_io.fill_holes), which defines what csrc/mesh_fill.hip computes.  Expected values are facts of the meshes
(counted by hand from the definition, or the audit twin's), never the code under test."""
import ctypes
import importlib
import math
import os
import sys

import numpy as np
import pytest

import mesh_audit_util as A
import mesh_fill_util as U
import mesh_simplify_util as S

mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")
_lib = importlib.import_module("one-2-3-45_amd._lib")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(U.TABLE))
def test_the_table_of_the_definition(name):
    v, f, n = U.cases()[name]
    out = U.twin(name)
    assert U.counts(out[5], v.shape[0], f.shape[0]) == U.TABLE[name] and all(type(x) is int for x in out[5].values())
    assert list(out[5]) == list(mio.FILL_COUNTS) and len(mio.FILL_COUNTS) == 8
    U.check_result(v, f, n, out)


@pytest.mark.parametrize("name", sorted(U.cases()))
def test_the_properties_of_the_definition(name):
    v, f, n = U.cases()[name]
    before, after = U.check_result(v, f, n, U.twin(name))
    if name in U.MANIFOLD:
        assert after["boundary_edges"] == 0 and after["watertight"] and after["oriented"] and before["oriented"] and not before["watertight"]


def test_a_hole_of_three_edges_gets_its_face_back():
    v, f, _ = U.cases()["tetrahedron_open"]
    wv, wf, _, _, hole, info = U.twin("tetrahedron_open")
    assert wv.shape == (4, 3) and hole.tolist() == [0] and wf[3].tolist() == [2, 3, 1]         # o = (2, 1, 3) from the leader 2 -> 1 on: (o_0, o_2, o_1)
    canon = lambda t: {tuple(np.roll(x, -int(np.argmin(x)))) for x in t.tolist()}
    assert canon(wf) == canon(A.tetrahedron()[1])
    r = mio.mesh_audit(wv, wf)
    assert r["watertight"] and r["oriented"] and abs(r["volume"] - 1.0 / 6.0) < 1e-15
    # a single triangle gains its reversed copy
    v1, f1, _ = U.cases()["grid_nt1"]
    w1 = U.twin("grid_nt1")
    assert w1[1].shape == (2, 3) and sorted(w1[1][1].tolist()) == sorted(f1[0].tolist()) and mio.mesh_audit(w1[0], w1[1])["boundary_edges"] == 0
    # nothing at all
    v0, f0, _ = U.cases()["grid_nt0"]
    w0 = mio.fill_holes(v0, f0)
    assert w0[0] is v0 and w0[1] is f0 and w0[4].shape == (0,)


def test_the_cube_gets_its_side_back():
    v, f, _ = U.cases()["cube_open"]
    wv, wf, _, _, hole, info = U.twin("cube_open")
    r = mio.mesh_audit(wv, wf)
    assert r["watertight"] and r["oriented"] and r["euler"] == 2 and r["unused_vertices"] == 81 and wf.shape[0] == f.shape[0] + 40 and wv.shape[0] == 603
    assert abs(S.signed_volume(wv, wf) - S.signed_volume(*S.cube10())) < 1e-9                  # the cap lies in the face's plane
    assert (hole == 0).all() and np.allclose(wv[602], [5.37, 3.79, 12.93], rtol=0, atol=1e-12)   # the centre of the side
    # under another numbering of the vertices: the same counts, and after mapping back the same vertex set and face set
    rv, rf, perm = A.relabelled(v, f)
    xv, xf, _, _, _, xinfo = U.twin("cube_open_relabelled")
    assert xinfo == info
    back = np.concatenate([np.argsort(perm), [602]])                     # new id -> old id; the new vertex stays the last
    assert np.array_equal(xv[:602][perm], v) and np.allclose(xv[602], wv[602], rtol=0, atol=1e-12)
    canon = lambda t: {tuple(np.roll(x, -int(np.argmin(x)))) for x in t.tolist()}
    assert canon(back[xf]) == canon(wf)


@pytest.mark.parametrize("k", U.CONES)
def test_the_centroid_is_the_sequential_sum(k):
    v, f, _ = U.cases()[f"cone{k}"]
    wv, wf, _, _, hole, info = U.twin(f"cone{k}")
    rim = wf[f.shape[0]:, 1]                                             # o_k in rank order
    assert wv.shape[0] == v.shape[0] + 1 and sorted(rim.tolist()) == list(range(2, 2 + k)) and (wf[f.shape[0]:, 2] == v.shape[0]).all()
    assert np.array_equal(wf[f.shape[0]:, 0], np.roll(rim, -1))
    for a in range(3):
        exact, scale = math.fsum(v[rim, a]) / k, math.fsum(np.abs(v[rim, a])) / k
        assert abs(wv[-1, a] - exact) <= 1e-12 * scale
        acc = 0.0
        for o in rim:
            acc = acc + float(v[o, a])
        assert wv[-1, a] == acc / k


def test_selection_by_length():
    v, f, n = U.cases()["sphere_small"]
    assert n == 3
    small, every = U.twin("sphere_small"), U.twin("sphere_all")
    long_hole = every[5]["longest"]
    assert every[5]["holes"] == 2 and every[5]["open"] == 0 and long_hole > 3 and every[5]["boundary"] == long_hole + 3
    assert U.counts(small[5], v.shape[0], f.shape[0]) == (long_hole + 3, 2, 1, 1, 0, long_hole, 0, 1)
    assert mio.mesh_audit(small[0], small[1])["boundary_edges"] == long_hole
    assert U.counts(every[5], v.shape[0], f.shape[0]) == (long_hole + 3, 2, 2, 0, 0, long_hole, 1, long_hole + 1)
    assert mio.fill_holes(v, f, long_hole)[5] == every[5] and mio.fill_holes(v, f, long_hole - 1)[5]["filled"] == 1
    for bad in (0, 1, 2, -3, 2 ** 31, 3.5, True):
        with pytest.raises(ValueError, match="max_edges"):
            mio.fill_holes(v, f, bad)
    with pytest.raises(ValueError, match="index outside"):
        mio.fill_holes(v[:10], f)


def test_the_pinholes_come_back_in_leader_order():
    v, f, removed = U.cube_pinholes()
    wv, wf, _, _, hole, info = U.twin("cube_pinholes")
    assert hole.tolist() == list(range(20)) and wv.shape == v.shape
    canon = lambda t: [tuple(np.roll(x, -int(np.argmin(x)))) for x in t.tolist()]
    assert set(canon(wf[f.shape[0]:])) == set(canon(removed)) and set(canon(wf)) == set(canon(S.cube10()[1]))
    # leader order: the smallest half-edge of every hole ascends with the hole's number
    half = {(int(a), int(b)): 3 * t + i for t, x in enumerate(f) for i, (a, b) in enumerate(zip(x, np.roll(x, -1)))}
    leaders = [min(half[(int(b), int(a))] for a, b in zip(x, np.roll(x, -1))) for x in wf[f.shape[0]:]]
    assert leaders == sorted(leaders)


def test_refusals_and_no_ops_leave_the_input():
    for name in ("three_on_an_edge", "bowtie_grids", "tetrahedron_one_reversed", "torus", "grid_one_reversed"):
        v, f, n = U.cases()[name]
        out = mio.fill_holes(v, f, n)
        assert out[0] is v and out[1] is f and out[4].shape == (0,) and out[5]["filled"] == 0 and out[5]["vertices"] == v.shape[0]
    # a repeated-index triangle next to a hole is copied through and takes no part
    v, f, _ = U.cases()["defects"]
    wv, wf = U.twin("defects")[:2]
    assert wf[:f.shape[0]].tolist() == f.tolist() and [4, 4, 5] in wf.tolist() and mio.mesh_audit(wv, wf)["repeated_faces"] == 1


def test_colours_and_normals_of_a_new_vertex_are_the_rims_means():
    v, f, _ = U.cases()["grid_3_2"]
    rng = np.random.default_rng(3)
    col, nrm = rng.integers(0, 256, (v.shape[0], 4)).astype(np.uint8), rng.standard_normal((v.shape[0], 3)).astype(np.float32)
    wv, wf, wc, wn, hole, info = mio.fill_holes(v, f.astype(np.int32), None, col, nrm)
    rim = wf[f.shape[0]:, 1]
    assert wf.dtype == np.int32 and wc.dtype == np.uint8 and wn.dtype == np.float32 and wc.shape == (13, 4) and wn.shape == (13, 3) and len(rim) == 10
    assert wc[:12].tobytes() == col.tobytes() and wn[:12].tobytes() == nrm.tobytes()
    assert wc[12].tolist() == [int(math.floor(col[rim, k].astype(np.int64).sum() / 10 + 0.5)) for k in range(4)]
    assert np.allclose(wn[12], nrm[rim].astype(np.float64).mean(0), atol=1e-6)


def test_convert_mesh_fills_on_the_way(tmp_path):
    v, f, _ = U.cases()["cube_open"]
    col = np.random.default_rng(5).integers(0, 256, (v.shape[0], 3)).astype(np.uint8)
    ply, off, on = str(tmp_path / "m.ply"), str(tmp_path / "off.glb"), str(tmp_path / "on.glb")
    mio.write_ply_numpy(ply, v.astype(np.float32), f.astype(np.int32), col)
    mio.convert_mesh(ply, off)
    mio.convert_mesh(ply, str(tmp_path / "zero.glb"), fill_holes=0)
    assert open(off, "rb").read() == open(str(tmp_path / "zero.glb"), "rb").read()
    mio.convert_mesh(ply, on, fill_holes=40)
    p, t, c, _ = mio.read_glb(on)
    assert p.shape == (603, 3) and t.shape == (f.shape[0] + 40, 3) and c.shape[0] == 603
    assert mio.mesh_audit(p.astype(np.float64), t)["boundary_edges"] == 0
    mio.convert_mesh(ply, str(tmp_path / "short.glb"), fill_holes=39)
    assert mio.read_glb(str(tmp_path / "short.glb"))[0].shape == (602, 3)


def test_config(monkeypatch):
    assert config.MESH_FILL_HOLES == 0 and config.mesh_fill_holes() == 0 and config.MESH_FILL_HOLES_ALL == 2 ** 31 - 1 == mio.FILL_HOLES_ALL
    assert config.mesh_fill_holes(3) == 3 and config.mesh_fill_holes(0) == 0 and config.mesh_fill_holes(config.MESH_FILL_HOLES_ALL) == 2 ** 31 - 1
    for bad in (1, 2, -1, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError):
            config.mesh_fill_holes(bad)
    monkeypatch.setattr(config, "MESH_FILL_HOLES", 64)
    assert config.mesh_fill_holes() == 64 and config.mesh_fill_holes(0) == 0
    # the environment variable, read at import
    import subprocess
    run = lambda value: subprocess.run([sys.executable, "-c", "import importlib; print(importlib.import_module('one-2-3-45_amd.config').MESH_FILL_HOLES)"],
                                       cwd=ROOT, env=dict(os.environ, O2345_MESH_FILL_HOLES=value), capture_output=True, text=True)
    assert run("40").stdout.strip() == "40" and run("").stdout.strip() == "0" and run("0").stdout.strip() == "0"
    assert run("2").returncode != 0 and "O2345_MESH_FILL_HOLES" in run("2").stderr
    # the option is a keyword of its own: the record of the mesh options is what it was
    assert config.MeshOptions._fields == ("min_component_faces", "keep_largest", "decimate_cell", "project_iterations", "project_max_move", "smooth_iterations",
                                          "texture_texel", "simplify_faces")
    assert config.mesh_options() == config.MeshOptions(0, False, 0.0, 0, 1.0, 0, 0, 0)


def test_the_entries_validate_before_touching_the_device():
    """o2345_mesh_fill_count rejects what it cannot do with a message, on the host, ahead of every HIP call (this test runs without a GPU)"""
    lib = _lib.lib()
    size = lambda nv, nt: _lib.call("o2345_mesh_fill_workspace_bytes", nv, nt)
    assert size(2 ** 30, 1) == 0 and size(-1, 1) == 0 and size(1, -1) == 0 and size(0, 2 ** 31 // 3 + 1) == 0 and size(0, 0) > 0
    assert size(100, 200) <= size(101, 200) <= size(101, 201) <= size(1000, 2000) and size(100, 200) % 16 == 0
    nv, nt = 100, 200
    wsb = size(nv, nt)
    dummy = 4096                                                         # non-null, 16-byte aligned, never dereferenced: every call below fails in the checks

    def call(tris=dummy, ib=8, nv=nv, nt=nt, max_edges=3, ws=dummy, wsb=wsb, counts=dummy):
        rc = lib.o2345_mesh_fill_count(ctypes.c_void_p(tris), ib, nv, nt, max_edges, ctypes.c_void_p(ws), ctypes.c_size_t(wsb), ctypes.c_void_p(counts), None)
        return rc, lib.o2345_last_error().decode()

    for kw, what in ((dict(ws=None), "null pointer"), (dict(wsb=wsb - 1), "workspace too small"), (dict(ws=dummy + 8), "16-byte aligned"),
                     (dict(ib=2), "index_bytes must be 4 or 8"), (dict(max_edges=2), "max_edges"), (dict(max_edges=2 ** 31), "max_edges"),
                     (dict(nv=2 ** 30), "bad sizes"), (dict(tris=None), "null pointer"), (dict(counts=None), "null pointer"),
                     (dict(counts=dummy + 4), "8-byte aligned")):
        rc, msg = call(**kw)
        assert rc != 0 and what in msg and msg.startswith("mesh_fill_count"), (kw, rc, msg)
    # the counts are a device array: the binding's census of host pointers does not grow, and the header declares no new struct
    params = {p.name: p for p in _lib.prototypes()["o2345_mesh_fill_count"][1]}
    assert params["counts"].elem == "int64" and not any(p.host for p in params.values())
    rc = lib.o2345_mesh_fill_emit(None, ctypes.c_void_p(dummy), 2, nv, nt, ctypes.c_void_p(dummy), None, None, None, None)
    assert rc != 0 and "index_bytes" in lib.o2345_last_error().decode()
    rc = lib.o2345_mesh_fill_emit(None, ctypes.c_void_p(dummy), 8, nv, nt, None, None, None, None, None)
    assert rc != 0 and "null pointer" in lib.o2345_last_error().decode()


def test_the_tool_on_the_host(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        tool = importlib.import_module("mesh_fill")
    finally:
        sys.path.pop(0)
    v, f, _ = U.cases()["cube_open"]
    col = np.random.default_rng(7).integers(0, 256, (v.shape[0], 4)).astype(np.uint8)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    mio.write_ply_numpy(src, v.astype(np.float32), f.astype(np.int32), col)
    info = tool.main([src, dst, "--host", "--json"])
    assert __import__("json").loads(capsys.readouterr().out) == info and info["filled"] == 1 and info["vertices"] == 603
    p, t, c = mio.read_ply(dst)
    assert p.shape == (603, 3) and t.shape == (f.shape[0] + 40, 3) and c[:602].tobytes() == col.tobytes()
    rim = t[f.shape[0]:, 1]
    assert c[602].tolist() == [int((2 * col[rim, k].astype(np.int64).sum() + 40) // 80) for k in range(4)]
    assert mio.mesh_audit(p.astype(np.float64), t)["watertight"]
    assert tool.main([src, str(tmp_path / "short.obj"), "--host", "--max-edges", "39"])["filled"] == 0
