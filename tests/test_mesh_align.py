"""CPU: the host twin of the mesh alignment (mesh_io.similarity_step / align_meshes: the definition of what csrc/mesh_align.hip and ops.mesh_align
compute), the unit's workspace sizes, its exported symbols and its kernels' resource usage.  No GPU needed."""
import ctypes
import importlib
import json
import math
import os
import sys

import numpy as np
import pytest

import mesh_align_util as A
import mesh_distance_util as U
import resource_usage

mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
_lib = importlib.import_module("one-2-3-45_amd._lib")


# ---- the solve -------------------------------------------------------------------------------------------------------------------------------------
def synthetic_row(u, seed=0, n=40):
    """the moments of n random Jacobians whose residuals are exactly J . u: the system's solution is u"""
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(n, 7))
    w = rng.uniform(0.5, 2.0, n)
    b = J @ u
    row = np.zeros(48)
    H = (w[:, None, None] * J[:, :, None] * J[:, None, :]).sum(0)
    row[:28] = H[np.triu_indices(7)]
    row[28:35] = (w[:, None] * J * b[:, None]).sum(0)
    return row


def test_similarity_step_solves_exact_rows_and_composes():
    u = np.array([0.02, -0.03, 0.01, 0.1, -0.2, 0.05, 0.04])
    M_inc, shift, got = mesh_io.similarity_step(synthetic_row(u))
    assert np.abs(got - u).max() < 1e-12 and np.abs(shift - u[3:6]).max() < 1e-12
    R = M_inc / math.exp(got[6])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14 and abs(np.cbrt(np.linalg.det(M_inc)) - math.exp(u[6])) < 1e-12
    assert np.abs(R - mesh_io.rodrigues(u[:3])).max() < 1e-12
    # without scale: the leading 6 x 6, sigma stays 0
    u6 = np.concatenate([u[:6], [0.0]])
    M6, _, got6 = mesh_io.similarity_step(synthetic_row(u6), scale=False)
    assert got6[6] == 0.0 and np.abs(got6 - u6).max() < 1e-12 and abs(np.linalg.det(M6) - 1.0) < 1e-14
    # M <- M_inc M, t <- M_inc (t - c) + c + tau: a point x goes to c + M_inc (T x - c) + tau
    T = np.concatenate([1.3 * mesh_io.rodrigues([0.3, 0.1, -0.2]), [[0.5], [-1.0], [2.0]]], 1)
    c, x = np.array([0.2, 0.4, -0.6]), np.array([1.0, -2.0, 0.5])
    T2 = mesh_io.compose_similarity(T, M_inc, shift, c)
    assert np.abs((T2[:, :3] @ x + T2[:, 3]) - (c + M_inc @ (T[:, :3] @ x + T[:, 3] - c) + shift)).max() < 1e-14
    # the small-angle series and the closed form of the rotation agree where they meet
    assert np.abs(mesh_io.rodrigues([0.99e-4, 0, 0]) - mesh_io.rodrigues([1.01e-4, 0, 0])).max() < 3e-6
    assert np.array_equal(mesh_io.rodrigues([0, 0, 0]), np.eye(3))


def test_similarity_step_reports_a_degenerate_system():
    assert mesh_io.similarity_step(np.zeros(48)) is None                                   # singular
    row = synthetic_row(np.ones(7) * 0.01)
    bad = row.copy(); bad[3] = np.nan
    assert mesh_io.similarity_step(bad) is None
    bad = row.copy(); bad[30] = np.inf
    assert mesh_io.similarity_step(bad) is None
    plane = np.zeros(48)                                              # every normal along z, every sample at the pivot: only tau_z is determined
    H = np.zeros((7, 7)); H[5, 5] = 3.0
    plane[:28] = H[np.triu_indices(7)]
    assert mesh_io.similarity_step(plane) is None and mesh_io.similarity_step(plane, scale=False) is None


def test_rotation_candidates():
    R = mesh_io.rotation_candidates(8)
    assert R.shape == (8, 3, 3) and np.array_equal(R[0], np.eye(3))
    assert np.abs(R[2] - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])).max() < 1e-15 and np.abs(R[4] - np.diag([-1.0, -1.0, 1.0])).max() < 1e-15
    Ry = mesh_io.rotation_candidates(4, up=(0, 2, 0))
    assert np.abs(Ry[1] @ np.array([0, 0, 1.0]) - np.array([1.0, 0, 0])).max() < 1e-15 and np.abs(Ry[:, :, 1] - np.array([0, 1.0, 0])).max() < 1e-15
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="n_azimuth"):
            mesh_io.rotation_candidates(bad)
    with pytest.raises(ValueError, match="up"):
        mesh_io.rotation_candidates(4, up=(0, 0, 0))


# ---- the twin on the fixture -------------------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_blob_of_the_issue():
    v, f = A.blob()
    assert v.shape == (162, 3) and f.shape == (320, 3) and len({tuple(sorted(t)) for t in f.tolist()}) == 320
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    assert len(np.unique(edges, axis=0)) == 480 and 2.5 < A.diameter() < 3.5       # closed: every edge twice; V - E + F = 2
    for name, s in (("small", 1.15), ("large", 0.8)):
        T = A.move(name)
        assert abs(np.cbrt(np.linalg.det(T[:3, :3])) - s) < 1e-15 and np.array_equal(T[:3, 3], A.SHIFT)
    assert np.abs(A.move("large")[:3, :3] @ np.array([0, 0, 1.0]) - np.array([0, 0, 0.8])).max() < 1e-15


def test_small_move_from_the_identity_converges_to_rounding():
    r = A.twin_run("small", 0)
    print("small: iterations", r["iterations"], "worst vertex", A.worst_vertex(r["transform"], "small"), "score", r["score"])
    assert r["converged"] and r["iterations"] <= 15 and r["candidate"] == 0 and len(r["candidate_scores"]) == 1
    assert A.worst_vertex(r["transform"], "small") <= 1e-9
    assert abs(r["scale"] - 1.15) < 1e-9 and np.abs(r["rotation"] @ r["rotation"].T - np.eye(3)).max() < 1e-12
    assert np.abs(r["transform"][:3, :3] - r["scale"] * r["rotation"]).max() < 1e-15 and np.array_equal(r["transform"][:3, 3], r["translation"])
    assert r["inlier_fraction"] == 1.0 and r["rms"] < 1e-12 and r["score"] < 1e-24
    h = r["history"]
    assert len(h) == r["iterations"] + 1 and h[-1]["update"] is None and h[-2]["update"] < 1e-9 and all(e["inliers"] == 320 and e["unmatched"] == 0 for e in h)
    assert h[0]["score"] > 1e-4 > h[-1]["score"] and all(e["transform"].shape == (3, 4) for e in h)


def test_large_move_needs_the_azimuth_search():
    alone = A.twin_run("large", 0)
    worst_alone = A.worst_vertex(alone["transform"], "large")
    r = A.twin_run("large", 8)
    print("large: identity alone ends", worst_alone, "of the diameter away; candidate scores", r["candidate_scores"], "worst vertex",
          A.worst_vertex(r["transform"], "large"))
    assert worst_alone >= 0.1
    assert r["candidate"] == 4 and r["converged"] and len(r["candidate_scores"]) == 8
    assert A.worst_vertex(r["transform"], "large") <= 1e-9
    assert r["candidate_scores"][4] * 100.0 <= r["candidate_scores"][0]
    assert abs(r["scale"] - 0.8) < 1e-9 and r["iterations"] >= 5 and len(r["history"]) == r["iterations"] + 1


def test_rigid_move_without_scale_and_a_given_start():
    v, f = A.blob()
    T = np.eye(4)
    T[:3, :3] = mesh_io.rodrigues(np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0) * np.deg2rad(20.0))
    T[:3, 3] = A.SHIFT
    b = v @ T[:3, :3].T + T[:3, 3]
    r = mesh_io.align_meshes(v, f, b, f, scale=False)
    err = np.sqrt(((mesh_io.transform_vertices(v, r["transform"]) - b) ** 2).sum(1)).max() / A.diameter(b)
    assert r["converged"] and err <= 1e-9 and abs(r["scale"] - 1.0) < 1e-14
    # init replaces moment matching: from the answer itself nothing is left to do
    r2 = mesh_io.align_meshes(v, f, b, f, scale=False, init=T)
    assert r2["converged"] and r2["iterations"] == 1 and r2["history"][0]["score"] < 1e-28
    r3 = mesh_io.align_meshes(v, f, b, f, init=T[:3], iterations=0)
    assert not r3["converged"] and r3["iterations"] == 0 and np.array_equal(r3["transform"], T) and len(r3["history"]) == 1


def test_max_distance_leaves_the_transform_of_the_clean_case():
    """a far-away extra component: in the target it is never the closest triangle and only moves the start (the moments of B's samples); in the source its
    samples are rejected"""
    v, f = A.blob()
    b = A.moved("small")
    clean = A.twin_run("small", 0)
    extra = U.octahedron((9.0, 4.0, -6.0), 0.02)
    tv, tf = U.joined((b, f), extra)
    r = mesh_io.align_meshes(v, f, tv, tf, max_distance=1.0)
    assert r["converged"] and np.abs(r["transform"] - clean["transform"]).max() <= 1e-9 * A.diameter(b) and r["inlier_fraction"] == 1.0
    sv, sf = U.joined((v, f), extra)
    r = mesh_io.align_meshes(sv, sf, b, f, max_distance=1.0)
    assert r["converged"] and np.abs(r["transform"] - clean["transform"]).max() <= 1e-9 * A.diameter(b)
    assert r["history"][-1]["rejected"] == 8 and r["history"][-1]["inliers"] == 320 and 0.99 < r["inlier_fraction"] < 1.0
    assert abs(r["score"] - (1.0 - r["inlier_fraction"])) < 1e-12                       # the rejected count max_distance^2 = 1 each
    loose = mesh_io.align_meshes(sv, sf, b, f)
    assert np.abs(loose["transform"] - clean["transform"]).max() > 1e-4                  # without the truncation the extra component pulls


def test_terms_without_a_target_give_centroid_and_radius():
    v, f = A.blob()
    pts, w, _ = mesh_io.surface_samples(v, f)
    t = mesh_io.align_terms(pts, w, np.eye(3, 4).reshape(1, 12))
    row = mesh_io.align_moments(t["terms"])[0]
    assert (row[:35] == 0).all() and row[36] == 0 and row[35] == row[37] == math.fsum(w) and (row[43], row[44], row[45], row[46], row[47]) == (320, 0, 0, 0, 0)
    c = row[39:42] / row[35]
    assert np.abs(c - (w[:, None] * pts).sum(0) / w.sum()).max() < 1e-14 and (t["nearest"] == -1).all() and (t["d2"] == 0).all()
    # an all-degenerate target: every pair is unmatched
    t = mesh_io.align_terms(pts, w, np.eye(3, 4).reshape(1, 12), v, np.array([[0, 0, 1], [2, 2, 2]]))
    assert (t["terms"][..., :45] == 0).all() and (t["terms"][..., 45] == 1).all() and np.isinf(t["d2"]).all() and (t["nearest"] == -1).all()


@pytest.mark.parametrize("what, kw", [
    ("iterations", dict(iterations=-1)),
    ("iterations", dict(iterations=2.5)),
    ("search_iterations", dict(search_iterations=-2)),
    ("tol", dict(tol=float("nan"))),
    ("candidates", dict(candidates=np.zeros((0, 3, 3)))),
    ("candidates", dict(candidates=np.tile(np.eye(3), (65, 1, 1)))),
    ("candidates", dict(candidates=np.eye(3))),
    ("candidates", dict(candidates=np.full((2, 3, 3), np.nan))),
    ("max_distance", dict(max_distance=-0.5)),
    ("max_distance", dict(max_distance=float("inf"))),
    ("max_distance", dict(max_distance=float("nan"))),
    ("init", dict(init=np.eye(3))),
    ("init", dict(init=np.full((3, 4), np.inf))),
    ("spacing", dict(spacing=0.0)),
])
def test_refusals_name_the_argument(what, kw):
    v, f = A.blob()
    with pytest.raises(ValueError, match=what):
        mesh_io.align_meshes(v, f, A.moved("small"), f, **kw)


def test_refusals_of_the_pieces():
    v, f = A.blob()
    with pytest.raises(ValueError, match="transforms"):
        mesh_io.align_terms(v, None, np.zeros((65, 12)))
    with pytest.raises(ValueError, match="non-finite"):
        mesh_io.align_terms(v, None, np.full((1, 12), np.nan))
    with pytest.raises(ValueError, match="align"):
        mesh_io.mesh_distance(v, f, v, f, align="yes")
    with pytest.raises(ValueError, match="mesh B has no surface"):
        mesh_io.align_meshes(v, f, v, np.array([[0, 0, 1]]))


def test_distance_with_alignment_and_unchanged_without():
    v, f = A.blob()
    b = A.moved("large")
    plain = mesh_io.mesh_distance(v, f, b, f)
    assert "alignment" not in plain and plain == mesh_io.mesh_distance(v, f, b, f, align=None) and plain["chamfer"] > 0.05 * A.diameter(b)
    r = mesh_io.mesh_distance(v, f, b, f, align=True)
    assert set(r) == set(plain) | {"alignment"} and r["alignment"]["candidate"] == 4 and r["chamfer"] <= 1e-9 * A.diameter(b)
    r1 = mesh_io.mesh_distance(v, f, b, f, align={"candidates": None})                      # a dict is taken as it is: the identity alone
    assert r1["alignment"]["candidate_scores"] == A.twin_run("large", 0)["candidate_scores"] and r1["chamfer"] > 1e-3 * A.diameter(b)


# ---- the device unit, as far as this machine can see it ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("o2345_mesh_align_workspace_bytes", "o2345_mesh_align_step")


def test_new_entries_are_declared_exported_and_additive():
    protos = _lib.prototypes()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in protos and getattr(lib, name) is not None, name
        assert name in open(_lib.HEADER).read().split("int o2345_version(void);")[0], f"{name} is missing from the header's list of additive entries"
    assert lib.o2345_version() == 231 and _lib.ABI_VERSION == 231
    assert protos["o2345_mesh_align_workspace_bytes"][0] is ctypes.c_size_t and protos["o2345_mesh_align_step"][0] is ctypes.c_int
    params = {p.name: p for p in protos["o2345_mesh_align_step"][1]}
    assert not any(p.host for p in params.values()) and len(params) == 24
    assert all(params[k].ctype is ctypes.c_double and params[k].elem is None for k in ("max_distance", "pivot_x", "pivot_y", "pivot_z"))
    assert params["tris"].elem == params["grid"].elem == "void" and params["moments"].elem == "float64" and params["nearest"].elem == "int32"


def test_workspace_sizes():
    """one row of 48 doubles per transform and tile of 4,096 samples (at least one row, so that 0 only ever means bad sizes)"""
    lib = _lib.lib()
    size = lib.o2345_mesh_align_workspace_bytes
    assert [size(n, 1) for n in (0, 1, 4096, 4097, 10 ** 6)] == [384, 384, 384, 768, 384 * 245]
    assert size(4097, 3) == 3 * 768 and size(1, 64) == 64 * 384 and size(2 ** 28 - 1, 1) == 384 * 65536
    assert [size(-1, 1), size(2 ** 28, 1), size(10, 0), size(10, -1), size(10, 65)] == [0] * 5


@pytest.mark.skipif(not resource_usage.HAVE_HIPCC, reason="needs hipcc")
def test_kernels_use_no_scratch(tmp_path):
    usage = resource_usage.kernel_usage("mesh_align.hip", r"(\S+)", lambda m: m.group(1), tmp_path)
    mine = {k: u for k, u in usage.items() if "k_ma_" in k}
    assert sum("k_ma_step" in k for k in mine) == 6 and sum("k_ma_final" in k for k in mine) == 1          # three modes x two index widths
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
    print({k[:40]: (u["VGPRs"], u["Occupancy"]) for k, u in mine.items()})


def test_command_line_tool_prints_the_twins_report(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        tool = importlib.import_module("mesh_distance")
    finally:
        sys.path.pop(0)
    v, f = A.blob()
    b = A.moved("large")
    for name, verts in (("a.ply", v), ("b.ply", b)):
        mesh_io.write_ply_numpy(str(tmp_path / name), verts.astype(np.float32), f.astype(np.int32))
    (va, fa), (vb, fb) = mesh_io.load_mesh_pair(str(tmp_path / "a.ply"), str(tmp_path / "b.ply"))          # the float32 vertices of the files
    saved = str(tmp_path / "moved.ply")
    out = tool.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--threshold", "0.01", "--align", "--host", "--save-aligned", saved])
    want = mesh_io.mesh_distance(va, fa, vb, fb, None, (0.01,), align=True)
    assert json.loads(capsys.readouterr().out) == out == json.loads(json.dumps(want, default=lambda x: x.tolist()))
    assert out["alignment"]["candidate"] == 4 and out["alignment"]["converged"] and out["fscore"] == [1.0] and out["hausdorff"] < 1e-5
    sv, sf = mesh_io.read_ply(saved)[:2]
    assert np.abs(sv - vb).max() < 1e-5 and np.array_equal(sf, fb)
    # the other options reach the twin: one azimuth is the identity alone, which stays in the wrong minimum
    out1 = tool.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--align-azimuths", "1", "--align-no-scale", "--align-max-distance", "5", "--host"])
    capsys.readouterr()
    want1 = mesh_io.mesh_distance(va, fa, vb, fb, align={"candidates": None, "scale": False, "max_distance": 5.0})
    assert out1 == json.loads(json.dumps(want1, default=lambda x: x.tolist())) and abs(out1["alignment"]["scale"] - 1.0) < 1e-14 and out1["hausdorff"] > 0.1
    up = tool.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--align-azimuths", "4", "--align-up", "0,0,2", "--host"])
    capsys.readouterr()
    assert up["alignment"]["candidate"] == 2 and len(up["alignment"]["candidate_scores"]) == 4 and up["hausdorff"] < 1e-5
