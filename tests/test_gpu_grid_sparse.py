"""GPU: the extraction lattice evaluated only where the scene has a latent (o2345_sdf_grid_sparse_x3: pre-pass k_grid_active_tiles + k_sdf_mlp_x3<true> on the
listed slots) against the full evaluation of the same library (o2345_sdf_grid_x3), same blob and tables, both signs: torch.equal, never a tolerance.
The activity rule itself is checked on the CPU (tests/test_grid_active_cpu.py).  A volume that is NOT zero wherever its mask is zero breaks the caller's
guarantee (include/o2345.h) and is outside these tests: its unkept-corner points get the background's value."""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
config = importlib.import_module("one-2-3-45_amd.config")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
synth = importlib.import_module("one-2-3-45_amd.synth")
_lib = importlib.import_module("one-2-3-45_amd._lib")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIGNS = (1.0, -1.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wt(dev):
    return pipeline.SceneWeights(dev, seed=0)


_BACKGROUND = {}


def _background(wt, R):
    """the background table of resolution R, built once through the op (not through SceneWeights.grid_background, whose counting test (e) is about)"""
    if R not in _BACKGROUND:
        empty = torch.zeros(2, 2, 2, 16, device=wt.sdf_blob.device)
        _BACKGROUND[R] = ops.sdf_mlp(wt.sdf_blob, empty, None, variant=0, grid_R=R, sign=1.0, grid_tables=wt.grid_tables(R))["sdf"]
    return _BACKGROUND[R]


def _volume(dev, D, kept, seed, zero_rows=()):
    """kept: bool [D,D,D] -> (vol_cl [D,D,D,16] with random latent rows on the kept voxels and zeros elsewhere, maskvol [D^3]); the kept voxels
    listed in zero_rows keep a latent row of zeros"""
    g = torch.Generator().manual_seed(seed)
    vol = torch.zeros(D, D, D, 16)
    vol[kept] = torch.randn(int(kept.sum()), 16, generator=g) * 0.5
    for v in zero_rows:
        assert kept[v]
        vol[v] = 0.0
    return vol.to(dev).contiguous(), kept.to(torch.float32).reshape(-1).to(dev).contiguous()


def _ball(D, centre, radius):
    ax = torch.linspace(-1, 1, D)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) <= radius ** 2


def _both(wt, vol_cl, maskvol, R, sign):
    """-> (full evaluation, sparse evaluation, listed slots)"""
    tabs = wt.grid_tables(R)
    full = ops.sdf_mlp(wt.sdf_blob, vol_cl, None, variant=0, grid_R=R, sign=sign, grid_tables=tabs)["sdf"]
    out = {"sdf": torch.full((R ** 3,), float("nan"), device=vol_cl.device)}              # a slot that neither kernel writes stays NaN and fails
    got = ops.sdf_mlp(wt.sdf_blob, vol_cl, None, variant=0, grid_R=R, sign=sign, grid_tables=tabs, maskvol=maskvol, grid_background=_background(wt, R),
                      out=out)["sdf"]
    return full, got, ops.sdf_grid_active_points(vol_cl.device)


def _tiles_with_a_sampled_point(R):
    """aligned 32-slot tiles with at least one point off the index-0 faces (where the sampler is on): what a FULL mask activates"""
    s = np.arange(R ** 3, dtype=np.int64)
    on = ((s % R) > 0) & (((s // R) % R) > 0) & ((s // (R * R)) > 0)
    pad = np.zeros(-(-R ** 3 // 32) * 32, bool)
    pad[:R ** 3] = on
    return int(pad.reshape(-1, 32).any(1).sum())


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("shape", ("blob", "scattered"))
def test_a_random_blob(dev, wt, sign, shape):
    """(a) R = 40 (tiles straddle rows), D = 16: about 30 % of the voxels kept -- one off-centre ball, or voxels drawn one by one -- with random latent rows"""
    R, D = 40, 16
    if shape == "blob":
        kept = _ball(D, (0.15, -0.1, 0.2), 0.8)
    else:
        kept = torch.rand(D, D, D, generator=torch.Generator().manual_seed(5)) < 0.3
    assert 0.2 < kept.float().mean() < 0.4
    vol_cl, maskvol = _volume(dev, D, kept, seed=1)
    full, got, listed = _both(wt, vol_cl, maskvol, R, sign)
    assert torch.equal(got, full)
    assert 0 < listed <= 32 * _tiles_with_a_sampled_point(R) and listed % 32 == 0
    assert torch.equal(got[:R * R], sign * _background(wt, R)[:R * R])          # the face ix = 0 is never sampled
    if shape == "blob":
        assert listed < 0.8 * R ** 3                        # the ball leaves the cube's corners to the background


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("case", ("first_corner", "last_corner", "zero_row"))
def test_b_single_voxels(dev, wt, sign, case):
    """(b) R = 64, D = 24: one kept voxel at a corner of the volume; a kept voxel whose latent row is all zeros (still listed and evaluated)"""
    R, D = 64, 24
    kept = torch.zeros(D, D, D, dtype=torch.bool)
    zero_rows = ()
    if case == "first_corner":
        kept[0, 0, 0] = True
    elif case == "last_corner":
        kept[D - 1, D - 1, D - 1] = True
    else:
        kept[11, 12, 13] = kept[11, 12, 14] = kept[5, 20, 2] = True
        zero_rows = ((11, 12, 13), (5, 20, 2))
    vol_cl, maskvol = _volume(dev, D, kept, seed=2, zero_rows=zero_rows)
    full, got, listed = _both(wt, vol_cl, maskvol, R, sign)
    assert torch.equal(got, full)
    # a voxel is a corner of the lattice points within one voxel of it: (2 * 63 / 23 + 1)^3 < 7^3 points, on at most 49 rows of two tiles each per voxel
    assert 0 < listed <= 32 * 2 * 49 * int(kept.sum())


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("R,D", ((40, 16), (33, 8)))
def test_c_empty_kept_set(dev, wt, sign, R, D):
    """(c) nothing kept: the count is 0, the network launch runs on an empty list, and the output is sign * background everywhere; R = 33 has the
    partial last tile"""
    vol_cl, maskvol = _volume(dev, D, torch.zeros(D, D, D, dtype=torch.bool), seed=3)
    full, got, listed = _both(wt, vol_cl, maskvol, R, sign)
    assert listed == 0
    assert torch.equal(got, sign * _background(wt, R))
    assert torch.equal(got, full)


@pytest.mark.parametrize("sign", SIGNS)
@pytest.mark.parametrize("R,D", ((40, 16), (33, 8)))
def test_d_full_kept_set(dev, wt, sign, R, D):
    """(d) everything kept: every tile with a point off the index-0 faces is listed (the others have no sampled point in any scene)"""
    vol_cl, maskvol = _volume(dev, D, torch.ones(D, D, D, dtype=torch.bool), seed=4)
    full, got, listed = _both(wt, vol_cl, maskvol, R, sign)
    assert listed == 32 * _tiles_with_a_sampled_point(R)
    assert torch.equal(got, full)


def test_arguments_come_together(dev, wt):
    R, D = 8, 4
    vol_cl, maskvol = _volume(dev, D, torch.ones(D, D, D, dtype=torch.bool), seed=6)
    with pytest.raises(ValueError):
        ops.sdf_mlp(wt.sdf_blob, vol_cl, None, variant=0, grid_R=R, grid_tables=wt.grid_tables(R), maskvol=maskvol)
    with pytest.raises(ValueError):
        ops.sdf_mlp(wt.sdf_blob, vol_cl, None, variant=0, grid_R=R, maskvol=maskvol, grid_background=_background(wt, R))
    with pytest.raises(ValueError):
        ops.sdf_mlp(wt.sdf_blob, vol_cl, None, variant=0, grid_R=R, grid_tables=wt.grid_tables(R), maskvol=maskvol[:-1], grid_background=_background(wt, R))


# ---- (e), (f): through pipeline.extract_mesh ---------------------------------------------------------------------------------------------------------
def _scenes(dev):
    """two small scenes (D = 32): latent balls of different place and size, colour maps and cameras of a 4-view rig"""
    sc = synth.make_scene(n_views=4, hw=(32, 32))
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dev).contiguous()
    proj, cam_pos = pipeline.camera_terms(t(sc["intrinsics"]).float(), t(sc["w2cs"]).float())
    g = torch.Generator().manual_seed(7)
    cmaps = ops.pack_color_maps(torch.rand(4, 56, 32, 32, generator=g).to(dev), t(sc["images"]))
    vols = []
    for seed, (centre, radius) in enumerate((((0.1, 0.0, -0.1), 0.7), ((-0.2, 0.15, 0.1), 0.55))):
        vol_cl, maskvol = _volume(dev, 32, _ball(32, centre, radius), seed=10 + seed)
        vols.append(dict(vol_cl=vol_cl, maskvol=maskvol, cmaps=cmaps))
    return vols, proj, cam_pos


def _digest(mesh):
    verts, tris, rgb, u = mesh
    h = hashlib.sha256()
    for a in (verts, tris, u):
        h.update(np.ascontiguousarray(a.cpu().numpy()).tobytes())
    return h.hexdigest(), int(verts.shape[0]), int(tris.shape[0])


def test_e_extract_mesh_three_times(dev, monkeypatch):
    """(e) three extractions on ONE weights object over two scenes (D = 32, R = 48): no table after the first, one after the second; u, vertices,
    triangles (and colours) of all three equal the full path's"""
    R = 48
    vols, proj, cam_pos = _scenes(dev)
    order = (0, 1, 0)
    monkeypatch.setattr(config, "GRID_BACKGROUND_MB", 0)
    wt_full = pipeline.SceneWeights(dev, seed=0)
    want = [pipeline.extract_mesh(wt_full, vols[i], proj, cam_pos, R) for i in sorted(set(order))]
    assert not wt_full._grid_bg
    assert not torch.equal(want[0][3], want[1][3]) and all(m[1].shape[0] > 100 for m in want)
    monkeypatch.setattr(config, "GRID_BACKGROUND_MB", 256)
    wt = pipeline.SceneWeights(dev, seed=0)
    assert torch.equal(wt.sdf_blob, wt_full.sdf_blob)
    for call, i in enumerate(order):
        got = pipeline.extract_mesh(wt, vols[i], proj, cam_pos, R)
        assert (R in wt._grid_bg) == (call >= 1), call
        if call >= 1:
            assert 0 < ops.sdf_grid_active_points(dev) < R ** 3
        for a, b in zip(got, want[i]):
            assert torch.equal(a, b), (call, i)
    assert list(wt._grid_bg) == [R] and wt._grid_bg[R].numel() == R ** 3


def child_main():
    """(f), in the child: two extractions with O2345_GRID_BACKGROUND_MB=0 in the environment -> digest of the second, and what was allocated"""
    dev = torch.device("cuda:0")
    vols, proj, cam_pos = _scenes(dev)
    wt = pipeline.SceneWeights(dev, seed=0)
    for _ in range(2):
        mesh = pipeline.extract_mesh(wt, vols[0], proj, cam_pos, 48)
    sparse_ws = [k for k in ops._ws_cache if k[0] == "sdf_grid_sparse"]
    print("CHILD", config.grid_background_mb(), len(wt._grid_bg), len(sparse_ws), *_digest(mesh))


def test_f_budget_zero_in_a_child_process(dev, monkeypatch):
    """(f) O2345_GRID_BACKGROUND_MB=0 in a fresh process: no table, no workspace, the full path's mesh"""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_gpu_grid_sparse as t; t.child_main()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, O2345_GRID_BACKGROUND_MB="0"), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("CHILD ")][-1].split()
    monkeypatch.setattr(config, "GRID_BACKGROUND_MB", 0)
    vols, proj, cam_pos = _scenes(dev)
    want = _digest(pipeline.extract_mesh(pipeline.SceneWeights(dev, seed=0), vols[0], proj, cam_pos, 48))
    assert line[1:4] == ["0", "0", "0"], r.stdout
    assert (line[4], int(line[5]), int(line[6])) == want
