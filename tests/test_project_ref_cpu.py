"""CPU: the references and input families of tests/project_ref.py, before any GPU time is spent on them.

  * the float32 references equal the oracle (oracle/recon.py) on every scene -- integer results bit for bit, floats within the oracle's 2e-5;
  * the oracle equals the imported reference modules at non-square sizes (marked `reference`), and the file tests/golden/ref_nonsquare.npz they wrote;
  * the host build of csrc/geom_math.h and csrc/costvol_math.h (tests/hostcheck) equals the references at non-square sizes;
  * the families reach what they were built for: enough pairs next to a border on both sides of it, few inside the band, exact borders on the rig, scenes
    that are neither all visible nor all invisible, an H / W swap that changes the kept set.  tests/test_gpu_project_units.py relies on these."""
import ctypes
import os

import numpy as np
import pytest
import torch

import project_ref as R
from oracle import recon as O
from oracle import ref_import as RI
from test_hostcheck import P, hc          # noqa: F401  (the host build of csrc/*_math.h as a fixture)

F32, F64 = R.F32, R.F64
HERE = os.path.dirname(os.path.abspath(__file__))
ALL_SCENES = R.SCENES + [(28, 44, 5, 14, R.NONCUBIC), (45, 24, R.SORT_VIEWS, 14)]


def rel(a, b):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item() if b.numel() else 0.0


def families(s):
    fam = {"random": R.random_points(), "offsets": R.offset_points(s), "faces": R.face_points()}
    if s["D"] == 17:
        fam["nodes"] = R.node_points(s)
    return fam


# ------------------------------------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("key", ALL_SCENES, ids=str)
def test_references_match_oracle(key):
    s = R.scene(*key)
    H, W, V, dims = s["H"], s["W"], s["V"], s["dims"]
    world = R.voxel_world(dims, s["voxel_size"], s["origin"], F32)
    assert torch.equal(world, O.voxel_lattice(dims) * s["voxel_size"] + s["origin"][None])
    pr = R.project(world, s["aff"], H, W, F32)
    gx, gy, z, m = O.project(world, s["aff"], H, W)
    amb = R.ambiguous_pairs(R.project(world, s["aff"], H, W, F64), R.Z_CLAMP_VOXEL)
    assert torch.equal(pr["mask"][~amb], m[~amb])
    ok = m & ~amb
    assert rel(pr["gx"][ok], gx[ok]) < 2e-5 and rel(pr["gy"][ok], gy[ok]) < 2e-5
    for C, feats in ((16, s["f16"]), (8, s["f16"][:, :8].contiguous())):
        cv = R.costvol(feats, s["aff"], dims, s["voxel_size"], s["origin"], F32)
        coords, vol, cnt = O.costvol(feats, s["aff"], list(dims), s["voxel_size"], s["origin"])
        assert torch.equal(cv["cnt"], cnt) and torch.equal(cv["coords"].int(), coords[:, :3])
        assert rel(cv["rows"], vol) < 2e-5
    pts = torch.cat(list(families(s).values()))
    pp = R.project_pts(pts, s["proj"], H, W, F32)
    ogx, ogy = O.project_pts(pts, None, None, W, H, Pm=s["proj"])
    # the two float32 evaluations order their operations differently: pairs inside the band (the offsets family aims at it) may fall on either side
    # (twice the band on the 2 x 3 image: see test_float32_and_float64_masks_differ_only_inside_the_band)
    amb_pt, amb = R.ambiguous_points(s, pts, R.BAND if (H, W) in R.NONDEGENERATE else 2 * R.BAND)
    assert torch.equal((pp["gx"] == 2)[~amb], (ogx == 2)[~amb]) and torch.equal((pp["gy"] == 2)[~amb], (ogy == 2)[~amb])
    far = ~amb & (R.project_pts(pts, s["proj"], H, W, F64)["z"] >= 0.1)         # g = x / z: next to a camera its rounding error grows like 1 / z
    assert rel(pp["gx"][far], ogx[far]) < 2e-5 and rel(pp["gy"][far], ogy[far]) < 2e-5
    assert rel(R.bilinear(s["fmaps"], ogx, ogy, F32), O.bilinear_zeros(s["fmaps"], ogx.T, ogy.T).permute(1, 0, 2)) < 2e-5
    for kw in (dict(query_cam=s["query_cam"]), dict(normals=R.unit_normals(len(pts)))):
        mine = R.project_features(s, pts, F32, **kw)
        geo, rf, rd, mask = O.projector(pts, s["dense"], s["maskvol"], s["fmaps"], s["images"], None, None, (W, H), proj=s["proj"], cam_pos=s["cam_pos"], **kw)
        assert torch.equal(mine["mask"][~amb], mask[~amb]) and torch.equal(mine["nviews"][~amb_pt], mask.sum(0)[~amb_pt])
        assert rel(mine["geo"][~amb_pt], geo[~amb_pt]) < 2e-5 and rel(mine["rgb_feat"][~amb], rf[~amb]) < 2e-5 and rel(mine["ray_diff"], rd) < 2e-5
    assert torch.equal(R.vis_signature(pts, s["proj"], H, W, F32), (pp["mask"].long() << torch.arange(V)[:, None]).sum(0))


def test_float32_and_float64_masks_differ_only_inside_the_band():
    """What the band is for: outside it, rounding does not move a pair across a border -- in any family, on the non-degenerate scenes and the rig.  On the
    2 x 3 image (H - 1 = 1, the principal point on the image's last row) g = 2 (Y / Z) / (H - 1) - 1 amplifies the rounding of Y more: one pair of the
    float32 reference flips at 11 u from the border, outside the band of 8 u; those scenes are measured, not asserted, here."""
    flips = 0
    for s in [R.scene(*k) for k in ALL_SCENES] + [R.exact_rig()]:
        world = R.voxel_world(s["dims"], s["voxel_size"], s["origin"], F32)
        p32, p64 = (R.project(world, s["aff"], s["H"], s["W"], t) for t in (F32, F64))
        amb = R.ambiguous_pairs(p64, R.Z_CLAMP_VOXEL)
        assert torch.equal(p32["mask"][~amb], p64["mask"][~amb])
        pts = torch.cat(list(families(s).values()) if s["sc"] is not None else [R.rig_points()])
        f32, f64 = (R.project_features(s, pts, t, query_cam=s["query_cam"]) for t in (F32, F64))
        amb_pt, amb_pair = R.ambiguous_points(s, pts)
        flips += int((f32["mask"] != f64["mask"]).sum())
        outside = int((f32["mask"] != f64["mask"])[~amb_pair].sum())
        if (s["H"], s["W"]) in R.SHAPES[2:]:
            print(f"{s['H']} x {s['W']}, V = {s['V']}: {outside} float32 / float64 flips outside the band")
            continue
        assert outside == 0 and torch.equal(f32["nviews"][~amb_pt], f64["nviews"][~amb_pt])
        assert torch.equal(R.vis_signature(pts, s["proj"], s["H"], s["W"], F32)[~amb_pt], R.vis_signature(pts, s["proj"], s["H"], s["W"], F64)[~amb_pt])
    print(f"float32 / float64 mask flips: {flips}")
    assert flips > 100                                                      # the families do reach the borders


# ------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("key", R.SCENES, ids=str)
def test_families_reach_the_borders(key):
    s = R.scene(*key)
    H, W = s["H"], s["W"]
    off, rnd = R.offset_points(s), R.random_points()
    share_off = R.ambiguous_points(s, off)[1].any(0).float().mean().item()
    share_rnd = R.ambiguous_points(s, rnd)[1].any(0).float().mean().item()
    raw = R.project_pts(off, s["proj"], H, W, F64)
    amb = R.ambiguous_pairs(raw, R.Z_CLAMP_POINT)
    # distance of a coordinate from its border, on either side of it, while the other coordinate lies inside the image
    ax, ay = raw["gx_raw"].abs(), raw["gy_raw"].abs()
    close_x, close_y = (ax - 1).abs() < 128 * R.U, (ay - 1).abs() < 128 * R.U
    inside = ((close_x & (ax < 1) & (ay < 1)) | (close_y & (ay < 1) & (ax < 1))) & ~amb
    outside = ((close_x & (ax > 1) & (ay < 1)) | (close_y & (ay > 1) & (ax < 1))) & ~amb
    assert torch.equal(raw["mask"][inside], torch.ones_like(raw["mask"][inside])) and not raw["mask"][outside].any()
    valid = R.project_pts(torch.cat([rnd, off, R.face_points()]), s["proj"], H, W, F64)["mask"].float().mean().item()     # the points the GPU tests use
    cv = R.project(R.voxel_world(s["dims"], s["voxel_size"], s["origin"], F32), s["aff"], H, W, F64)["mask"].float().mean().item()
    print(f"{key}: offsets {len(off)} points, ambiguous share {share_off:.3f}; random {share_rnd:.5f}; non-ambiguous pairs within 128 u of a border: "
          f"{int(inside.sum())} inside, {int(outside.sum())} outside; valid pairs: points {valid:.3f}, voxels {cv:.3f}")
    assert share_off <= 0.25 and share_rnd <= 0.001
    if (H, W) in R.NONDEGENERATE:
        assert int(inside.sum()) >= 200 and int(outside.sum()) >= 200
    # the 2 x 3 image's frustum covers less of the lattice: 5 to 6 % of its voxel-view pairs are valid (51 or more kept voxels)
    assert 0.1 <= valid <= 0.9 and (0.1 if (H, W) in R.NONDEGENERATE else 0.05) <= cv <= 0.9


def test_exact_rig_has_exact_borders():
    s = R.exact_rig()
    H, W = s["H"], s["W"]
    world = R.voxel_world(s["dims"], s["voxel_size"], s["origin"], F32)
    p32, p64 = (R.project(world, s["aff"], H, W, t) for t in (F32, F64))
    on = ((p64["gx"].abs() == 1) | (p64["gy"].abs() == 1)) & (p64["gx"].abs() <= 1) & (p64["gy"].abs() <= 1) & (p64["z"] > 0)
    for k in ("gx", "gy"):                                                  # the coordinate on the border is the same number in both precisions
        b = on & (p64[k].abs() == 1)
        assert torch.equal(p32[k].double()[b], p64[k][b])
    assert int(on.sum()) >= 32 and p64["mask"][on].all() and not R.ambiguous_pairs(p64, R.Z_CLAMP_VOXEL)[on].any()
    assert int((p64["gy"].abs() == 1)[on].sum()) >= 8                       # some through the division by H - 1 = 12
    pts = R.rig_points()
    q32, q64 = (R.project_pts(pts, s["proj"], H, W, t) for t in (F32, F64))
    onp = ((q64["gx"].abs() == 1) & (q64["gy"].abs() <= 1)) | ((q64["gy"].abs() == 1) & (q64["gx"].abs() <= 1))
    assert int(onp.sum()) >= 32 and not q64["mask"][onp].any() and not q32["mask"][onp].any()      # the colour path's border is open
    assert not R.ambiguous_points(s, pts)[1][onp].any()
    print(f"exact rig: {int(on.sum())} voxel-view pairs and {int(onp.sum())} point-view pairs on a border exactly")
    # the decision is <= against <: the cost volume counts these pairs, and a strict test would keep another set
    strict = (p64["gx"].abs() < 1) & (p64["gy"].abs() < 1) & (p64["z"] > 0)
    assert not torch.equal(strict.sum(1) > 1, p64["mask"].sum(1) > 1)


def test_noncubic_volume_is_sensitive_to_an_h_w_swap():
    s = R.scene(28, 44, 5, 14, R.NONCUBIC)
    a = R.costvol(s["f16"], s["aff"], s["dims"], s["voxel_size"], s["origin"], F64)
    world = R.voxel_world(s["dims"], s["voxel_size"], s["origin"], F32)
    swapped = R.project(world, s["aff"], s["W"], s["H"], F64)["mask"]
    flips = int((swapped != a["pairs"]["mask"]).sum())
    print(f"non-cubic {R.NONCUBIC}: kept {int(a['keep'].sum())}, with H and W swapped {int((swapped.sum(1) > 1).sum())}, {flips} of {swapped.numel()} mask bits flip")
    assert not torch.equal(swapped.sum(1) > 1, a["keep"]) and flips > 100


def test_query_at_a_source_camera_has_zero_difference():
    s = R.scene(28, 44, 5, 14)
    pts = R.random_points(257)
    for t in (F32, F64):
        rd = R.ray_diff(pts, R.query_dir(pts, t, query_cam=s["cam_pos"][2]), s["cam_pos"], t)
        n = (s["cam_pos"][2].double()[None] - pts.double()).norm(dim=-1)
        assert (rd[2, :, :3] == 0).all() and ((rd[2, :, 3].double() - (n / (n + 1e-6)) ** 2).abs() <= 4 * R.ULP).all()


# ------------------------------------------------------------------------------------------------ the host build of the kernels' per-element math
@pytest.mark.parametrize("key", [k for k in ALL_SCENES if k[2] > 1], ids=str)
def test_host_build_at_nonsquare_sizes(hc, key):
    s = R.scene(*key)
    H, W, V, dims = s["H"], s["W"], s["V"], s["dims"]
    nvox = dims[0] * dims[1] * dims[2]
    nhwc = np.ascontiguousarray(s["f16"].numpy().transpose(0, 2, 3, 1))
    aff, org = s["aff"].numpy(), s["origin"].numpy()
    cnt = np.zeros(nvox, np.uint8); row = np.zeros(nvox, np.int32); coords = np.zeros((nvox, 4), np.int32); rows = np.zeros((nvox, 32), np.float32)
    n = hc.hc_costvol(P(nhwc), P(aff), V, H, W, dims[0], dims[1], dims[2], ctypes.c_float(s["voxel_size"]), P(org), 1, P(cnt), P(row), P(coords), P(rows))
    r32, r64 = (R.costvol(s["f16"], s["aff"], dims, s["voxel_size"], s["origin"], t) for t in (F32, F64))
    amb = R.ambiguous_pairs(r64["pairs"], R.Z_CLAMP_VOXEL).any(1)
    assert np.array_equal(cnt[~amb.numpy()], r64["cnt"][~amb].numpy().astype(np.uint8))
    cnt2 = np.zeros(nvox, np.uint8)
    hc.hc_visible_views(P(aff), V, H, W, dims[0], dims[1], dims[2], ctypes.c_float(s["voxel_size"]), P(org), P(cnt2))
    assert np.array_equal(cnt2, cnt)
    assert np.array_equal(row >= 0, cnt > 1) and n == int((cnt > 1).sum()) and np.array_equal(coords[:n, :3], R.lattice(dims)[torch.from_numpy(cnt > 1)].numpy())
    both = torch.from_numpy(cnt > 1) & r64["keep"] & ~amb                  # rows of voxels both sides keep, off the band
    got = torch.from_numpy(rows)[torch.from_numpy(row).long()[both]]
    e_ref, bound = R.rule_e_bound(r32["rows"][r32["inverse"][both]], r64["rows"][r64["inverse"][both]])
    err = (got.double() - r64["rows"][r64["inverse"][both]]).abs().max().item()
    print(f"{key}: host build, {int(both.sum())} rows, e_ref {e_ref:.2e}, err {err:.2e}, bound {bound:.2e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ the oracle against the reference, non-square
def _reference_volume(s, sdfnet):
    return sdfnet.get_conditional_volume(feature_maps=s["fmaps"][None], partial_vol_origin=s["origin"][None], proj_mats=s["aff"][None],
                                         sizeH=s["H"], sizeW=s["W"], lod=0)


@pytest.mark.parametrize("hw", R.NONDEGENERATE, ids=str)
@pytest.mark.reference
@pytest.mark.skipif(not RI.available(), reason="/root/reference not present")
@torch.no_grad()
def test_oracle_matches_reference_modules_nonsquare(hw):
    Rf = RI.load()
    H, W = hw
    D, V = 14, 5
    s = R.scene(H, W, V, D)
    sc = s["sc"]
    T = torch.from_numpy
    sdfnet, rnet, var, renderer = RI.build_networks(D, seed=11)
    cv = _reference_volume(s, sdfnet)
    dense, mask = cv["dense_volume_scale0"], cv["valid_mask_volume_scale0"]
    cl = sdfnet.compress_layer
    feats = O.abn_train(torch.nn.functional.conv2d(s["fmaps"], cl.conv.weight, padding=1), cl.bn.weight, cl.bn.bias)
    coords, vol, cnt = O.costvol(feats, s["aff"], [D, D, D], sdfnet.voxel_size, s["origin"])
    kept = torch.zeros(D, D, D)
    kept[coords[:, 0].long(), coords[:, 1].long(), coords[:, 2].long()] = 1
    assert torch.equal(kept, mask[0, 0]) and torch.equal(torch.nonzero(mask[0, 0]).int(), coords[:, :3])
    up = torch.cat([torch.zeros(len(coords), 1), coords[:, :3].float()], 1)
    mv, mm = Rf.back_project_sparse_type(up, s["origin"][None], sdfnet.voxel_size, feats[:, None], s["aff"][:, None], sizeH=H, sizeW=W)
    ref_vol = sdfnet.aggregate_multiview_features(mv, mm)
    assert rel(vol, ref_vol) < 2e-5
    names = ["conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11"]
    sd = sdfnet.sparse_costreg_net.state_dict()
    w = {n: (sd[f"{n}.net.0.kernel"], sd[f"{n}.net.1.weight"], sd[f"{n}.net.1.bias"]) for n in names}
    odense, omask = O.scatter_dense(coords, O.sparse_costreg(vol, coords, w)[0], [D, D, D])
    assert rel(odense, dense) < 5e-5
    pts = torch.cat([R.random_points(1024), R.offset_points(s, k_min=64)])
    kw = dict(geometryVolume=dense[0], geometryVolumeMask=mask[0], rendering_feature_maps=s["fmaps"], color_maps=s["images"], w2cs=T(sc["w2cs"]),
              intrinsics=T(sc["intrinsics"]), img_wh=[W, H], query_img_idx=0, query_c2w=T(sc["query_c2w"])[None])
    geo, rf, rd, vm, _, _ = renderer.rendering_projector.compute(pts.clone(), **kw)
    og, orf, ord_, om = O.projector(pts, dense[0], mask[0, 0], s["fmaps"], s["images"], T(sc["w2cs"]), T(sc["intrinsics"]), (W, H),
                                    query_cam=T(sc["query_c2w"])[:3, 3])
    assert torch.equal(om, vm[:, 0]) and 0.1 < vm.float().mean() < 0.9
    assert rel(og, geo[0]) < 2e-5 and rel(orf, rf[:, 0]) < 2e-5 and rel(ord_, rd[:, 0]) < 2e-5
    RW = {k: v for k, v in rnet.state_dict().items()}
    rgb, _ = rnet(geo, rf, rd, vm)
    orgb, onv = O.rendering_network(RW, og, orf, ord_, om)
    assert rel(orgb, rgb[0]) < 1e-4
    with torch.enable_grad():
        grad = sdfnet.gradient(pts.clone(), dense, 0).squeeze(1).detach()
        geo2, rf2, rd2, vm2, _, _ = renderer.rendering_projector.compute_view_independent(pts.clone(), lod=0, sdf_network=sdfnet, target_candidate_w2cs=None, **kw)
    nrm = torch.nn.functional.normalize(grad, p=2, dim=-1, eps=1e-6)
    _, _, ord2, om2 = O.projector(pts, dense[0], mask[0, 0], s["fmaps"], s["images"], T(sc["w2cs"]), T(sc["intrinsics"]), (W, H), normals=nrm)
    assert torch.equal(om2, vm2[:, 0]) and rel(ord2, rd2[:, 0].detach()) < 2e-5 and torch.equal(geo2, geo) and torch.equal(rf2, rf)
    # and the plain references of this change, in float32, on the reference's volume
    s2 = dict(s, dense=dense[0], maskvol=mask[0, 0])
    mine = R.project_features(s2, pts, F32, query_cam=s["query_cam"])
    amb = R.ambiguous_points(s2, pts)[1]
    assert torch.equal(mine["mask"][~amb], vm[:, 0][~amb]) and rel(mine["rgb_feat"], rf[:, 0]) < 2e-5 and rel(mine["geo"], geo[0]) < 2e-5


# ------------------------------------------------------------------------------------------------ the golden file
def load_nonsquare():
    """tests/golden/ref_nonsquare.npz with its regenerated inputs -> (file dict, scene, points); shared with tests/test_gpu_project_units.py."""
    import golden_util                                                      # noqa: F401  (puts tests/golden on the path)
    import make_golden as MG
    g = dict(np.load(os.path.join(HERE, "golden", "ref_nonsquare.npz")))
    assert {k[4:]: int(v) for k, v in g.items() if k.startswith("cfg_")} == MG.NONSQUARE, "golden file was generated with a different configuration"
    s, pts = MG.nonsquare_inputs()
    assert np.array_equal(pts.numpy(), g["pts"]) and np.float64(s["fmaps"].double().sum()) == g["chk_fmaps"] and np.float64(s["aff"].double().sum()) == g["chk_aff"]
    return g, s, pts


def test_oracle_matches_nonsquare_golden_file():
    from golden_util import costreg_sd, load
    g, s, pts = load_nonsquare()
    G = load()
    assert os.path.getsize(os.path.join(HERE, "golden", "ref_nonsquare.npz")) <= 1 << 20
    H, W, D = s["H"], s["W"], s["D"]
    T = torch.from_numpy
    sd = G["sdf_sd"]
    feats = O.abn_train(torch.nn.functional.conv2d(s["fmaps"], sd["compress_layer.conv.weight"], padding=1), sd["compress_layer.bn.weight"],
                        sd["compress_layer.bn.bias"])
    coords, vol, cnt = O.costvol(feats, s["aff"], [D, D, D], 2.0 / (D - 1), s["origin"])
    assert torch.equal(coords[:, :3], T(g["coords"]))
    from scene_util import costreg_oracle_weights
    dense, mask = O.scatter_dense(coords, O.sparse_costreg(vol, coords, costreg_oracle_weights(costreg_sd(G)))[0], [D, D, D])
    assert torch.equal(mask[0, 0], T(g["mask"])) and rel(dense[0], T(g["dense"])) < 5e-5
    sc = s["sc"]
    args = (pts, T(g["dense"]), T(g["mask"]), s["fmaps"], s["images"], T(sc["w2cs"]), T(sc["intrinsics"]), (W, H))
    geo, rf, rd, m = O.projector(*args, query_cam=T(sc["query_c2w"])[:3, 3])
    assert torch.equal(m, T(g["mask_views"])) and rel(geo, T(g["geo"])) < 2e-5 and rel(rf, T(g["rgb_feat"])) < 2e-5 and rel(rd, T(g["ray_diff"])) < 2e-5
    assert rel(O.rendering_network(G["ren_sd"], geo, rf, rd, m)[0], T(g["rgb"])) < 1e-4
    nrm = torch.nn.functional.normalize(T(g["vi_grad"]), p=2, dim=-1, eps=1e-6)
    geo2, rf2, rd2, m2 = O.projector(*args, normals=nrm)
    assert torch.equal(m2, m) and rel(rd2, T(g["vi_ray_diff"])) < 2e-5 and rel(O.rendering_network(G["ren_sd"], geo2, rf2, rd2, m2)[0], T(g["vi_rgb"])) < 1e-4
