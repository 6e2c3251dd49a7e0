"""The projecting entries, one by one, at non-square image sizes and at the borders of the source views' frusta, against the plain references of
tests/project_ref.py (pinned on the CPU by tests/test_project_ref_cpu.py, which also asserts that the shared families reach the borders).

  integer results   counts, kept sets, masks, sort keys: equal to the float64 reference on every item outside the border band (project_ref: 8 * 2^-24
                    around a threshold; an exactly representable border is not ambiguous and decides <= against <)
  device = device   view_count, the nviews of color_points (both numerical forms, query_cam and normals, with and without an index list), the column
                    sums of project_features' mask and the nviews of color_from_features agree on ALL points, ambiguous ones included
  rule E (floats)   max |gpu - ref64| <= 4 e_ref + 4 ulp of the output's magnitude, e_ref = max |ref32 - ref64| on the same non-ambiguous items

Image shapes (28, 44), (45, 24) and (2, 3); 1, 3, 5 and (list sort) 9 views; volumes of 14^3, 17^3 (lattice coordinates exact in float32) and
9 x 14 x 11; P in {1, 31, 33, 257} and the families in full.  Every float comparison prints its measured error and bound."""
import functools
import importlib

import numpy as np
import pytest
import torch

import project_ref as R

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("one-2-3-45_amd")
F32, F64 = R.F32, R.F64
RIG = "rig"
COST_KEYS = R.SCENES + [(28, 44, 5, 14, R.NONCUBIC), (45, 24, R.SORT_VIEWS, 14), RIG]
POINT_KEYS = R.SCENES + [RIG]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


def scene_of(key):
    return R.exact_rig() if key == RIG else R.scene(*key)


def rule_e(got, ref32, ref64, what):
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    e_ref, bound = R.rule_e_bound(ref32, ref64)
    err = (got - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f"{what}: e_ref {e_ref:.2e}, device err {err:.2e}, bound {bound:.2e} ({err / bound if bound else 0:.2f})")
    assert err <= bound, f"{what}: device err {err:.3e} > 4 * {e_ref:.3e} + 4 ulp = {bound:.3e}"


# ------------------------------------------------------------------------------------------------ cost volume
@functools.lru_cache(maxsize=None)
def cost_case(key, C=16):
    """The float32 and float64 cost volumes of a scene (V = 1: min_views = 0, so that a set is kept) and its ambiguous voxels."""
    s = scene_of(key)
    mv = 0 if s["V"] == 1 else 1
    feats = s["f16"][:, :C].contiguous()
    r32, r64 = (R.costvol(feats, s["aff"], s["dims"], s["voxel_size"], s["origin"], t, min_views=mv) for t in (F32, F64))
    return s, mv, feats, r32, r64, R.ambiguous_pairs(r64["pairs"], R.Z_CLAMP_VOXEL).any(1)


def cost_index(ops, dev, key):
    s, mv, _, _, _, _ = cost_case(key)
    return ops.costvol_index(s["aff"].to(dev), s["V"], s["H"], s["W"], s["dims"], s["voxel_size"], s["origin"], min_views=mv)


@pytest.mark.parametrize("key", COST_KEYS, ids=str)
def test_costvol_index(dev, ops, key):
    """k_vis_count + the compaction: counts exact off the band (on the rig: pairs with |g| = 1 exactly count, <=), kept coordinates in lattice order and
    the inverse map consistent with the device's own counts on every voxel."""
    s, mv, _, _, r64, amb = cost_case(key)
    cnt, row, coords, n = cost_index(ops, dev, key)
    cnt, row, coords = cnt.cpu(), row.cpu().long(), coords.cpu()
    assert torch.equal(cnt.long()[~amb], r64["cnt"][~amb]), f"{int((cnt.long() != r64['cnt'])[~amb].sum())} counts differ off the band"
    keep = cnt.long() > mv
    assert n == int(keep.sum()) > 0 and torch.equal(keep[~amb], r64["keep"][~amb])
    assert torch.equal(coords[:, :3].long(), R.lattice(s["dims"])[keep]) and not coords[:, 3].any()
    inverse = torch.full_like(row, -1)
    inverse[keep] = torch.arange(n)
    assert torch.equal(row, inverse)
    print(f"{key}: {n} kept of {keep.numel()}, {int(amb.sum())} ambiguous voxels, {int((cnt.long() != r64['cnt']).sum())} counts differ inside the band")


@pytest.mark.parametrize("key", COST_KEYS, ids=str)
def test_visible_count_list_on_a_reversed_list(dev, ops, key):
    s, mv, _, _, r64, amb = cost_case(key)
    cnt, row, coords, n = cost_index(ops, dev, key)
    rev = coords.flip(0).contiguous()
    dx, dy, dz = s["dims"]
    lin = ((rev[:, 0].long() * dy + rev[:, 1].long()) * dz + rev[:, 2].long()).cpu()
    got = ops.visible_count_list(s["aff"].to(dev), s["H"], s["W"], s["voxel_size"], s["origin"], rev).cpu()
    assert torch.equal(got, cnt.cpu()[lin])                                  # the same function of the same voxel, on all of them
    assert torch.equal(got.long()[~amb[lin]], r64["cnt"][lin][~amb[lin]])


@pytest.mark.parametrize("C", [8, 16])
@pytest.mark.parametrize("key", COST_KEYS, ids=str)
def test_costvol_gather(dev, ops, key, C):
    """k_costvol_gather<8|16> and the list form on the reversed list: rows by rule E on the voxels both sides keep off the band; the two forms bit-equal."""
    s, mv, feats, r32, r64, amb = cost_case(key, C)
    cnt, row, coords, n = cost_index(ops, dev, key)
    nhwc = feats.permute(0, 2, 3, 1).contiguous().to(dev)
    aff = s["aff"].to(dev)
    rows = ops.costvol_gather(nhwc, aff, s["dims"], s["voxel_size"], s["origin"], cnt, coords)
    keep = cnt.cpu().long() > mv
    both = keep & r64["keep"] & ~amb
    assert int(both.sum()) > 0.9 * n
    pick = lambda r: r["rows"][r["inverse"][both]]
    rule_e(rows.cpu()[row.cpu().long()[both]], pick(r32), pick(r64), f"costvol_gather C={C} {key}")
    rev = coords.flip(0).contiguous()
    cnt_row = ops.visible_count_list(aff, s["H"], s["W"], s["voxel_size"], s["origin"], rev)
    rows_list = ops.costvol_gather_list(nhwc, aff, s["voxel_size"], s["origin"], cnt_row, rev)
    assert torch.equal(rows_list, rows.flip(0))
    assert torch.equal(ops.costvol_gather(nhwc, aff, s["dims"], s["voxel_size"], s["origin"], cnt, rev), rows_list)


# ------------------------------------------------------------------------------------------------ colour path
@functools.lru_cache(maxsize=None)
def point_case(key):
    """A scene's points (offsets first, so that the short prefixes lie at the borders), their float32 / float64 references in both query forms, and
    what is ambiguous.  The rig: its lattice nodes."""
    s = scene_of(key)
    if key == RIG:
        pts = R.rig_points()
    else:
        fam = [R.offset_points(s), R.random_points(), R.face_points()] + ([R.node_points(s)] if s["D"] == 17 else [])
        pts = torch.cat(fam).contiguous()
    nrm = R.unit_normals(len(pts))
    r32, r64 = (R.project_features(s, pts, t, query_cam=s["query_cam"]) for t in (F32, F64))
    n32, n64 = (R.ray_diff(pts, R.query_dir(pts, t, normals=nrm), s["cam_pos"], t) for t in (F32, F64))
    amb_pt, amb_pair = R.ambiguous_points(s, pts)
    return s, pts, nrm, r32, r64, n32, n64, amb_pt, amb_pair


@functools.lru_cache(maxsize=None)
def device_scene(key):
    ops = importlib.import_module("one-2-3-45_amd.ops")
    dev = torch.device("cuda:0")
    s = scene_of(key)
    sd = pkg.weights.init_color_state_dict(0)
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dev)
    return dict(vol_cl=s["dense"].permute(1, 2, 3, 0).contiguous().to(dev), maskvol=s["maskvol"].reshape(-1).contiguous().to(dev),
                cmaps=ops.pack_color_maps(s["fmaps"].to(dev), s["images"].to(dev)), proj=s["proj"].to(dev), cam_pos=s["cam_pos"].to(dev),
                query_cam=s["query_cam"].to(dev), x3=t(pkg.weights.pack_color_x3_blob(sd)), mfma=t(pkg.weights.pack_color_mfma_blob(sd)))


def counts_of(ops, d, s, pts, nrm, index=None):
    """Every entry that reports how many views see a point -> dict name -> int64 [P] on the host."""
    scene = (d["vol_cl"], d["maskvol"], d["cmaps"], d["proj"], d["cam_pos"])
    out = {"view_count": ops.view_count(pts, d["maskvol"], s["D"], d["proj"], s["V"], s["H"], s["W"])}
    for form, blob in (("x3", d["x3"]), (True, d["mfma"])):
        out[f"color_points {form} query_cam"] = ops.color_points(blob, *scene, pts, query_cam=d["query_cam"], mfma=form, index=index)[1]
        out[f"color_points {form} normals"] = ops.color_points(blob, *scene, pts, normals=nrm, mfma=form, index=index)[1]
    geo, rf, rd, m = ops.project_features(*scene, pts, query_cam=d["query_cam"])
    assert bool(((m == 0) | (m == 1)).all())
    out["project_features mask"] = m.sum(0)
    for x3, blob in ((True, d["x3"]), (False, d["mfma"])):
        out[f"color_from_features x3={x3}"] = ops.color_from_features(blob, geo, rf, rd, m, x3=x3)[1]
    return {k: v.cpu().long() for k, v in out.items()}, m.cpu()


@pytest.mark.parametrize("key", POINT_KEYS, ids=str)
def test_view_counts_agree_and_match_the_reference(dev, ops, key):
    """k_view_count, k_color_pts (both forms), k_project_features, color_from_features: one count per point on ALL points; that count and the mask equal
    to the float64 reference off the band (on the rig: pairs with |g| = 1 exactly do not count, <).

    What this test found: with the projection's rows evaluated as products and sums, (2, 3, 3, 17) missed by one count of 14068.  Point 2713 of the
    offsets family, view 1, has gy = -1 + 11.08 * 2^-24 in float64 -- outside the band -- and Y = P4 x + P5 y + P6 z + P7 cancels there from terms of
    size 1.36 to 1.4e-7 at depth 0.41 (H - 1 = 1 on the 2 x 3 image), which the six roundings of that form put at or below 0.  The reference forms the
    rows with a matrix product, one FMA chain (project_row of csrc/geom_math.h, as project_voxel always did): every kernel evaluates that now, and no
    count differs off the band in any case.  The band was not widened."""
    s, pts, nrm, _, r64, _, _, amb_pt, amb_pair = point_case(key)
    d = device_scene(key)
    counts, m = counts_of(ops, d, s, pts.to(dev), nrm.to(dev))
    base = counts["view_count"]
    for name, c in counts.items():
        diff = int((c != base).sum())
        print(f"{key}: {name}: {diff} of {len(pts)} counts differ from view_count's ({int(((c != base) & ~amb_pt).sum())} off the band)")
    for name, c in counts.items():
        assert torch.equal(c, base), f"{name} and view_count disagree on {int((c != base).sum())} points"
    assert torch.equal(base[~amb_pt], r64["nviews"][~amb_pt]), f"{int((base != r64['nviews'])[~amb_pt].sum())} counts differ from the reference off the band"
    assert torch.equal(m.bool()[~amb_pair], r64["mask"][~amb_pair])
    assert 0 < int((base > 0).sum()) < len(pts)


@pytest.mark.parametrize("key", [(28, 44, 5, 14), (45, 24, 3, 17), (2, 3, 1, 14)], ids=str)
def test_view_counts_of_prefixes_and_index_lists(dev, ops, key):
    """P in {1, 31, 33, 257}: the same counts as in the full run; a reversed index list of every other point: the same counts in the listed slots and
    zero elsewhere."""
    s, pts, nrm, _, r64, _, _, amb_pt, _ = point_case(key)
    d = device_scene(key)
    P = 257
    full, _ = counts_of(ops, d, s, pts[:P].to(dev).contiguous(), nrm[:P].to(dev).contiguous())
    for n in R.POINT_COUNTS[:-1]:
        part, _ = counts_of(ops, d, s, pts[:n].to(dev).contiguous(), nrm[:n].to(dev).contiguous())
        for name in full:
            assert torch.equal(part[name], full[name][:n]), (name, n)
    assert torch.equal(full["view_count"][~amb_pt[:P]], r64["nviews"][:P][~amb_pt[:P]])
    index = torch.arange(P - 1, -1, -2, dtype=torch.int32, device=dev)
    listed = torch.zeros(P, dtype=torch.bool)
    listed[index.cpu().long()] = True
    scene = (d["vol_cl"], d["maskvol"], d["cmaps"], d["proj"], d["cam_pos"])
    for form, blob in (("x3", d["x3"]), (True, d["mfma"])):
        rgb0, _ = ops.color_points(blob, *scene, pts[:P].to(dev).contiguous(), query_cam=d["query_cam"], mfma=form)
        rgb, nv = ops.color_points(blob, *scene, pts[:P].to(dev).contiguous(), query_cam=d["query_cam"], mfma=form, index=index)
        assert torch.equal(nv.cpu().long()[listed], full["view_count"][listed]) and not nv.cpu()[~listed].any()
        assert torch.equal(rgb.cpu()[listed], rgb0.cpu()[listed]) and not rgb.cpu()[~listed].any()


@pytest.mark.parametrize("key", POINT_KEYS, ids=str)
def test_project_features_floats(dev, ops, key):
    """k_project_features: the trilinear gather of the latent (all points), the bilinear gather of the colour and feature maps (pairs off the band: a
    coordinate replaced by 2 samples nothing) and ray_diff in both query forms (all pairs), each by rule E."""
    s, pts, nrm, r32, r64, n32, n64, amb_pt, amb_pair = point_case(key)
    d = device_scene(key)
    scene = (d["vol_cl"], d["maskvol"], d["cmaps"], d["proj"], d["cam_pos"])
    geo, rf, rd, m = ops.project_features(*scene, pts.to(dev), query_cam=d["query_cam"])
    rule_e(geo, r32["geo"], r64["geo"], f"geometry_feat {key}")
    ok = ~amb_pair
    rule_e(rf.cpu()[ok], r32["rgb_feat"][ok], r64["rgb_feat"][ok], f"rgb_feat {key}")
    rule_e(rd, r32["ray_diff"], r64["ray_diff"], f"ray_diff query_cam {key}")
    geo2, rf2, rd2, m2 = ops.project_features(*scene, pts.to(dev), normals=nrm.to(dev))
    assert torch.equal(geo2, geo) and torch.equal(rf2, rf) and torch.equal(m2, m)
    rule_e(rd2, n32, n64, f"ray_diff normals {key}")


@pytest.mark.parametrize("key", [(28, 44, 5, 14), (45, 24, 3, 17)], ids=str)
def test_query_at_a_source_camera(dev, ops, key):
    """query_cam bit-equal to cam_pos[v]: both directions are one expression of the same numbers, so ray_diff[v, :, :3] is exactly 0; its fourth entry
    is |u|^2 of u = t / (|t| + 1e-6), 2e-6 / |t| below 1: within 4 ulp of that."""
    s, pts, nrm, *_ = point_case(key)
    d = device_scene(key)
    v = s["V"] // 2
    scene = (d["vol_cl"], d["maskvol"], d["cmaps"], d["proj"], d["cam_pos"])
    _, _, rd, _ = ops.project_features(*scene, pts.to(dev), query_cam=d["cam_pos"][v].contiguous())
    rd = rd.cpu()
    n = (s["cam_pos"][v].double()[None] - pts.double()).norm(dim=-1)
    err = (rd[v, :, 3].double() - (n / (n + 1e-6)) ** 2).abs().max().item()
    print(f"{key}: ray_diff at a source camera: direction part max {rd[v, :, :3].abs().max().item():.1e}, dot err {err / R.ULP:.2f} ulp")
    assert not rd[v, :, :3].any() and err <= 4 * R.ULP
    ref = R.ray_diff(pts, R.query_dir(pts, F64, query_cam=s["cam_pos"][v]), s["cam_pos"], F64)
    assert (rd.double() - ref).abs().max().item() < 2e-5


# ------------------------------------------------------------------------------------------------ list sort
def sort_into_sentinels(ops, pts, index, proj, H, W, count):
    """ops.list_sort_by_visibility's call with the output list pre-filled with -7."""
    n, V = int(index.shape[0]), int(proj.shape[0])
    out = torch.full_like(index, -7)
    keys = torch.empty(n, dtype=torch.int32, device=index.device)
    ws, wsb = ops._scratch("o2345_list_sort_workspace_bytes", (n, V), index.device, "lsort")
    with torch.cuda.device(index.device):
        ops.call("o2345_list_sort_by_visibility", pts, index, count, n, proj, V, int(H), int(W), out, keys, ws, wsb)
    return out, keys


@pytest.mark.parametrize("n", [1, 1023, 1025, 4097])
def test_list_sort_keys(dev, ops, n):
    """k_sort_hist's keys on nine views (two radix digits) of a non-square image: equal to the strict-inside signature of the float64 reference on
    every entry whose point is not ambiguous; a stable ascending permutation of the first `count` entries; the rest untouched."""
    key = (45, 24, R.SORT_VIEWS, 14)
    s = R.scene(*key)
    pts = torch.cat([R.offset_points(s), R.random_points(2048)]).contiguous()
    index = R.sort_list(n, len(pts))                                         # ascending distinct slots: stability is visible in the values
    n_valid = max(1, n - 7)
    count = torch.tensor([n_valid], dtype=torch.int32, device=dev)
    out, keys = sort_into_sentinels(ops, pts.to(dev), index.to(dev), s["proj"].to(dev), s["H"], s["W"], count)
    o, k = out[:n_valid].cpu().long(), keys[:n_valid].cpu().long() & 0xFFFFFFFF
    assert torch.equal(torch.sort(o)[0], torch.sort(index[:n_valid].long())[0]), "not a permutation of the valid entries"
    assert bool((k[1:] >= k[:-1]).all()), "signatures not ascending"
    same = k[1:] == k[:-1]
    assert bool((o[1:][same] > o[:-1][same]).all()), "not stable inside a signature"
    assert torch.equal(out[n_valid:].cpu(), torch.full((n - n_valid,), -7, dtype=torch.int32)), "entries past the count were written"
    ref = R.vis_signature(pts, s["proj"], s["H"], s["W"], F64)[o]
    amb = R.ambiguous_points(s, pts)[1].any(0)[o]                           # projection only: the geometry mask plays no part in the signature
    assert torch.equal(k[~amb], ref[~amb]), f"{int((k != ref)[~amb].sum())} keys differ off the band"
    print(f"n = {n}: {int(amb.sum())} ambiguous entries, {int((k != ref).sum())} keys differ inside the band, {int(torch.unique(k).numel())} signatures, "
          f"{int((k >= 256).sum())} with a view of the second digit")
    if n > 1000:
        assert int(torch.unique(k).numel()) > 3 and int((k >= 256).sum()) > 0 and int((~amb).sum()) > 0.5 * n_valid


# ------------------------------------------------------------------------------------------------ against the reference's own file
@pytest.fixture(scope="module")
def G(dev):
    from golden_util import load
    from test_project_ref_cpu import load_nonsquare
    pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
    g, s, pts = load_nonsquare()
    W = load()
    wt = pipeline.SceneWeights.from_state_dicts(dev, W["sdf_sd"], W["ren_sd"], W["var_sd"]["variance"])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sc = s["sc"]
    with torch.no_grad():
        vol = pipeline.build_volume(wt, T(s["images"].numpy()), s["aff"].to(dev), sc["partial_vol_origin"], s["D"], 2.0 / (s["D"] - 1), fmaps=s["fmaps"].to(dev))
    proj, cam_pos = pipeline.camera_terms(T(sc["intrinsics"]), T(sc["w2cs"]))
    ref_vol = dict(vol_cl=T(g["dense"]).permute(1, 2, 3, 0).contiguous(), maskvol=T(g["mask"]).reshape(-1).contiguous())      # the REFERENCE's volume
    return dict(g=g, s=s, pts=pts, W=W, wt=wt, vol=vol, proj=proj, cam_pos=cam_pos, T=T, ref_vol=ref_vol, pipeline=pipeline)


def rel(a, b):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / max(1.0, b.abs().max().item())).item()


def test_build_volume_matches_the_nonsquare_golden_file(G):
    """pipeline.build_volume on the 28 x 44 scene against get_conditional_volume(sizeH=28, sizeW=44): kept set exact off the band, dense volume 5e-5."""
    g, s, vol = G["g"], G["s"], G["vol"]
    D = s["D"]
    world = R.voxel_world(s["dims"], s["voxel_size"], s["origin"], F32)
    amb = R.ambiguous_pairs(R.project(world, s["aff"], s["H"], s["W"], F64), R.Z_CLAMP_VOXEL).any(1).view(D, D, D)
    mask = vol["maskvol"].view(D, D, D).cpu()
    assert torch.equal(mask[~amb], torch.from_numpy(g["mask"])[~amb]) and torch.equal(vol["coords"][:, :3].cpu(), torch.from_numpy(g["coords"]))
    err = rel(vol["vol_cl"].permute(3, 0, 1, 2), g["dense"])
    print(f"non-square dense volume vs the reference: {err:.2e} (5e-5), {vol['n_voxels']} voxels, {int(amb.sum())} ambiguous")
    assert err < 5e-5


@pytest.mark.parametrize("form", ["x3", True], ids=["x3", "mfma"])
def test_projector_and_colours_match_the_nonsquare_golden_file(G, ops, form):
    """project_features and color_points on the reference's own volume against Projector.compute / compute_view_independent(img_wh=[44, 28]) and
    GeneralRenderingNetwork: feature tensors 2e-5, colour 1e-4, masks exact off the band."""
    g, s, pts, wt, T = G["g"], G["s"], G["pts"], G["wt"], G["T"]
    scene = (G["ref_vol"]["vol_cl"], G["ref_vol"]["maskvol"], G["vol"]["cmaps"], G["proj"], G["cam_pos"])
    s2 = dict(s, maskvol=torch.from_numpy(g["mask"]))
    amb_pt, amb = R.ambiguous_points(s2, pts)
    qc = T(s["sc"]["query_c2w"][:3, 3].copy())
    geo, rf, rd, m = ops.project_features(*scene, pts.to(qc.device), query_cam=qc)
    gm = torch.from_numpy(g["mask_views"])
    assert torch.equal(m.cpu().bool()[~amb], gm[~amb]) and int(gm.sum()) > 100
    same = (m.cpu().bool() == gm)
    errs = dict(geo=rel(geo, g["geo"]), rgb_feat=rel(rf.cpu()[same], torch.from_numpy(g["rgb_feat"])[same]), ray_diff=rel(rd, g["ray_diff"]))
    blob = wt.color_xblob if form == "x3" else wt.color_mblob
    rgb, nv = ops.color_points(blob, *scene, pts.to(qc.device), query_cam=qc, mfma=form)
    nrm = torch.nn.functional.normalize(torch.from_numpy(g["vi_grad"]), p=2, dim=-1, eps=1e-6).to(qc.device)
    rgb2, nv2 = ops.color_points(blob, *scene, pts.to(qc.device), normals=nrm, mfma=form)
    _, _, rd2, _ = ops.project_features(*scene, pts.to(qc.device), normals=nrm)
    agree = same.all(0)                                                      # points whose every pair has the reference's mask
    assert torch.equal(nv.cpu().long()[agree], gm.sum(0)[agree]) and torch.equal(nv2, nv) and int(agree.sum()) > 0.9 * len(pts)
    errs.update(vi_ray_diff=rel(rd2, g["vi_ray_diff"]), rgb=rel(rgb.cpu()[agree], torch.from_numpy(g["rgb"])[agree]),
                vi_rgb=rel(rgb2.cpu()[agree], torch.from_numpy(g["vi_rgb"])[agree]))
    print(f"non-square golden file, {form}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs["geo"], errs["rgb_feat"], errs["ray_diff"], errs["vi_ray_diff"]) < 2e-5 and max(errs["rgb"], errs["vi_rgb"]) < 1e-4


def test_render_core_on_the_nonsquare_scene(G, ops, dev):
    """ops.render_core on 33 rays of the 28 x 44 query image against the oracle's render_core on identical sample lists (the oracle's own sampler's), at
    the downstream tolerances of tests/render_check.py: base + 4 x the oracle's sensitivity to float32-class SDF noise; colour mask
    exact."""
    import render_check as RC
    from golden_util import sdf_weights
    g, s, wt, W = G["g"], G["s"], G["wt"], G["W"]
    sc, H, Wd = s["sc"], s["H"], s["W"]
    Tc = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    a = dict(volume=Tc(g["dense"]), maskvol=Tc(g["mask"]), W={k: torch.from_numpy(np.array(v)) for k, v in sdf_weights(W).items()}, RW=W["ren_sd"],
             feat_maps=s["fmaps"], color_maps=s["images"], w2cs=Tc(sc["w2cs"]), K=Tc(sc["intrinsics"]), img_wh=(Wd, H), query_c2w=Tc(sc["query_c2w"]))
    ro, rd = pkg.synth.gen_rays(sc["query_intrinsic"], sc["query_c2w"], H, Wd)
    rng = np.random.default_rng(5)
    sel = rng.integers(H // 4, 3 * H // 4, 33) * Wd + rng.integers(Wd // 4, 3 * Wd // 4, 33)
    ro, rd = Tc(ro[sel]), Tc(rd[sel])
    near, far = float(sc["query_near_far"][0]), float(sc["query_near_far"][1])
    var_t = torch.tensor(0.2)
    ref, _ = RC._render(a, ro, rd, near, far, var_t, 1.0, 1.0, 33)
    z = ref["z_vals"].contiguous()
    scene = dict(sdf_blob=wt.sdf_blob, color_mfma_blob=wt.color_mblob, color_x3_blob=wt.color_xblob, cmaps=G["vol"]["cmaps"], proj=G["proj"],
                 cam_pos=G["cam_pos"], **G["ref_vol"])
    out = ops.render_core(scene, ro.to(dev), rd.to(dev), z.t().contiguous().to(dev), (far - near) / 64, wt.inv_s, 1.0, 1.0,
                          G["T"](sc["query_c2w"][:3, 3].copy()))
    hip = RC._hip(dict(out, z_vals=z.t().to(dev)))
    core = RC._core(a, ro, rd, z, near, far, var_t, 1.0, 1.0, 33)
    noisy = RC._noisy(lambda: RC._core(a, ro, rd, z, near, far, var_t, 1.0, 1.0, 33))
    assert int((core["weights_sum"] > 0.01).sum()) > 8                       # the rays do meet the volume
    for name, k in RC.PAIRS:
        err = float((hip[k] - core[k]).abs().max())
        bound = RC.BASE[name] * max(1.0, float(core[k].abs().max())) + 4 * max(float((n[k] - core[k]).abs().max()) for n in noisy)
        print(f"render_core non-square {name}: err {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (name, err, bound)
    assert torch.equal(hip["color_fine_mask"], core["color_fine_mask"])
