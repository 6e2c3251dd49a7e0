"""Every view-count regime of the kernels, unit by unit: V = 33 (past the list sort's 32 views), 64 (the last count with k_color_pts' wave-uniform view
skip and its 64-bit mask of active views), 65 (the first without; the second block of k_camera_terms), 255 (the uint8 maximum of a count), and 34 where
the quad walk of costvol_row_quad16 matters (V mod 4 = 1, 2, 0, 1, 3).  synth.make_scene's rig has 32 source views, so the cameras come from
project_ref.sphere_scene and the points from project_ref.sphere_points; tests/test_many_views_cpu.py is the gate that shows, from the float64
references alone, that those inputs reach the branches (a tile some views see and others do not, a tile no view sees, a tile every view sees, the
count 255, the masks of trained_weights.many_view_mask).

The suite's rules, unchanged:
  exact             counts, kept sets, masks, nviews, work counters, form against form (view skip on / off, list sort on / off), untouched outputs
  rule E            fp32 forms: max |gpu - ref64| <= 4 e_ref + 4 ulp of the output's magnitude, e_ref = max |ref32 - ref64| on the same case
  split-f16 forms   rule E + 5e-6 for the colour, under the ceiling 1e-4 max(1, magnitude) (trained_weights.color_bound)
  fused / material  2e-5 max(1, magnitude)
  render            clauses (1) and (2) of render_check.three_clause
No point or voxel of these families lies in project_ref's border band (the gate asserts it), so the integer results are compared on all of them.
Every float comparison prints e_ref, the device error and the bound.

Shapes: images 20 x 28, lattices of side 11 (cost volume) and 13, P in {1, 33, 257}, 40 rays; the sort gate alone needs R * S >= 2^20.

Observed on an MI355X (error, and its share of the bound; DESIGN.md section 4, "View counts: what pins what").  Every case passed at first run, no
kernel was changed and no bound was touched:
  cost volume      0 counts differ; rows C = 16: 8.4e-6 ... 1.6e-5 (0.15 ... 0.30), C = 8: 6.3e-6 ... 1.6e-5 (0.20 ... 0.35), e_ref 7.0e-6 ... 2.4e-5
  view counts      eight entries agree on all 257 points and equal float64; 39 ... 45 points with the count V (39 at 255), 32 ... 45 with 0
  projector        geometry_feat <= 3.6e-6 (0.23), rgb_feat <= 2.7e-5 (0.24), ray_diff <= 3.2e-5 (0.28), with normals <= 7.3e-6 (0.10 ... 0.60)
  colour network   fp32 <= 5.8e-7 at e_ref <= 3.7e-7 (0.07 ... 0.42; at V = 255 <= 0.33), split-f16 <= 5.8e-7 (<= 0.09); one view per point 6.0e-8 (0.14)
  fused            1.8e-7 ... 3.6e-7 of 2e-5 against the network on materialised tensors
  counters         the partly seen tile: 7 of 33 and 7 of 64 (tile, view) pairs in both passes; all 9 tiles: 205 / 271 of 297 at V = 33, 454 / 519 of 576
                   at 64 (pooling / network); at 65 and 255 every pair in both passes (585, 2295) and all 9 tiles with every view
  render           sampler <= 1.4e-5; colour 5.4e-7 of 3.4e-5, depth 1.4e-6 of 4.6e-5; no guard byte touched; sorted = unsorted byte for byte
  front end        camera_terms proj <= 2.8e-6 (0.10), cam_pos 5.9e-8 (0.04); conv raw / (scale | shift) / activated 0.18 / 0.06 / 0.19 fp32 and
                   0.21 / 0.10 / 0.13 split-f16; fpn_level 7.0e-7, pyramid_pack 7.2e-7
One-line faults built as scratch libraries: the skip threshold at 128 fails test_work_counters_show_the_regime[65-*] alone (the results stay right:
the 64-bit mask aliases view 64 onto view 0, which only evaluates more); the active mask shifted by v & 31 fails 19 cases here and no earlier test;
the last view of costvol_row_quad16's two-view tail left out fails test_costvol_rows[34-16] alone (tails of one and three already ran at V = 1, 3, 5,
9: leaving the last view out of every ragged round also fails tests/test_gpu_project_units.py::test_costvol_gather)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import convnet_ref as C
import frontend_ref as FR
import project_ref as R
import trained_weights as TW
from test_gpu_guard import guard                                  # noqa: F401  (the fixture that carves every device buffer out of a guarded allocation)
from test_gpu_project_units import counts_of, rule_e

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
pkg = importlib.import_module("one-2-3-45_amd")
Wn = pkg.weights
H, W = R.SPHERE_HW
POINT_D, COST_D = 13, 11
FORMS = [("x3", True), (True, False)]                             # (color_points' mfma argument, color_from_features' x3 argument)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


@pytest.fixture(scope="module")
def color_blobs(dev):
    sd = TW.trained_color_state_dict()
    return {False: torch.from_numpy(Wn.pack_color_mfma_blob(sd)).to(dev), True: torch.from_numpy(Wn.pack_color_x3_blob(sd)).to(dev)}


def check(got, ref64, eb, what):
    """a case's (e_ref, bound): prints and asserts -> the device error"""
    e_ref, bound = eb
    got = got.detach().cpu()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f"{what}: e_ref {e_ref:.2e}, device err {err:.2e}, bound {bound:.2e} ({err / bound if bound else 0.0:.2f})")
    assert err <= bound, f"{what}: device err {err:.3e} > bound {bound:.3e} (e_ref {e_ref:.3e})"
    return err


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ a. cost volume
@functools.lru_cache(maxsize=None)
def cost_case(V, C_=16):
    s = R.sphere_scene(H, W, V, COST_D)
    feats = s["f16"][:, :C_].contiguous()
    r32, r64 = (R.costvol(feats, s["aff"], s["dims"], s["voxel_size"], s["origin"], t, min_views=1) for t in (F32, F64))
    assert not R.ambiguous_pairs(r64["pairs"], R.Z_CLAMP_VOXEL).any()
    return s, feats, r32, r64


@pytest.mark.parametrize("V", R.MANY_VIEWS)
def test_costvol_counts_and_kept_sets(dev, ops, V):
    """k_vis_count, the compaction and k_vis_count_list: the counts, V itself among them (255: the uint8 maximum), and the sets kept at min_views = 1,
    V - 2 and V - 1 (keep = cnt > min_views: the last keeps the voxels every view sees) equal to the float64 reference on every voxel"""
    s, _, _, r64 = cost_case(V)
    aff = s["aff"].to(dev)
    for mv in (1, V - 2, V - 1):
        cnt, row, coords, n = ops.costvol_index(aff, V, H, W, s["dims"], s["voxel_size"], s["origin"], min_views=mv)
        assert cnt.dtype == torch.uint8 and torch.equal(cnt.cpu().long(), r64["cnt"]), f"{int((cnt.cpu().long() != r64['cnt']).sum())} counts differ"
        assert int(cnt.max()) == V and int((cnt == V).sum()) >= 8
        keep = r64["cnt"] > mv
        assert n == int(keep.sum()) > 0 and torch.equal(coords[:, :3].cpu().long(), R.lattice(s["dims"])[keep]) and not coords[:, 3].any()
        inverse = torch.full((keep.numel(),), -1, dtype=torch.long)
        inverse[keep] = torch.arange(n)
        assert torch.equal(row.cpu().long(), inverse)
        rev = coords.flip(0).contiguous()
        got = ops.visible_count_list(aff, H, W, s["voxel_size"], s["origin"], rev)
        assert torch.equal(got.cpu().long(), r64["cnt"][keep].flip(0))
        if mv == V - 1:
            assert bool((got == V).all())
        print(f"V = {V}, min_views = {mv}: {n} of {keep.numel()} voxels kept")


@pytest.mark.parametrize("C_", [16, 8])
@pytest.mark.parametrize("V", R.MANY_VIEWS)
def test_costvol_rows(dev, ops, V, C_):
    """k_costvol_gather<16> (costvol_row_quad16: four views per round, a tail of V mod 4) and <8> (costvol_row), and the list form on the reversed
    list: var | mean by rule E on every kept voxel; the two forms bit-equal"""
    s, feats, r32, r64 = cost_case(V, C_)
    aff = s["aff"].to(dev)
    cnt, row, coords, n = ops.costvol_index(aff, V, H, W, s["dims"], s["voxel_size"], s["origin"], min_views=1)
    assert torch.equal(cnt.cpu().long(), r64["cnt"])
    nhwc = feats.permute(0, 2, 3, 1).contiguous().to(dev)
    rows = ops.costvol_gather(nhwc, aff, s["dims"], s["voxel_size"], s["origin"], cnt, coords)
    rule_e(rows, r32["rows"], r64["rows"], f"costvol_gather C={C_} V={V} (V mod 4 = {V % 4})")
    rev = coords.flip(0).contiguous()
    cnt_row = ops.visible_count_list(aff, H, W, s["voxel_size"], s["origin"], rev)
    rows_list = ops.costvol_gather_list(nhwc, aff, s["voxel_size"], s["origin"], cnt_row, rev)
    assert torch.equal(rows_list, rows.flip(0))
    assert torch.equal(ops.costvol_gather(nhwc, aff, s["dims"], s["voxel_size"], s["origin"], cnt, rev), rows_list)


# ------------------------------------------------------------------------------------------------ b. view counts and the projector
@functools.lru_cache(maxsize=None)
def point_case(V):
    s = R.sphere_scene(H, W, V, POINT_D)
    pts, nv, mask = R.sphere_points(H, W, V, POINT_D)
    nrm = R.unit_normals(len(pts), seed=V)
    r32, r64 = (R.project_features(s, pts, t, query_cam=s["query_cam"]) for t in (F32, F64))
    n32, n64 = (R.ray_diff(pts, R.query_dir(pts, t, normals=nrm), s["cam_pos"], t) for t in (F32, F64))
    assert torch.equal(r64["nviews"], nv)
    return s, pts, nrm, r32, r64, n32, n64


@functools.lru_cache(maxsize=None)
def device_scene(V):
    ops = importlib.import_module("one-2-3-45_amd.ops")
    dev = torch.device("cuda:0")
    s = R.sphere_scene(H, W, V, POINT_D)
    sd = TW.trained_color_state_dict()
    d = dict(vol_cl=s["dense"].permute(1, 2, 3, 0).contiguous().to(dev), maskvol=s["maskvol"].reshape(-1).contiguous().to(dev),
             cmaps=ops.pack_color_maps(s["fmaps"].to(dev), s["images"].to(dev)), proj=s["proj"].to(dev), cam_pos=s["cam_pos"].to(dev),
             query_cam=s["query_cam"].to(dev), x3=torch.from_numpy(Wn.pack_color_x3_blob(sd)).to(dev), mfma=torch.from_numpy(Wn.pack_color_mfma_blob(sd)).to(dev))
    d["scene"] = (d["vol_cl"], d["maskvol"], d["cmaps"], d["proj"], d["cam_pos"])
    return d


@pytest.mark.parametrize("V", TW.MANY_VS)
def test_view_counts_agree_and_match_the_reference(dev, ops, V):
    """k_view_count, k_color_pts (both forms, query_cam and normals), k_project_features' mask and color_from_features: one count per point, equal to
    the float64 reference on all 257 points; the counts 0 and V (255 included) occur"""
    s, pts, nrm, _, r64, _, _ = point_case(V)
    counts, m = counts_of(ops, device_scene(V), s, pts.to(dev), nrm.to(dev))
    base = counts["view_count"]
    for name, c in counts.items():
        assert torch.equal(c, base), f"{name} and view_count disagree on {int((c != base).sum())} points"
    assert torch.equal(base, r64["nviews"]), f"{int((base != r64['nviews']).sum())} counts differ from the reference"
    assert torch.equal(m.bool(), r64["mask"])
    assert int(base.max()) == V and int((base == V).sum()) >= 32 and int((base == 0).sum()) >= 32
    print(f"V = {V}: {len(counts)} entries agree on {len(pts)} points; {int((base == V).sum())} points with the count {V}, {int((base == 0).sum())} with 0")


@pytest.mark.parametrize("V", TW.MANY_VS)
def test_project_features_floats(dev, ops, V):
    """k_project_features' four tensors: latent, pixel features, ray_diff in both query forms by rule E; the mask exact"""
    s, pts, nrm, r32, r64, n32, n64 = point_case(V)
    d = device_scene(V)
    geo, rf, rd, m = ops.project_features(*d["scene"], pts.to(dev), query_cam=d["query_cam"])
    assert torch.equal(m.cpu().bool(), r64["mask"]) and bool(((m == 0) | (m == 1)).all())
    rule_e(geo, r32["geo"], r64["geo"], f"geometry_feat V={V}")
    rule_e(rf, r32["rgb_feat"], r64["rgb_feat"], f"rgb_feat V={V}")
    rule_e(rd, r32["ray_diff"], r64["ray_diff"], f"ray_diff query_cam V={V}")
    geo2, rf2, rd2, m2 = ops.project_features(*d["scene"], pts.to(dev), normals=nrm.to(dev))
    assert torch.equal(geo2, geo) and torch.equal(rf2, rf) and torch.equal(m2, m)
    rule_e(rd2, n32, n64, f"ray_diff normals V={V}")


# ------------------------------------------------------------------------------------------------ c. the colour network on materialised tensors
def network(ops, dev, blob, c, x3):
    return ops.color_from_features(blob, c["geo"].to(dev), c["rf"].to(dev), c["rd"].to(dev), c["mask"].float().to(dev), x3=x3)


@pytest.mark.parametrize("x3", [True, False], ids=["x3", "fp32"])
@pytest.mark.parametrize("V,P", TW.MANY_CASES)
def test_color_from_features(dev, ops, color_blobs, V, P, x3):
    """k_color_pts<., FEATS> with trained-like weights on color_case's random mask and on the four masks it never draws (many_view_mask: a tile hidden
    from every view from 32 on, the same with one blind point, every view valid, one view per point): nviews exact, colour by color_bound"""
    for kind in (None,) + TW.MASK_KINDS:
        c = TW.many_view_case(V, P, kind)
        rgb, nv = network(ops, dev, color_blobs[x3], c, x3)
        assert nv.dtype == torch.uint8 and torch.equal(nv.cpu().double(), c["nviews"].double()), kind
        if kind == "all_views":
            assert bool((nv == V).all())
        check(rgb, c["r64"], TW.color_bound(c["r32"], c["r64"], x3), f"colour V={V} P={P} {'f16x3' if x3 else 'fp32'} mask {kind or 'random'}")


# ------------------------------------------------------------------------------------------------ e. the fused kernel
def index_list(P, dev):
    """every other point from the last one down, and a device-side count that leaves the last seven entries out -> (index, n_dev, listed bool [P])"""
    index = torch.arange(P - 1, -1, -2, dtype=torch.int32, device=dev)
    n = index.numel() - 7
    listed = torch.zeros(P, dtype=torch.bool)
    listed[index[:n].cpu().long()] = True
    return index, torch.tensor([n], dtype=torch.int32, device=dev), listed


def fused_runs(ops, dev, V):
    """color_points in every form on the sphere points -> {(form, query form, listed?): (rgb, nviews)}; the listed runs write into pre-filled outputs"""
    s, pts, nrm, *_ = point_case(V)
    d = device_scene(V)
    p, n = pts.to(dev), nrm.to(dev)
    index, n_dev, _ = index_list(len(pts), dev)
    out = {}
    for form, x3 in FORMS:
        blob = d["x3" if x3 else "mfma"]
        for q, kw in (("query_cam", dict(query_cam=d["query_cam"])), ("normals", dict(normals=n))):
            out[x3, q, False] = ops.color_points(blob, *d["scene"], p, mfma=form, **kw)
            pre = (torch.full((len(pts), 3), 7.0, device=dev), torch.full((len(pts),), 9, dtype=torch.uint8, device=dev))
            out[x3, q, True] = ops.color_points(blob, *d["scene"], p, mfma=form, index=index, n_dev=n_dev, out=pre, **kw)
    return out


@pytest.mark.parametrize("V", TW.MANY_VS)
def test_color_points_equals_the_network_on_projected_features(dev, ops, V):
    """k_color_pts fused (both forms, query_cam and normals, with and without an index list and a device-side count) against color_from_features on the
    tensors project_features materialises for the same points, at 2e-5; the tile some views see, the tile none sees and the tile all see are the
    first three waves.  Listed slots carry the bits of the full run, every other slot keeps what it held."""
    s, pts, nrm, *_ = point_case(V)
    d = device_scene(V)
    runs = fused_runs(ops, dev, V)
    _, _, listed = index_list(len(pts), dev)
    for q, kw in (("query_cam", dict(query_cam=d["query_cam"])), ("normals", dict(normals=nrm.to(dev)))):
        geo, rf, rd, m = ops.project_features(*d["scene"], pts.to(dev), **kw)
        for form, x3 in FORMS:
            rgb, nv = ops.color_from_features(d["x3" if x3 else "mfma"], geo, rf, rd, m, x3=x3)
            fused, fnv = runs[x3, q, False]
            assert torch.equal(fnv, nv) and int(nv.max()) == V and int((nv == 0).sum()) >= 32
            err, bound = float((fused - rgb).abs().max()), 2e-5 * max(1.0, float(rgb.abs().max()))
            print(f"colour points V={V} {'f16x3' if x3 else 'fp32'} {q}: fused against materialised {err:.2e}, bound {bound:.2e} ({err / bound:.2f})")
            assert bool(torch.isfinite(fused).all()) and err <= bound
            lrgb, lnv = runs[x3, q, True]
            assert same_bits(lrgb[listed], fused[listed]) and torch.equal(lnv[listed], fnv[listed])
            assert bool((lrgb[~listed] == 7.0).all()) and bool((lnv[~listed] == 9).all())


@pytest.mark.parametrize("form,x3", FORMS, ids=["x3", "fp32"])
@pytest.mark.parametrize("V", TW.MANY_VS)
def test_work_counters_show_the_regime(dev, ops, V, form, x3):
    """color_stats_buffer: up to 64 views the partly seen tile skips views in both passes and the run has tiles that did; from 65 on every (tile, view)
    pair is evaluated in both passes"""
    s, pts, nrm, *_ = point_case(V)
    d = device_scene(V)
    blob = d["x3" if x3 else "mfma"]
    t0 = 32 * R.SPHERE_TILES["partial"]
    for what, p, tiles in (("the partly seen tile", pts[t0:t0 + 32], 1), ("all points", pts, (len(pts) + 31) // 32)):
        st = ops.color_stats_buffer(dev)
        ops.color_points(blob, *d["scene"], p.contiguous().to(dev), query_cam=d["query_cam"], mfma=form, stats=st)
        c = ops.color_stats_read(st)
        print(f"V = {V} {'f16x3' if x3 else 'fp32'}, {what}: {c}")
        assert c["tiles"] == tiles
        if V <= 64:
            assert 0 < c["pairs_network"] < tiles * V and c["pairs_pooling"] <= c["pairs_network"] and c["tiles_all_views"] < tiles
        else:
            assert c["pairs_pooling"] == c["pairs_network"] == tiles * V and c["tiles_all_views"] == tiles


# ------------------------------------------------------------------------------------------------ d. form against form, bit for bit
@pytest.mark.parametrize("V", [33, 64])
def test_view_skipping_is_bit_identical(dev, ops, color_blobs, lib_instance, V):
    """the default library against an instance that evaluates every view (O2345_COLOR_SCHED bit 2) on the masks of (c) at P = 257 and on the fused
    runs of (e): rgb and nviews byte-equal"""
    def runs():
        out = {}
        for x3 in (True, False):
            for kind in TW.MASK_KINDS:
                out["network", x3, kind] = network(ops, dev, color_blobs[x3], TW.many_view_case(V, 257, kind), x3)
        out.update(fused_runs(ops, dev, V))
        return out
    skipping = runs()
    assert b"color_sched=4 " in lib_instance({"O2345_COLOR_SCHED": "4"}).o2345_knobs() + b" "
    st = ops.color_stats_buffer(dev)
    d = device_scene(V)
    ops.color_points(d["x3"], *d["scene"], point_case(V)[1].to(dev), query_cam=d["query_cam"], stats=st)
    c = ops.color_stats_read(st)
    assert c["pairs_pooling"] == c["pairs_network"] == c["tiles"] * V, c                    # the instance does evaluate every pair
    every = runs()
    assert set(skipping) == set(every) and len(every) == 16
    for key in every:
        assert same_bits(skipping[key][0], every[key][0]) and same_bits(skipping[key][1], every[key][1]), key


# ------------------------------------------------------------------------------------------------ f. render
@functools.lru_cache(maxsize=None)
def render_case(V, n_rays):
    """the sphere scene with the initialisers' networks, as device dict and as oracle arguments, and n_rays seeded rays of the query camera"""
    ops = importlib.import_module("one-2-3-45_amd.ops")
    dev = torch.device("cuda:0")
    s = R.sphere_scene(H, W, V, POINT_D)
    sdfW, color_sd = Wn.init_sdf_weights(0), Wn.init_color_state_dict(0)
    a = dict(volume=s["dense"], maskvol=s["maskvol"], W={k: torch.from_numpy(np.array(v)) for k, v in sdfW.items()},
             RW={k: torch.as_tensor(np.asarray(v), dtype=F32) for k, v in color_sd.items()}, feat_maps=s["fmaps"], color_maps=s["images"], w2cs=s["w2cs"],
             K=s["K"], img_wh=(W, H), query_c2w=s["query_c2w"])
    proj, cam_pos = ops.camera_terms(s["K"].to(dev), s["w2cs"].to(dev))                   # the same cameras as the oracle's, formed in float32 like its own
    scene = dict(sdf_blob=torch.from_numpy(Wn.pack_sdf_blob(sdfW)).to(dev), color_mfma_blob=torch.from_numpy(Wn.pack_color_mfma_blob(color_sd)).to(dev),
                 color_x3_blob=torch.from_numpy(Wn.pack_color_x3_blob(color_sd)).to(dev), vol_cl=s["dense"].permute(1, 2, 3, 0).contiguous().to(dev),
                 maskvol=s["maskvol"].reshape(-1).contiguous().to(dev), cmaps=ops.pack_color_maps(s["fmaps"].to(dev), s["images"].to(dev)), proj=proj,
                 cam_pos=cam_pos)
    ro, rd = pkg.synth.gen_rays(s["query_K"].numpy(), s["query_c2w"].numpy(), H, W)
    sel = np.random.default_rng(V).integers(0, H * W, n_rays)
    return s, a, scene, torch.from_numpy(ro[sel]), torch.from_numpy(rd[sel])


NEAR, FAR = 0.9, 3.2                                                   # the query camera is 2.07 from the origin: the whole volume lies between


@pytest.mark.parametrize("V", [33, 65])
def test_render_rays_without_the_sort(dev, ops, V):
    """render_rays on 40 rays with the sort-free workspace layout: the sampler on identical inputs and everything downstream of it on the device's own
    sample lists against the oracle (clauses 1 and 2 of render_check.three_clause; its end-to-end caps, calibrated on the rig's scenes, are off)"""
    import render_check as RC
    s, a, scene, ro, rd = render_case(V, 40)
    res = RC.three_clause(ops, dev, scene, a, ro, rd, NEAR, FAR, 0.2, 1.0, 1.0, "f16x3", label=f"sphere V={V}", quantiles=False, e2e_caps=False,
                          strict_e2e=False)
    print(f"V = {V}: sampler dz max {res['sampler_dz_max']:.2e}; downstream " +
          ", ".join(f"{k} {v['err']:.2e} of {v['bound']:.2e}" for k, v in res["downstream"].items() if isinstance(v, dict)))
    assert res["rays_hitting_surface"] >= 5, res


@pytest.mark.parametrize("V", [33, 65])
def test_render_rays_writes_inside_its_buffers(dev, ops, guard, V):
    """the same call with every output and the workspace carved out of guarded allocations: no canary is touched"""
    s, a, scene, ro, rd = render_case(V, 40)
    for R_ in (40, 33):
        o = ops.render_rays(scene, ro[:R_].to(dev).contiguous(), rd[:R_].to(dev).contiguous(), NEAR, FAR, 64, 64, 7.4, 1.0, 1.0,
                            s["query_cam"].to(dev), want_z=True, want_scalars=True, color_stats=ops.color_stats_buffer(dev))
        assert bool(torch.isfinite(o["color"]).all())
        bad = guard.check()
        assert not bad, (R_, bad)
    assert len(guard.live) > 20, "the guard must see the call's buffers"


@pytest.mark.parametrize("V", [32, 33])
def test_the_sort_gate(dev, ops, lib_instance, V):
    """R * S = 2^20, where a call of up to 32 views groups its point list by visibility and one of 33 does not: the default library and an instance
    with O2345_LIST_SORT=0 return byte-equal outputs either way"""
    s, a, scene, ro, rd = render_case(V, 8192)
    qcam = s["query_cam"].to(dev)
    call = lambda: ops.render_rays(scene, ro.to(dev).contiguous(), rd.to(dev).contiguous(), NEAR, FAR, 64, 64, 7.4, 1.0, 1.0, qcam, want_z=True)
    assert ro.shape[0] * 128 >= 2 ** 20
    sorted_ = call()
    assert b"list_sort=0 " in lib_instance({"O2345_LIST_SORT": "0"}).o2345_knobs()
    plain = call()
    for k in sorted_:
        assert same_bits(sorted_[k], plain[k]), k
    assert float(sorted_["weights_sum"].max()) > 0.5 and int(sorted_["nviews"].max()) >= min(V, 20)


# ------------------------------------------------------------------------------------------------ g. the front end's batch axis
@pytest.mark.parametrize("V", [64, 65, 255])
def test_camera_terms(dev, ops, V):
    """k_camera_terms runs blocks of 64 views: one at 64, a second with one live thread at 65, four at 255"""
    s = R.sphere_scene(H, W, V, POINT_D)
    proj, cam = ops.camera_terms(s["K"].to(dev), s["w2cs"].to(dev))
    ref = lambda t: ((s["K"].to(t)[:, :, :, None] * s["w2cs"].to(t)[:, None, :3, :]).sum(2), torch.inverse(s["w2cs"].to(t))[:, :3, 3])
    (p32, c32), (p64, c64) = ref(F32), ref(F64)
    rule_e(proj, p32, p64, f"camera_terms proj V={V}")
    rule_e(cam, c32, c64, f"camera_terms cam_pos V={V}")
    assert float((proj.cpu() - s["proj"]).abs().max()) < 1e-5 and float((cam.cpu() - s["cam_pos"]).abs().max()) < 1e-6


def test_layout_kernels_at_65_views(dev, ops):
    d = FR.pack_inputs((65, 7, 9))
    assert torch.equal(ops.pack_color_maps(d["feat"].to(dev), d["rgb"].to(dev)).cpu(), FR.pack_color_maps(d["feat"], d["rgb"]))
    for C_, hw in ((8, (5, 13)), (16, (7, 9)), (64, (8, 16))):
        x = R._t(R._rng(28, C_, *hw).normal(0.0, 1.0, (65, C_) + hw))
        got = ops.nchw_to_nhwc(x.to(dev))
        assert got.is_contiguous() and torch.equal(got.cpu(), FR.nchw_to_nhwc(x))


@functools.lru_cache(maxsize=None)
def conv_case_65():
    """convnet_ref.case's fused "normal" kind (in_ss of both signs, no bias, batch norm with abs_gamma) for the 8 -> 8 layer on 65 views of 8 x 12: the
    statistics run over 65 * 96 = 6240 values per channel"""
    cin, cout, k, stride = shape = (8, 8, 3, 1)
    V, Hi, Wi = 65, 8, 12
    g = C._rng("convnet-views", *shape, V)
    x = C._t(g.normal(0.2, 1.0, (V, cin, Hi, Wi)))
    w = C._t(g.normal(0.0, 1.0, (cout, cin, k, k)) / np.sqrt(cin * k * k))
    in_ss = C._t(np.concatenate([C._both_signs(g, -1.5, 1.5, cin), g.normal(0.0, 0.3, cin)]))
    gamma, beta = C._t(C._both_signs(g, -1.5, 1.5, cout)), C._t(g.normal(0.0, 0.2, cout))
    args = (x, w, None, stride, in_ss, C.SLOPE)
    ref64, ref32, split = C.conv_ref(*args), C.conv_ref32_loop(*args), C.conv_split_model(*args)
    ss64, ss32, ss_s = (C.abn_stats(r, gamma, beta) for r in (ref64, ref32, split))
    act64 = C.abn_act(ref64, ss64)
    return dict(x=x, w=w, stride=stride, bias=None, in_ss=in_ss, gamma=gamma, beta=beta, bn=True, shape=shape, ref64=ref64, ss64=ss64, act64=act64,
                mag=C._mag(ref64), mag_ss=C._mag(ss64), mag_act=C._mag(act64), e_ref=C._err(ref32, ref64), e_split=C._err(split, ref64),
                e_ref_ss=C._err(ss32, ss64), e_split_ss=C._err(ss_s, ss64), e_ref_act=C._err(C.abn_act(ref32, ss32), act64),
                e_split_act=C._err(C.abn_act(split, ss_s), act64))


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_conv2d_with_batch_statistics_at_65_views(dev, ops, prec):
    """ops.conv2d with the fused statistics, then scale_shift_act, on 65 views of an 8 x 12 map: raw output, (scale | shift) and the activated output
    by the feature network units' rule E (convnet_ref.bound)"""
    from test_gpu_convnet_units import check_fused
    check_fused(ops, dev, conv_case_65(), prec, "(8, 8, 3, 1) 65 views of 8 x 12 fused")


@pytest.mark.parametrize("C_", [8, 16])
def test_fpn_level_and_pyramid_pack_at_65_views(dev, ops, C_):
    from test_gpu_frontend_units import close, on
    d = FR.fpn_inputs(C_, True, (65, 6, 10))
    g = on(dev, d)
    close(ops.fpn_level(g["fine"], g["coarse"], g["weight"], g["bias"], g["fine_ss"], FR.FPN_SLOPE),
          FR.fpn_level(d["fine"], d["coarse"], d["weight"], d["bias"], d["fine_ss"], FR.FPN_SLOPE), f"fpn_level C={C_} 65 views")
    if C_ == 8:
        d = FR.pyramid_inputs((65, 8, 12))
        g = on(dev, d)
        fm, cm = ops.pyramid_pack(g["f2"], g["s1"], g["s0"], g["rgb"])
        rfm, rcm = FR.pyramid(d["f2"], d["s1"], d["s0"], d["rgb"])
        close(cm, rcm, "pyramid_pack cmaps 65 views")
        close(fm, rfm, "pyramid_pack fmaps 65 views")
        assert torch.equal(cm[..., 3:59].cpu(), fm.permute(0, 2, 3, 1).cpu()) and torch.equal(cm[..., 59:].cpu(), torch.zeros(65, 8, 12, 5))


# ------------------------------------------------------------------------------------------------ h. refusals are statuses
RH, RW_, RD, RP = 4, 6, 5, 33                                           # the refusal scene: 4 x 6 images, a 5^3 volume, 33 points
SENTINEL = 0x5A


def prefilled(dev, shape, dtype):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev).view(dtype).view(shape)


def untouched(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def refusal_scene():
    """every buffer sized for 256 views, so that a call that states 256 and was NOT refused would still read and write inside them"""
    dev = torch.device("cuda:0")
    s = R.sphere_scene(RH, RW_, 255, RD)
    g = R._rng(29)
    more = lambda t: torch.cat([t, t[:1]]).contiguous().to(dev)
    t = lambda *shape: R._t(g.normal(0.0, 1.0, shape)).to(dev)
    sd = TW.trained_color_state_dict()
    return dict(s=s, proj=more(s["proj"]), aff=more(s["aff"]), cam_pos=more(s["cam_pos"]), cmaps=t(256, RH, RW_, 64), vol_cl=t(RD, RD, RD, 16),
                maskvol=torch.ones(RD ** 3, device=dev), pts=R._t(g.uniform(-0.9, 0.9, (RP, 3))).to(dev), query_cam=s["query_cam"].to(dev),
                geo=t(RP, 16), rf=t(256, RP, 59), rd=t(256, RP, 4), mask=(t(256, RP) > -0.5).float().contiguous(),
                x3=torch.from_numpy(Wn.pack_color_x3_blob(sd)).to(dev), mfma=torch.from_numpy(Wn.pack_color_mfma_blob(sd)).to(dev))


def refusal_calls(ops, dev, r):
    """-> {name: f(V, keep=None)}: makes the entry's call on pre-filled outputs and returns them; keep (a list) receives them BEFORE the call, for the
    caller that expects the call to raise"""
    def made(keep, *out):
        if keep is not None:
            keep.extend(out)
        return out

    def color_points(V, keep=None, entry="o2345_color_points_x3", blob="x3"):
        out = made(keep, prefilled(dev, (RP, 3), F32), prefilled(dev, (RP,), torch.uint8))
        ops.call(entry, r[blob], r["vol_cl"], r["maskvol"], RD, r["cmaps"], r["proj"], r["cam_pos"], V, RH, RW_, r["pts"], None, None, RP, r["query_cam"], None,
                 out[0], out[1], None)
        return out

    def color_from_features(V, keep=None, x3=1):
        out = made(keep, prefilled(dev, (RP, 3), F32), prefilled(dev, (RP,), torch.uint8))
        ops.call("o2345_color_from_features", r["x3" if x3 else "mfma"], x3, r["geo"], r["rf"], r["rd"], r["mask"], V, RP, out[0], out[1])
        return out

    def project_features(V, keep=None):
        out = made(keep, prefilled(dev, (RP, 16), F32), prefilled(dev, (256, RP, 59), F32), prefilled(dev, (256, RP, 4), F32), prefilled(dev, (256, RP), F32))
        ops.call("o2345_project_features", r["vol_cl"], r["maskvol"], RD, r["cmaps"], r["proj"], r["cam_pos"], V, RH, RW_, r["pts"], RP, r["query_cam"], None, *out)
        return out

    def view_count(V, keep=None):
        out = made(keep, prefilled(dev, (RP,), torch.uint8))
        ops.call("o2345_view_count", r["pts"], RP, r["maskvol"], RD, r["proj"], V, RH, RW_, out[0])
        return out

    def costvol_index(V, keep=None):
        n = RD ** 3
        out = made(keep, prefilled(dev, (n,), torch.uint8), prefilled(dev, (n,), torch.int32), prefilled(dev, (n, 4), torch.int32), prefilled(dev, (1,), torch.int32))
        ws, wsb = ops._scratch("o2345_costvol_workspace_bytes", (RD, RD, RD), dev)
        ops.call("o2345_costvol_index", r["aff"], V, RH, RW_, RD, RD, RD, 2.0 / (RD - 1), ops._host3(r["s"]["origin"]), 1, *out, ws, wsb)
        return out

    return dict(color_points_x3=color_points, color_points_mfma=lambda V, keep=None: color_points(V, keep, "o2345_color_points_mfma", "mfma"),
                color_from_features_x3=color_from_features, color_from_features_fp32=lambda V, keep=None: color_from_features(V, keep, 0),
                project_features=project_features, view_count=view_count, costvol_index=costvol_index)


REFUSED = ("color_points_x3", "color_points_mfma", "color_from_features_x3", "color_from_features_fp32", "project_features", "view_count", "costvol_index")


@pytest.mark.parametrize("name", REFUSED)
def test_zero_and_256_views_are_refused(dev, ops, name):
    """V = 0 and V = 256: the library's error, the pre-filled outputs keep their bytes, and the next valid call (33 views of the same buffers) on the
    same stream returns what it returned before"""
    fn = refusal_calls(ops, dev, refusal_scene())[name]
    before = fn(33)
    torch.cuda.synchronize()
    for V in (0, 256):
        held = []
        with pytest.raises(RuntimeError, match="o2345 .* failed"):
            fn(V, held)
        torch.cuda.synchronize()
        assert held and all(untouched(t) for t in held), (name, V)
        after = fn(33)
        assert all(same_bits(x, y) for x, y in zip(before, after)), (name, V)
    if name == "project_features":          # 33 views of buffers sized for 256: the rows of the views that were not asked for stay as they were
        assert all(untouched(t[33:]) and not untouched(t[:33]) for t in before[1:])
    else:
        assert not any(untouched(t) for t in before)


def test_the_list_sort_refuses_33_views(dev, ops):
    from test_gpu_project_units import sort_into_sentinels
    s = R.sphere_scene(H, W, 33, POINT_D)
    pts = R.sphere_points(H, W, 33, POINT_D)[0].to(dev)
    index = R.sort_list(200, len(pts)).to(dev)
    count = torch.tensor([200], dtype=torch.int32, device=dev)
    proj = s["proj"].to(dev)
    before = sort_into_sentinels(ops, pts, index, proj[:32].contiguous(), H, W, count)
    out = torch.full_like(index, -7)
    keys = torch.full((200,), -7, dtype=torch.int32, device=dev)
    ws, wsb = ops._scratch("o2345_list_sort_workspace_bytes", (200, 32), dev, "lsort")
    with pytest.raises(RuntimeError, match="1..32 views"):
        ops.call("o2345_list_sort_by_visibility", pts, index, count, 200, proj, 33, H, W, out, keys, ws, wsb)
    with pytest.raises(RuntimeError, match="1..32 views"):
        ops.list_sort_by_visibility(pts, index, proj, H, W)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((keys == -7).all())
    after = sort_into_sentinels(ops, pts, index, proj[:32].contiguous(), H, W, count)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and not bool((after[0] == -7).any())
