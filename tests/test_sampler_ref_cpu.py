"""The references of tests/sampler_ref.py pinned on the CPU, and the conditions the shared seeded inputs must meet (a seed that stops meeting them
fails HERE, without a GPU):

  * the float32 run of every reference against the oracle (oracle/recon.py) on small-scene inputs: selections equal, values BIT-EQUAL -- the references
    restate the oracle's whole-tensor expressions operation by operation, so no reordering has to be allowed for.  Two places regroup: the per-ray
    gradient-error sums (the oracle returns only their ratio over the call: compared to a few roundings), and the inverse CDF's normaliser and cdf,
    which the reference accumulates section by section in its dtype by default (sampler_ref.inverse_cdf: why) -- with serial_sum=False it is
    bit-equal with O.sample_pdf_det, with the default the oracle passes rule Z against it;
  * the float32 run against the host build of csrc/render_math.h (hc_upsample, hc_merge, hc_composite) on the edge inputs of the GPU unit tests, under
    the very rules E and Z the GPU tests apply (merge: bit-equal) -- the host build walks a ray sample by sample like the kernels do;
  * the caps of the rules: e_ref <= 1e-5 (x max(1, magnitude) for the composite's sums) for every output under rule E; rule Z's normalised deviation
    <= (S + 8) 2^-24 + 2 ulp(z) / sens per sample; switch-band samples and samples whose bound exceeds their bin's width <= 1 % of a case (on these
    inputs also at S = 255, n_imp = 256: no combination is dropped from rule Z).

Measured here (float32 reference against float64): section weights e_ref 0 .. 8.9e-7; composite e_ref <= 1.7e-6 x max(1, magnitude) over all outputs
and cases (printed per case); rule Z normalised deviation <= 2.0e-6 and <= 0.73 S 2^-24; switch-band samples 0, bounds wider than their bin 0 ... 1
of 512 samples.  The host build sits at <= 0.25 of rule Z's bound and <= 0.6 of rule E's."""
import ctypes

import numpy as np
import pytest
import torch

import sampler_ref as SR
from oracle import recon as O
from scene_util import color_t, rays_for, sdfW_t, small_scene
from test_hostcheck import P, hc          # noqa: F401  (the host build of csrc/*_math.h as a fixture)

F32, F64 = torch.float32, torch.float64
E_REF_CAP = 1e-5


def np_sm(t):
    return np.ascontiguousarray(SR.sm(t).numpy())


# ------------------------------------------------------------------------------------------------ float32 run == oracle
@pytest.fixture(scope="module")
def traced():
    """one oracle render() of 24 small-scene rays with 16 + 32 samples: the sampler's state per round, and render_core's outputs"""
    s = small_scene()
    sc = s["sc"]
    ro, rd = rays_for(s, 24, seed=4)
    a = dict(volume=s["dense"][0], maskvol=s["mask"][0, 0], W=sdfW_t(s["sdfW"]), RW=color_t(s["color_sd"]), variance=torch.tensor(0.3),
             feat_maps=torch.from_numpy(s["fmaps"]), color_maps=torch.from_numpy(sc["images"]), w2cs=torch.from_numpy(sc["w2cs"]),
             K=torch.from_numpy(sc["intrinsics"]), img_wh=(s["W"], s["H"]), query_c2w=torch.from_numpy(sc["query_c2w"]))
    near, far = torch.tensor(float(sc["query_near_far"][0])), torch.tensor(float(sc["query_near_far"][1]))
    tro, trd = torch.from_numpy(ro), torch.from_numpy(rd)
    t_rand = torch.rand(24, 16, generator=torch.Generator().manual_seed(2))
    trace = []
    with torch.no_grad():
        out = O.render(tro, trd, near, far, a["volume"], a["maskvol"], a["W"], a["RW"], a["variance"], a["feat_maps"], a["color_maps"], a["w2cs"], a["K"],
                       a["img_wh"], a["query_c2w"], n_samples=16, n_importance=32, alpha_inter_ratio=0.5, background_rgb=1.0, t_rand=t_rand, trace=trace)
    return dict(a=a, ro=tro, rd=trd, near=near, far=far, t_rand=t_rand, trace=trace, out=out, sample_dist=float((far - near) / 16))


def test_coarse_float32_is_the_oracle(traced):
    t = traced
    z, pts = SR.coarse(t["ro"], t["rd"], float(t["near"]), float(t["far"]), 16, t["t_rand"], dtype=F32)
    assert torch.equal(z, t["trace"][0]["z"])                                       # render()'s jittered coarse depths, bit for bit
    z0, _ = SR.coarse(t["ro"], t["rd"], float(t["near"]), float(t["far"]), 16, dtype=F32)
    assert torch.equal(z0, (t["near"] + (t["far"] - t["near"]) * torch.linspace(0, 1, 16))[None].repeat(24, 1))
    nr, fr = torch.full((24,), float(t["near"])), torch.full((24,), float(t["far"]))
    assert torch.equal(SR.coarse(t["ro"], t["rd"], nr, fr, 16, t["t_rand"], dtype=F32)[0], z)
    assert torch.equal(pts, t["ro"][:, None] + t["rd"][:, None] * z[..., None])


def test_upsample_float32_is_the_oracle(traced):
    t = traced
    mask = t["a"]["maskvol"]
    assert len(t["trace"]) == 4
    for rnd in t["trace"]:
        z, sdf, inv_s = rnd["z"], rnd["sdf"], rnd["inv_s"]
        pts = SR.ray_points(t["ro"], t["rd"], z)
        m = SR.occupancy(mask, pts)
        assert torch.equal(m, O.mask_nearest(mask, pts.reshape(-1, 3)).reshape(z.shape))
        assert 0 < int((m > 0).sum()) < m.numel()
        w = SR.upsample_weights(z, sdf, m, inv_s, dtype=F32)
        new_z, lo, mass, width = SR.inverse_cdf(z, w, 8, dtype=F32, serial_sum=False)
        assert torch.equal(new_z, rnd["new_z"])                                     # O.up_sample, bit for bit (ATen's pairwise normaliser)
        diag = []
        assert torch.equal(O.sample_pdf_det(z, w - SR.EPS5, 8, diag), SR.inverse_cdf(z, (w - SR.EPS5) + SR.EPS5, 8, dtype=F32, serial_sum=False)[0])
        assert torch.equal(diag[0], SR.inverse_cdf(z, (w - SR.EPS5) + SR.EPS5, 8, dtype=F32, serial_sum=False)[2])
        assert bool((lo >= 0).all()) and bool((lo <= z.shape[1] - 1).all()) and bool((width >= 0).all())
        # the default, serial normaliser: the same function in another summation order -- the oracle passes rule Z against it
        q = SR.rule_z(z, w)(8)
        every = torch.ones(z.shape[0], dtype=torch.bool)
        bz = SR.rule_z_bound(q, 4 * float(q["dev32"].max()), every)
        assert bool(((rnd["new_z"].double() - q["new_z"]).abs() <= bz).all())
        assert float((SR.inverse_cdf(z, w, 8, dtype=F32)[1] != lo).double().mean()) <= 0.01
        assert float((SR.inverse_cdf(z, w, 8, dtype=F64)[0] - SR.inverse_cdf(z, w, 8, dtype=F64, serial_sum=False)[0]).abs().max()) <= 1e-14


def test_merge_is_the_oracle(traced):
    t = traced
    a = t["a"]
    for i in range(3):
        rnd, nxt = t["trace"][i], t["trace"][i + 1]
        pts = SR.ray_points(t["ro"], t["rd"], rnd["new_z"]).reshape(-1, 3)
        m = O.mask_nearest(a["maskvol"], pts) > 0
        new_sdf = torch.full((pts.shape[0],), 100.0)
        assert int(m.sum()) > 1
        new_sdf[m] = O.sdf(pts[m], a["volume"], a["W"])[0][:, 0]
        zz, ss = SR.merge(rnd["z"], rnd["sdf"], rnd["new_z"], new_sdf.reshape(rnd["new_z"].shape))
        cz, cs = O.cat_z(t["ro"], t["rd"], rnd["z"], rnd["new_z"], rnd["sdf"], a["volume"], a["maskvol"], a["W"])
        assert torch.equal(zz, cz) and torch.equal(ss, cs) and torch.equal(zz, nxt["z"]) and torch.equal(ss, nxt["sdf"])


def test_finalize_and_composite_float32_are_the_oracle(traced):
    t = traced
    a, out = t["a"], t["out"]
    z = out["z_vals"]
    R, S = z.shape
    f = SR.finalize(t["ro"], t["rd"], z, t["sample_dist"], a["maskvol"], dtype=F32)
    assert torch.equal(f["mid_z"], out["mid_z_vals"]) and torch.equal(f["pm"], out["inside_sphere"])
    assert torch.equal(f["dists"][:, :-1], z[:, 1:] - z[:, :-1]) and bool((f["dists"][:, -1] == np.float32(t["sample_dist"])).all())
    assert 0 < int((f["pm"] > 0).sum()) < R * S
    # the per-sample colours and view counts the way render_core obtains them
    pts = f["pts"].reshape(-1, 3)
    with torch.no_grad():
        geo, rf, rdiff, vmask = O.projector(pts, a["volume"], a["maskvol"], a["feat_maps"], a["color_maps"], a["w2cs"], a["K"], a["img_wh"],
                                            query_cam=a["query_c2w"][:3, 3])
        rgb, nvalid = O.rendering_network(a["RW"], geo, rf, rdiff, vmask)
    inv_s = float(torch.exp(a["variance"] * 10.0).clip(1e-6, 1e6))
    c = SR.composite(t["rd"], f["mid_z"], f["dists"], f["pm"], out["sdf"].reshape(R, S), out["gradients"], rgb.reshape(R, S, 3),
                     nvalid.reshape(R, S).long(), inv_s, 0.5, 1.0, dtype=F32)
    assert torch.equal(c["color_mask"], out["color_fine_mask"][:, 0])                # selections equal
    for mine, theirs in (("color", out["color_fine"]), ("depth", out["depth"][:, 0]), ("weights", out["weights"]), ("weights_sum", out["weights_sum"][:, 0]),
                         ("weights_max", out["weights_max"][:, 0]), ("depth_var", out["depth_variance"][:, 0]), ("cdf", out["cdf_fine"])):
        assert torch.equal(c[mine], theirs), mine                                   # values bit-equal: the same expressions
    assert torch.equal(c["alpha_sum"].mean(), out["alpha_sum"])
    # the oracle returns the gradient error of the whole call only: per-ray sums regroup its one sum -> a few roundings of the total
    gerr = c["grad_err"][:, 0].sum() / (c["grad_err"][:, 1].sum() + 1e-5)
    assert abs(float(gerr) - float(out["gradient_error_fine"])) <= 8 * SR.ULP * float(out["gradient_error_fine"])
    assert float(out["weights_sum"].max()) > 0.5 and bool(out["color_fine_mask"].any())


# ------------------------------------------------------------------------------------------------ inputs and caps
@pytest.mark.parametrize("R,S,variant", SR.COARSE_CASES)
def test_coarse_inputs(R, S, variant):
    d = SR.coarse_inputs(R, S, variant)
    z64, p64 = SR.coarse(d["rays_o"], d["rays_d"], d["near"], d["far"], S, d["t_rand"])
    z32, p32 = SR.coarse(d["rays_o"], d["rays_d"], d["near"], d["far"], S, d["t_rand"], dtype=F32)
    bz, bp = SR.coarse_bounds(d, z64, p64)
    assert bool(((z32.double() - z64).abs() <= bz).all()) and bool(((p32.double() - p64).abs() <= bp).all())       # the derived bound holds for ATen's float32
    assert float(bz.max()) < 1e-3 * (SR.FAR - SR.NEAR) / S                                                       # and is far below a misplaced sample


@pytest.mark.parametrize("R,S,inv_s", SR.UPSAMPLE_CASES)
def test_upsample_inputs_and_caps(R, S, inv_s, hc):
    d = SR.upsample_inputs(R, S, inv_s)
    z, sdf, m, fam = d["z"], d["sdf"], d["m"], d["family"]
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    w32, w64 = SR.upsample_weights(z, sdf, m, inv_s, F32), SR.upsample_weights(z, sdf, m, inv_s, F64)
    e_ref, bound = SR.rule_e_bound(w32, w64)
    print(f"upsample R={R} S={S} inv_s={inv_s:g}: weights e_ref {e_ref:.2e}")
    assert e_ref <= E_REF_CAP
    if R >= 5:                                                                      # the families are what they are named
        sign = torch.sign(sdf)
        crossings = (sign[:, 1:] != sign[:, :-1]).sum(1)
        assert bool((crossings[fam == 0] <= 1).all()) and bool((crossings[fam == 1] == 0).all())
        if S >= 9:
            assert int(crossings[fam == 2].max()) >= 2
            assert bool(((z[:, 1:] == z[:, :-1]).sum(1)[fam == 4] >= 1).all())
        k = fam == 3
        assert bool((sdf[k][m[k] == 0] == 100.0).all())
    if R >= 63:
        mm = (m[:, 1:] * m[:, :-1])
        assert 0 < int((mm > 0).sum()) < mm.numel() and bool(((sdf == 100.0).sum(1)[fam == 3] > 1).any())
    # the host build: the scratch rows hold the section weights (rule E), the new depths follow rule Z on those rows
    zs, ss = np_sm(z), np_sm(sdf)
    mask = np.ascontiguousarray(SR.synthetic_mask().numpy())
    ro, rd = d["rays_o"].numpy(), d["rays_d"].numpy()
    fine = SR.fine_rays(d)
    for n_imp in SR.UPSAMPLE_NIMP:
        wbuf = np.zeros((S, R), np.float32)
        nz = np.zeros((n_imp, R), np.float32)
        hc.hc_upsample(P(ro), P(rd), R, P(zs), P(ss), S, ctypes.c_float(inv_s), P(mask), SR.MASK_D, P(wbuf), n_imp, P(nz))
        hw = torch.from_numpy(wbuf[:S - 1].T.copy())
        assert float((hw.double() - w64).abs().max()) <= bound
        got = torch.from_numpy(nz.T.copy())
        assert bool((got[:, 1:] >= got[:, :-1]).all()) and bool((got >= z[:, :1]).all()) and bool((got <= z[:, -1:]).all())
        if R == 1 and n_imp == 1:                                                   # exactly ONE new sample inside the mask: the case k_quirk_min2 reports as none
            assert int((SR.occupancy(SR.synthetic_mask(), SR.ray_points(d["rays_o"], d["rays_d"], got)) > 0).sum()) == 1
        q = SR.rule_z(z, hw)(n_imp)
        raw = float(q["dev32"][fine].max()) if bool(fine.any()) else 0.0
        # the deviation in units of the cdf: the cdf and the normaliser are serial sums of S - 1 float32 terms (<= (S - 1) 2^-24 at the end), u and
        # the quotient add a few roundings; the product and the final sum round the depth itself (2 ulp(z), whatever the bin's sensitivity)
        assert bool((q["dev32"] <= (S + 8) * 2.0 ** -24 + 2 * SR.ULP * q["new_z"].abs() / q["sens"].clamp(min=1e-300))[fine].all()), raw
        if not bool(fine.any()):
            continue
        n = q["band"][fine].numel()
        assert int(q["band"][fine].sum()) <= 0.01 * n + 0.5
        C = 4 * raw
        bz = SR.rule_z_bound(q, C, fine)
        wide = int((bz[fine] > q["width"][fine] + 4 * SR.ULP * q["new_z"][fine].abs()).sum()) - int(q["band"][fine].sum())
        err = (got.double() - q["new_z"]).abs()
        print(f"  n_imp={n_imp}: raw deviation {raw:.2e} ({raw / (S * 2.0 ** -24):.2f} S 2^-24), band {int(q['band'][fine].sum())}/{n}, "
              f"bound wider than the bin {wide}/{n}, host err/bound {float((err / bz)[fine].max()):.2f}")
        if (S, n_imp) in SR.RULE_Z_DROPPED:
            continue
        assert wide <= 0.01 * n + 0.5
        assert bool((err <= bz).all())


@pytest.mark.parametrize("R,S,n_new", SR.MERGE_CASES)
def test_merge_inputs_and_host_build(R, S, n_new, hc):
    d = SR.merge_inputs(R, S, n_new)
    zz, ss = SR.merge(d["z"], d["sdf"], d["new_z"], d["new_sdf"])
    assert bool((zz[:, 1:] >= zz[:, :-1]).all())
    if R >= 63 and S >= 16:                                                          # ties between list and block, duplicates inside the block: present
        tie = d["content"] == SR.MERGE_CONTENT.index("ties")
        assert bool(((d["new_z"][tie][:, :, None] == d["z"][tie][:, None, :]).any(2).sum(1) >= 1).all())
        dup = d["content"] == SR.MERGE_CONTENT.index("duplicates")
        if n_new > 2:
            assert bool(((torch.sort(d["new_z"][dup], 1).values.diff(dim=1) == 0).sum(1) >= 1).all())
    zc = np.zeros((S + n_new, R), np.float32); sc = np.zeros((S + n_new, R), np.float32)
    zc[:S] = np_sm(d["z"]); sc[:S] = np_sm(d["sdf"])
    hc.hc_merge(R, P(zc), P(sc), S, P(np_sm(d["new_z"])), P(np_sm(d["new_sdf"])), n_new)
    assert np.array_equal(zc.T, zz.numpy()) and np.array_equal(sc.T, ss.numpy())


@pytest.mark.parametrize("R,S", SR.FINALIZE_CASES)
def test_finalize_inputs(R, S):
    d = SR.finalize_inputs(R, S)
    f32_, f64_ = (SR.finalize(d["rays_o"], d["rays_d"], d["z"], d["sample_dist"], SR.synthetic_mask(), dtype=t) for t in (F32, F64))
    if R * S >= 16:
        assert 0 < int((f32_["pm"] > 0).sum()) < R * S
    assert float((f32_["pm"].double() != f64_["pm"]).double().mean()) <= 0.02       # points on a voxel boundary are rare: the float32 flags are compared
    for k, b in SR.finalize_bounds(d, f64_).items():                                # the derived roundings hold for ATen's float32
        assert bool(((f32_[k].double() - f64_[k]).abs() <= b).all()), k
    assert float(SR.finalize_bounds(d, f64_)["pts"].max()) < 1e-6


@pytest.mark.parametrize("R,S,air,inv_s,bg", SR.COMPOSITE_CASES)
def test_composite_inputs_and_caps(R, S, air, inv_s, bg, hc):
    d = SR.composite_inputs(R, S, air, inv_s, bg)
    r32, r64 = SR.composite_refs(d)
    assert torch.equal(r32["color_mask"], r64["color_mask"]) and torch.equal(r32["grad_err"][:, 1].double(), r64["grad_err"][:, 1])
    seen = (d["nviews"] >= 2).sum(1)
    if S >= 9:
        assert bool((seen[d["kind"] == 1] == 8).all()) and bool((seen[d["kind"] == 2] == 9).all())
        assert not bool(r64["color_mask"][d["kind"] == 1].any()) and bool(r64["color_mask"][d["kind"] == 2].all())
    assert bool((d["pm"][d["kind"] == 0] == 0).all()) and bool((d["sdf"][d["pm"] == 0] == 100.0).all())
    if inv_s >= 1e5:                                                                # the step function: both precisions on the same side of every step
        for sg in (-1.0, 1.0):
            h32 = SR.composite_half(d["rays_d"], d["grad"], d["pm"], d["dists"], air, F32)
            h64 = SR.composite_half(d["rays_d"], d["grad"], d["pm"], d["dists"], air, F64)
            a32, a64 = d["sdf"] + sg * h32, d["sdf"].double() + sg * h64
            assert torch.equal(torch.sign(a32).double(), torch.sign(a64)) and float(a64.abs().min()) >= SR.STEP_MARGIN
    host = {k: np.zeros(tuple(SR.sm(v).shape) if v.dim() == 2 and k in ("weights", "cdf") else tuple(v.shape),
                        np.uint8 if k == "color_mask" else np.float32) for k, v in r32.items()}
    hc.hc_composite(P(d["rays_o"].numpy()), P(d["rays_d"].numpy()), R, S, P(np_sm(d["mid_z"])), P(np_sm(d["dists"])), P(np_sm(d["pm"])), P(np_sm(d["sdf"])),
                    P(np_sm(d["grad"])), P(np_sm(d["rgb"])), P(np_sm(d["nviews"])), ctypes.c_float(inv_s), ctypes.c_float(air), ctypes.c_float(bg),
                    *[P(host[k]) for k in SR.COMPOSITE_OUTPUTS])
    assert np.array_equal(host["color_mask"].astype(bool), r64["color_mask"].numpy())
    assert np.array_equal(host["grad_err"][:, 1], r64["grad_err"][:, 1].numpy())
    for k in SR.COMPOSITE_OUTPUTS[:-1]:
        ref32, ref64 = (r[k][:, 0] if k == "grad_err" else r[k] for r in (r32, r64))
        got = torch.from_numpy(host[k][:, 0].copy() if k == "grad_err" else (host[k].T.copy() if k in ("weights", "cdf") else host[k]))
        e_ref, bound = SR.rule_e_bound(ref32, ref64)
        mag = max(1.0, float(ref64.abs().max()))
        err = float((got.double() - ref64).abs().max())
        print(f"composite R={R} S={S} inv_s={inv_s:g} {k}: e_ref {e_ref:.2e} (magnitude {float(ref64.abs().max()):.3g}), host err {err:.2e}, bound {bound:.2e}")
        assert e_ref <= E_REF_CAP * mag, k                                          # the cap: no input widens its own tolerance
        assert err <= bound, k
