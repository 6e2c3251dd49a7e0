"""CPU: the trained-like families of tests/trained_weights.py do what tests/test_gpu_trained_weights.py relies on.

  family conditions   distinct non-zero biases; softplus' pre-activations in all three regimes (near zero, the linear branch, the flat branch)
  sensitivity gate    a bias (or w2 row) read at the wrong place -- stood for, on the reference side, by exchanging the vector's largest and smallest
                      entry -- moves every output that depends on the vector by at least 10 x the bound the GPU test applies to that case and output.
                      The gate runs on the cases with 33 points or more: a single point (n = 1, P = 1) is a shape case (one live lane), and cannot pin
                      an exchange of two neurons that are both saturated at it.  What depends on what: b0, b1, the w2 rows -> SDF, features, gradient
                      (not the latent, which depends on no weight); b2 -> the features (variant 1 reads all 128 entries), and b2[0] <-> b2[1] for the SDF
                      of the kernels that read entry 0 alone; b2 drops out of the gradient.  Colour: every bias vector by exchange, the three scalars
                      by zeroing, s by 0.2 for V >= 5 (with two views the pooling weights are 1 and 0 whatever s is).  rgb_fc.4.bias shifts every
                      view's score alike and cancels in the softmax: NOTHING can pin it (asserted below as a change under 1e-12).  Gated as well, on
                      their own rows and bounds: the subset that the index + n_dev run compares, the voxel centres of the given-latents run, the
                      lattices.  The perturbations are trained_weights.sdf_perturbations / color_perturbations; the GPU file packs them into blobs.
  floor and ok        float32 and float64 agree on the cell and on the inside test of every random point and every planted row: no point is left out
                      of a comparison, and all planted rows are compared for value and gradient (trained_weights.PLANT_BOTH and node0..node3)
  weight-norm fold    g != ||v||: both folds of the product reproduce W to 1 ulp, each with a gain made from the float32 norm it uses itself (torch's
                      for the state-dict reader, numpy's for fold_weight_norm), and agree with torch.nn.utils.weight_norm's forward to 5 x 2^-24
  emulators           the lane-by-lane emulators of tests/weights_emulators.py on the packed blobs of both families, at their tolerances"""
import numpy as np
import pytest
import torch

import trained_weights as TW
import weights_emulators as EMU
from oracle import recon as O

F32, F64 = TW.F32, TW.F64
GATE = 10.0
SDF_GATE_CASES = [c for c in TW.SDF_CASES if c[1] >= 33]
COLOR_GATE_CASES = [c for c in TW.COLOR_CASES if c[1] >= 33]


# ------------------------------------------------------------------------------------------------ family conditions
def test_biases_are_distinct_and_non_zero():
    W = TW.trained_sdf_weights()
    allb = np.concatenate([W[k] for k in TW.SDF_BIAS_KEYS])
    assert allb.size == 384 and len(set(allb.tolist())) == 384 and bool((allb != 0).all())
    row = W["w2"][0, :128]
    assert (row < 0).sum() >= 10 and (row > 0).sum() >= 64 and row.std() > 0.05                 # a spread row with both signs
    assert W["w0"][:, 3:].std() > 0.08 and W["w1"][:, 128:].std() > 0.08 and W["w2"][:, 128:].std() > 0.08
    sd = TW.trained_color_state_dict()
    for k, v in sd.items():
        if k.endswith(".bias"):
            assert bool((v != 0).all()) and len(set(v.tolist())) == v.size, k
    assert float(sd["s"]) < 0


@pytest.mark.parametrize("D,n", [(17, 2048), (20, 2048)])
def test_preactivations_cover_the_three_softplus_regimes(D, n):
    c = TW.sdf_case(D, n)
    Wd = TW.sdf_t(TW.trained_sdf_weights(), F64)
    pts = c["pts"][c["keep"]].double()
    a0 = O.embed(pts) @ Wd["w0"].T + Wd["b0"]
    a1 = torch.cat([O.softplus100(a0), O.trilinear_ref(c["vol"].double(), pts)], 1) @ Wd["w1"].T + Wd["b1"]
    for name, a in (("a0", a0), ("a1", a1)):
        shares = [float(m.double().mean()) for m in ((100 * a).abs() < 5, 100 * a > 16.7, 100 * a < -16.7)]
        print(name, D, n, shares)
        assert min(shares) >= 0.05, (name, shares)


# ------------------------------------------------------------------------------------------------ sensitivity gate
def _sdf_outputs(r):
    return dict(sdf=r["y"][:, 0], feat=r["y"], grad=r["grad"])


def _gate_sdf(tag, pts, vol, base_r32, base_r64):
    """every perturbation of trained_weights.sdf_perturbations against the bounds sdf_bounds gives for these rows (the larger of the two precisions')"""
    bounds = TW.sdf_bounds(base_r32, base_r64)
    bound = {out: max(b for (o, _), (_, b) in bounds.items() if o == out) for out in ("sdf", "feat", "grad")}
    base = _sdf_outputs(base_r64)
    for what, W2, outs in TW.sdf_perturbations(TW.trained_sdf_weights()):
        got = _sdf_outputs(TW.sdf_eval(pts, vol, W2, F64))
        for out in outs:
            ch = float((got[out] - base[out]).abs().max())
            print(f"{tag} {what} -> {out}: change {ch:.2e}, bound {bound[out]:.2e}, ratio {ch / bound[out]:.0f}")
            assert ch >= GATE * bound[out], (what, out, ch, bound[out])


@pytest.mark.parametrize("D,n", SDF_GATE_CASES)
def test_sensitivity_gate_sdf(D, n):
    c = TW.sdf_case(D, n)
    _gate_sdf(f"D={D} n={n}", c["pts"][c["keep"]], c["vol"], c["r32"], c["r64"])


@pytest.mark.parametrize("D", TW.INDEX_DS)
def test_sensitivity_gate_index_subset(D):
    """the rows that the index + n_dev run compares, with the bounds built on those rows"""
    c = TW.index_case(D)
    assert c["cmp_rows"].numel() >= 90 and len(set(c["idx"].tolist())) == TW.INDEX_LISTED
    _gate_sdf(f"D={D} index subset", c["pts"][c["cmp_rows"]], c["vol"], c["r32"], c["r64"])


@pytest.mark.parametrize("D", TW.INDEX_DS)
def test_sensitivity_gate_given_latents(D):
    """get_sdf_volume's call compares the SDF alone"""
    c = TW.given_latents_case(D)
    assert 8 <= int(c["kept"].sum()) <= D ** 3 // 2                    # voxels on both sides: kept ones to compare, others to stay at 1
    _, bound = TW.bounded(c["r32"], c["r64"])
    for what, W2, outs in TW.sdf_perturbations(TW.trained_sdf_weights()):
        if "sdf" in outs:
            ch = float((TW.given_latents_eval(c["pts"][c["kept"]], c["vol"], c["kept"], W2, F64) - c["r64"]).abs().max())
            print(f"D={D} given latents {what}: change {ch:.2e}, bound {bound:.2e}, ratio {ch / bound:.0f}")
            assert ch >= GATE * bound, what


@pytest.mark.parametrize("R,D", TW.LATTICE_CASES)
def test_sensitivity_gate_lattice(R, D):
    """the lattice forms compare the SDF alone: b0 (the tables' bias), b1, b2[0] and both parts of the w2 row; the masked volume of the sparse form too"""
    for masked in (False, True):
        c = TW.lattice_case(R, D, masked)
        _, bound = TW.bounded(c["r32"], c["r64"], extra=2e-6 * max(1.0, float(c["r64"].abs().max())))
        for what, W2, outs in TW.sdf_perturbations(TW.trained_sdf_weights()):
            if "sdf" in outs:
                got = TW.O.sdf(c["pts"].double(), c["vol"].double(), TW.sdf_t(W2, F64))[0][:, 0]
                ch = float((got - c["r64"]).abs().max())
                print(f"R={R} D={D} masked={masked} {what}: change {ch:.2e}, bound {bound:.2e}")
                assert ch >= GATE * bound, (what, masked)


@pytest.mark.parametrize("V,P", COLOR_GATE_CASES)
def test_sensitivity_gate_color(V, P):
    c = TW.color_case(V, P)
    sd = TW.trained_color_state_dict()
    bound = max(TW.color_bound(c["r32"], c["r64"], x3)[1] for x3 in (False, True))
    change = lambda sd2: float((TW.color_eval(c, sd2, F64)[0] - c["r64"]).abs().max())
    for what, sd2, pinned in TW.color_perturbations(sd):
        ch = change(sd2)
        print(f"V={V} P={P} {what}: change {ch:.2e}, bound {bound:.2e}, ratio {ch / bound:.0f}")
        if pinned == "never":
            assert ch < 1e-12                                    # cancels in the softmax over the views: nothing can pin it
        elif pinned == "yes" or V >= 5:
            assert ch >= GATE * bound, what
    assert change(dict(sd, s=np.float32(-TW.COLOR_S))) == 0.0   # the network takes |s|


@pytest.mark.parametrize("V,P", TW.COLOR_CASES)
def test_color_inputs_hold_what_they_were_built_for(V, P):
    c = TW.color_case(V, P)
    nv = c["mask"].sum(0)
    assert torch.equal(c["nviews"], nv.double().to(c["nviews"].dtype))
    if P >= 33:
        assert int(nv[0]) == 0 and int(nv[1]) == 1
    if P >= 257:
        assert 0.2 < 1 - float(c["mask"][:, 2:].float().mean()) < 0.4
    assert bool(torch.isfinite(c["r64"]).all()) and bool((c["r64"] >= 0).all()) and bool((c["r64"] <= 1).all())


# ------------------------------------------------------------------------------------------------ floor and ok
@pytest.mark.parametrize("D,n", TW.SDF_CASES)
def test_float32_and_float64_pick_the_same_cell(D, n):
    c = TW.sdf_case(D, n)
    pts, rows = c["pts"], c["rows"]
    (_, f32_, ok32), (_, f64_, ok64) = TW.index_of(pts, D, F32), TW.index_of(pts, D, F64)
    keep = c["keep"]
    same = (f32_.double() == f64_).all(-1) & (ok32 == ok64)
    assert int((~same[keep]).sum()) == 0                        # no point is left out: random and planted rows alike
    if n >= 33:
        want = set(TW.PLANT_BOTH) | {"nan", "huge"} | ({"node0", "node1", "node2", "node3"} if D == 17 else set())
        assert set(rows) == want
        i32 = TW.index_of(pts, D, F32)[0]
        axis = lambda name: rows[name] % 3 if name in TW.PLANT_BOTH else None
        at = lambda name: float(i32[rows[name], axis(name)])
        assert at("minus_one") == 0.0 and not bool(ok32[rows["minus_one"]])
        assert 0.0 < at("above_minus_one") < 1e-6 and bool(ok32[rows["above_minus_one"]])
        assert at("plus_one") == D - 1 and bool(ok32[rows["plus_one"]])
        assert D - 1 < at("corner_band") < D and bool(ok32[rows["corner_band"]])
        assert at("beyond") >= D and not bool(ok32[rows["beyond"]])
        below = torch.tensor(np.nextafter(np.float32(pts[rows["beyond"], axis("beyond")].item()), np.float32(0.0)))
        assert float(TW.index_of(below.reshape(1, 1), D, F32)[0]) < D or float(TW.index_of(below.reshape(1, 1), D, F64)[0]) < D
        assert not bool(ok32[rows["nan"]]) and not bool(ok32[rows["huge"]]) and not bool(keep[rows["nan"]]) and not bool(keep[rows["huge"]])
        if D == 17:
            i = i32[rows["node2"]]
            assert torch.equal(i, torch.floor(i)) and bool(ok32[rows["node2"]])
            for name, ax, node in (("node0", 0, 5.0), ("node1", 1, 16.0), ("node3", 2, 1.0)):
                assert float(i32[rows[name], ax]) == node and bool(ok32[rows[name]])
        # the latent of the rows outside is zero, of the rows just inside it is not
        lat = c["r64"]["lat"]
        pos = {name: int(keep[:r].sum()) for name, r in rows.items() if bool(keep[r])}
        assert float(lat[pos["minus_one"]].abs().max()) == 0.0 and float(lat[pos["beyond"]].abs().max()) == 0.0
        for name in ("above_minus_one", "plus_one", "corner_band"):
            assert float(lat[pos[name]].abs().max()) > 0.0, name


@pytest.mark.parametrize("R,D", TW.LATTICE_CASES)
def test_lattice_points_pick_the_same_cell(R, D):
    pts = TW.lattice_points(R)
    (i32, f32_, ok32), (_, f64_, ok64) = TW.index_of(pts, D, F32), TW.index_of(pts, D, F64)
    assert bool((f32_.double() == f64_).all()) and torch.equal(ok32, ok64)
    if (R, D) == (9, 17):
        assert torch.equal(i32, torch.floor(i32))                # every lattice point on a node
    kept = TW.kept_voxels(D)
    assert 0 < int(kept.sum()) <= 29 and bool(kept[0, 0, 0]) and bool(kept[D - 1, D - 1, D - 1])
    c = TW.lattice_case(R, D, masked=True)
    assert float(c["vol"][:, ~kept].abs().max()) == 0.0 and float(c["vol"][:, kept].abs().min()) > 0.0


# ------------------------------------------------------------------------------------------------ weight-norm fold
def test_weight_norm_fold_with_gains_that_are_not_the_norm():
    W = TW.trained_sdf_weights()
    sd = TW.trained_sdf_state_dict(W)
    read = TW.Wn.sdf_weights_from_state_dict({"sdf_layer." + k: v for k, v in sd.items()})
    ulps = lambda a, b: float((np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b))).max())
    for i in range(3):
        g, v, w = sd[f"lin{i}.weight_g"], sd[f"lin{i}.weight_v"], W[f"w{i}"]
        ratio = (g[:, 0] / v.norm(dim=1)).numpy()
        assert bool((np.abs(ratio - 1.0) > 0.4).all()) and set(np.round(ratio, 3).tolist()) == {0.5, 2.0}        # g != ||v|| in every row, both ways
        lin = torch.nn.utils.weight_norm(torch.nn.Linear(w.shape[1], 128))
        lin.load_state_dict({"bias": sd[f"lin{i}.bias"], "weight_g": g, "weight_v": v})
        lin(torch.zeros(1, w.shape[1]))                          # weight_norm's own forward computes .weight
        torch_w = lin.weight.detach().numpy()
        # each fold with a gain made from the norm it uses itself: the reader takes torch's float32 norm (the state dict's g), fold_weight_norm numpy's,
        # whose summation order is another and which lies one or two ulp from torch's; either way g = ||W|| and ||v|| = f ||W|| exactly
        g_np = np.linalg.norm(np.asarray(w, np.float32), axis=1, keepdims=True)
        assert g_np.dtype == np.float32 and bool((np.abs(g_np / np.linalg.norm(v.numpy(), axis=1, keepdims=True) - 1.0) > 0.4).all())
        folds = {"sdf_weights_from_state_dict": read[f"w{i}"], "fold_weight_norm": TW.Wn.fold_weight_norm(g_np, v.numpy())}
        # torch evaluates v * (g / ||v||) with a norm of its own summation order: three roundings (norm, quotient, product) against a fold's two
        # (product, quotient), 2^-24 relative each -> a fold and torch's forward agree to 5 * 2^-24 of the entry
        rel = lambda a, b: float((np.abs(a.astype(np.float64) - b) / np.abs(b)).max())
        assert rel(torch_w, w) <= 3 * 2.0 ** -24
        for name, f in folds.items():
            print(f"lin{i} {name}: {ulps(f, w):.1f} ulp from W, {ulps(f, torch_w):.1f} ulp ({rel(f, torch_w) * 2 ** 24:.2f} x 2^-24) from torch's weight_norm")
            assert f.dtype == np.float32 and ulps(f, w) <= 1.0 and rel(f, torch_w) <= 5 * 2.0 ** -24, (i, name)
        assert np.array_equal(read[f"b{i}"], W[f"b{i}"])


# ------------------------------------------------------------------------------------------------ emulators
def test_sdf_blob_emulators_on_the_trained_family():
    """as tests/test_weights_packing.py: the fp32 kernel's dataflow against the oracle at 2e-5, its gradient pieces at 2e-4, the split-f16 forward at 2e-6"""
    W = TW.trained_sdf_weights()
    blob = TW.Wn.pack_sdf_blob(W)
    c = TW.sdf_case(20, 2048)
    pts = c["pts"][c["keep"]][:29]
    lat = O.trilinear_ref(c["vol"], pts)
    assert float(lat.abs().max()) > 0.5
    y, gpe, glat = EMU.emulate_sdf_blob(blob, pts.numpy(), lat.numpy())
    Wt = TW.sdf_t(W)
    ref = O.sdf_mlp(pts, lat, Wt).numpy()
    assert np.abs(y - ref).max() < 2e-5
    with torch.enable_grad():
        pe = O.embed(pts).requires_grad_(True)
        lt = lat.clone().requires_grad_(True)
        sp = lambda t: torch.nn.functional.softplus(t, beta=100)
        h = sp(pe @ Wt["w0"].T + Wt["b0"])
        h = sp(torch.cat([h, lt], 1) @ Wt["w1"].T + Wt["b1"])
        out = (torch.cat([h, lt], 1) @ Wt["w2"].T + Wt["b2"])[:, 0].sum()
        gpe_ref, glat_ref = torch.autograd.grad(out, [pe, lt])
    assert np.abs(gpe - gpe_ref.numpy()).max() < 2e-4 * max(1.0, gpe_ref.abs().max().item())
    assert np.abs(glat - glat_ref.numpy()).max() < 2e-4 * max(1.0, glat_ref.abs().max().item())
    sdf = EMU.emulate_sdf_blob_x3(blob, pts.numpy(), lat.numpy())
    ref64 = O.sdf_mlp(pts.double(), lat.double(), TW.sdf_t(W, F64))[:, 0].numpy()
    assert np.abs(sdf - ref64).max() < 2e-6 * max(1.0, np.abs(ref64).max())


def test_sdf_grid_tables_on_the_trained_family():
    """the tabulated layer 0 with a non-zero b0: b0 + Tx + Ty + Tz in the kernels' lane order and t domain against W0 . embed(p) + b0"""
    W = TW.trained_sdf_weights()
    order = np.array([TW.Wn.neuron_of(nb, r, h) for h in (0, 1) for nb in range(4) for r in range(16)])
    for R, _ in TW.LATTICE_CASES:
        axes, bias = TW.Wn.sdf_grid_tables(W, R)
        assert np.array_equal(bias, (W["b0"].astype(np.float64)[order] * TW.Wn.SOFTPLUS_SCALE).astype(np.float32))
        idx = np.random.default_rng(R).integers(0, R, (300, 3))
        lin = torch.linspace(-1, 1, R)
        p = torch.stack([lin[idx[:, 0]], lin[idx[:, 1]], lin[idx[:, 2]]], -1)
        Wd = TW.sdf_t(W, F64)
        ref = (O.embed(p.double()) @ Wd["w0"].T + Wd["b0"]).numpy()[:, order]
        got = (axes[0][idx[:, 0]].astype(np.float64) + axes[1][idx[:, 1]] + axes[2][idx[:, 2]] + bias) / TW.Wn.SOFTPLUS_SCALE
        assert np.abs(got - ref).max() < 5e-6


@pytest.mark.parametrize("G", [8, 4, 32])
def test_color_blob_emulator_on_the_trained_family(G):
    """as tests/test_weights_packing.py: one wave tile of 32 / G points and G views against the oracle at 2e-5, the split-f16 form within 5e-6 of it"""
    sd = TW.trained_color_state_dict()
    blob, xblob = TW.Wn.pack_color_mfma_blob(sd), TW.Wn.pack_color_x3_blob(sd)
    so = TW.Wn.CM_LAYOUT["S_SCALAR"][0]
    assert blob[so] == np.float32(TW.COLOR_S) and bool((blob[so + 1:so + 4] != 0).all())
    d = TW.color_inputs(G, 33)
    P = 32 // G
    sub = dict(geo=d["geo"][:P], rf=d["rf"][:, :P], rd=d["rd"][:, :P], mask=d["mask"][:, :P])
    ref = TW.color_eval(sub, sd, F32)[0].numpy()
    rf64 = np.concatenate([sub["rf"].permute(1, 0, 2).numpy(), np.zeros((P, G, 5), np.float32)], -1)
    a = (sub["geo"].numpy(), rf64, sub["rd"].permute(1, 0, 2).numpy(), sub["mask"].permute(1, 0).float().numpy(), G)
    got = EMU.emulate_color_mfma(blob, *a)
    assert np.abs(got - ref).max() < 2e-5
    gotx = EMU.emulate_color_mfma(blob, *a, x3_blob=xblob)
    assert np.abs(gotx - got).max() < 5e-6
