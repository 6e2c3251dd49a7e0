"""The SDF and colour network kernels on trained-like weights (tests/trained_weights.py: distinct non-zero biases, a spread w2 row, PE and latent weights
of O(0.1), g != ||v||, a negative s) against the float64 oracle, and the suite's bit-for-bit claims repeated on this family.  With the initialisers'
weights every bias vector is zero or constant, and a bias read at the wrong lane, block or scale returns the right answer; here it moves the output by
32 to 290,000 times the bound (tests/test_trained_weights_cpu.py, the sensitivity gate, which asks for 10).

Tolerances (trained_weights.sdf_bounds / color_bound), per case and output, e_ref = max |oracle in float32 - oracle in float64| on the same case:
  fp32 forms        rule E: max |gpu - ref64| <= 4 e_ref + 4 ulp of the output's magnitude
  split-f16 forms   rule E + 2e-6 max(1, |sdf|max) for the SDF, + 5e-6 for the colour, rule E alone for the gradient
  ceiling           2e-5 max(1, magnitude) for SDF, features and latent, 1e-4 max(1, magnitude) for gradient and colour
  exact             form against form (lattice against explicit points, sparse against full, sign, mesh_project's field, the mirror module), nviews,
                    slots not listed by an index
Every comparison prints e_ref, the device error and the bound.

Shapes: latent volumes of side 2, 3, 17, 20; 1, 33, 257, 2048 points (one live lane, two tiles, two workgroups, eight workgroups = the per-XCD tile
schedule), rows planted on the volume's edges (trained_weights.sdf_points); the NaN and 1e30 rows have no finite embedding, so what is asserted of
them is what the sampler promises: a latent of exactly zero (every fp32 variant returns it) and no effect on any other row.  What any form writes
as the SDF, the features or the gradient of such a row is unspecified, and is not looked at.  Colour: V in 2, 5, 8, 19 and P in 1, 33, 257.

Observed on an MI355X, maxima over the cases (error, and its share of the bound; DESIGN.md section 4, "Trained-like weights: what pins what").  No bound
had to be raised, and the gradient of the split-f16 kernel stays inside rule E alone:
  fp32 kernel      sdf 3.2e-6 at e_ref 3.1e-6 (0.23; 0.55 at n = 1, where e_ref is one point's 2.6e-8), features 5.6e-6 (0.23), latent 5.2e-6 = e_ref (0.24),
                   gradient 1.5e-4 at a magnitude of 37 and e_ref 1.6e-4 (0.23; 0.39 on the side-2 volume)
  split-f16        sdf 3.0e-6 (0.14), gradient 1.5e-4 (0.22; 0.51 at D = 2, n = 1: 3.8e-6 of 7.4e-6)
  index + n_dev    sdf 1.6e-6 (0.21), gradient 5.4e-5 (0.23; 0.29 for the split-f16 form at D = 3); given latents 1.2e-6 (0.11)
  lattice          fp32 1.2e-6 (0.15); split-f16 with the embedding per point 1.7e-6 (0.09), tabulated 1.3e-6 (0.08), sparse 1.1e-6 (0.08)
  colour           fp32 2.5e-7 at e_ref 1.7e-7 (0.22; 0.32 at P = 1), split-f16 4.6e-7 (0.08); fused against materialised 2.4e-7 of 2e-5
Blobs packed from weights with one vector's extremes exchanged (a scalar zeroed, s = 0.2), the device-side twin of the CPU gate
(test_a_perturbed_*_blob_is_noticed), miss the truth by 52 (vis_fc.2's row 32 zeroed, split-f16) to 129,000 (vis_fc.2's vector, fp32) times the bound."""
import importlib

import numpy as np
import pytest
import torch

import trained_weights as TW
from mesh_scene_util import sdf_field
from scene_util import small_scene

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64

pkg = importlib.import_module("one-2-3-45_amd")
Wn = pkg.weights
mio = importlib.import_module("one-2-3-45_amd.mesh_io")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


@pytest.fixture(scope="module")
def blob(dev):
    """the SDF blob packed from the trained-like W"""
    return torch.from_numpy(Wn.pack_sdf_blob(TW.trained_sdf_weights())).to(dev)


@pytest.fixture(scope="module")
def color_blobs(dev):
    sd = TW.trained_color_state_dict()
    return {False: torch.from_numpy(Wn.pack_color_mfma_blob(sd)).to(dev), True: torch.from_numpy(Wn.pack_color_x3_blob(sd)).to(dev)}


def cl(vol, dev):
    """[16,D,D,D] -> the samplers' channel-last layout on the device"""
    return vol.permute(1, 2, 3, 0).contiguous().to(dev)


def check(got, ref64, eb, what):
    """rule E with the case's (e_ref, bound): prints and asserts -> the device error"""
    e_ref, bound = eb
    got = got.detach().cpu()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err = (got.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f"{what}: e_ref {e_ref:.2e}, device err {err:.2e}, bound {bound:.2e} ({err / bound if bound else 0.0:.2f})")
    assert err <= bound, f"{what}: device err {err:.3e} > bound {bound:.3e} (e_ref {e_ref:.3e})"
    return err


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ SDF against float64
@pytest.mark.parametrize("D,n", TW.SDF_CASES)
def test_sdf_fp32(dev, ops, blob, D, n):
    """the fp32 MFMA kernel: variant 0 with the latent, variant 1 with all 128 features, variant 2; sign = -1"""
    c = TW.sdf_case(D, n)
    keep, r64 = c["keep"], c["r64"]
    b = TW.sdf_bounds(c["r32"], r64)
    vol, pts = cl(c["vol"], dev), c["pts"].to(dev)
    tag = f"fp32 D={D} n={n}"
    r0 = ops.sdf_mlp(blob, vol, pts, variant=0, want_lat=True, precision="fp32")
    check(r0["sdf"].cpu()[keep], r64["y"][:, 0], b["sdf", "fp32"], tag + " variant 0 sdf")
    check(r0["lat"].cpu()[keep], r64["lat"], b["lat", "fp32"], tag + " variant 0 latent")
    r1 = ops.sdf_mlp(blob, vol, pts, variant=1, want_lat=True, precision="fp32")
    check(r1["sdf"].cpu()[keep], r64["y"][:, 0], b["sdf", "fp32"], tag + " variant 1 sdf")
    check(r1["feat"].cpu()[keep], r64["y"], b["feat", "fp32"], tag + " variant 1 features")
    r2 = ops.sdf_mlp(blob, vol, pts, variant=2, want_lat=True, precision="fp32")
    for variant, r in enumerate((r0, r1, r2)):
        for name in ("nan", "huge"):
            if name in c["rows"]:                               # outside for the sampler: a latent of exactly zero, in every variant that returns it
                assert float(r["lat"][c["rows"][name]].abs().max()) == 0.0, (variant, name)
        if variant:
            check(r["lat"].cpu()[keep], r64["lat"], b["lat", "fp32"], tag + f" variant {variant} latent")
    check(r2["sdf"].cpu()[keep], r64["y"][:, 0], b["sdf", "fp32"], tag + " variant 2 sdf")
    check(r2["grad"].cpu()[keep], r64["grad"], b["grad", "fp32"], tag + " variant 2 gradient")
    neg = ops.sdf_mlp(blob, vol, pts, variant=2, sign=-1.0, precision="fp32")
    assert same_bits(neg["sdf"].cpu()[keep], -r2["sdf"].cpu()[keep]) and same_bits(neg["grad"].cpu()[keep], r2["grad"].cpu()[keep])


@pytest.mark.parametrize("D,n", TW.SDF_CASES)
def test_sdf_x3(dev, ops, blob, D, n):
    """the split-f16 kernels: variant 0 and variant 2 (its workgroup barrier inside the tile loop; n = 2048 is on the per-XCD schedule); sign = -1"""
    c = TW.sdf_case(D, n)
    keep, r64 = c["keep"], c["r64"]
    b = TW.sdf_bounds(c["r32"], r64)
    vol, pts = cl(c["vol"], dev), c["pts"].to(dev)
    tag = f"f16x3 D={D} n={n}"
    r0 = ops.sdf_mlp(blob, vol, pts, variant=0, precision="f16x3")
    check(r0["sdf"].cpu()[keep], r64["y"][:, 0], b["sdf", "f16x3"], tag + " variant 0 sdf")
    r2 = ops.sdf_mlp(blob, vol, pts, variant=2, precision="f16x3")
    check(r2["sdf"].cpu()[keep], r64["y"][:, 0], b["sdf", "f16x3"], tag + " variant 2 sdf")
    check(r2["grad"].cpu()[keep], r64["grad"], b["grad", "f16x3"], tag + " variant 2 gradient")
    for variant, pos in ((0, r0), (2, r2)):
        neg = ops.sdf_mlp(blob, vol, pts, variant=variant, sign=-1.0, precision="f16x3")
        assert same_bits(neg["sdf"].cpu()[keep], -pos["sdf"].cpu()[keep]), variant
        if variant == 2:
            assert same_bits(neg["grad"].cpu()[keep], pos["grad"].cpu()[keep])


@pytest.mark.parametrize("D", TW.INDEX_DS)
@pytest.mark.parametrize("prec,variant", [("fp32", 2), ("f16x3", 0), ("f16x3", 2)])
def test_sdf_index_and_device_count(dev, ops, blob, D, prec, variant):
    """n = 257 through an index list and a device-side count (the grid is then sized to every compute unit) into pre-filled outputs: the first
    n_dev listed slots against float64, every other slot untouched"""
    c = TW.index_case(D)
    idx, n_dev, listed, cmp_rows, r64 = c["idx"], TW.INDEX_N_DEV, c["listed"], c["cmp_rows"], c["r64"]
    b = TW.sdf_bounds(c["r32"], r64)
    out = {"sdf": torch.full((257,), 100.0, device=dev)}
    if variant == 2:
        out["grad"] = torch.full((257, 3), 7.0, device=dev)
    ops.sdf_mlp(blob, cl(c["vol"], dev), c["pts"].to(dev), variant=variant, index=idx.to(dev), n_dev=torch.tensor([n_dev], dtype=torch.int32, device=dev),
                out=out, precision=prec)
    tag = f"{prec} variant {variant} D={D} index + n_dev"
    check(out["sdf"].cpu()[cmp_rows], r64["y"][:, 0], b["sdf", prec], tag + " sdf")
    rest = torch.ones(257, dtype=torch.bool)
    rest[listed] = False
    assert bool((out["sdf"].cpu()[rest] == 100.0).all())
    if variant == 2:
        check(out["grad"].cpu()[cmp_rows], r64["grad"], b["grad", prec], tag + " gradient")
        assert bool((out["grad"].cpu()[rest] == 7.0).all())


@pytest.mark.parametrize("D", TW.INDEX_DS)
def test_sdf_given_latents_as_get_sdf_volume_calls_it(dev, ops, blob, D):
    """lat_in with an index: every kept voxel's centre with the voxel's OWN latent row, into a volume pre-filled with ones"""
    c = TW.given_latents_case(D)
    vol, pts, kept, r32, r64 = c["vol"], c["pts"], c["kept"], c["r32"], c["r64"]
    idx = torch.nonzero(kept)[:, 0].to(torch.int32)
    vol_cl = cl(vol, dev)
    out = {"sdf": torch.ones(D ** 3, device=dev)}
    ops.sdf_mlp(blob, vol_cl, pts.to(dev), variant=0, index=idx.to(dev), out=out, lat_in=vol_cl.reshape(-1, 16))
    check(out["sdf"].cpu()[kept], r64, TW.bounded(r32, r64), f"lat_in + index D={D} sdf")
    assert bool((out["sdf"].cpu()[~kept] == 1.0).all())


# ------------------------------------------------------------------------------------------------ the lattice forms
def _tables(ops, dev, R):
    axes, bias = Wn.sdf_grid_tables(TW.trained_sdf_weights(), R)
    return ops.sdf_grid_tables(torch.from_numpy(axes).to(dev), torch.from_numpy(bias).to(dev))


@pytest.mark.parametrize("R,D", TW.LATTICE_CASES)
def test_sdf_lattice_forms(dev, ops, blob, R, D):
    """the lattice by per-point embedding (both precisions), with layer 0 tabulated (b0 folded into tab_xy), and evaluated only where the scene has a
    latent: the background is the bias-laden field of the empty scene, built as pipeline.SceneWeights.grid_background builds it"""
    c = TW.lattice_case(R, D)
    x3 = 2e-6 * max(1.0, float(c["r64"].abs().max()))
    eb32, ebx = TW.bounded(c["r32"], c["r64"]), TW.bounded(c["r32"], c["r64"], extra=x3)
    vol = cl(c["vol"], dev)
    tag = f"lattice R={R} D={D}"
    check(ops.sdf_mlp(blob, vol, None, variant=0, grid_R=R, precision="fp32")["sdf"], c["r64"], eb32, tag + " fp32")
    check(ops.sdf_mlp(blob, vol, None, variant=0, grid_R=R, precision="f16x3")["sdf"], c["r64"], ebx, tag + " f16x3, embedding per point")
    tabs = _tables(ops, dev, R)
    full = ops.sdf_mlp(blob, vol, None, variant=0, grid_R=R, precision="f16x3", grid_tables=tabs)["sdf"]
    check(full, c["r64"], ebx, tag + " f16x3, layer 0 tabulated")
    u = ops.sdf_mlp(blob, vol, None, variant=0, grid_R=R, sign=-1.0, precision="f16x3", grid_tables=tabs)["sdf"]
    assert same_bits(u, -full)
    # the sparse form on a volume that is zero outside a few kept voxels
    m = TW.lattice_case(R, D, masked=True)
    mvol = cl(m["vol"], dev)
    maskvol = TW.kept_voxels(D).to(F32).reshape(-1).contiguous().to(dev)
    empty = torch.zeros(2, 2, 2, 16, dtype=F32, device=dev)
    background = ops.sdf_mlp(blob, empty, None, variant=0, grid_R=R, sign=1.0, precision="f16x3", grid_tables=tabs)["sdf"]
    ebm = TW.bounded(m["r32"], m["r64"], extra=2e-6 * max(1.0, float(m["r64"].abs().max())))
    for sign in (1.0, -1.0):
        mfull = ops.sdf_mlp(blob, mvol, None, variant=0, grid_R=R, sign=sign, precision="f16x3", grid_tables=tabs)["sdf"]
        out = {"sdf": torch.full((R ** 3,), float("nan"), device=dev)}
        sparse = ops.sdf_mlp(blob, mvol, None, variant=0, grid_R=R, sign=sign, precision="f16x3", grid_tables=tabs, maskvol=maskvol,
                             grid_background=background, out=out)["sdf"]
        assert same_bits(sparse, mfull), sign
        assert 0 < ops.sdf_grid_active_points(dev) < R ** 3
        check(sign * sparse, m["r64"], ebm, tag + f" f16x3, sparse, sign {sign:+.0f}")


@pytest.mark.parametrize("prec,variant", [("fp32", 0), ("fp32", 1), ("fp32", 2), ("f16x3", 0), ("f16x3", 2)])
def test_sdf_lattice_equals_explicit_points(dev, ops, blob, prec, variant):
    R, D = TW.LATTICE_CASES[0]
    vol = cl(TW.sdf_volume(D), dev)
    a = ops.sdf_mlp(blob, vol, None, variant=variant, grid_R=R, precision=prec)
    b = ops.sdf_mlp(blob, vol, TW.lattice_points(R).to(dev), variant=variant, precision=prec)
    assert set(a) == set(b) == [{"sdf"}, {"sdf", "feat"}, {"sdf", "grad"}][variant]
    for k in a:
        assert a[k].shape[0] == R ** 3 and same_bits(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
    assert bool(torch.isfinite(a["sdf"]).all()) and float(a["sdf"].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ the gate, seen from the device
NOTICED = 9.0      # the gate moves the reference by >= 10 bounds, the device stays within 1 bound of its own truth: >= 9 bounds from the unperturbed one
SDF_PERTURBED = [name for name, _, _ in TW.sdf_perturbations(TW.trained_sdf_weights())]
COLOR_PERTURBED = [name for name, _, _ in TW.color_perturbations(TW.trained_color_state_dict())]


def _far(got, ref64, eb, what):
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    print(f"{what}: device err {err:.2e}, bound {eb[1]:.2e} ({err / eb[1]:.0f})")
    assert err >= NOTICED * eb[1], f"{what}: a perturbed blob within {err / eb[1]:.1f} bounds of the unperturbed truth"


@pytest.mark.parametrize("which", range(len(SDF_PERTURBED)), ids=SDF_PERTURBED)
def test_a_perturbed_sdf_blob_is_noticed(dev, ops, which):
    """a blob packed from weights with one vector's extremes exchanged (trained_weights.sdf_perturbations: what a kernel reading the wrong lane would
    see) misses the unperturbed truth by nine bounds or more in every output that depends on the vector, in both precisions: the packer puts every
    entry where the kernels read it, and the comparisons above would fail"""
    name, W2, outs = TW.sdf_perturbations(TW.trained_sdf_weights())[which]
    bad = torch.from_numpy(Wn.pack_sdf_blob(W2)).to(dev)
    c = TW.sdf_case(20, 2048)
    keep, r64 = c["keep"], c["r64"]
    b = TW.sdf_bounds(c["r32"], r64)
    vol, pts = cl(c["vol"], dev), c["pts"].to(dev)
    r1 = ops.sdf_mlp(bad, vol, pts, variant=1, precision="fp32")
    if "feat" in outs:
        _far(r1["feat"][keep.to(dev)], r64["y"], b["feat", "fp32"], f"{name}: fp32 features")
    for prec in ("fp32", "f16x3"):
        r0 = ops.sdf_mlp(bad, vol, pts, variant=0, precision=prec)
        r2 = ops.sdf_mlp(bad, vol, pts, variant=2, precision=prec)
        if "sdf" in outs:
            _far(r0["sdf"][keep.to(dev)], r64["y"][:, 0], b["sdf", prec], f"{name}: {prec} variant 0 sdf")
            _far(r2["sdf"][keep.to(dev)], r64["y"][:, 0], b["sdf", prec], f"{name}: {prec} variant 2 sdf")
        if "grad" in outs:
            _far(r2["grad"][keep.to(dev)], r64["grad"], b["grad", prec], f"{name}: {prec} gradient")


@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("which", range(len(COLOR_PERTURBED)), ids=COLOR_PERTURBED)
def test_a_perturbed_color_blob_is_noticed(dev, ops, which, x3):
    """the same for the colour blobs (trained_weights.color_perturbations) at V = 8, P = 257; rgb_fc.4.bias, which cancels, still passes the bound"""
    name, sd2, pinned = TW.color_perturbations(TW.trained_color_state_dict())[which]
    bad = torch.from_numpy((Wn.pack_color_x3_blob if x3 else Wn.pack_color_mfma_blob)(sd2)).to(dev)
    c = TW.color_case(8, 257)
    rgb, _ = ops.color_from_features(bad, c["geo"].to(dev), c["rf"].to(dev), c["rd"].to(dev), c["mask"].float().to(dev), x3=x3)
    eb = TW.color_bound(c["r32"], c["r64"], x3)
    what = f"{name}: colour {'f16x3' if x3 else 'fp32'}"
    if pinned == "never":
        check(rgb, c["r64"], eb, what)
    else:
        _far(rgb, c["r64"], eb, what)


# ------------------------------------------------------------------------------------------------ bit-for-bit claims of other units
@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_mesh_project_evaluates_variant_2(dev, ops, blob, prec):
    """ops.mesh_project against its host twin with the device's own variant-2 kernel as the field: bytes and info equal"""
    R, D = 33, 20
    vol = cl(TW.sdf_volume(D), dev)
    hv = np.random.default_rng(4).uniform(0.0, R - 1.0, (300, 3))
    v, info = ops.mesh_project(blob, vol, torch.from_numpy(hv).to(dev), R, 2, precision=prec)
    wv, winfo = mio.project_vertices(hv, sdf_field(blob, vol, prec), R, 2)
    assert info == winfo and info["evaluated"][0] == 300 and info["max_before"] > 1e-2, (info, winfo)
    assert v.cpu().numpy().tobytes() == wv.tobytes()


def test_mirror_module_loaded_from_the_state_dict(dev, ops):
    """recon.SparseSdfNetwork with lin{0,1,2}.{bias,weight_g,weight_v} of the trained-like family (g != ||v||): sdf(), gradient() and get_sdf_volume()
    return what ops.sdf_mlp returns on the blob packed from the folded weights (W to 1 ulp: tests/test_trained_weights_cpu.py)"""
    recon = importlib.import_module("one-2-3-45_amd.recon")
    D = 17
    sd = TW.trained_sdf_state_dict(TW.trained_sdf_weights())
    net = recon.SparseSdfNetwork(lod=0, ch_in=56, voxel_size=2.0 / (D - 1), vol_dims=[D, D, D], hidden_dim=128, cost_type="variance_mean",
                                 d_pyramid_feature_compress=16, regnet_d_out=16, num_sdf_layers=4, multires=6).to(dev)
    missing = net.load_state_dict({"sdf_layer." + k: v for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and not any(k.startswith("sdf_layer.") for k in missing.missing_keys)
    want = torch.from_numpy(Wn.pack_sdf_blob(Wn.sdf_weights_from_state_dict(sd, ""))).to(dev)
    assert torch.equal(net.sdf_layer.blob(), want)
    c = TW.sdf_case(D, 257)
    pts = c["pts"][c["keep"]].contiguous().to(dev)
    volume = c["vol"][None].contiguous().to(dev)                                     # the reference's layout [1,16,D,D,D]
    vol_cl = cl(c["vol"], dev)
    got = net.sdf(pts, volume, 0)
    r1 = ops.sdf_mlp(want, vol_cl, pts, variant=1, want_lat=True)
    assert same_bits(got["sdf_pts_scale0"], r1["feat"][:, :1]) and same_bits(got["sdf_features_pts_scale0"], r1["feat"][:, 1:])
    assert same_bits(got["sampled_latent_scale0"], r1["lat"])
    assert same_bits(net.gradient(pts, volume, 0), ops.sdf_mlp(want, vol_cl, pts, variant=2)["grad"].unsqueeze(1))
    kept = torch.rand(D, D, D, generator=torch.Generator().manual_seed(D)) < 0.3
    lattice = net._voxel_lattice((D, D, D), dev)
    sv = net.get_sdf_volume(volume, kept[None, None].float().to(dev), lattice, torch.tensor([[-1.0, -1.0, -1.0]], device=dev))
    centres = (lattice.reshape(3, -1).t() * (2.0 / (D - 1)) + torch.tensor([[-1.0, -1.0, -1.0]], device=dev)).contiguous().float()
    out = {"sdf": torch.ones(D ** 3, device=dev)}
    ops.sdf_mlp(want, vol_cl, centres, variant=0, index=torch.nonzero(kept.reshape(-1))[:, 0].to(torch.int32).to(dev), out=out,
                lat_in=vol_cl.reshape(-1, 16))
    assert tuple(sv.shape) == (1, 1, D, D, D) and same_bits(sv.reshape(-1), out["sdf"])
    assert bool((sv.reshape(-1).cpu()[~kept.reshape(-1)] == 1.0).all()) and float((sv.reshape(-1).cpu()[kept.reshape(-1)] - 1.0).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ colour
@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("V,P", TW.COLOR_CASES)
def test_color_from_features(dev, ops, color_blobs, V, P, x3):
    """the colour network on materialised tensors against float64; the count of valid views is exact"""
    c = TW.color_case(V, P)
    rgb, nv = ops.color_from_features(color_blobs[x3], c["geo"].to(dev), c["rf"].to(dev), c["rd"].to(dev), c["mask"].float().to(dev), x3=x3)
    assert torch.equal(nv.cpu().double(), c["nviews"].double())
    check(rgb, c["r64"], TW.color_bound(c["r32"], c["r64"], x3), f"colour V={V} P={P} {'f16x3' if x3 else 'fp32'}")


@pytest.mark.parametrize("kernel", ["pts", "tiles"])
@pytest.mark.parametrize("x3", [True, False])
@pytest.mark.parametrize("V", [5, 8])
def test_color_points_equals_the_network_on_projected_features(dev, ops, color_blobs, lib_instance, V, x3, kernel):
    """the fused projector + network kernel (and the test-only tiles kernel) on a small scene against the network kernel on the tensors
    ops.project_features materialises for the same points, at the suite's 2e-5; the projection itself has its own unit tests"""
    if kernel == "tiles":
        assert b"color_tiles=1" in lib_instance({"O2345_COLOR_KERNEL": "tiles"}, variant="tiles").o2345_knobs()
    s = small_scene(V=V, HW=40, D=16)
    sc = s["sc"]
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dev)
    vol_cl = s["dense"][0].permute(1, 2, 3, 0).contiguous().to(dev)
    maskvol = s["mask"][0, 0].contiguous().to(dev)
    Kt, w2c = torch.from_numpy(sc["intrinsics"]), torch.from_numpy(sc["w2cs"])
    proj = (Kt @ w2c[:, :3, :]).contiguous().to(dev)
    cam_pos = torch.inverse(w2c)[:, :3, 3].contiguous().to(dev)
    cmaps = ops.pack_color_maps(t(s["fmaps"]).contiguous(), t(sc["images"]).contiguous())
    qcam = torch.from_numpy(sc["query_c2w"][:3, 3].copy()).to(dev)
    pts = torch.from_numpy(np.random.default_rng(V).uniform(-0.9, 0.9, (321, 3)).astype(np.float32))
    pts[:5] = torch.tensor([1.5, 0.0, 0.0])                                          # no view, no latent
    pts = pts.to(dev)
    fused, nv = ops.color_points(color_blobs[x3], vol_cl, maskvol, cmaps, proj, cam_pos, pts, query_cam=qcam, mfma="x3" if x3 else True)
    geo, rf, rd, m = ops.project_features(vol_cl, maskvol, cmaps, proj, cam_pos, pts, query_cam=qcam)
    rgb, nv2 = ops.color_from_features(color_blobs[x3], geo, rf, rd, m, x3=x3)
    assert torch.equal(nv, nv2) and int(nv.max()) >= 2 and int(nv[:5].max()) == 0
    err = float((fused - rgb).abs().max())
    bound = 2e-5 * max(1.0, float(rgb.abs().max()))
    print(f"colour points V={V} {'f16x3' if x3 else 'fp32'} {kernel}: fused against materialised {err:.2e}, bound {bound:.2e}")
    assert bool(torch.isfinite(fused).all()) and err <= bound
