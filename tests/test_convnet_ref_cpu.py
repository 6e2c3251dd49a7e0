"""tests/convnet_ref.py checked on the CPU: the references against each other and against definitions written out as loops, what the seeded families
reach (every fp32 tier against the thresholds read from csrc/convnet.hip, the partial-block count of the strided statistics loop, ragged tiles, both
input parities of the stride-2 layers, a mean that dominates the variance, subnormal lo halves), the domain of the split-f16 form as a table that is
printed and asserted, and a sensitivity gate: the indexing mistakes a convolution kernel can make move the float64 output by at least ten times the
bound the GPU tests (tests/test_gpu_convnet_units.py) hold the kernels to.  No GPU, no product package."""
import math
import pathlib
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnet_ref as C

SRC = (pathlib.Path(__file__).resolve().parents[1] / "one-2-3-45_amd" / "csrc" / "convnet.hip").read_text()
ids = lambda s: "-".join(map(str, s))


def conv_args(c):
    return c["x"], c["w"], c["bias"], c["stride"], c["in_ss"], C.SLOPE


# ------------------------------------------------------------------------------------------------ the references against each other
def direct_conv(x, w, bias, stride, in_ss, slope):
    """The definition, pixel by pixel in float64: out[v, o, y, x] = bias[o] + sum over (c, i, j) of w[o, c, i, j] * act(in)[v, c, s y + i - p, s x + j - p],
    where act(in) is 0 outside the image."""
    a = C.act_input(x, in_ss, slope, C.F64)
    cout, cin, k, _ = w.shape
    V, _, Hi, Wi = a.shape
    Ho, Wo = C.out_size(Hi, Wi, k, stride)
    p = k // 2
    ap = torch.zeros(V, cin, Hi + 2 * p, Wi + 2 * p, dtype=C.F64)
    ap[:, :, p:p + Hi, p:p + Wi] = a
    out = torch.zeros(V, cout, Ho, Wo, dtype=C.F64)
    for y in range(Ho):
        for xx in range(Wo):
            out[:, :, y, xx] = torch.einsum("vcij,ocij->vo", ap[:, :, stride * y:stride * y + k, stride * xx:stride * xx + k], w.double())
    return out if bias is None else out + bias.double().view(1, -1, 1, 1)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("fam", ["pixel", "tile"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_conv_ref_is_the_direct_sum(shape, fam, fused):
    c = C.case(shape, fam, fused)
    want = direct_conv(*conv_args(c))
    assert want.shape == c["ref64"].shape
    assert (want - c["ref64"]).abs().max().item() <= 1e-13 * max(1.0, c["mag"])


@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_the_loop_yardstick_and_atens_float32_convolution(shape):
    """Both are float32 evaluations of the same sums: within 8 x of each other (the loop is the plainer, and here never the better, of the two)."""
    for fused in (False, True):
        c = C.case(shape, "ragged", fused)
        e_aten = C._err(C.conv_ref(*conv_args(c), dtype=C.F32), c["ref64"])
        print(f"{shape} fused {fused}: loop {c['e_ref']:.2e} ({c['e_ref'] / c['mag']:.2e} of the magnitude), ATen float32 {e_aten:.2e}, ratio {c['e_ref'] / e_aten:.2f}")
        assert e_aten / 8 <= c["e_ref"] <= 8 * e_aten and c["e_ref"] > 0


def test_the_split_model_is_exact_on_powers_of_two():
    """hi holds a power of two exactly and lo is 0, products and sums of a few dyadic numbers are exact in float64."""
    g = C._rng("pow2")
    for cin, cout, k, stride in ((3, 8, 3, 1), (16, 32, 5, 2), (32, 32, 1, 1)):
        x = C._t(np.ldexp(g.choice([-1.0, 1.0], (2, cin, 9, 11)), g.integers(-3, 4, (2, cin, 9, 11))))
        w = C._t(np.ldexp(g.choice([-1.0, 1.0], (cout, cin, k, k)), g.integers(-6, 1, (cout, cin, k, k))))
        b = C._t(np.ldexp(1.0, g.integers(-2, 2, cout)))
        assert torch.equal(C.conv_split_model(x, w, b, stride), C.conv_ref(x, w, b, stride))
        assert torch.equal(C.conv_ref32_loop(x, w, b, stride).double(), C.conv_ref(x, w, b, stride))


def test_the_split_model_drops_what_the_form_drops():
    """One value with 24 significant bits times a weight of 1: hi = 1, lo = f16(2^-11 + 2^-23) toward zero = 2^-11 -- hi + lo keeps 22 bits."""
    x = torch.tensor([[[[1.0 + 2.0 ** -11 + 2.0 ** -23]]]])
    w = torch.ones(1, 1, 1, 1)
    got = C.conv_split_model(x, w).item()
    assert got <= x.item() and 0 < x.item() - got <= 2.0 ** -21


@pytest.mark.parametrize("shape", C.SHAPES + C.ODD_COUNTS, ids=ids)
def test_packings(shape):
    cin, cout, k, _ = shape
    w = C._rng("pack", *shape).normal(0, 0.1, (cout, cin, k, k)).astype(np.float32)
    fp = C.pack_fp32(w)
    x3 = C.pack_x3(w)
    nu = (cin + 15) // 16
    assert fp.shape == (cin * k * k * cout,) and x3.shape == (k * k, nu, 2, 64, 8) and x3.dtype == np.float16
    for ci in range(cin):
        for t in range(k * k):
            assert np.array_equal(fp[(ci * k * k + t) * cout:(ci * k * k + t + 1) * cout], w[:, ci, t // k, t % k])
    for tap in range(k * k):
        for u in range(nu):
            for lane in range(64):
                for t in range(8):
                    co, ci = lane & 31, 16 * u + 8 * (lane >> 5) + t
                    v = w[co, ci, tap // k, tap % k] if co < cout and ci < cin else np.float32(0)
                    hi = np.float16(v)
                    assert x3[tap, u, 0, lane, t] == hi and x3[tap, u, 1, lane, t] == np.float16(v - np.float32(hi))


def test_abn_against_batch_norm():
    c = C.case((16, 32, 5, 2), "ragged", True)
    for abs_gamma in (True, False):
        ss = C.abn_stats(c["ref64"], c["gamma"], c["beta"], C.EPS, abs_gamma)
        g = c["gamma"].double().abs() + C.EPS if abs_gamma else c["gamma"].double()
        want = F.leaky_relu(F.batch_norm(c["ref64"], None, None, g, c["beta"].double(), True, 0.0, C.EPS), C.SLOPE)
        assert (C.abn_act(c["ref64"], ss) - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    ss32 = C.abn_stats(c["ref64"].float(), c["gamma"], c["beta"])
    assert ss32.dtype == torch.float32 and C.abn_act(c["ref64"].float(), ss32).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ what the families reach
def kernel_table():
    """The rows of o2345_conv2d's dispatch: (cin, cout, k, stride) -> (CC, PX4, B4, B2, B1)."""
    rows = re.findall(r"^\s*O2345_CONV\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", SRC, re.M)
    return {tuple(map(int, r[:4])): tuple(map(int, r[4:])) for r in rows}


def tier_of(pixels):
    hi, lo = map(int, re.search(r"const int tier = pix >= (\d+) \? 2 : pix >= (\d+) \? 1 : 0;", SRC).groups())
    return 2 if pixels >= hi else 1 if pixels >= lo else 0


def test_the_families_reach_every_tier_of_the_fp32_dispatch():
    m = re.search(r"const int tier = pix >= (\d+) \? 2 : pix >= (\d+) \? 1 : 0;", SRC)
    assert m and tuple(map(int, m.groups())) == (400000, 100000), "the tier thresholds of o2345_conv2d changed: the map families were sized for 100,000 and 400,000"
    assert re.search(r"const long long pix = \(long long\)V \* a\.Ho \* a\.Wo;", SRC)
    pixels = {f: v * h * w for f, (v, h, w) in C.MAPS.items()}
    assert [tier_of(pixels[f]) for f in ("pixel", "tile", "ragged", "blocks", "tier1", "tier2")] == [0, 0, 0, 0, 1, 2]
    assert pixels["blocks"] == 97500 and pixels["tier1"] == 100162 and pixels["tier2"] == 400282
    table = kernel_table()
    assert set(table) == set(C.SHAPES) and len(table) == 11
    # tier 2 of the 5 x 5 layers launches two pixels per thread, the arguments of tier 1: left out of tier2
    assert {s for s, r in table.items() if r[1] == 4} == set(C.tier2_shapes()) and all(r[1] == 2 and r[2] == r[3] for s, r in table.items() if s[3] == 2)
    # more than one channel group per tile (conv_part_write at a non-zero c0) in every tier
    for col in (2, 3):                                        # tiers 2 and 1: 16 of 32 output channels per blockIdx.z
        assert {s for s, r in table.items() if s[1] // r[col] == 2} == {(16, 32, 5, 2), (32, 32, 3, 1), (32, 32, 1, 1)}
    assert all(s[1] // r[4] == s[1] // 8 for s, r in table.items())       # tier 0: 8 per blockIdx.z, up to four groups


def test_tile_sizes_and_ragged_edges():
    tx, th = map(int, re.search(r"constexpr int CV_TX = (\d+), CV_TH = (\d+);", SRC).groups())
    assert (tx, th) == (32, 8)
    assert re.search(r"launch_conv_x3<16, 5, 2, 1>", SRC) and len(re.findall(r"launch_conv_x3<\d+, [13], 1, 2(?:, true)?>\(a", SRC)) == 4    # x3 tiles: 32 x 4 ROWS
    V, Ho, Wo = C.MAPS["tile"]
    assert (Ho, Wo) == (th, tx)
    for fam in ("ragged", "tier1", "tier2"):
        V, Ho, Wo = C.MAPS[fam]
        assert all(Wo % wd for wd in (32, 64, 128)) and all(Ho % h for h in (4, 8)), fam
    V, Ho, Wo = C.MAPS["ragged"]
    assert (Ho - th, Wo - tx) == (1, 3) and V == 5
    # the partial blocks per channel that k_conv_stats_finish sums in a strided loop of 256 threads
    V, Ho, Wo = C.MAPS["blocks"]
    for tile_w, tile_h in ((tx, th), (32, 8), (32, 4)):
        nblk = math.ceil(Wo / tile_w) * math.ceil(Ho / tile_h) * V
        assert nblk > 256 and nblk % 256
    assert math.ceil(Wo / tx) * math.ceil(Ho / th) * V == 432


def test_both_input_parities_of_the_stride_2_layers():
    for fam in C.MAPS:
        sizes = [C.in_size(s, fam) for s in C.SHAPES if s[3] == 2]
        assert {h % 2 for _, h, _ in sizes} == {0, 1} and {w % 2 for _, _, w in sizes} == {0, 1}
        for s in C.SHAPES:
            V, Hi, Wi = C.in_size(s, fam)
            assert (V,) + C.out_size(Hi, Wi, s[2], s[3]) == C.MAPS[fam]


def test_white_has_a_mean_that_dominates_the_variance():
    c = C.case((3, 8, 3, 1), "ragged", True, "white")
    x = c["x"]
    assert (x == 1.0).float().mean().item() > 0.6 and ((x >= 0) & (x < 1)).float().mean().item() > 0.15 and x.max().item() == 1.0
    m, v = c["ref64"].mean((0, 2, 3)), c["ref64"].var((0, 2, 3), unbiased=False)
    print("white: mean^2 / var per channel", [round(r, 2) for r in (m * m / v).tolist()])
    assert (m * m / v > 3).all() and (m > 0).any() and (m < 0).any()


def test_signs_and_dead_channel():
    for shape in C.SHAPES:
        c = C.case(shape, "ragged", True)
        s = c["in_ss"][:shape[0]]
        assert (s > 0).any() and (s < 0).any() and (c["gamma"] > 0).any() and (c["gamma"] < 0).any()
        d = C.case(shape, "ragged", True, "deadchannel")
        dead = shape[1] // 2
        assert (d["ref64"][:, dead] == 0).all() and all((d["ref64"][:, o] != 0).any() for o in range(shape[1]) if o != dead)
        assert torch.equal(d["act64"][:, dead], C.leaky(d["beta"].double(), C.SLOPE)[dead].expand_as(d["act64"][:, dead]))


def test_lo_halves_are_subnormal_from_2_to_the_minus_3_on():
    tiny = 2.0 ** -14                                        # the smallest normal float16
    for shape in C.SCALE_SHAPES:
        for e in C.WSCALE_E:
            lo = np.abs(C.split_weights(C.case(shape, "ragged", True, "wscale", e)["w"].numpy())[1])
            assert ((lo > 0) & (lo < tiny)).any()
        for e, want in zip(C.XSCALE_E, (True, False)):
            c = C.case(shape, "ragged", True, "xscale", e)
            a = C.act_input(c["x"], c["in_ss"], C.SLOPE, C.F32).numpy()
            lo = np.abs(C.split_activations(a)[1])
            assert (((lo > 0) & (lo < tiny)).mean() > 0.5) == want
            if e > 0:
                assert 32 <= np.abs(a).max() < 65504


# ------------------------------------------------------------------------------------------------ the domain of the split-f16 form
CEILING = 2e-5                                                # of max(1, magnitude): the tolerance tests/test_gpu_parity.py has for a conv + ABN


def in_domain(c):
    return C.bound(c, True, "_act") <= CEILING * max(1.0, c["mag_act"])


@pytest.mark.parametrize("shape", C.SCALE_SHAPES, ids=ids)
def test_the_domain_of_the_split_form(shape):
    """The form's error relative to the output grows as the weights shrink: lo = f16(w - hi) is a subnormal below |w| of about 2^-4, its absolute error
    stops shrinking with w, and the batch norm that follows divides the output by its standard deviation.  In the domain (the activated layer output's
    bound stays under the parity tolerance of a conv + ABN): weights at N(0, 1) / sqrt(fan-in) times 1 and times 2^-3, and activations times 2^-6 and
    2^6.  Outside: weights times 2^-6 and 2^-9.  Per step of 2^-3 the relative error of the raw output grows 4 to 16 times wherever the larger scale is
    inside the regime already -- from 2^-3 down on every shape, and from 1 down where most weights have a subnormal lo at scale 1, i.e. where their
    standard deviation 1 / sqrt(cin k^2) is below 2^-4; on the two shapes above that ((3, 8, 3, 1) and (32, 32, 1, 1)) the first step only has to grow."""
    cin, cout, k, stride = shape
    rel = {}
    print(f"{shape}: kind e | raw: e_ref e_split magnitude | activated: e_ref e_split bound ceiling")
    for kind, e in [("normal", 0)] + [("wscale", e) for e in C.WSCALE_E] + [("xscale", e) for e in C.XSCALE_E]:
        c = C.case(shape, "ragged", True, kind, e)
        print(f"  {kind:7s} {e:3d} | {c['e_ref']:.2e} {c['e_split']:.2e} {c['mag']:.2e} ({c['e_split'] / c['mag']:.2e}) | {c['e_ref_act']:.2e} {c['e_split_act']:.2e} "
              f"{C.bound(c, True, '_act'):.2e} {CEILING * max(1.0, c['mag_act']):.2e} {'in' if in_domain(c) else 'OUT'}")
        assert in_domain(c) == ((kind, e) in (("normal", 0), ("wscale", -3), ("xscale", -6), ("xscale", 6))), (kind, e)
        if kind != "xscale":
            rel[e] = c["e_split"] / c["mag"]
        assert c["e_ref"] / c["mag"] < 2e-6                   # the float32 loop does not care about the scale
    for hi, lo in ((-3, -6), (-6, -9)):
        assert 4 <= rel[lo] / rel[hi] <= 16, (hi, lo, rel)
    first = rel[-3] / rel[0]
    assert (4 if 1 / math.sqrt(cin * k * k) < 2.0 ** -4 else 1) < first <= 16, rel


# ------------------------------------------------------------------------------------------------ the sensitivity gate
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_indexing_mistakes_move_the_output_by_ten_bounds(shape):
    """On the `normal` case at `ragged`, against the LOOSER of the two bounds (the x3 kernels')."""
    cin, cout, k, stride = shape
    c = C.case(shape, "ragged", True)
    x, w, bias, stride, in_ss, slope = conv_args(c)
    b = C.bound(c, True)
    assert b >= C.bound(c, False)
    ss = in_ss.view(2, cin)
    moved = {"in_ss of channel c + 1": C.conv_ref(x, w, bias, stride, ss.roll(-1, 1).reshape(-1), slope),
             "in_ss of channel c - 1": C.conv_ref(x, w, bias, stride, ss.roll(1, 1).reshape(-1), slope),
             "last input channel dropped": C.conv_ref(x[:, :-1], w[:, :-1], bias, stride, ss[:, :-1].reshape(-1), slope)}
    for ky, kx in {(0, 0), (k // 2, k // 2), (k - 1, k - 1)}:
        w1 = w.clone()
        w1[:, :, ky, kx] = 0
        moved[f"tap ({ky}, {kx}) dropped"] = C.conv_ref(x, w1, bias, stride, in_ss, slope)
    if k > 1:                                                 # a 1 x 1 layer has neither a second axis nor padding
        moved["ky and kx swapped"] = C.conv_ref(x, w.transpose(2, 3), bias, stride, in_ss, slope)
        p = k // 2
        moved["padding before the activation"] = F.conv2d(C.act_input(F.pad(x, (p, p, p, p)), in_ss, slope, C.F64), w.double(), None, stride, 0)
    for what, out in moved.items():
        d = (out - c["ref64"]).abs().max().item()
        print(f"{shape} {what}: moves the output by {d:.2e} = {d / b:.0f} bounds")
        assert d >= 10 * b, what


# ------------------------------------------------------------------------------------------------ the cropped yardstick of the large maps
@pytest.mark.parametrize("shape", [(3, 8, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1), (56, 16, 3, 1)], ids=ids)
def test_the_cropped_yardstick_is_representative(shape):
    """tier1 and tier2 take e_ref on the first CROP_ROWS output rows of view 0; at `blocks`, where both are affordable, that is within 2 x of the whole map's."""
    c = C.case(shape, "blocks", True)
    crop = C.conv_ref32_loop(*conv_args(c), rows=C.CROP_ROWS)
    assert tuple(crop.shape) == (1, shape[1], C.CROP_ROWS, C.MAPS["blocks"][2])
    e_crop = C._err(crop, c["ref64"][:1, :, :C.CROP_ROWS])
    print(f"{shape} blocks: e_ref of the whole map {c['e_ref']:.2e}, of the crop {e_crop:.2e} ({e_crop / c['e_ref']:.2f})")
    assert c["e_ref"] / 2 <= e_crop <= c["e_ref"]
    full = C.conv_ref32_loop(*conv_args(c))
    assert torch.equal(full[:1, :, :C.CROP_ROWS], crop)


def test_x3_dispatch_matches_the_source():
    """x3_dispatch restates o2345_conv2d_x3's branch list; every branch of the source is one of its five."""
    got = {(int(k), int(s), int(ci)) for k, s, ci in re.findall(r"if \(k == (\d) && stride == (\d) && cinp == (\d+)\) launch_conv_x3<", SRC)}
    assert got == {(3, 1, 16), (3, 1, 32), (3, 1, 64), (5, 2, 16), (1, 1, 32)}
    assert all(C.x3_dispatch(*s) is not None for s in C.SHAPES)
    assert [C.x3_dispatch(*s) is not None for s in C.ODD_COUNTS] == [True, True, True, True, True, False]
