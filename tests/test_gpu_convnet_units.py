"""The feature network's convolution units one by one: ops.conv2d in both numerical forms (csrc/convnet.hip: k_conv2d in every tier of its dispatch,
k_conv2d_x3, k_conv2d_x3_staged in both arms, the fused batch statistics and k_conv_stats_finish), ops.conv2d_pack (k_conv_pack, k_conv_pack_x3),
ops.scale_shift_act and ops.abn_nchw, each entry alone, against the references of tests/convnet_ref.py (checked on the CPU by
tests/test_convnet_ref_cpu.py, which also asserts what the seeded families reach).

Float results are compared with float64 under rule E with NO floor of 1 under the magnitude: max |gpu - ref64| <= 4 e + 4 ulp of
the output's magnitude, where e is, for the fp32 kernels, e_ref = max |float32 loop - ref64| of the same case and, for the matrix-core kernels,
max(e_ref, e_split), e_split = max |split model - ref64| (the error the split-f16 form has by construction).  The same two yardsticks pushed through
abn_stats / abn_act bound the (scale | shift) pair and the activated layer output.  Every float comparison prints e_ref, e_split, the device error and
its share of the bound.  Packings, channel-last against channel-first input, a second call, the dead channel and NHWC against NCHW are bit for bit.
Outputs the test hands to the C entries are filled with NaN beforehand: every element is written.

Maps (output sizes): pixel 1 x 1 x 1, tile 2 x 8 x 32, ragged 5 x 9 x 35, blocks 3 x 65 x 500 (tier 0, 432 partial blocks per channel), tier1
2 x 61 x 821 and tier2 2 x 61 x 3281 (two and four pixels per thread; fp32 form only, yardsticks on 16 rows of view 0).

Measured on the MI355X (yardsticks computed on the CPU; DESIGN.md section 4, "Feature network units: what pins what"), as share of the bound: fp32
kernels on the small maps raw 0.07 ... 0.24, (scale | shift) 0.02 ... 0.16, activated 0.12 ... 0.24; tier 1 raw up to 0.32, tier 2 up to 0.38
(32 -> 8); matrix-core kernels raw 0.10 ... 0.27, (scale | shift) up to 0.22, activated up to 0.26; with the weights at 2^-3 and below the
matrix-core kernels' error equals the split model's to two digits (share 0.25); channel-last 0.12 ... 0.24; odd channel counts 0.09 ... 0.25;
scale_shift_act and abn_nchw 0.06 ... 0.25.  Every case passed at first run; no kernel was changed."""
import importlib

import numpy as np
import pytest
import torch

import convnet_ref as C

pytestmark = pytest.mark.gpu
NAN = float("nan")
ids = lambda s: "-".join(map(str, s)) if isinstance(s, tuple) else str(s)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


def rule_e(got, ref64, c, x3, what, part=""):
    """Rule E of a case's raw output (part ""), its (scale | shift) ("_ss") or its activated output ("_act")."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite values (an element that was never written is NaN)"
    b, y = C.bound(c, x3, part), C.yard(c, x3, part)
    err = (got - ref64).abs().max().item()
    es = c["e_split" + part]
    print(f"{what} [{'x3' if x3 else 'fp32'}] {part or '_raw'}: e_ref {c['e_ref' + part]:.2e}, e_split {'-' if es is None else format(es, '.2e')}, "
          f"device err {err:.2e}, bound {b:.2e} ({err / b:.2f}), magnitude {c['mag' + part]:.2e}")
    assert err <= b, f"{what}{part}: device err {err:.3e} > 4 * {y:.3e} + 4 ulp of {c['mag' + part]:.3g} = {b:.3e}"


def run_conv(ops, dev, c, prec, nhwc=None):
    """o2345_conv2d / o2345_conv2d_x3 through the C entry on NaN-filled outputs -> (raw output, scale | shift or None).  nhwc = (map, channel offset)."""
    w = c["w"].to(dev)
    cout, cin, k, _ = w.shape
    if nhwc is None:
        x, pix, c0 = c["x"].to(dev), 0, 0
        V, _, Hi, Wi = x.shape
    else:
        x, pix, c0 = nhwc[0], nhwc[0].shape[3], nhwc[1]
        V, Hi, Wi, _ = x.shape
    Ho, Wo = C.out_size(Hi, Wi, k, c["stride"])
    out = torch.full((V, cout, Ho, Wo), NAN, dtype=torch.float32, device=dev)
    bn = c["bn"]
    ss = gamma = beta = ws = None
    nbytes = 0
    if bn:
        ss = torch.full((2 * cout,), NAN, dtype=torch.float32, device=dev)
        gamma, beta = c["gamma"].to(dev), c["beta"].to(dev)
        nbytes = ops.call("o2345_conv2d_workspace_bytes", V, cout, Ho, Wo)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    ops.call("o2345_conv2d_x3" if prec == "f16x3" else "o2345_conv2d", x, V, cin, Hi, Wi, pix, c0, None if c["in_ss"] is None else c["in_ss"].to(dev), C.SLOPE,
             ops.conv2d_pack(w, prec), None if c["bias"] is None else c["bias"].to(dev), cout, k, c["stride"], out, gamma, beta, C.EPS if bn else 0.0, 1, ss,
             ws, nbytes)
    return out, ss


PLAIN = [(s, f, p) for s in C.SHAPES for f in C.SMALL_MAPS for p in ("fp32", "f16x3")] + [(s, "tier1", "fp32") for s in C.SHAPES] + \
        [(s, "tier2", "fp32") for s in C.tier2_shapes()]
FUSED = [t for t in PLAIN if t[1] != "pixel"]


# ------------------------------------------------------------------------------------------------ 1. plain: bias, no in_ss, no batch norm
@pytest.mark.parametrize("shape,fam,prec", PLAIN, ids=ids)
def test_conv2d_plain(dev, ops, shape, fam, prec):
    c = C.case(shape, fam, False)
    y, ss = run_conv(ops, dev, c, prec)
    assert ss is None
    rule_e(y, c["ref64"], c, prec == "f16x3", f"{shape} {fam} plain")
    y2, _ = ops.conv2d(c["x"].to(dev), c["w"].to(dev), c["bias"].to(dev), c["stride"], precision=prec)
    assert torch.equal(y, y2), "ops.conv2d differs from the C entry on the same arguments"


# ------------------------------------------------------------------------------------------------ 2. fused: in_ss, batch statistics
def check_fused(ops, dev, c, prec, what, note=""):
    x3 = prec == "f16x3"
    cout = c["w"].shape[0]
    y, ss = run_conv(ops, dev, c, prec)
    rule_e(y, c["ref64"], c, x3, what + note)
    assert c["ref64"].numel() // cout >= C.STATS_FLOOR
    rule_e(ss, c["ss64"], c, x3, what + note, "_ss")
    act, nhwc = ops.scale_shift_act(y, ss, C.SLOPE, want_nchw=True, want_nhwc=True)
    rule_e(act, c["act64"], c, x3, what + note, "_act")
    assert torch.equal(nhwc, act.permute(0, 2, 3, 1))
    y2, ss2 = run_conv(ops, dev, c, prec)
    assert torch.equal(y, y2) and torch.equal(ss, ss2), f"{what}: a second call differs (the statistics are reduced in a fixed order)"
    return y, ss, act


@pytest.mark.parametrize("shape,fam,prec", FUSED, ids=ids)
def test_conv2d_fused(dev, ops, shape, fam, prec):
    check_fused(ops, dev, C.case(shape, fam, True), prec, f"{shape} {fam} fused")


# ------------------------------------------------------------------------------------------------ 3. white, dead channel, operand scales
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_white_background(dev, ops, prec):
    check_fused(ops, dev, C.case((3, 8, 3, 1), "ragged", True, "white"), prec, "white (3, 8, 3, 1) ragged")


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=ids)
def test_dead_channel(dev, ops, shape, prec):
    """An output channel whose weights are all zero: raw output exactly 0, variance 0, activated output exactly leaky(beta)."""
    c = C.case(shape, "ragged", True, "deadchannel")
    y, ss, act = check_fused(ops, dev, c, prec, f"dead channel {shape} ragged")
    dead = shape[1] // 2
    assert bool((y[:, dead] == 0).all())
    want = torch.where(c["beta"] >= 0, c["beta"], c["beta"] * C.SLOPE)[dead]
    assert ss[shape[1] + dead].item() == c["beta"][dead].item()
    assert torch.equal(act[:, dead].cpu(), want.expand_as(act[:, dead])), "leaky(beta), bit for bit"


SCALED = [(s, k, e) for s in C.SCALE_SHAPES for k, es in (("wscale", C.WSCALE_E), ("xscale", C.XSCALE_E)) for e in es]


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("shape,kind,e", SCALED, ids=ids)
def test_operand_scales(dev, ops, shape, kind, e, prec):
    """Weights times 2^e and activations times 2^e: the matrix-core kernels follow the split model wherever it goes.  At weights times 2^-6 and 2^-9 the
    model -- and with it the bound -- is outside the form's documented domain: LOOSE in absolute terms, 1e-4 to 1e-3 of an
    activated output of magnitude 1 to 5; what the comparison checks there is that the kernel IS the form (a kernel that flushed subnormal lo halves
    would err by about 5e-4 of the magnitude already at 2^-3, where the model's error is 2e-6 of it)."""
    c = C.case(shape, "ragged", True, kind, e)
    loose = prec == "f16x3" and C.bound(c, True, "_act") > 2e-5 * max(1.0, c["mag_act"])
    check_fused(ops, dev, c, prec, f"{kind}({e}) {shape} ragged", " -- OUTSIDE the split form's domain, the bound is loose" if loose else "")


# ------------------------------------------------------------------------------------------------ 4. channel-last input
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("fam", ["ragged", "blocks"])
@pytest.mark.parametrize("cin,cout,pix_stride,offset", C.CHANNEL_LAST)
def test_channel_last_input(dev, ops, cin, cout, pix_stride, offset, fam, fused, prec):
    """The compress layer's addressing (56 channels from channel 3 of a 64-channel map: the staged matrix-core kernel's channel-last arm) and a
    32-channel layer inside maps of 64 and of 40 channels: rule E, and the same bits as from the channel-first copy."""
    c = C.case((cin, cout, 3, 1), fam, fused)
    cm = C.channel_last_map(c, pix_stride, offset).to(dev)
    y0, ss0 = run_conv(ops, dev, c, prec)
    y1, ss1 = run_conv(ops, dev, c, prec, nhwc=(cm, offset))
    rule_e(y1, c["ref64"], c, prec == "f16x3", f"{cin}->{cout} {fam} channel-last ({pix_stride}, {offset}) fused {fused}")
    assert torch.equal(y0, y1) and (ss0 is None) == (ss1 is None) and (ss0 is None or torch.equal(ss0, ss1))
    if fused:
        rule_e(ss1, c["ss64"], c, prec == "f16x3", f"{cin}->{cout} {fam} channel-last", "_ss")


# ------------------------------------------------------------------------------------------------ 5. channel counts only the entry accepts
@pytest.mark.parametrize("fam", ["ragged", "tile"])
@pytest.mark.parametrize("shape", C.ODD_COUNTS, ids=ids)
def test_x3_channel_counts_the_product_never_passes(dev, ops, shape, fam):
    """o2345_conv2d_x3 pads cin to 16, 32 or 64 and takes any cout <= 32: either the right answer (zeros beyond cin and cout staged, read and written
    nowhere) or its own "no kernel for" error -- never a wrong answer."""
    c = C.odd_case(shape, fam)
    if C.x3_dispatch(*shape) is None:
        with pytest.raises(RuntimeError, match="no kernel for"):
            run_conv(ops, dev, c, "f16x3")
        return
    y, ss = run_conv(ops, dev, c, "f16x3")
    rule_e(y, c["ref64"], c, True, f"{shape} {fam} odd counts")
    rule_e(ss, c["ss64"], c, True, f"{shape} {fam} odd counts", "_ss")


# ------------------------------------------------------------------------------------------------ 6. the packers
@pytest.mark.parametrize("shape", C.SHAPES + C.ODD_COUNTS, ids=ids)
def test_packers(dev, ops, shape):
    cin, cout, k, _ = shape
    w = C._t(C._rng("pack", *shape).normal(0, 0.1, (cout, cin, k, k)))
    fp = ops.conv2d_pack(w.to(dev), "fp32").cpu().numpy()
    assert fp.tobytes() == C.pack_fp32(w.numpy()).tobytes()
    x3 = ops.conv2d_pack(w.to(dev), "f16x3").cpu().numpy()
    want = C.pack_x3(w.numpy())
    assert x3.dtype == np.float32 and x3.size * 2 == want.size and x3.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ 7. ops.abn_nchw, ops.scale_shift_act
def run_act(ops, dev, entry, c, want, abs_gamma=True):
    """o2345_scale_shift_act (on the case's float32 scale | shift) or o2345_abn_nchw through the C entry on NaN-filled outputs -> (NCHW, NHWC)."""
    x = c["x"].to(dev)
    V, Cn, H, W = x.shape
    y1 = torch.full((V, Cn, H, W), NAN, dtype=torch.float32, device=dev) if want[0] else None
    y2 = torch.full((V, H, W, Cn), NAN, dtype=torch.float32, device=dev) if want[1] else None
    if entry == "scale_shift_act":
        ops.call("o2345_scale_shift_act", x, V, Cn, H, W, c["ss32"].to(dev), C.SLOPE, y1, y2)
    else:
        nbytes = ops.call("o2345_abn_workspace_bytes", Cn)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        ops.call("o2345_abn_nchw", x, V, Cn, H, W, c["gamma"].to(dev), c["beta"].to(dev), C.EPS, C.SLOPE, int(abs_gamma), y1, y2, ws, nbytes)
    for y in (y1, y2):
        assert y is None or not bool(torch.isnan(y).any()), "an element was not written"
    return y1, y2


def check_layouts(ops, dev, entry, c, abs_gamma=True):
    """Every legal (want_nchw, want_nhwc): the same values whichever outputs are asked for, NHWC = NCHW permuted, bit for bit -> the NCHW output."""
    a1, a2 = run_act(ops, dev, entry, c, (True, True), abs_gamma)
    assert torch.equal(a2, a1.permute(0, 2, 3, 1))
    assert torch.equal(run_act(ops, dev, entry, c, (True, False), abs_gamma)[0], a1)
    assert torch.equal(run_act(ops, dev, entry, c, (False, True), abs_gamma)[1], a2)
    return a1


@pytest.mark.parametrize("V", C.ABN_V)
@pytest.mark.parametrize("hw", C.ABN_HW)
@pytest.mark.parametrize("Cn", C.ABN_C)
def test_scale_shift_act_and_abn_layouts(dev, ops, Cn, hw, V):
    c = C.abn_case(Cn, V, *C.ABN_HW[hw])
    x64, ss = c["x"].double(), c["ss32"]
    want = C.abn_act(x64, ss.double())                                      # the given float32 pair, applied in float64
    k = dict(e_ref_act=C._err(C.abn_act(c["x"], ss), want), e_split_act=None, mag_act=C._mag(want))
    rule_e(check_layouts(ops, dev, "scale_shift_act", c), want, k, False, f"scale_shift_act C {Cn} V {V} HW {hw}", "_act")
    ops_y1, ops_y2 = ops.scale_shift_act(c["x"].to(dev), ss.to(dev), C.SLOPE, want_nchw=True, want_nhwc=True)
    assert torch.equal(ops_y2, ops_y1.permute(0, 2, 3, 1))
    for abs_gamma in (True, False):
        ca = C.abn_case(Cn, V, *C.ABN_HW[hw], abs_gamma)
        y = check_layouts(ops, dev, "abn_nchw", ca, abs_gamma)
        if V * hw >= C.STATS_FLOOR:
            rule_e(y, ca["act64"], ca, False, f"abn_nchw C {Cn} V {V} HW {hw} abs_gamma {abs_gamma}", "_act")


@pytest.mark.parametrize("abs_gamma", [True, False])
@pytest.mark.parametrize("Cn", C.ABN_C)
def test_abn_nchw_on_the_ragged_map(dev, ops, Cn, abs_gamma):
    V, H, W = C.MAPS["ragged"]
    c = C.abn_case(Cn, V, H, W, abs_gamma)
    assert (c["gamma"] > 0).any() and (c["gamma"] < 0).any()
    y = check_layouts(ops, dev, "abn_nchw", c, abs_gamma)
    rule_e(y, c["act64"], c, False, f"abn_nchw C {Cn} ragged abs_gamma {abs_gamma}", "_act")
    y1, y2 = ops.abn_nchw(c["x"].to(dev), c["gamma"].to(dev), c["beta"].to(dev), C.EPS, C.SLOPE, abs_gamma, want_nhwc=True)
    assert torch.equal(y1, y) and torch.equal(y2, y.permute(0, 2, 3, 1))
