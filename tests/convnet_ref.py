"""Plain references of the feature network's 2-D convolution units (csrc/convnet.hip, and the channel-first InPlaceABN of csrc/sparse.hip), and the
seeded cases their tests share -- TEST INFRASTRUCTURE ONLY.

torch and numpy on the CPU; the product package is not imported here and nothing is derived from a kernel's output.  Every reference is written from
the DEFINITION of its operation: a layer is nn.Conv2d with padding k // 2 of leaky(x * scale + shift) -- the producer's InPlaceABN, applied BEFORE the
zero padding; its batch statistics turn into (scale | shift) as abn_scale_shift of csrc/block_kernels.h defines them (biased variance as E[x^2] - mean^2,
|gamma| + eps when abs_gamma); the activated layer output is leaky(raw * scale + shift).

  conv_ref          ATen's convolution in float64: the truth.
  conv_ref32_loop   the float32 yardstick: one accumulator per output, one (ci, ky, kx) term at a time in that order, product and sum in float32.  A
                    loop for the reason sparse_ref.conv_offsets and sampler_ref give: ATen's own float32 convolution may sum more favourably and
                    understate the yardstick (tests/test_convnet_ref_cpu.py prints both).
  conv_split_model  the value the split-f16 form has by construction, without the device's accumulation order: activations split toward zero
                    (csrc/split_f16.h, C form), weights to nearest (k_conv_pack_x3, like weights.pack_sparse_conv_x3), x_hi W_hi + x_hi W_lo + x_lo W_hi
                    summed in float64.
  abn_stats, abn_act, pack_fp32, pack_x3, and `case`, which draws a seeded case and evaluates all of the above on it.

Rule E: max |gpu - ref64| <= 4 e + 4 ulp of the output's magnitude, with NO floor of 1 under the magnitude; e = e_ref for the fp32
kernels and max(e_ref, e_split) for the matrix-core kernels.  tests/test_convnet_ref_cpu.py checks these references against each other and asserts what
the families reach; tests/test_gpu_convnet_units.py compares the HIP kernels with them on the very same inputs."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from sparse_ref import ULP, _rng, _t, split_activations, split_weights

F64, F32 = torch.float64, torch.float32
EPS = float(np.float32(1e-5))
SLOPE = 0.01

# (cin, cout, k, stride): CONV_SHAPES of tests/test_gpu_parity.py, the shapes o2345_conv2d has a kernel for
SHAPES = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1), (32, 32, 1, 1), (32, 16, 3, 1), (32, 8, 3, 1),
          (56, 16, 3, 1), (56, 8, 3, 1))
SCALE_SHAPES = ((3, 8, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1), (32, 32, 1, 1), (56, 16, 3, 1))       # the shapes of the wscale and xscale families

# the map families as OUTPUT sizes (V, Ho, Wo)
MAPS = {"pixel": (1, 1, 1),            # every staged value but one is padding
        "tile": (2, 8, 32),            # exactly one fp32 tile, one or two x3 tiles, no ragged edge
        "ragged": (5, 9, 35),          # one row and three columns past a tile on both axes; V = 5
        "blocks": (3, 65, 500),        # 97,500 pixels: tier 0 with 432 partial blocks per channel, not a multiple of 256
        "tier1": (2, 61, 821),         # 100,162 pixels: two pixels per thread, ragged on both axes
        "tier2": (2, 61, 3281)}        # 400,282 pixels: four pixels per thread; stride-1 shapes only
SMALL_MAPS = ("pixel", "tile", "ragged", "blocks")
CROP_ROWS = 16                         # tier1, tier2: the float32 loop runs on the first 16 output rows of view 0 (the float64 truth stays full size)
STATS_FLOOR = 256                      # statistics of fewer values stay uncompared (tests/test_gpu_parity.py, test_conv2d_maps_smaller_than_a_tile)
WSCALE_E, XSCALE_E = (-3, -6, -9), (-6, 6)


def tier2_shapes():
    """tier2 leaves out the 5 x 5 stride-2 shapes: their tier 2 launches the template arguments of tier 1."""
    return tuple(s for s in SHAPES if s[3] == 1)


def in_size(shape, fam):
    """-> (V, Hi, Wi).  Stride 2: (8, 16) takes 2 Ho - 1 rows and 2 Wo columns, (16, 32) 2 Ho rows and 2 Wo - 1 columns -- both parities on both axes."""
    cin, cout, k, stride = shape
    V, Ho, Wo = MAPS[fam]
    if stride == 1:
        return V, Ho, Wo
    odd_rows = cin == 8
    return V, 2 * Ho - (1 if odd_rows else 0), 2 * Wo - (0 if odd_rows else 1)


def out_size(Hi, Wi, k, stride):
    p = k // 2
    return (Hi + 2 * p - k) // stride + 1, (Wi + 2 * p - k) // stride + 1


# ------------------------------------------------------------------------------------------------ the operations
def leaky(t, slope):
    return torch.where(t >= 0, t, t * slope)


def act_input(x, in_ss, slope, dtype):
    """leaky(x * scale + shift) per input channel in `dtype`, or x itself without in_ss."""
    x = x.to(dtype)
    if in_ss is None:
        return x
    cin = x.shape[1]
    ss = in_ss.to(dtype)
    return leaky(x * ss[:cin].view(1, -1, 1, 1) + ss[cin:].view(1, -1, 1, 1), slope)


def conv_ref(x, w, bias=None, stride=1, in_ss=None, slope=SLOPE, dtype=F64):
    """The layer through ATen in `dtype` (float64: the truth): the activation first, then the zero padding k // 2 of the convolution."""
    return F.conv2d(act_input(x, in_ss, slope, dtype), w.to(dtype), None if bias is None else bias.to(dtype), stride, w.shape[-1] // 2)


def conv_ref32_loop(x, w, bias=None, stride=1, in_ss=None, slope=SLOPE, rows=None):
    """The float32 yardstick: every output has one float32 accumulator (starting at the bias) that takes the terms (ci, ky, kx) one at a time in that
    order, each a float32 product added in float32; vectorised over views, output channels and pixels.  rows = n: the first n output rows of view 0."""
    xa = act_input(x, in_ss, slope, F32)
    cout, cin, k, _ = w.shape
    V, _, Hi, Wi = xa.shape
    Ho, Wo = out_size(Hi, Wi, k, stride)
    p = k // 2
    if rows is not None:
        V, Ho = 1, min(rows, Ho)
    xp = F.pad(xa[:V], (p, p, p, p))[:, :, :(Ho - 1) * stride + k]
    w32 = w.to(F32)
    acc = torch.zeros(V, cout, Ho, Wo, dtype=F32) if bias is None else bias.to(F32).view(1, -1, 1, 1).expand(V, cout, Ho, Wo).clone()
    term = torch.empty_like(acc)
    for ci in range(cin):
        for ky in range(k):
            for kx in range(k):
                xs = xp[:, ci:ci + 1, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
                torch.mul(xs, w32[:, ci, ky, kx].view(1, -1, 1, 1), out=term)
                acc += term
    return acc


def conv_split_model(x, w, bias=None, stride=1, in_ss=None, slope=SLOPE):
    """The split-f16 form's value: the float32 activated input split toward zero, the weights to nearest, hi * (hi + lo) + lo * hi summed in float64."""
    xa = act_input(x, in_ss, slope, F32)
    xh, xl = (torch.from_numpy(a).double() for a in split_activations(xa.numpy()))
    wh, wl = (torch.from_numpy(a).double() for a in split_weights(w.to(F32).numpy()))
    p = w.shape[-1] // 2
    out = F.conv2d(xh, wh + wl, None, stride, p) + F.conv2d(xl, wh, None, stride, p)
    return out if bias is None else out + bias.double().view(1, -1, 1, 1)


def abn_stats(raw, gamma, beta, eps=EPS, abs_gamma=True):
    """(scale | shift) [2 C] of InPlaceABN from the batch statistics of raw [V,C,H,W] over (V, H, W), as abn_scale_shift (csrc/block_kernels.h) defines
    them, in the precision of raw: float64 or float32."""
    dt = raw.dtype
    n = raw.shape[0] * raw.shape[2] * raw.shape[3]
    mean = raw.sum((0, 2, 3)) / n
    var = ((raw * raw).sum((0, 2, 3)) / n - mean * mean).clamp_min(0)
    g = gamma.to(dt)
    if abs_gamma:
        g = g.abs() + eps
    scale = g / torch.sqrt(var + eps)
    return torch.cat([scale, beta.to(dt) - mean * scale])


def abn_act(raw, ss, slope=SLOPE):
    C = raw.shape[1]
    ss = ss.to(raw.dtype)
    return leaky(raw * ss[:C].view(1, -1, 1, 1) + ss[C:].view(1, -1, 1, 1), slope)


def pack_fp32(w):
    """nn.Conv2d weight [cout,cin,k,k] -> float32 [cin][k][k][cout], flat (k_conv_pack)."""
    return np.ascontiguousarray(np.asarray(w, np.float32).transpose(1, 2, 3, 0)).reshape(-1)


def pack_x3(w):
    """nn.Conv2d weight [cout,cin,k,k] -> float16 [tap][group][hi | lo][64 lanes][8] (k_conv_pack_x3): lane (i = lane & 31, h = lane >> 5) of step
    (tap, u) holds W[i][16 u + 8 h + t][tap], t = 0 .. 7, zeros beyond cout and cin; hi = f16(w), lo = f16(w - hi), both to nearest."""
    w = np.asarray(w, np.float32)
    cout, cin, k, _ = w.shape
    nu = (cin + 15) // 16
    wp = np.zeros((32, nu * 16, k * k), np.float32)
    wp[:cout, :cin] = w.reshape(cout, cin, k * k)
    hi = wp.astype(np.float16)
    lo = (wp - hi.astype(np.float32)).astype(np.float16)
    halves = np.stack([hi, lo])                                             # [half][i][c][tap], c = (u, h, t)
    out = halves.reshape(2, 32, nu, 2, 8, k * k).transpose(5, 2, 0, 3, 1, 4)   # [tap][u][half][h][i][t]: lane = 32 h + i
    return np.ascontiguousarray(out).reshape(k * k, nu, 2, 64, 8)


def x3_dispatch(cin, cout, k, stride):
    """What o2345_conv2d_x3 does with a shape, read from its dispatch: the kernel's (padded cin, k, stride), or None for its "no kernel for" error."""
    if not (1 <= cout <= 32 and 1 <= cin <= 64):
        return None
    cinp = (cin + 15) // 16 * 16
    return (cinp, k, stride) if (k, stride, cinp) in ((3, 1, 16), (3, 1, 32), (3, 1, 64), (5, 2, 16), (1, 1, 32)) else None


# ------------------------------------------------------------------------------------------------ the seeded cases
def white_image(g, V, H, W):
    """An object on a white background: exactly 1.0 outside an ellipse of a quarter of the map's area, uniform in [0, 1) inside it -> [V,3,H,W]."""
    yy, xx = np.meshgrid((np.arange(H) + 0.5) / H - 0.5, (np.arange(W) + 0.5) / W - 0.5, indexing="ij")
    inside = yy * yy + xx * xx < 0.25 / np.pi                               # radius r in units of the map's sides: pi r^2 = 1 / 4
    img = np.ones((V, 3, H, W))
    img[:, :, inside] = g.uniform(0.0, 1.0, (V, 3, int(inside.sum())))
    return _t(img)


def _both_signs(g, lo, hi, n):
    """uniform(lo, hi, n) with both signs present (n >= 2: the first two entries get one each)."""
    v = g.uniform(lo, hi, n)
    if n >= 2:
        v[0], v[1] = abs(v[0]), -abs(v[1])
    return v


def _err(a, ref64):
    return (a.double() - ref64).abs().max().item() if ref64.numel() else 0.0


def _mag(ref64):
    return ref64.abs().max().item() if ref64.numel() else 0.0


@functools.lru_cache(maxsize=12)
def case(shape, fam, fused=False, kind="normal", e=0):
    """One seeded case with all its references.  Plain: bias, no in_ss, no batch norm.  Fused: in_ss with both signs of scale, no bias, bn = (gamma of both
    signs, beta, 1e-5, abs_gamma = True).  kind: "normal" -- x N(0.2, 1), weights N(0, 1) / sqrt(cin k^2); "white" -- white_image with the identity as
    in_ss (the product's first layer reads the images as they are) and every output channel's weights shifted to sum to +-1.5; "wscale" -- the normal weights times 2^e; "xscale" -- in_ss, scale and shift,
    times 2^e: the activated input is the normal one's times 2^e; "deadchannel" -- output channel cout // 2 has all-zero weights.
    -> dict: x, w, bias, in_ss, gamma, beta, bn (= fused), stride, ref64, e_ref, e_split (None on tier1 / tier2, where no x3 kernel runs), mag; fused also ss64,
    act64 and e_ref / e_split / mag of both (suffix _ss, _act).  On tier1 / tier2 every yardstick is taken on the first CROP_ROWS rows of view 0."""
    cin, cout, k, stride = shape
    V, Hi, Wi = in_size(shape, fam)
    g = _rng("convnet", *shape, fam)                                        # one stream per (shape, map): the kinds share x, w and the rest
    x = _t(g.normal(0.2, 1.0, (V, cin, Hi, Wi)))
    w = _t(g.normal(0.0, 1.0, (cout, cin, k, k)) / np.sqrt(cin * k * k))
    bias = _t(g.normal(0.0, 0.3, cout))
    in_ss = _t(np.concatenate([_both_signs(g, -1.5, 1.5, cin), g.normal(0.0, 0.3, cin)]))
    gamma, beta = _t(_both_signs(g, -1.5, 1.5, cout)), _t(g.normal(0.0, 0.2, cout))
    if kind == "white":
        assert (cin, cout) == (3, 8)
        x, in_ss = white_image(g, V, Hi, Wi), _t(np.concatenate([np.ones(cin), np.zeros(cin)]))
        # the 27 weights of output channel c shifted to sum to +-1.5 (signs alternating): the background maps to that constant, the mean the statistics carry
        target = torch.tensor([1.5, -1.5] * (cout // 2), dtype=F64)
        w = (w.double() + ((target - w.double().sum((1, 2, 3))) / (cin * k * k)).view(-1, 1, 1, 1)).float()
    elif kind == "wscale":
        w = w * 2.0 ** e
    elif kind == "xscale":
        in_ss = in_ss * 2.0 ** e
    elif kind == "deadchannel":
        w[cout // 2] = 0.0
    else:
        assert kind == "normal" and e == 0
    assert fused or kind == "normal"
    c = dict(x=x, w=w, stride=stride, bias=None if fused else bias, in_ss=in_ss if fused else None, gamma=gamma, beta=beta, bn=fused, shape=shape, fam=fam)
    args = (x, w, c["bias"], stride, c["in_ss"], SLOPE)
    ref64 = conv_ref(*args)
    assert tuple(ref64.shape) == (MAPS[fam][0], cout) + MAPS[fam][1:]
    crop = CROP_ROWS if fam in ("tier1", "tier2") else None
    ref32 = conv_ref32_loop(*args, rows=crop)
    r64 = ref64 if crop is None else ref64[:1, :, :crop]                     # what the yardsticks are compared with
    split = None if crop else conv_split_model(*args)
    c.update(ref64=ref64, mag=_mag(ref64), e_ref=_err(ref32, r64), e_split=None if split is None else _err(split, r64))
    if fused:
        ss64 = abn_stats(ref64, gamma, beta)
        act64 = abn_act(ref64, ss64)
        ss_y = abn_stats(r64, gamma, beta)                                   # the truth of the yardsticks' own map (the crop, or all of it)
        act_y = abn_act(r64, ss_y)
        ss32 = abn_stats(ref32, gamma, beta)
        c.update(ss64=ss64, act64=act64, mag_ss=_mag(ss64), mag_act=_mag(act64), e_ref_ss=_err(ss32, ss_y), e_ref_act=_err(abn_act(ref32, ss32), act_y),
                 e_split_ss=None, e_split_act=None)
        if split is not None:
            ss_s = abn_stats(split, gamma, beta)
            c.update(e_split_ss=_err(ss_s, ss_y), e_split_act=_err(abn_act(split, ss_s), act_y))
    return c


def rule_e_bound(e_yard, magnitude):
    """Rule E on a yardstick error: 4 e + 4 ulp of the output's magnitude -- no floor of 1 under the magnitude."""
    return 4 * e_yard + 4 * ULP * magnitude


def bound(c, x3, what=""):
    """Rule E of a case: 4 e + 4 ulp of the magnitude, e = e_ref (fp32 kernels) or max(e_ref, e_split) (x3 kernels); what = "", "_ss" or "_act"."""
    return rule_e_bound(yard(c, x3, what), c["mag" + what])


def yard(c, x3, what=""):
    return max(c["e_ref" + what], c["e_split" + what]) if x3 else c["e_ref" + what]


# channel counts o2345_conv2d_x3 accepts but the product never passes: (cin, cout, k, stride)
ODD_COUNTS = ((1, 1, 3, 1), (17, 5, 3, 1), (20, 31, 3, 1), (64, 32, 3, 1), (9, 7, 5, 2), (33, 8, 1, 1))


@functools.lru_cache(maxsize=None)
def odd_case(shape, fam="ragged"):
    """A case of ODD_COUNTS on the output map of `fam` (stride 2: 2 Ho - 1 rows, 2 Wo columns) with bias, in_ss and batch statistics at once -> as `case`,
    raw output and (scale | shift)."""
    cin, cout, k, stride = shape
    V, Ho, Wo = MAPS[fam]
    Hi, Wi = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo)
    g = _rng("convnet-odd", *shape, fam)
    x = _t(g.normal(0.2, 1.0, (V, cin, Hi, Wi)))
    w = _t(g.normal(0.0, 1.0, (cout, cin, k, k)) / np.sqrt(cin * k * k))
    bias = _t(g.normal(0.0, 0.3, cout))
    in_ss = _t(np.concatenate([_both_signs(g, -1.5, 1.5, cin), g.normal(0.0, 0.3, cin)]))
    gamma, beta = _t(_both_signs(g, -1.5, 1.5, cout)), _t(g.normal(0.0, 0.2, cout))
    args = (x, w, bias, stride, in_ss, SLOPE)
    ref64, ref32, split = conv_ref(*args), conv_ref32_loop(*args), conv_split_model(*args)
    ss64 = abn_stats(ref64, gamma, beta)
    return dict(x=x, w=w, bias=bias, in_ss=in_ss, stride=stride, gamma=gamma, beta=beta, bn=True, ref64=ref64, mag=_mag(ref64), e_ref=_err(ref32, ref64),
                e_split=_err(split, ref64), ss64=ss64, mag_ss=_mag(ss64), e_ref_ss=_err(abn_stats(ref32, gamma, beta), ss64),
                e_split_ss=_err(abn_stats(split, gamma, beta), ss64), shape=shape, fam=fam)


# channel-last inputs: (cin, cout, pixel stride, channel offset)
CHANNEL_LAST = ((56, 16, 64, 3), (56, 8, 64, 3), (32, 16, 64, 5), (32, 16, 40, 8))


def channel_last_map(c, pix_stride, offset):
    """The case's input as channels offset .. offset + cin of a channel-last map [V,Hi,Wi,pix_stride] whose other channels hold seeded noise."""
    x = c["x"]
    V, cin, Hi, Wi = x.shape
    cm = _t(_rng("convnet-cl", *c["shape"], c["fam"], pix_stride, offset).normal(0.0, 1.0, (V, Hi, Wi, pix_stride)))
    cm[..., offset:offset + cin] = x.permute(0, 2, 3, 1)
    return cm.contiguous()


# ------------------------------------------------------------------------------------------------ ABN on channel-first maps
ABN_HW = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 128: (8, 16)}     # around the 64-pixel tile of launch_nchw_to_nhwc
ABN_C, ABN_V = (8, 16, 32), (1, 3)
WANTS = ((True, False), (False, True), (True, True))                          # (want_nchw, want_nhwc): at least one


@functools.lru_cache(maxsize=None)
def abn_case(C, V, H, W, abs_gamma=True):
    """x N(-0.2, 1.5) [V,C,H,W], gamma of both signs, beta N(0, 0.2) -> the float64 ABN (ss64, act64) and the float32 evaluation's error against it."""
    g = _rng("convnet-abn", C, V, H, W)
    x = _t(g.normal(-0.2, 1.5, (V, C, H, W)))
    gamma, beta = _t(_both_signs(g, -1.5, 1.5, C)), _t(g.normal(0.0, 0.2, C))
    ss64 = abn_stats(x.double(), gamma, beta, EPS, abs_gamma)
    act64 = abn_act(x.double(), ss64)
    ss32 = abn_stats(x, gamma, beta, EPS, abs_gamma)
    return dict(x=x, gamma=gamma, beta=beta, ss64=ss64, act64=act64, ss32=ss32, mag_ss=_mag(ss64), mag_act=_mag(act64), e_ref_ss=_err(ss32, ss64),
                e_ref_act=_err(abn_act(x, ss32), act64), e_split_ss=None, e_split_act=None)
