"""Plain float64 references of the volume front end's glue operations, and the seeded inputs their tests share -- TEST INFRASTRUCTURE ONLY.

torch and numpy on the CPU, nothing else: the product package is not imported here.  Every reference is written from the DEFINITION of its
operation (the formula of bilinear interpolation, of batch normalisation, of a box dilation, an index expression for a layout change), not from the
kernel that implements it.  tests/test_frontend_ref_cpu.py checks each reference against an independent implementation and asserts that the
generated inputs exercise the edges they were chosen for; tests/test_gpu_frontend_units.py compares the HIP kernels with the references on the very
same inputs."""
import numpy as np
import torch

F64 = torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def leaky(t, slope):
    return torch.where(t >= 0, t, t * slope)


# ------------------------------------------------------------------------------------------------ references
def _axis(n_in, n_out):
    """align_corners=True: source coordinate of every destination index -> (i0, i1, weight of i1)."""
    dst = torch.arange(n_out, dtype=F64)
    src = dst * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros(n_out, dtype=F64)
    i0 = src.floor().long().clamp(0, n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.to(F64)


def bilinear_up(x, factor):
    """[V,C,h,w] -> [V,C,h*factor,w*factor] in float64, bilinear, align_corners=True."""
    x = x.to(F64)
    h, w = x.shape[2:]
    y0, y1, ly = _axis(h, h * factor)
    x0, x1, lx = _axis(w, w * factor)
    rows = x[:, :, y0, :] * (1 - ly)[None, None, :, None] + x[:, :, y1, :] * ly[None, None, :, None]
    return rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx


def fpn_level(fine, coarse, weight, bias, fine_ss=None, slope=0.01):
    """up2(coarse) + 1x1 convolution (weight [32,C], bias [32]) of the fine map; fine_ss = (scale | shift) [2C]: leaky(fine * scale + shift) first."""
    fine = fine.to(F64)
    C = fine.shape[1]
    if fine_ss is not None:
        ss = fine_ss.to(F64)
        fine = leaky(fine * ss[:C].view(1, C, 1, 1) + ss[C:].view(1, C, 1, 1), slope)
    lateral = torch.einsum("oc,vchw->vohw", weight.to(F64).reshape(32, C), fine) + bias.to(F64).view(1, 32, 1, 1)
    return bilinear_up(coarse, 2) + lateral


def pyramid(f2, s1, s0, rgb):
    """-> (fmaps [V,56,H,W] = up4(f2) | up2(s1) | s0, cmaps [V,H,W,64] = rgb | fmaps | 5 zeros), float64."""
    fm = torch.cat([bilinear_up(f2, 4), bilinear_up(s1, 2), s0.to(F64)], 1)
    V, _, H, W = fm.shape
    cm = torch.cat([rgb.to(F64), fm, torch.zeros(V, 5, H, W, dtype=F64)], 1).permute(0, 2, 3, 1).contiguous()
    return fm, cm


def bn_rows(x, gamma, beta, eps=1e-5, slope=0.0, abs_gamma=False, skip=None):
    """Batch normalisation of rows [n,C] with the batch's own statistics -> (y, mean, biased variance), float64; two-pass variance;
    abs_gamma: the |gamma| + eps convention of InPlaceABN; the activation comes before the skip addition."""
    x = x.to(F64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    g = gamma.to(F64).abs() + eps if abs_gamma else gamma.to(F64)
    y = leaky((x - mean) / torch.sqrt(var + eps) * g + beta.to(F64), slope)
    if skip is not None:
        y = y + skip.to(F64)
    return y, mean, var


def prune_dilate(sdf, mask, D, thr, r, inclusive=False):
    """uint8 [D^3]: mask > 0 AND some voxel of the (2r+1)^3 box around the voxel, clipped to the volume, has |sdf| < thr (strict, in float32).
    ``inclusive`` replaces < by <=: only the input-condition checks use it."""
    a = np.abs(np.asarray(sdf, dtype=np.float32).reshape(D, D, D))
    near = a <= np.float32(thr) if inclusive else a < np.float32(thr)
    hit = np.zeros((D, D, D), dtype=bool)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dz in range(-r, r + 1):
                if max(abs(dx), abs(dy), abs(dz)) >= D:
                    continue
                dst = tuple(slice(max(0, -d), D - max(0, d)) for d in (dx, dy, dz))          # voxels whose neighbour at +d lies inside
                src = tuple(slice(max(0, d), D - max(0, -d)) for d in (dx, dy, dz))
                hit[dst] |= near[src]
    keep = hit & (np.asarray(mask, dtype=np.float32).reshape(D, D, D) > 0)
    return torch.from_numpy(keep.reshape(-1).astype(np.uint8))


def nchw_to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def pack_color_maps(feat, rgb):
    """[V,56,H,W] features + [V,3,H,W] colours -> [V,H,W,64]: channel k = rgb[k] (k < 3), feat[k - 3] (k < 59), 0."""
    V, _, H, W = feat.shape
    out = torch.zeros(V, H, W, 64, dtype=feat.dtype)
    out[..., 0:3] = rgb.permute(0, 2, 3, 1)
    out[..., 3:59] = feat.permute(0, 2, 3, 1)
    return out


def scatter_dense(rows, row_of_voxel, dims):
    """-> (channel-last [dx,dy,dz,C], channel-first [1,C,dx,dy,dz], mask [1,1,dx,dy,dz]): voxel v holds rows[row_of_voxel[v]], or zeros for -1."""
    dx, dy, dz = dims
    C = rows.shape[1]
    r = row_of_voxel.long()
    cl = torch.zeros(dx * dy * dz, C, dtype=rows.dtype)
    if rows.shape[0]:
        cl[r >= 0] = rows[r[r >= 0]]
    cl = cl.view(dx, dy, dz, C)
    return cl, cl.permute(3, 0, 1, 2).contiguous()[None], (r >= 0).to(rows.dtype).view(1, 1, dx, dy, dz)


# ------------------------------------------------------------------------------------------------ the cases and their seeded inputs
def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


FPN_SHAPES = [(1, 2, 2), (2, 6, 10), (3, 14, 18), (2, 18, 30)]             # coarse map 1 x 1 | less than one wave | one block, ragged last wave | three blocks, 28 live threads in the last
FPN_CASES = [(C, with_ss, shape) for C in (8, 16) for with_ss in (False, True) for shape in FPN_SHAPES]
FPN_SLOPE = 0.01


def fpn_inputs(C, with_ss, shape):
    V, H, W = shape
    g = _rng(1, C, with_ss, V, H, W)
    d = dict(fine=_t(g.normal(0.0, 1.0, (V, C, H, W))), coarse=_t(g.normal(0.0, 1.0, (V, 32, H // 2, W // 2))),
             weight=_t(g.uniform(-1.0, 1.0, (32, C)) / np.sqrt(C)), bias=_t(g.normal(0.0, 0.3, 32)), fine_ss=None)
    if with_ss:                                                             # scales of both signs: both leaky branches occur in every channel
        d["fine_ss"] = _t(np.concatenate([g.uniform(-1.5, 1.5, C), g.normal(0.0, 0.3, C)]))
    return d


def fpn_preactivations(d):
    C = d["fine"].shape[1]
    return d["fine"].double() * d["fine_ss"][:C].double().view(1, C, 1, 1) + d["fine_ss"][C:].double().view(1, C, 1, 1)


PYRAMID_SHAPES = [(1, 4, 4), (2, 8, 12), (3, 12, 20), (2, 20, 28)]        # coarse maps 1 x 1 | 96 pixels: half-live wave + two dead ones | 240 | 560: 48-pixel tail


def pyramid_inputs(shape):
    V, H, W = shape
    g = _rng(2, V, H, W)
    return dict(f2=_t(g.normal(0.0, 1.0, (V, 32, H // 4, W // 4))), s1=_t(g.normal(0.0, 1.0, (V, 16, H // 2, W // 2))),
                s0=_t(g.normal(0.0, 1.0, (V, 8, H, W))), rgb=_t(g.uniform(0.0, 1.0, (V, 3, H, W))))


BN_EPS = 1e-5
BN_CHANNELS = (16, 32, 64)
BN_CONFIGS = {"relu_skip": dict(slope=0.0, abs_gamma=False, skip=True),           # costreg.py: BatchNorm + ReLU, then the U-Net's skip addition
              "identity_stats": dict(slope=1.0, abs_gamma=False, skip=False),      # the torchsparse shim's BatchNorm: no activation, batch statistics returned
              "leaky_abs_gamma": dict(slope=0.01, abs_gamma=True, skip=False)}     # the InPlaceABN convention


def bn_sizes(C):
    """Row counts: 1, 3, one short of / one past a single block's rows (256 // C rows per pass, 8 passes), several blocks with a ragged last one,
    and the first size past 1024 blocks, where the partial-sum kernel walks its grid-stride loop."""
    rpb = 256 // C
    return [1, 3, rpb * 8 - 1, rpb * 8 + 1, 5003, 1024 * rpb * 8 + 37]


BN_CASES = [(C, n, cfg) for C in BN_CHANNELS for n in bn_sizes(C) for cfg in BN_CONFIGS]


def bn_const_channel(C):
    return C // 3


def bn_inputs(C, n, cfg):
    """x ~ normal(mean_c, std_c) with per-channel means in [-3, 3] and stds in [0.2, 2]; channel bn_const_channel(C) is constant (variance exactly 0)."""
    k = BN_CONFIGS[cfg]
    g = _rng(3, C, n, sorted(BN_CONFIGS).index(cfg))
    mean, std = g.uniform(-3.0, 3.0, C), g.uniform(0.2, 2.0, C)
    x = g.normal(0.0, 1.0, (n, C)) * std[None] + mean[None]
    x[:, bn_const_channel(C)] = np.float32(mean[bn_const_channel(C)])
    gamma = g.uniform(0.5, 1.5, C)
    if k["abs_gamma"]:
        gamma *= np.where(np.arange(C) % 3 == 1, -1.0, 1.0)                 # gammas of both signs
    return dict(x=_t(x), gamma=_t(gamma), beta=_t(g.normal(0.0, 0.3, C)), skip=_t(g.normal(0.0, 1.0, (n, C))) if k["skip"] else None,
                slope=k["slope"], abs_gamma=k["abs_gamma"])


SHIM_BN_C = 32
SHIM_BN_ROWS = (2, 777)                                                     # the two training-mode forwards; the eval-mode forward reuses the second batch


def shim_bn_inputs():
    g = _rng(4)
    mean, std = g.uniform(-3.0, 3.0, SHIM_BN_C), g.uniform(0.2, 2.0, SHIM_BN_C)
    return dict(batches=[_t(g.normal(0.0, 1.0, (n, SHIM_BN_C)) * std[None] + mean[None]) for n in SHIM_BN_ROWS],
                gamma=_t(g.uniform(0.5, 1.5, SHIM_BN_C)), beta=_t(g.normal(0.0, 0.3, SHIM_BN_C)))


PRUNE_THR = 0.25
PRUNE_CASES = [(D, r) for D in (5, 13, 24) for r in (0, 1, 3)]              # D = 5, r = 3: every box is clipped on both sides


def prune_inputs(D, r):
    """sdf: multiples of 1/64 in [-1, 1], a quarter of them at |sdf| == thr exactly; about one voxel per (2r+1)^3 box is below the threshold (a quarter
    of them for r = 0), so that the dilated set neither fills the volume nor leaves it empty; the others lie above.  mask: about 30 % zeros."""
    g = _rng(5, D, r)
    n = D ** 3
    k = int(PRUNE_THR * 64)
    sdf = g.integers(k + 1, 65, n)                                          # above the threshold
    at = g.random(n) < 0.25
    sdf[at] = k
    n_sub = max(1, round(n / (2 * r + 1) ** 3)) if r else n // 4
    sdf[g.choice(n, n_sub, replace=False)] = g.integers(0, k, n_sub)        # below it (strictly)
    sdf = sdf * g.choice([-1, 1], n)
    return dict(sdf=_t(sdf / 64.0), mask=_t((g.random(n) >= 0.3).astype(np.float32)), D=D, r=r, thr=PRUNE_THR)


def prune_corner_inputs(D=13, r=3):
    """The only voxels below the threshold are the eight corners: every box that reaches one is clipped by the border on three sides."""
    g = _rng(6, D, r)
    n = D ** 3
    k = int(PRUNE_THR * 64)
    sdf = (g.integers(k, 65, n) * g.choice([-1, 1], n)).reshape(D, D, D)    # |sdf| >= thr, equality included
    for cx in (0, D - 1):
        for cy in (0, D - 1):
            for cz in (0, D - 1):
                sdf[cx, cy, cz] = g.integers(-k + 1, k)
    return dict(sdf=_t(sdf.reshape(-1) / 64.0), mask=_t((g.random(n) >= 0.3).astype(np.float32)), D=D, r=r, thr=PRUNE_THR)


NHWC_CASES = [(C, hw) for C in (8, 16, 64) for hw in ((1, 1), (7, 9), (5, 13), (8, 16))]        # HW = 1, 63, 65, 128 around the 64-pixel tile


def nhwc_inputs(C, hw):
    return _t(_rng(7, C, *hw).normal(0.0, 1.0, (2, C) + tuple(hw)))


PACK_SHAPES = [(2, 7, 9), (3, 12, 20)]


def pack_inputs(shape):
    V, H, W = shape
    g = _rng(8, V, H, W)
    return dict(feat=_t(g.normal(0.0, 1.0, (V, 56, H, W))), rgb=_t(g.uniform(0.0, 1.0, (V, 3, H, W))))


SCATTER_CASES = [(C, dims) for C in (8, 16) for dims in ((5, 6, 7), (8, 8, 8))]


def scatter_inputs(C, dims):
    """rows [n,C] and an index map with about half the voxels at -1, the others a permutation of the rows."""
    g = _rng(9, C, *dims)
    nvox = dims[0] * dims[1] * dims[2]
    kept = np.flatnonzero(g.random(nvox) < 0.5)
    row = np.full(nvox, -1, dtype=np.int32)
    row[kept] = g.permutation(len(kept)).astype(np.int32)
    return dict(rows=_t(g.normal(0.0, 1.0, (len(kept), C))), row_of_voxel=torch.from_numpy(row))
