"""Torch-tensor wrappers over the C ABI (include/o2345.h).  PyTorch is plumbing only: device memory + streams.
Every library call goes through ``call``: _lib checks dtype / device / contiguity of every pointer and the range of every integer against the
header's declaration, passes raw pointers, and raises on a non-zero status."""
import ctypes
import functools
from collections import namedtuple
import threading

import numpy as np
import torch

from . import _lib, config, mesh_io


# No call below names its stream: _lib.call fills in the current HIP stream of the CURRENT device, and every public op runs under _on_device, which makes
# the device of its tensor arguments current first (the C side sizes persistent grids from hipGetDevice()).
call = _lib.call


def _stats_block(name, device, *rows):
    """Device memory for a stats block the header declares (a struct has no torch dtype: uint8 of exactly its size), or ``rows`` of them."""
    return torch.empty(*rows, ctypes.sizeof(_lib.STRUCTS[name]), dtype=torch.uint8, device=device)


def _first_cuda_tensor(objs):
    for o in objs:
        if torch.is_tensor(o):
            if o.is_cuda:
                return o
        elif isinstance(o, dict):
            t = _first_cuda_tensor(o.values())
            if t is not None:
                return t
    return None


def _on_device(fn):
    """Run the op with the device of its (first) CUDA tensor argument current, so that the launch stream, the workspace and
    the C side's device queries all refer to the tensors' device even when the caller never called torch.cuda.set_device."""
    @functools.wraps(fn)
    def wrapped(*args, **kw):
        t = _first_cuda_tensor(list(args) + list(kw.values()))
        if t is None:
            raise ValueError(f"o2345 ops.{fn.__name__}: needs CUDA tensors (the HIP library has no CPU fallback)")
        with torch.cuda.device(t.device):
            return fn(*args, **kw)
    return wrapped


def _f(t):
    return t.detach().to(torch.float32).contiguous()


def host_f32(a):                          # a tensor or an array -> a contiguous float32 host array (the small arguments: bounds, matrices, cameras)
    return np.ascontiguousarray(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float32))


def _double_of_bits(u):                   # a double that a stats block carries as its bit pattern (uint64, so that the device can take integer maxima)
    return float(np.uint64(u).view(np.float64))


def _host3(v):
    return host_f32(v).reshape(-1)[:3]


def _bounds(bound_min, bound_max, what):
    """The box of a lattice, validated -> (bound_min, bound_max): three float32 each, on the host."""
    bmin, bmax = _host3(bound_min), _host3(bound_max)
    if bmin.shape != (3,) or bmax.shape != (3,) or not (np.isfinite(bmin).all() and np.isfinite(bmax).all() and (bmax > bmin).all()):
        raise ValueError(f"{what}: bound_max must be above bound_min on every axis, both finite, got {bound_min!r} and {bound_max!r}")
    return bmin, bmax


def _vertices(verts_idx, what=None):
    if verts_idx.dtype != torch.float64 or verts_idx.dim() != 2 or verts_idx.shape[1] != 3:
        raise ValueError((f"{what}: " if what else "") + f"expected vertices [N,3] float64, got {tuple(verts_idx.shape)} {verts_idx.dtype}")


def _resolution(resolution, what):
    if isinstance(resolution, bool) or int(resolution) != resolution or resolution < 2:
        raise ValueError(f"{what}: resolution must be an integer >= 2, got {resolution!r}")
    return int(resolution)


def _obj_digits(K, bounds, n, what):
    """The integer digits of an OBJ's coordinate fields: ``K``, or taken from ``bounds`` (one small D2H copy); range-checked before any use."""
    if K is None:
        K = mesh_io.obj_coordinate_digits(bounds.cpu().numpy() if torch.is_tensor(bounds) else bounds) if n else 1
    if not 1 <= int(K) <= 9:
        raise ValueError(f"{what}: K = {K} integer digits (1 .. 9)")
    return int(K)


def to_host_numpy(*tensors):
    """Device tensors -> numpy arrays: the copies go into pinned blocks of torch's caching host allocator, queued back to back, ONE stream
    synchronisation at the end (a pageable ``.cpu()`` per tensor synchronises per tensor and stages through a bounce buffer: the 67 MB extraction field
    took 6 - 60 ms that way, depending on what was still in flight).  Tensors that already live on the host are returned as they are."""
    out, dev = [], None
    for t in tensors:
        if t.is_cuda:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            dev = t.device
            out.append(h)
        else:
            out.append(t)
    if dev is not None:
        torch.cuda.current_stream(dev).synchronize()
    return [h.numpy() for h in out]


_preloaded = set()
_preload_lock = threading.Lock()


def preload(device):
    """Load every code object of the library on ``device`` now (o2345_preload) -- once per device and process.  The mirrors call it when weights are loaded
    and on the first packing for a device (recon/packs.py: an nn.DataParallel replica's device), so that the HIP runtime's lazy per-translation-unit loading
    (5 - 60 ms each) does not land inside the first timed call of a fresh process.  Thread-safe: nn.DataParallel's device threads may call it at once."""
    device = torch.device(device)
    if device.type != "cuda" or device in _preloaded:
        return
    with _preload_lock:
        if device in _preloaded:
            return
        with torch.cuda.device(device):
            call("o2345_preload")
            if config.warm_aten():
                _warm_aten(device)
        _preloaded.add(device)


def _warm_aten(device):
    """The handful of ATen kernels that the UNCHANGED trainer (and the mirrors' glue) launch inside the reference's timing brackets, each once on a tiny tensor:
    the first launch of an ATen kernel in a process loads its code object (a few ms each: the valid-ray rule's four kernels cost 20 ms in the first
    rendering_network call of a fresh process without this, tools/dropin_bench.py --cold with O2345_WARM_ATEN=0).  Same operators and dtypes as the call sites:
    trainer_generic.py:1119-1123 (bilinear x4 / x2 up-sampling + cat of the pyramid), :1322 (float64 vertices -> float32 on the device),
    rendering_network.py:122-129 (valid-ray rule), generate_grids.py:4-19 (voxel lattice), the per-chunk normal map of val_step (:528-543)."""
    F = torch.nn.functional
    z = torch.zeros(1, 8, 4, 4, device=device)
    torch.cat([F.interpolate(z, scale_factor=4, mode="bilinear", align_corners=True), F.interpolate(z.repeat(1, 1, 2, 2), scale_factor=2, mode="bilinear", align_corners=True),
               z.repeat(1, 1, 4, 4)], dim=1)
    torch.zeros(1, 4, 2, 2, 2, device=device)[0].permute(1, 2, 3, 0).contiguous()
    nv = torch.zeros(2, 64, dtype=torch.uint8, device=device)
    ((nv >= 2).float().sum(1) > 8).cpu()
    torch.stack(torch.meshgrid(*[torch.arange(2, dtype=torch.float32, device=device)] * 3, indexing="ij"))[None]
    torch.zeros(4, 3, dtype=torch.float64).to(z)
    g, w = torch.zeros(2, 4, 3, device=device), torch.zeros(2, 4, device=device)
    (g * w[:, :4, None] * w[..., None]).sum(dim=1).detach().cpu()
    (torch.rand(2, 3, pin_memory=True).to(device, non_blocking=True) * 2 - 1).sum()
    k = torch.eye(3, device=device)[None].repeat(2, 1, 1).clone()              # trainer_generic.py:853-854: intrinsics.clone(); [:, :2] *= 0.25
    k[:, :2] *= 0.25


_ws_cache = {}


def _workspace(nbytes, device, tag="ws"):
    """Scratch buffer per (purpose, device, stream): two streams of one device never share scratch memory.  Host threads are safe as long as each
    enqueues on its OWN stream: nn.DataParallel gives every replica its own device (its thread's key differs by device); two threads that launch onto
    ONE stream of ONE device would overwrite each other's scratch between launches -- code that runs replicas on one device (tests) gives each thread
    its own stream.  ``nbytes`` None: the buffer that is there, or None -- a reader, which allocates nothing."""
    key = (tag, str(device), torch.cuda.current_stream(device).cuda_stream)
    t = _ws_cache.get(key)
    if nbytes is not None and (t is None or t.numel() < nbytes):
        t = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
        _ws_cache[key] = t
    return t


def _scratch(entry, sizes, device, tag="ws"):
    """-> (the scratch buffer of _workspace, its size): as many bytes as the library's ``entry`` (an o2345_*_workspace_bytes function) asks for ``sizes``."""
    nbytes = call(entry, *sizes)
    return _workspace(nbytes, device, tag), nbytes


# ---------------------------------------------------------------------------------------------------------- cost volume
@_on_device
def nchw_to_nhwc(x):
    V, C, H, W = x.shape
    out = torch.empty(V, H, W, C, device=x.device, dtype=torch.float32)
    call("o2345_nchw_to_nhwc", x, out, V, C, H, W)
    return out


def conv_x3(precision=None):
    """True when the convolutions run on the matrix cores (split-f16 form, the default numerical mode), False for the strict fp32 VALU kernels."""
    return config.color_precision(precision) == "f16x3"


@_on_device
def conv2d_pack(weight, precision=None):
    """nn.Conv2d weight [cout,cin,k,k] -> the operand packing of the convolution kernels for the numerical mode in force (one tiny launch; callers
    that own the parameter cache the result, see featurenet.packed_weight): split-f16 MFMA A operands [tap][cin/16][hi|lo][64 lanes][8 f16]
    or, in fp32 mode, [cin][k][k][cout] for the scalar-load VALU kernels."""
    cout, cin, k, k2 = weight.shape
    if k != k2:
        raise ValueError("conv2d: square kernels only")
    if conv_x3(precision):
        t = torch.empty(call("o2345_conv2d_x3_weight_floats", cin, k), dtype=torch.float32, device=weight.device)
        call("o2345_conv2d_pack_weights_x3", _f(weight), cout, cin, k, t)
    else:
        t = torch.empty(cin * k * k * cout, dtype=torch.float32, device=weight.device)
        call("o2345_conv2d_pack_weights", _f(weight), cout, cin, k, t)
    return t


@_on_device
def conv2d(x, weight, bias=None, stride=1, in_scale_shift=None, slope=0.01, bn=None, packed=None, precision=None, nhwc_offset=None):
    """nn.Conv2d (padding k // 2) of FeatureNet / the compress layer as a HIP kernel (csrc/convnet.hip): implicit GEMM on the matrix cores in the
    default mode, direct fp32 VALU convolution in fp32 mode.
    ``in_scale_shift`` [2*cin]: x is the RAW output of a convolution whose InPlaceABN (scale | shift, leaky ``slope``) is applied while x is read.
    ``bn`` = (gamma, beta, eps, abs_gamma): also reduce the batch statistics of the output and return this layer's own (scale | shift) [2*cout]
    for the consumer to apply.  ``packed``: conv2d_pack(weight, precision) kept by the caller.  ``nhwc_offset`` = c0: x is a channel-last map
    [V,Hi,Wi,C] and the convolution reads its channels c0 .. c0 + cin (the compress layer on the [V,H,W,64] colour map, c0 = 3).
    -> (raw output [V,cout,Ho,Wo], scale_shift or None)."""
    cout, cin, k, _ = weight.shape
    if nhwc_offset is None:
        V, cx, Hi, Wi = x.shape
        pix_stride, c0 = 0, 0
        if cx != cin:
            raise ValueError(f"conv2d: weight expects {cin} input channels, got {cx}")
    else:
        V, Hi, Wi, pix_stride = x.shape
        c0 = int(nhwc_offset)
        if c0 < 0 or c0 + cin > pix_stride:
            raise ValueError(f"conv2d: channels {c0}..{c0 + cin} do not fit a channel-last map with {pix_stride} channels")
    pad = k // 2
    Ho, Wo = (Hi + 2 * pad - k) // stride + 1, (Wi + 2 * pad - k) // stride + 1
    out = torch.empty(V, cout, Ho, Wo, dtype=torch.float32, device=x.device)
    ss = gamma = beta = ws = None
    eps, abs_gamma, wsb = 0.0, 0, 0
    if bn is not None:
        gamma, beta, eps, abs_gamma = bn
        ss = torch.empty(2 * cout, dtype=torch.float32, device=x.device)
        ws, wsb = _scratch("o2345_conv2d_workspace_bytes", (V, cout, Ho, Wo), x.device, "conv2d")
    call("o2345_conv2d_x3" if conv_x3(precision) else "o2345_conv2d", x, V, cin, Hi, Wi, int(pix_stride), c0, in_scale_shift, float(slope),
         packed if packed is not None else conv2d_pack(weight, precision), None if bias is None else _f(bias), cout, k, int(stride), out,
         None if gamma is None else _f(gamma), None if beta is None else _f(beta), float(eps), int(abs_gamma), ss, ws, wsb)
    return out, ss


@_on_device
def scale_shift_act(x, scale_shift, slope=0.01, want_nchw=True, want_nhwc=False):
    """leaky_relu(x * scale + shift) of a raw convolution output [V,C,H,W] -> (NCHW or None, channel-last NHWC or None)."""
    V, C, H, W = x.shape
    y1 = torch.empty_like(x) if want_nchw else None
    y2 = torch.empty(V, H, W, C, dtype=torch.float32, device=x.device) if want_nhwc else None
    call("o2345_scale_shift_act", x, V, C, H, W, scale_shift, float(slope), y1, y2)
    return y1, y2


@_on_device
def fpn_level(fine, coarse, weight, bias, fine_scale_shift=None, slope=0.01):
    """FeatureNet._upsample_add(coarse, lateral_1x1(fine)) in one kernel: fine [V,C,H,W] (C = 8 | 16), coarse [V,32,H/2,W/2] -> [V,32,H,W].
    ``fine_scale_shift``: fine is a raw convolution output, its InPlaceABN is applied on load."""
    V, C, H, W = fine.shape
    if C not in (8, 16) or H % 2 or W % 2 or H < 2 or W < 2:
        raise ValueError(f"fpn_level: fine map must be [V,8|16,H,W] with even H and W, got {tuple(fine.shape)}")
    if tuple(coarse.shape) != (V, 32, H // 2, W // 2):
        raise ValueError(f"fpn_level: coarse map must be [V,32,H/2,W/2], got {tuple(coarse.shape)} for fine {tuple(fine.shape)}")
    out = torch.empty(V, 32, H, W, dtype=torch.float32, device=fine.device)
    call("o2345_fpn_level_act", fine, fine_scale_shift, float(slope), C, coarse, _f(weight).reshape(32, C), _f(bias), V, H, W, out)
    return out


@_on_device
def pyramid_pack(f2, s1, s0, rgb, want_nchw=True):
    """Fused pyramid -> (fmaps [V,56,H,W] or None, cmaps [V,H,W,64] = rgb | 56 features | pad)."""
    V, _, H, W = s0.shape
    if H % 4 or W % 4 or H < 4 or W < 4:
        raise ValueError(f"pyramid_pack: map sizes must be multiples of 4, got {H} x {W}")
    if tuple(f2.shape) != (V, 32, H // 4, W // 4) or tuple(s1.shape) != (V, 16, H // 2, W // 2) or tuple(rgb.shape) != (V, 3, H, W) or s0.shape[1] != 8:
        raise ValueError("pyramid_pack: expected f2 [V,32,H/4,W/4], s1 [V,16,H/2,W/2], s0 [V,8,H,W], rgb [V,3,H,W]")
    fm = torch.empty(V, 56, H, W, dtype=torch.float32, device=s0.device) if want_nchw else None
    cm = torch.empty(V, H, W, 64, dtype=torch.float32, device=s0.device)
    call("o2345_pyramid_pack", f2, s1, s0, rgb, V, H, W, fm, cm)
    return fm, cm


@_on_device
def costvol_index(proj, V, H, W, dims, voxel_size, origin, min_views=1):
    """-> cnt u8 [D^3], row_of_voxel i32 [D^3], coords i32 [N,4] (x,y,z,b), N (python int; one 4-byte D2H read)."""
    dx, dy, dz = (int(d) for d in dims)
    nvox = dx * dy * dz
    dev = proj.device
    cnt = torch.empty(nvox, dtype=torch.uint8, device=dev)
    row = torch.empty(nvox, dtype=torch.int32, device=dev)
    coords = torch.empty(nvox, 4, dtype=torch.int32, device=dev)
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, wsb = _scratch("o2345_costvol_workspace_bytes", (dx, dy, dz), dev)
    call("o2345_costvol_index", proj, V, H, W, dx, dy, dz, float(voxel_size), _host3(origin), int(min_views), cnt, row, coords, n_dev, ws, wsb)
    n = int(n_dev.item())
    return cnt, row, coords[:n], n


@_on_device
def costvol_gather(feats_nhwc, proj, dims, voxel_size, origin, cnt, coords):
    V, H, W, C = feats_nhwc.shape
    n = coords.shape[0]
    out = torch.empty(n, 2 * C, dtype=torch.float32, device=feats_nhwc.device)
    if n == 0:
        return out
    dx, dy, dz = (int(d) for d in dims)
    call("o2345_costvol_gather", feats_nhwc, proj, V, H, W, C, dx, dy, dz, float(voxel_size), _host3(origin), cnt, coords, n, out)
    return out


@_on_device
def visible_count_list(proj, H, W, voxel_size, origin, coords):
    """coords [M,4] int32 (x,y,z,b), any order -> number of views that see each listed voxel (u8 [M])."""
    M = coords.shape[0]
    cnt = torch.empty(M, dtype=torch.uint8, device=coords.device)
    if M == 0:
        return cnt
    call("o2345_visible_count_list", proj, proj.shape[0], H, W, float(voxel_size), _host3(origin), coords, M, cnt)
    return cnt


@_on_device
def costvol_gather_list(feats_nhwc, proj, voxel_size, origin, cnt_row, coords):
    V, H, W, C = feats_nhwc.shape
    n = coords.shape[0]
    out = torch.empty(n, 2 * C, dtype=torch.float32, device=feats_nhwc.device)
    if n == 0:
        return out
    call("o2345_costvol_gather_list", feats_nhwc, proj, V, H, W, C, float(voxel_size), _host3(origin), cnt_row, coords, n, out)
    return out


@_on_device
def build_index_grid(coords, ts, cells):
    nx, ny, nz = (int(c) for c in cells)
    grid = torch.empty(nx * ny * nz, dtype=torch.int32, device=coords.device)
    call("o2345_build_index_grid", coords if coords.shape[0] else None, coords.shape[0], int(ts), nx, ny, nz, grid)
    return grid


@_on_device
def prune_dilate(sdf_vol, mask_vol, D, threshold, radius=3):
    out = torch.empty(D * D * D, dtype=torch.uint8, device=sdf_vol.device)
    call("o2345_prune_dilate", sdf_vol, mask_vol, D, float(threshold), int(radius), out)
    return out


@_on_device
def scatter_dense(rows, row_of_voxel, dims, want_cf=True):
    dx, dy, dz = (int(d) for d in dims)
    nvox, C = dx * dy * dz, rows.shape[1]
    dev = rows.device
    if rows.shape[0] == 0:           # nothing kept: all-zero volumes (the kernel needs a non-null rows pointer)
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)
        return z(dx, dy, dz, C), (z(1, C, dx, dy, dz) if want_cf else None), z(1, 1, dx, dy, dz)
    cl = torch.empty(dx, dy, dz, C, dtype=torch.float32, device=dev)
    cf = torch.empty(1, C, dx, dy, dz, dtype=torch.float32, device=dev) if want_cf else None
    mask = torch.empty(1, 1, dx, dy, dz, dtype=torch.float32, device=dev)
    call("o2345_scatter_dense", rows, row_of_voxel, C, nvox, cl, cf, mask)
    return cl, cf, mask


# ---------------------------------------------------------------------------------------------------------- sparse CNN
@_on_device
def sparse_downsample(coords, ts, fine_cells):
    """coords [n,4] int32 at tensor stride ts on a lattice of fine_cells cells/axis -> (grid, coords_c, n_c, cells_c)."""
    nc = tuple((int(c) + 1) // 2 + 1 for c in fine_cells)
    dev, ncell = coords.device, nc[0] * nc[1] * nc[2]
    if coords.shape[0] == 0:
        return torch.full((ncell,), -1, dtype=torch.int32, device=dev), torch.zeros(0, 4, dtype=torch.int32, device=dev), 0, nc
    grid = torch.empty(ncell, dtype=torch.int32, device=dev)
    cc = torch.empty(ncell, 4, dtype=torch.int32, device=dev)
    n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    ws, wsb = _scratch("o2345_sparse_downsample_workspace_bytes", nc, dev)
    call("o2345_sparse_downsample", coords, coords.shape[0], int(ts), nc[0], nc[1], nc[2], grid, cc, n_dev, ws, wsb)
    n = int(n_dev.item())
    return grid, cc[:n], n, nc


@_on_device
def sparse_conv3d(mode, x, in_grid, in_cells, out_coords, ts_out, kernel):
    n_out, cin, cout = out_coords.shape[0], x.shape[1], kernel.shape[2]
    out = torch.empty(n_out, cout, dtype=torch.float32, device=x.device)
    if n_out == 0 or x.shape[0] == 0:
        return out.zero_()
    call("o2345_sparse_conv3d", int(mode), x, cin, in_grid, in_cells[0], in_cells[1], in_cells[2], out_coords, n_out, int(ts_out), kernel, cout, out)
    return out


@_on_device
def sparse_conv3d_x3(mode, x, in_grid, in_cells, out_coords, ts_out, wblob, cout, identity_rows=False):
    """Matrix-core form of sparse_conv3d (csrc/sparse_mfma.hip); wblob = weights.pack_sparse_conv_x3(kernel) on the device.
    identity_rows=True (mode 0): the caller guarantees out_coords IS the coordinate list in_grid was built from, in the same order (a stride-1
    spnn.Conv3d) -- the precondition of the LDS-tiled brick kernel (32 -> 16 channels), which never reads out_coords.  Default: the gather form,
    correct for any subset / order of out_coords."""
    n_out, cin = out_coords.shape[0], x.shape[1]
    out = torch.empty(n_out, cout, dtype=torch.float32, device=x.device)
    if n_out == 0 or x.shape[0] == 0:
        return out.zero_()
    if identity_rows and (int(mode) != 0 or n_out != x.shape[0]):
        raise ValueError(f"sparse_conv3d_x3: identity_rows needs mode 0 and one output row per input row (mode {mode}, {n_out} vs {x.shape[0]} rows)")
    call("o2345_sparse_conv3d_x3", int(mode), x, cin, in_grid, in_cells[0], in_cells[1], in_cells[2], out_coords, n_out, int(ts_out), wblob, int(cout),
         int(bool(identity_rows)), out)
    return out


@_on_device
def bn_act_rows(x, gamma, beta, eps=1e-5, slope=0.0, abs_gamma=False, skip=None, want_stats=False):
    n, C = x.shape
    y = torch.empty_like(x)
    if n == 0:
        return (y, torch.zeros(2, C, device=x.device)) if want_stats else y
    ws, wsb = _scratch("o2345_bn_workspace_bytes", (C,), x.device, "bn")
    mv = torch.empty(2, C, dtype=torch.float32, device=x.device) if want_stats else None
    call("o2345_bn_act_rows", x, n, C, gamma, beta, float(eps), float(slope), int(abs_gamma), skip, y, mv, ws, wsb)
    return (y, mv) if want_stats else y


@_on_device
def abn_nchw(x, gamma, beta, eps=1e-5, slope=0.01, abs_gamma=True, want_nchw=True, want_nhwc=False):
    V, C, H, W = x.shape
    ws, wsb = _scratch("o2345_abn_workspace_bytes", (C,), x.device, "abn")
    y1 = torch.empty_like(x) if want_nchw else None
    y2 = torch.empty(V, H, W, C, dtype=torch.float32, device=x.device) if want_nhwc else None
    call("o2345_abn_nchw", x, V, C, H, W, gamma, beta, float(eps), float(slope), int(abs_gamma), y1, y2, ws, wsb)
    return y1, y2


# ---------------------------------------------------------------------------------------------------------- SDF network
@_on_device
def sdf_grid_tables(tab_axes, bias_lane_order):
    """(tab_axes [3,R,128], bias [128]) from weights.sdf_grid_tables, on the device -> (tab_xy [R*R,128] = x + y + bias, tab_z [R,128])."""
    R = tab_axes.shape[1]
    tab_xy = torch.empty(R * R, 128, dtype=torch.float32, device=tab_axes.device)
    call("o2345_sdf_grid_tables", tab_axes, bias_lane_order, R, tab_xy)
    return tab_xy, tab_axes[2]


@_on_device
def sdf_mlp(blob, vol_cl, pts=None, variant=0, grid_R=0, sign=1.0, index=None, n_dev=None, want_lat=False, out=None, lat_in=None,
            precision=None, grid_tables=None, maskvol=None, grid_background=None):
    """variant 0: sdf; 1: sdf + 128 features; 2: sdf + gradient.  pts [P,3] or grid_R.  lat_in [P,16]: given latents instead of
    sampling the volume (get_sdf_volume).  precision "f16x3" (default): split-f16 MFMA at fp32-class accuracy (variants 0 and 2; variant 1 / lat_in
    run on the fp32 kernel); "fp32": the exact fp32 MFMA kernels.  grid_tables (f16x3, variant 0, lattice mode): (tab_xy, tab_z) from
    ops.sdf_grid_tables -- layer 0 read from per-axis tables instead of being evaluated per point.
    maskvol [D^3] + grid_background [R^3] (with grid_tables only; both or neither): the lattice is evaluated only where the scene has a latent
    (o2345_sdf_grid_sparse_x3).  The caller guarantees that vol_cl is zero wherever maskvol is zero (ops.scatter_dense's pair) and that grid_background
    is this call's own result with sign = +1 on a volume of zeros (pipeline.SceneWeights.grid_background); the result is the full evaluation's bit for
    bit.  Every other form -- the fp32 lattice mode (k_sdf_mlp<0>) among them -- keeps the full evaluation and rejects the two arguments.
    Returns dict of tensors."""
    precision = config.sdf_precision(precision)
    D = vol_cl.shape[0]
    dev = vol_cl.device
    if pts is not None:
        P = pts.shape[0]
    else:
        P = int(grid_R) ** 3
    n = P if index is None else index.shape[0]
    res = out or {}
    if "sdf" not in res:
        res["sdf"] = torch.empty(P, dtype=torch.float32, device=dev)
    if variant == 1 and "feat" not in res:
        res["feat"] = torch.empty(P, 128, dtype=torch.float32, device=dev)
    if variant == 2 and "grad" not in res:
        res["grad"] = torch.empty(P, 3, dtype=torch.float32, device=dev)
    if want_lat and "lat" not in res:
        res["lat"] = torch.empty(P, 16, dtype=torch.float32, device=dev)
    sparse = maskvol is not None or grid_background is not None
    if sparse and not (maskvol is not None and grid_background is not None and precision == "f16x3" and variant == 0 and not want_lat and lat_in is None
                       and grid_tables is not None and pts is None and index is None and n_dev is None):
        raise ValueError("sdf_mlp: maskvol and grid_background come together and with grid_tables only (f16x3, variant 0, the whole lattice)")
    if P == 0 or (n == 0 and n_dev is None):
        return res
    if precision == "f16x3" and variant == 0 and not want_lat and lat_in is None:
        if grid_tables is not None and pts is None and index is None and n_dev is None:
            tab_xy, tab_z = grid_tables                  # lattice mode with layer 0 tabulated (weights.sdf_grid_tables + ops.sdf_grid_tables)
            if tuple(tab_xy.shape) != (int(grid_R) ** 2, 128) or tuple(tab_z.shape) != (int(grid_R), 128):
                raise ValueError(f"sdf_mlp: grid tables were built for another resolution than {grid_R}")
            if sparse:
                if maskvol.numel() != D ** 3 or grid_background.numel() != P or P >= 2 ** 31:
                    raise ValueError(f"sdf_mlp: maskvol [{D}^3] and grid_background [{grid_R}^3 < 2^31] expected, got {maskvol.numel()} and "
                                     f"{grid_background.numel()} elements")
                ws, wsb = _scratch("o2345_sdf_grid_sparse_workspace_bytes", (int(grid_R),), dev, "sdf_grid_sparse")
                call("o2345_sdf_grid_sparse_x3", blob, vol_cl, maskvol, D, int(grid_R), float(sign), tab_xy, tab_z, grid_background, res["sdf"], ws, wsb)
            else:
                call("o2345_sdf_grid_x3", blob, vol_cl, D, int(grid_R), float(sign), tab_xy, tab_z, res["sdf"])
        else:
            call("o2345_sdf_mlp_x3", blob, vol_cl, D, pts, index, n_dev, n, int(grid_R), float(sign), res["sdf"])
    elif precision == "f16x3" and variant == 2 and not want_lat and lat_in is None:
        call("o2345_sdf_grad_x3", blob, vol_cl, D, pts, index, n_dev, n, int(grid_R), float(sign), res["sdf"], res["grad"])
    else:
        call("o2345_sdf_mlp_ex", int(variant), blob, vol_cl, D, pts, index, n_dev, n, int(grid_R), float(sign), lat_in, res["sdf"], res.get("feat"),
             res.get("lat"), res.get("grad"))
    return res


def sdf_grid_active_points(device):
    """Lattice slots that the last sdf_mlp(..., maskvol=, grid_background=) call on the current stream of ``device`` listed for evaluation (32 per active
    tile), read from the device-side count in its workspace, or None before any such call.  Synchronises: for tests and profiling notes."""
    with torch.cuda.device(device):
        ws = _workspace(None, torch.device(device), "sdf_grid_sparse")
    return None if ws is None else int(ws[:4].view(torch.int32).item())


# ---------------------------------------------------------------------------------------------------------- colour
@_on_device
def pack_color_maps(feat_nchw, color_nchw):
    V, _, H, W = feat_nchw.shape
    out = torch.empty(V, H, W, 64, dtype=torch.float32, device=feat_nchw.device)
    call("o2345_pack_color_maps", feat_nchw, color_nchw, V, H, W, out)
    return out


@_on_device
def camera_terms(intrinsics, w2cs):
    """intrinsics [V,3,3], w2cs [V,4,4] -> (proj [V,3,4] = K @ w2c[:3] (render_utils.py:106), cam_pos [V,3] = inverse(w2c)[:3, 3]) in one launch --
    no BLAS / solver library (the first torch.matmul + torch.inverse of a process initialise rocBLAS and rocSOLVER: 180 ms)."""
    V = intrinsics.shape[0]
    if tuple(intrinsics.shape) != (V, 3, 3) or tuple(w2cs.shape) != (V, 4, 4):
        raise ValueError(f"camera_terms: intrinsics [V,3,3] and w2cs [V,4,4] expected, got {tuple(intrinsics.shape)}, {tuple(w2cs.shape)}")
    proj = torch.empty(V, 3, 4, dtype=torch.float32, device=w2cs.device)
    cam = torch.empty(V, 3, dtype=torch.float32, device=w2cs.device)
    call("o2345_camera_terms", _f(intrinsics), _f(w2cs), V, proj, cam)
    return proj, cam


def color_stats_buffer(device):
    """Zeroed work counters [4] (int64 on the device) for ``color_points(..., stats=buf)`` / ``render_rays(..., color_stats=buf)``: the launches ADD
    (32-point tile, view) pairs evaluated in the pooling pass / the network pass, tiles, tiles that evaluated every view.  Caller-owned: no library state."""
    return torch.zeros(4, dtype=torch.int64, device=device)


def tile_queue_buffer(device):
    """Eight int32 on the device for ``color_points(..., tile_queue=buf)``: the heads of the launch's tile queue
    (csrc/common.h).  The call clears them on its stream; a buffer serves one launch at a time."""
    return torch.empty(8, dtype=torch.int32, device=device)


def _tile_queue(buf):
    if buf.dtype != torch.int32 or buf.numel() < 8 or not buf.is_contiguous():
        raise ValueError("tile_queue: 8 contiguous int32 on the device expected (ops.tile_queue_buffer)")
    return buf


def color_stats_read(buf):
    out = [int(x) for x in buf.cpu().tolist()]
    return dict(pairs_pooling=out[0], pairs_network=out[1], tiles=out[2], tiles_all_views=out[3])


@_on_device
def color_points(blob, vol_cl, maskvol, cmaps, proj, cam_pos, pts, query_cam=None, normals=None, index=None, n_dev=None,
                 want_nviews=True, mfma="x3", stats=None, tile_queue=None, out=None):
    """Projector + GeneralRenderingNetwork fused (k_color_pts).  mfma="x3": split-f16 matrix steps (blob from weights.pack_color_x3_blob, the default
    numerical mode); mfma=True: fp32 matrix-core form (pack_color_mfma_blob).  Any view count from 1 to 255 (nviews is uint8; 0 and 256 raise), in three
    regimes with the same results: up to 32 views render_rays groups its point list by visibility before this kernel (list_sort_by_visibility, which
    refuses more), up to 64 the kernel skips the views that see none of a tile's 32 points (a 64-bit mask of active views), from 65 on it evaluates
    every (tile, view) pair -- tests/test_gpu_many_views.py runs V = 33, 64, 65 and 255.  stats: color_stats_buffer().
    tile_queue: tile_queue_buffer() -- the tail of the tile list is claimed by the waves that finish first (the _q entry points); same results bit for
    bit.  out: (rgb [P,3] float32, nviews [P] uint8 or None) to write into instead of fresh zeroed tensors (slots not listed stay untouched)."""
    if mfma is False or mfma is None:
        raise ValueError("color_points: the pure-VALU colour kernel was removed in ABI 2.0; pass mfma='x3' (split-f16) or mfma=True (fp32 MFMA)")
    V, H, W, _ = cmaps.shape
    P = pts.shape[0]
    n = P if index is None else index.shape[0]
    if out is not None:
        rgb, nv = out
        if tuple(rgb.shape) != (P, 3) or rgb.dtype != torch.float32 or (nv is not None and (tuple(nv.shape) != (P,) or nv.dtype != torch.uint8)):
            raise ValueError(f"color_points: out = (rgb [{P},3] float32, nviews [{P}] uint8 or None) expected")
    else:
        rgb = torch.zeros(P, 3, dtype=torch.float32, device=pts.device)
        nv = torch.zeros(P, dtype=torch.uint8, device=pts.device) if want_nviews else None
    if P == 0 or (n == 0 and n_dev is None):
        return rgb, nv
    entry = "o2345_color_points_x3" if mfma == "x3" else "o2345_color_points_mfma"
    if tile_queue is not None:
        call(entry + "_q", blob, vol_cl, maskvol, vol_cl.shape[0], cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, rgb, nv, stats,
             _tile_queue(tile_queue))
    else:
        call(entry, blob, vol_cl, maskvol, vol_cl.shape[0], cmaps, proj, cam_pos, V, H, W, pts, index, n_dev, n, query_cam, normals, rgb, nv, stats)
    return rgb, nv


@_on_device
def project_features(vol_cl, maskvol, cmaps, proj, cam_pos, pts, query_cam=None, normals=None):
    """Projector.compute (query_cam) / compute_view_independent (normals) materialised in the reference's layout:
    -> geometry_feat [P,16], rgb_feat [V,P,59], ray_diff [V,P,4], mask [V,P] (1 / 0)."""
    V, H, W, _ = cmaps.shape
    P = pts.shape[0]
    dev = pts.device
    geo = torch.empty(P, 16, dtype=torch.float32, device=dev)
    rf = torch.empty(V, P, 59, dtype=torch.float32, device=dev)
    rd = torch.empty(V, P, 4, dtype=torch.float32, device=dev)
    m = torch.empty(V, P, dtype=torch.float32, device=dev)
    call("o2345_project_features", vol_cl, maskvol, vol_cl.shape[0], cmaps, proj, cam_pos, V, H, W, pts, P, query_cam, normals, geo, rf, rd, m)
    return geo, rf, rd, m


@_on_device
def color_from_features(blob, geometry_feat, rgb_feat, ray_diff, mask, x3=True, want_nviews=True):
    """GeneralRenderingNetwork.forward on materialised tensors in the reference's layout: geometry_feat [P,16], rgb_feat [V,P,59],
    ray_diff [V,P,4], mask [V,P] -> (rgb [P,3], valid views uint8 [P]).  blob: pack_color_x3_blob (x3) or pack_color_mfma_blob."""
    V, P, C = rgb_feat.shape
    if C != 59 or tuple(geometry_feat.shape) != (P, 16) or tuple(ray_diff.shape) != (V, P, 4) or tuple(mask.shape) != (V, P):
        raise ValueError(f"color_from_features: expected geometry_feat [P,16], rgb_feat [V,P,59], ray_diff [V,P,4], mask [V,P]; got "
                         f"{tuple(geometry_feat.shape)}, {tuple(rgb_feat.shape)}, {tuple(ray_diff.shape)}, {tuple(mask.shape)}")
    rgb = torch.empty(P, 3, dtype=torch.float32, device=rgb_feat.device)
    nv = torch.empty(P, dtype=torch.uint8, device=rgb_feat.device) if want_nviews else None
    if P:
        call("o2345_color_from_features", blob, int(bool(x3)), _f(geometry_feat), _f(rgb_feat), _f(ray_diff), _f(mask), V, P, rgb, nv)
    return rgb, nv


@_on_device
def view_count(pts, maskvol, D, proj, V, H, W):
    out = torch.empty(pts.shape[0], dtype=torch.uint8, device=pts.device)
    call("o2345_view_count", pts, pts.shape[0], maskvol, D, proj, V, H, W, out)
    return out


@_on_device
def list_sort_by_visibility(pts, index, proj, H, W, count=None, want_keys=False):
    """index [n] int32 slots into pts [P,3] -> the same entries grouped, stably, by view-visibility signature (what o2345_render_rays does to its
    occupied-point list before the network kernels; csrc/list_sort.hip).  count (optional int32[1] on the device): number of valid entries."""
    n = int(index.shape[0])
    V = int(proj.shape[0])
    out = torch.empty_like(index)
    if n == 0:
        return (out, torch.empty(0, dtype=torch.int32, device=index.device)) if want_keys else out
    if count is None:
        count = torch.tensor([n], dtype=torch.int32, device=index.device)
    keys = torch.empty(n, dtype=torch.int32, device=index.device) if want_keys else None
    ws, wsb = _scratch("o2345_list_sort_workspace_bytes", (n, V), index.device, "lsort")
    call("o2345_list_sort_by_visibility", pts, index, count, n, proj, V, int(H), int(W), out, keys, ws, wsb)
    return (out, keys) if want_keys else out


# ---------------------------------------------------------------------------------------------------------- rays
_SCENE_KEYS = ("sdf_blob", "vol_cl", "maskvol", "cmaps", "proj", "cam_pos")


def _color_network(scene, what):
    """-> (entry point's name, blob) of the colour network the scene's precision selects: o2345_color_points_x3 with color_x3_blob in f16x3 mode (when
    the scene has that blob), else o2345_color_points_mfma with color_mfma_blob."""
    xb, mb = scene.get("color_x3_blob"), scene.get("color_mfma_blob")
    if xb is not None and config.color_precision(scene.get("color_precision")) == "f16x3":
        return "o2345_color_points_x3", xb
    if mb is None:
        raise ValueError(f"{what}: scene needs color_x3_blob (f16x3 mode) or color_mfma_blob (fp32 mode)")
    return "o2345_color_points_mfma", mb


@_on_device
def render_rays(scene, rays_o, rays_d, near, far, n_samples=64, n_importance=64, inv_s=None, alpha_inter_ratio=1.0,
                background=1.0, query_cam=None, want_z=False, t_rand=None, sample_dist=None, want_scalars=False, color_stats=None,
                weight_cull=None, segment_rays=0):
    """scene: dict(sdf_blob, color_x3_blob and / or color_mfma_blob, vol_cl, maskvol [D^3], cmaps, proj [V,3,4], cam_pos [V,3]).
    near / far: python floats, or two float32 tensors [R] on the device (the reference's per-ray [N_rays, 1] form; then ``sample_dist`` =
    ((far - near) / n_samples).mean() must be given, sparse_neus_renderer.py:484).
    t_rand [R, n_samples] (optional): the reference's stratified jitter of the coarse samples (perturb > 0, :506-515), drawn by the caller.
    want_scalars: also ``scalars`` [4] = (alpha_sum.mean(), alpha_sum.sum() / (R S), gradient error, evaluated points).  color_stats: color_stats_buffer().
    weight_cull (None: config.weight_cull(), default 2^-24; 0: exhaustive like the reference): the colour network is evaluated only on occupied samples whose
    compositing weight is >= weight_cull -- a ray's colour moves by <= (n_samples + n_importance) * weight_cull (include/o2345.h, O2345RenderIO.weight_cull).
    segment_rays (0: one render() call): the rays are consecutive render() calls of that many rays evaluated together (O2345RenderIO.segment_rays).
    Returns dict of SAMPLE-MAJOR tensors ([S,R,...]) + per-ray results."""
    R = rays_o.shape[0]
    if query_cam is None:
        raise ValueError("render_rays: query_cam [3] (the query camera centre, query_c2w[:3, 3]) is required")
    if inv_s is None:
        raise ValueError("render_rays: inv_s is required")
    if rays_d.shape != rays_o.shape or rays_o.dim() != 2 or rays_o.shape[1] != 3:
        raise ValueError(f"render_rays: rays_o / rays_d must both be [R,3] (got {tuple(rays_o.shape)}, {tuple(rays_d.shape)})")
    if (n_samples + n_importance) * R >= 2 ** 31:
        raise ValueError("render_rays: R * (n_samples + n_importance) must stay below 2^31; split the ray batch")
    dev = rays_o.device
    io = _lib.RenderIO()
    for k in _SCENE_KEYS:
        io.point(**{k: scene[k]})                      # contiguous cuda float32, or ValueError
        if scene[k].device != dev:
            raise ValueError(f"render_rays: scene[{k!r}] is on {scene[k].device}, the rays on {dev}")
    Dv = scene["vol_cl"].shape[0]
    cm = scene["cmaps"]
    if scene["vol_cl"].dim() != 4 or scene["maskvol"].numel() != Dv ** 3 or cm.dim() != 4 or cm.shape[-1] != 64:
        raise ValueError("render_rays: vol_cl [D,D,D,C], maskvol [D^3], cmaps [V,H,W,64] expected")
    V, H, W, _ = cm.shape
    if tuple(scene["proj"].shape) != (V, 3, 4) or tuple(scene["cam_pos"].shape) != (V, 3):
        raise ValueError("render_rays: proj [V,3,4] and cam_pos [V,3] must match the V of cmaps")
    if t_rand is not None and tuple(t_rand.shape) != (R, n_samples):
        raise ValueError(f"render_rays: t_rand must be [R, n_samples] = {(R, n_samples)}, got {tuple(t_rand.shape)}")
    S = n_samples + n_importance
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    o = dict(mid_z=f(S, R), dists=f(S, R), pm=f(S, R), sdf=f(S, R), grad=f(S, R, 3), rgb=f(S, R, 3),
             nviews=torch.empty(S, R, dtype=torch.uint8, device=dev), color=f(R, 3), depth=f(R), weights=f(S, R), cdf=f(S, R),
             weights_sum=f(R), weights_max=f(R), depth_var=f(R), alpha_sum=f(R), grad_err=f(R, 2),
             color_mask=torch.empty(R, dtype=torch.uint8, device=dev))
    if want_z:
        o["z_vals"] = f(S, R)
    segment_rays = int(segment_rays)
    if segment_rays < 0 or segment_rays % 64:
        raise ValueError(f"render_rays: segment_rays must be 0 or a multiple of 64, got {segment_rays}")
    n_seg = (R + segment_rays - 1) // segment_rays if segment_rays else 0
    if want_scalars:
        o["scalars"] = f(n_seg, 4) if segment_rays else f(4)
    entry, blob = _color_network(scene, "render_rays")
    io.point(color_x3_blob=blob if entry == "o2345_color_points_x3" else None, color_mfma_blob=scene.get("color_mfma_blob"), t_rand=t_rand,
             rays_o=rays_o, rays_d=rays_d, query_cam=query_cam, color_stats=color_stats, **o)         # z_vals / scalars stay NULL unless asked for
    io.sdf_mode = 2 if config.sdf_precision(scene.get("sdf_precision")) == "f16x3" else 0
    io.D, io.V, io.H, io.W, io.R = Dv, V, H, W, R
    if torch.is_tensor(near) or torch.is_tensor(far):
        if not (torch.is_tensor(near) and torch.is_tensor(far)) or near.numel() != R or far.numel() != R or sample_dist is None:
            raise ValueError("render_rays: per-ray near / far are two tensors of R elements, and sample_dist must be given")
        io.point(near_ray=near, far_ray=far)                   # near = far = 0.0, as the fresh struct has them
    else:
        io.near, io.far = float(near), float(far)
    io.sample_dist = float(sample_dist) if sample_dist is not None else 0.0
    io.n_samples, io.n_importance = n_samples, n_importance
    io.inv_s, io.alpha_inter_ratio, io.background = float(inv_s), float(alpha_inter_ratio), float(background)
    io.weight_cull = float(config.weight_cull(scene.get("weight_cull") if weight_cull is None else weight_cull))
    io.segment_rays = int(segment_rays)
    ws, wsb = _scratch("o2345_render_workspace_bytes", (R, n_samples, n_importance, V), dev, "render")
    call("o2345_render_rays", io, ws, wsb)
    return o


@_on_device
def ray_coarse(rays_o, rays_d, near, far, n_samples, t_rand=None):
    """Stage entry points of the coarse samples (sparse_neus_renderer.py:486-515): z = near + (far - near) * linspace(0, 1, n_samples), with the
    stratified jitter t_rand [R, n_samples] (ray-major, what torch.rand(z_vals.shape) returns) when given.  near / far: python floats
    (o2345_ray_coarse, o2345_ray_coarse_jitter), or two float32 tensors [R] on the device (o2345_ray_coarse_per_ray).
    -> (z SAMPLE-MAJOR [n_samples,R], pts [n_samples,R,3])."""
    if rays_d.shape != rays_o.shape or rays_o.dim() != 2 or rays_o.shape[1] != 3:
        raise ValueError(f"ray_coarse: rays_o / rays_d must both be [R,3] (got {tuple(rays_o.shape)}, {tuple(rays_d.shape)})")
    R, S = rays_o.shape[0], int(n_samples)
    if S < 2:
        raise ValueError(f"ray_coarse: at least 2 samples per ray (got {S})")
    if t_rand is not None and tuple(t_rand.shape) != (R, S):
        raise ValueError(f"ray_coarse: t_rand must be [R, n_samples] = {(R, S)}, got {tuple(t_rand.shape)}")
    dev = rays_o.device
    z = torch.empty(S, R, dtype=torch.float32, device=dev)
    pts = torch.empty(S, R, 3, dtype=torch.float32, device=dev)
    if torch.is_tensor(near) or torch.is_tensor(far):
        if not (torch.is_tensor(near) and torch.is_tensor(far)) or near.numel() != R or far.numel() != R:
            raise ValueError("ray_coarse: per-ray near / far are two tensors of R elements")
        call("o2345_ray_coarse_per_ray", rays_o, rays_d, R, near, far, S, t_rand, z, pts)
    elif t_rand is not None:
        call("o2345_ray_coarse_jitter", rays_o, rays_d, R, float(near), float(far), S, t_rand, z, pts)
    else:
        call("o2345_ray_coarse", rays_o, rays_d, R, float(near), float(far), S, z, pts)
    return z, pts


@_on_device
def ray_merge(z, sdf, new_z, new_sdf):
    """Stage entry point of cat_z_vals' merge (sparse_neus_renderer.py:139-149): the sorted lists z, sdf SAMPLE-MAJOR [S,R] and a block of new samples
    new_z, new_sdf [n_new,R] in any order -> (z, sdf) [S + n_new,R], a stable merge in which, among equal depths, existing samples stay in front of
    new ones.  The arguments are left as they are."""
    if z.dim() != 2 or sdf.shape != z.shape or new_z.dim() != 2 or new_sdf.shape != new_z.shape or new_z.shape[1] != z.shape[1]:
        raise ValueError(f"ray_merge: z / sdf [S,R] and new_z / new_sdf [n_new,R] expected (got {tuple(z.shape)}, {tuple(sdf.shape)}, "
                         f"{tuple(new_z.shape)}, {tuple(new_sdf.shape)})")
    (S, R), n_new = z.shape, new_z.shape[0]
    if S < 1 or n_new < 1 or R < 1:
        raise ValueError(f"ray_merge: at least one ray, one sample and one new sample (got R = {R}, S = {S}, n_new = {n_new})")
    _lib.bind("o2345_ray_merge", (R, z, sdf, S, new_z, new_sdf, n_new, None))          # the merge runs in place on copies: refuse bad originals before copying
    zm = torch.cat([z, torch.zeros_like(new_z)], 0)           # capacity S + n_new: merged in place
    sm = torch.cat([sdf, torch.zeros_like(new_sdf)], 0)
    nz, ns = new_z.clone(), new_sdf.clone()
    call("o2345_ray_merge", R, zm, sm, S, nz, ns, n_new)
    return zm, sm


@_on_device
def ray_upsample(rays_o, rays_d, z, sdf, inv_s, maskvol, D, n_imp, streaming=None, want_weights=False):
    """Stage entry point of the hierarchical sampler (up_sample + sample_pdf, sparse_neus_renderer.py:73-115, render_utils.py:8-51):
    z, sdf SAMPLE-MAJOR [S,R] -> (new_z [n_imp,R], new_pts [n_imp,R,3], valid-point list int32 [<= n_imp*R] of slots t*R + r).
    want_weights: also the scratch rows [S-1,R] -- the streaming kernel leaves its section weights alpha * T + 1e-5 there (sample_pdf's
    `weights + 1e-5`); the sixteen-lane kernel keeps them in LDS and does not write the rows."""
    S, R = z.shape
    dev = z.device
    if want_weights and streaming is False:
        raise ValueError("ray_upsample: want_weights needs the scratch rows (streaming=False hands none over)")
    # streaming=None: scratch is handed over and the library picks the kernel by R (O2345_RAY_STREAM_MIN); False: no scratch -> the LDS-staged kernel
    wbuf = None if streaming is False else torch.empty(S, R, dtype=torch.float32, device=dev)
    new_z = torch.empty(n_imp, R, dtype=torch.float32, device=dev)
    new_pts = torch.empty(n_imp, R, 3, dtype=torch.float32, device=dev)
    new_sdf = torch.empty(n_imp, R, dtype=torch.float32, device=dev)
    lst = torch.empty(n_imp * R, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    call("o2345_ray_upsample", rays_o, rays_d, R, z, sdf, S, float(inv_s), maskvol, int(D), wbuf, int(n_imp), new_z, new_pts, new_sdf, lst, cnt)
    if want_weights:
        return new_z, new_pts, lst[:int(cnt.item())], wbuf[:S - 1]
    return new_z, new_pts, lst[:int(cnt.item())]


@_on_device
def ray_finalize(rays_o, rays_d, z, sample_dist, maskvol, D):
    """Stage entry point of render_core's head (sparse_neus_renderer.py:204-231): z SAMPLE-MAJOR [S,R] -> dict(mid_z, dists, pm [S,R], pts [S,R,3],
    sdf [S,R] = 100, grad / rgb [S,R,3] = 0 (the reference's defaults in EVERY slot), list int32 (occupied slots s*R + r, wave-major), count)."""
    S, R = z.shape
    dev = z.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    o = dict(mid_z=f(S, R), dists=f(S, R), pts=f(S, R, 3), pm=f(S, R), sdf=f(S, R), grad=f(S, R, 3), rgb=f(S, R, 3),
             list=torch.empty(S * R, dtype=torch.int32, device=dev), count=torch.zeros(1, dtype=torch.int32, device=dev))
    call("o2345_ray_finalize", rays_o, rays_d, R, z, S, float(sample_dist), maskvol, int(D), o["mid_z"], o["dists"], o["pts"], o["pm"], o["sdf"], o["grad"],
         o["rgb"], o["list"], o["count"])
    return o


@_on_device
def ray_composite(rays_o, rays_d, mid_z, dists, pm, sdf, grad, rgb, nviews, inv_s, alpha_inter_ratio=1.0, background=1.0):
    """Stage entry point of render_core's tail (sparse_neus_renderer.py:340-455): NeuS opacities from (sdf, gradient, section length), transmittance,
    weights, colour / depth / depth variance, the per-ray colour mask (> 8 samples seen by >= 2 views).  Per-sample inputs SAMPLE-MAJOR [S,R(,3)],
    nviews uint8 [S,R].  -> dict(color [R,3], depth, weights_sum, weights_max, depth_var, alpha_sum [R], grad_err [R,2], color_mask uint8 [R],
    weights / cdf [S,R])."""
    S, R = mid_z.shape
    dev = mid_z.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    o = dict(color=f(R, 3), depth=f(R), weights=f(S, R), cdf=f(S, R), weights_sum=f(R), weights_max=f(R), depth_var=f(R), alpha_sum=f(R),
             grad_err=f(R, 2), color_mask=torch.empty(R, dtype=torch.uint8, device=dev))
    call("o2345_ray_composite", rays_o, rays_d, R, S, mid_z, dists, pm, sdf, grad, rgb, nviews, float(inv_s), float(alpha_inter_ratio), float(background),
         o["color"], o["depth"], o["weights"], o["cdf"], o["weights_sum"], o["weights_max"], o["depth_var"], o["alpha_sum"], o["grad_err"], o["color_mask"])
    return o


@_on_device
def render_core(scene, rays_o, rays_d, z, sample_dist, inv_s, alpha_inter_ratio=1.0, background=1.0, query_cam=None):
    """The reference's render_core (sparse_neus_renderer.py:171-455) on GIVEN sample depths ``z`` SAMPLE-MAJOR [S,R] -- everything of a render() call that
    lies downstream of the hierarchical sampler, composed from the public stage entries in the order o2345_render_rays runs them: o2345_ray_finalize
    (mid points, section lengths, occupancy, defaults, occupied-point list; the "first 100 points" rule of :222-223 when no point is occupied) ->
    SDF + analytic gradient on the listed points -> valid-view counts of the unlisted points -> Projector + GeneralRenderingNetwork on the listed points
    -> o2345_ray_composite.  scene: the dict of render_rays.  -> dict: render_rays' per-sample / per-ray keys (+ ``list``)."""
    S, R = z.shape
    D = scene["vol_cl"].shape[0]
    V, H, W, _ = scene["cmaps"].shape
    o = ray_finalize(rays_o, rays_d, z, sample_dist, scene["maskvol"], D)
    n = int(o["count"])                                        # (a stage composition on the host: one read-back; o2345_render_rays keeps the count on the device)
    if n < 1:                                                  # :222-223 -- the first 100 points in the reference's ray-major order: point t = (ray t // S, sample t % S)
        n = min(100, S * R)
        t = torch.arange(n, dtype=torch.int32, device=z.device)
        o["list"][:n] = (t % S) * R + t // S
    lst = o["list"][:n].contiguous()
    pts = o["pts"].view(-1, 3)
    sdf_precision = config.sdf_precision(scene.get("sdf_precision"))
    res = {"sdf": o["sdf"].view(-1), "grad": o["grad"].view(-1, 3)}
    sdf_mlp(scene["sdf_blob"], scene["vol_cl"], pts, variant=2, index=lst, out=res, precision=sdf_precision)
    nviews = torch.zeros(S * R, dtype=torch.uint8, device=z.device)
    call("o2345_view_count_unlisted", pts, S * R, o["pm"], scene["maskvol"], D, scene["proj"], V, H, W, nviews)
    entry, blob = _color_network(scene, "render_core")
    call(entry, blob, scene["vol_cl"], scene["maskvol"], D, scene["cmaps"], scene["proj"], scene["cam_pos"], V, H, W, pts, lst, None, n, query_cam, None,
         o["rgb"], nviews, None)
    c = ray_composite(rays_o, rays_d, o["mid_z"], o["dists"], o["pm"], o["sdf"], o["grad"], o["rgb"], nviews.view(S, R), inv_s, alpha_inter_ratio, background)
    c.update(mid_z=o["mid_z"], dists=o["dists"], pm=o["pm"], sdf=o["sdf"], grad=o["grad"], rgb=o["rgb"], nviews=nviews.view(S, R), list=lst, z_vals=z)
    return c


# ---------------------------------------------------------------------------------------------------------- marching cubes
def _triangles(tris, what=None):
    """A triangle tensor, validated -> (the tensor, index_bytes) as the library's entries take them (`void* tris`: the width is this check's)."""
    if tris.dtype not in (torch.int32, torch.int64) or tris.dim() != 2 or tris.shape[1] != 3:
        raise ValueError((f"{what}: " if what else "") + f"expected triangles [M,3] int32 or int64, got {tuple(tris.shape)} {tris.dtype}")
    return tris, 8 if tris.dtype == torch.int64 else 4


def _mesh_frame(bound_min, bound_max, scale_mat, trans_mat):
    """Bounds (3 numbers each) and the two 4x4 matrices (tensors, arrays or None) -> four float32 host arrays or None, as the entries take them."""
    mat = lambda a: None if a is None else host_f32(a).reshape(-1, 4, 4)[0].copy()
    return [host_f32(bound_min).reshape(3), host_f32(bound_max).reshape(3), mat(scale_mat), mat(trans_mat)]


@_on_device
def mesh_pack(verts_idx, tris, grid_R, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None, rgb=None):
    """Index-space vertices (fp64 [N,3]) + triangles -> (vertex records uint8 [N,16|12], face records uint8 [M,13]) of a binary PLY;
    frame transforms and colour quantisation as in trainer_generic.py:1365-1377.  Matrices / bounds are small host arrays."""
    dev = verts_idx.device
    n, m = verts_idx.shape[0], tris.shape[0]
    frame = _mesh_frame(bound_min, bound_max, scale_mat, trans_mat)
    vrec = torch.empty(n, 16 if rgb is not None else 12, dtype=torch.uint8, device=dev)
    frec = torch.empty(m, 13, dtype=torch.uint8, device=dev)
    call("o2345_mesh_pack_vertices", verts_idx, n, int(grid_R), *frame, rgb, vrec)
    call("o2345_mesh_pack_faces", *_triangles(tris), m, frec)
    return vrec, frec


@_on_device
def mesh_asset_pack(verts_idx, tris, grid_R, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None, rgb=None, grad=None):
    """Index-space vertices (fp64 [N,3]) + triangles -> the buffers of a GLB / OBJ in the asset frame (utils/utils.py:31-47: (x, y, z) -> (x, z, y),
    faces reversed): (positions float32 [N,3], rgba uint8 [N,4] or None, normals float32 [N,3] or None, indices uint32-valued int32 storage [M,3],
    bounds float32 [2,3] = per-axis min, max of positions), all on the device.  ``rgb`` fp32 [N,3] in [0,1]; ``grad`` fp32 [N,3], the SDF gradient."""
    dev = verts_idx.device
    n, m = verts_idx.shape[0], tris.shape[0]
    frame = _mesh_frame(bound_min, bound_max, scale_mat, trans_mat)
    pos = torch.empty(n, 3, dtype=torch.float32, device=dev)
    rgba = None if rgb is None else torch.empty(n, 4, dtype=torch.uint8, device=dev)
    nrm = None if grad is None else torch.empty(n, 3, dtype=torch.float32, device=dev)
    idx = torch.empty(m, 3, dtype=torch.int32, device=dev)              # uint32 bit patterns (torch has no general uint32): vertex counts stay below 2^31
    bounds = torch.empty(2, 3, dtype=torch.float32, device=dev)
    ws, wsb = _scratch("o2345_mesh_bounds_workspace_bytes", (n,), dev, "mesh_bounds")
    call("o2345_mesh_asset_vertices", verts_idx, n, int(grid_R), *frame, rgb, grad, pos, rgba, nrm, bounds, ws, wsb)
    call("o2345_mesh_asset_indices", *_triangles(tris), m, idx)
    return pos, rgba, nrm, idx, bounds


_obj_tables = {}


def _obj_color_table(device):
    """mesh_io.obj_color_table() (256 x 11 bytes, formatted once on the host) on ``device``, kept per device."""
    key = str(device)
    if key not in _obj_tables:
        _obj_tables[key] = torch.from_numpy(mesh_io.obj_color_table()).to(device)
    return _obj_tables[key]


@_on_device
def obj_text(positions, indices, rgba=None, normals=None, K=None, bounds=None):
    """The buffers of mesh_asset_pack -> the bytes of a Wavefront OBJ (uint8 tensor on the device): fixed-width "v" [+ colour], "vn", "f" records
    (include/o2345.h).  ``K``: integer digits of the coordinate fields; taken from ``bounds`` (one small D2H copy) when not given."""
    n, m = positions.shape[0], indices.shape[0]
    K = _obj_digits(K, bounds, n, "obj_text")
    text = torch.empty(call("o2345_obj_text_bytes", n, m, K, int(rgba is not None), int(normals is not None)), dtype=torch.uint8, device=positions.device)
    table = _obj_color_table(positions.device) if rgba is not None else None
    call("o2345_obj_text", positions, rgba, normals, n, indices, m, K, table, text)
    return text


@_on_device
def mc_verts_to_world(verts_idx, grid_R, bound_min, bound_max):
    """Index-space marching-cubes vertices (fp64 [N,3] on the device) -> world coordinates IN PLACE: v / (R - 1) * (bound_max - bound_min) + bound_min in
    fp64 (sparse_neus_renderer.py:936), the same IEEE expression numpy evaluates on the host.  bound_min / bound_max: three float32 numbers each."""
    b0, b1 = host_f32(bound_min).reshape(3), host_f32(bound_max).reshape(3)
    ext = np.ascontiguousarray((b1 - b0).astype(np.float64))          # the reference subtracts its float32 bound arrays, numpy promotes afterwards
    off = np.ascontiguousarray(b0.astype(np.float64))
    call("o2345_mc_verts_to_world", verts_idx, verts_idx.shape[0], int(grid_R), ext, off)
    return verts_idx


@_on_device
def marching_cubes(u, iso=0.0, index_dtype=torch.int64):
    """u: float32 cuda tensor [n0,n1,n2].  Returns (verts float64 [Nv,3] index coords, tris [Nt,3]) on the device."""
    n0, n1, n2 = u.shape
    ws, wsb = _scratch("o2345_mc_workspace_bytes", (n0, n1, n2), u.device, "mc")
    nv, nt = ctypes.c_longlong(), ctypes.c_longlong()
    call("o2345_marching_cubes_count", u, n0, n1, n2, float(iso), ws, wsb, nv, nt)
    verts = torch.empty(nv.value, 3, dtype=torch.float64, device=u.device)
    tris = torch.empty(nt.value, 3, dtype=index_dtype, device=u.device)
    call("o2345_marching_cubes_emit", u, n0, n1, n2, float(iso), ws, verts, *_triangles(tris))
    return verts, tris


# ---------------------------------------------------------------------------------------------------------- mesh components
def _mesh_components_count(tris, nv, min_faces, keep_largest, labels):
    """Pass 1 of the two-call protocol -> (workspace, components, components_kept, nv_kept, nt_kept)."""
    tris, ib = _triangles(tris)
    nt = tris.shape[0]
    ws, wsb = _scratch("o2345_mesh_components_workspace_bytes", (nv, nt), tris.device, "mesh_components")
    nc, nck, nvk, ntk = (ctypes.c_longlong() for _ in range(4))
    call("o2345_mesh_components_count", tris, ib, nv, nt, min(int(min_faces), 2 ** 31 - 1), int(bool(keep_largest)), ws, wsb, labels, nc, nck, nvk, ntk)
    return ws, nc.value, nck.value, nvk.value, ntk.value


@_on_device
def mesh_component_labels(tris, n_vertices):
    """tris [M,3] int32 / int64 on the device -> int32 [n_vertices]: the smallest vertex index of every vertex's connected component
    (== mesh_io.component_labels, exactly)."""
    labels = torch.empty(int(n_vertices), dtype=torch.int32, device=tris.device)
    _mesh_components_count(tris, int(n_vertices), 0, False, labels)
    return labels


@_on_device
def mesh_filter_components(verts_idx, tris, min_faces=0, keep_largest=False):
    """Drops connected components of a mesh on the device by face count (== mesh_io.filter_components, exactly; definitions in csrc/mesh_components.hip).
    verts_idx fp64 [N,3], tris [M,3] int32 / int64 -> (verts, tris, kept, info): kept vertices / triangles in their original order, triangles renumbered,
    ``kept`` int32 new -> old vertex index (gather any per-vertex attribute with it), ``info`` = {"components", "components_kept"}.
    With nothing selected no kernel is launched: the inputs are returned as they are, ``kept`` and ``info`` are None."""
    min_faces = config.mesh_min_component_faces(min_faces)
    if min_faces == 0 and not keep_largest:
        return verts_idx, tris, None, None
    nv = verts_idx.shape[0]
    ws, nc, nck, nvk, ntk = _mesh_components_count(tris, nv, min_faces, keep_largest, None)
    dev = verts_idx.device
    verts = torch.empty(nvk, 3, dtype=torch.float64, device=dev)
    tris_out = torch.empty(ntk, 3, dtype=tris.dtype, device=dev)
    kept = torch.empty(nvk, dtype=torch.int32, device=dev)
    call("o2345_mesh_components_emit", verts_idx, *_triangles(tris), nv, tris.shape[0], ws, verts, tris_out, kept)
    return verts, tris_out, kept, {"components": nc, "components_kept": nck}


# ---------------------------------------------------------------------------------------------------------- mesh adjacency and smoothing
@_on_device
def mesh_vertex_adjacency(tris, n_vertices):
    """tris [M,3] int32 / int64 on the device -> (offsets int32 [n + 1], neighbours int32 [E], boundary uint8 [n]): the vertex -> neighbours table in CSR
    form, rows ascending, and the flag of the vertices on an edge with one triangle (== mesh_io.vertex_adjacency, exactly; definitions in
    csrc/mesh_smooth.hip)."""
    tris, ib = _triangles(tris)
    nv, nt, dev = int(n_vertices), tris.shape[0], tris.device
    ws, wsb = _scratch("o2345_mesh_adjacency_workspace_bytes", (nv, nt), dev, "mesh_adjacency")
    ne = ctypes.c_longlong()
    call("o2345_mesh_adjacency_count", tris, ib, nv, nt, ws, wsb, ne)
    offsets = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    neighbours = torch.empty(ne.value, dtype=torch.int32, device=dev)
    boundary = torch.empty(nv, dtype=torch.uint8, device=dev)
    call("o2345_mesh_adjacency_emit", ws, nv, offsets, neighbours, boundary)
    return offsets, neighbours, boundary


@_on_device
def mesh_smooth(verts_idx, tris, iterations, lam=None, mu=None, pin_boundary=None):
    """Taubin's lambda|mu smoothing of a mesh's vertex positions on the device (== mesh_io.smooth_vertices, to the last bit; definitions in
    csrc/mesh_smooth.hip).  verts_idx fp64 [N,3], tris [M,3] int32 / int64 -> a new fp64 [N,3] tensor; the input is not written.  ``lam`` / ``mu`` /
    ``pin_boundary``: None = the config default (0.5, -0.53, pinned).  With ``iterations == 0`` nothing is launched and ``verts_idx`` itself is returned."""
    iterations = config.mesh_smooth_iterations(iterations)
    lam, mu, pin = config.mesh_smooth_lambda(lam), config.mesh_smooth_mu(mu), config.mesh_smooth_pin_boundary(pin_boundary)
    if iterations == 0:
        return verts_idx
    if iterations >= 2 ** 30:
        raise ValueError(f"mesh_smooth: {iterations} iterations")
    nv = verts_idx.shape[0]
    offsets, neighbours, boundary = mesh_vertex_adjacency(tris, nv)
    out = torch.empty(nv, 3, dtype=torch.float64, device=verts_idx.device)
    tmp = _workspace(24 * nv, verts_idx.device, "mesh_smooth")
    call("o2345_mesh_smooth", verts_idx, nv, offsets, neighbours, boundary if pin else None, iterations, lam, mu, tmp.view(torch.float64), out)
    return out


# ---------------------------------------------------------------------------------------------------------- mesh decimation
@_on_device
def mesh_decimate(verts_idx, tris, cell=None):
    """Decimation by vertex clustering on the device (== mesh_io.decimate_mesh, to the last bit; definitions in csrc/mesh_decimate.hip).  verts_idx fp64
    [N,3], tris [M,3] int32 / int64, ``cell`` in the units of ``verts_idx`` (None: the config default) -> (verts fp64 [Nc,3], tris [Mk,3] of the same dtype,
    cluster int32 [N]: the new index of every old vertex's cluster or -1, info = {"clusters", "vertices", "triangles", "degenerate", "duplicate"}).  The
    inputs are not written; Nc = 0 and Mk = 0 are legal.  With ``cell == 0`` no kernel is launched: the inputs are returned as they are, ``cluster`` and
    ``info`` are None."""
    cell = config.mesh_decimate_cell(cell)
    if cell == 0.0:
        return verts_idx, tris, None, None
    tris, ib = _triangles(tris)
    _vertices(verts_idx)
    nv, nt, dev = verts_idx.shape[0], tris.shape[0], verts_idx.device
    ws, wsb = _scratch("o2345_mesh_decimate_workspace_bytes", (nv, nt), dev, "mesh_decimate")
    ncl, nvo, nto, ndeg, ndup = (ctypes.c_longlong() for _ in range(5))
    call("o2345_mesh_decimate_count", verts_idx, tris, ib, nv, nt, cell, ws, wsb, ncl, nvo, nto, ndeg, ndup)
    verts = torch.empty(nvo.value, 3, dtype=torch.float64, device=dev)
    tris_out = torch.empty(nto.value, 3, dtype=tris.dtype, device=dev)
    cluster = torch.empty(nv, dtype=torch.int32, device=dev)
    call("o2345_mesh_decimate_emit", verts_idx, tris, ib, nv, nt, ws, verts, tris_out, cluster)
    return verts, tris_out, cluster, {"clusters": ncl.value, "vertices": nvo.value, "triangles": nto.value, "degenerate": ndeg.value, "duplicate": ndup.value}


# ---------------------------------------------------------------------------------------------------------- mesh simplification
_SIMPLIFY_STOPPED = ("target", "blocked", "rounds")              # by O2345_SIMPLIFY_STOPPED_*


def simplify_info(stats):
    """The stats block of o2345_mesh_simplify_count (O2345SimplifyStats and the collapses of every round behind it, on the host) -> the info dict of
    mesh_io.simplify_mesh."""
    st = _lib.read_struct("O2345SimplifyStats", stats)
    collapses = np.frombuffer(stats, np.int64, st.rounds, ctypes.sizeof(st))
    return {"rounds": st.rounds, "vertices": st.vertices, "triangles": st.triangles, "collapses": collapses.tolist(),
            "max_cost": _double_of_bits(st.max_cost_bits), "stopped": _SIMPLIFY_STOPPED[st.stopped]}


@_on_device
def mesh_simplify(verts_idx, tris, target_faces=None, max_error=None, max_rounds=None):
    """Simplification by quadric-error half-edge collapses on the device (== mesh_io.simplify_mesh, to the last bit; definitions in csrc/mesh_simplify.hip).
    verts_idx fp64 [N,3], tris [M,3] int32 / int64; ``target_faces``: at most that many triangles if reachable; ``max_error``: the largest quadric error
    of a collapse (inf: no limit); ``max_rounds``; None: the config defaults -> (verts fp64 [Nk,3], tris [Mk,3] of the same dtype, source int32 [Nk]: new
    -> old vertex index, merged int32 [N]: the new index of the vertex every old vertex ended in or -1, info = {"rounds", "vertices", "triangles",
    "collapses", "max_cost", "stopped"}).  The kept vertices are bit copies; the inputs are not written.  One synchronisation per round.  With a target of
    0 and no error limit the stage is off: no kernel is launched, the inputs are returned as they are, ``source``, ``merged`` and ``info`` are None.  A
    target of 0 WITH an error limit runs until the limit blocks every collapse."""
    target = config.mesh_simplify_faces(target_faces)
    max_error, max_rounds = config.mesh_simplify_max_error(max_error), config.mesh_simplify_max_rounds(max_rounds)
    if target == 0 and max_error == float("inf"):
        return verts_idx, tris, None, None, None
    tris, ib = _triangles(tris)
    _vertices(verts_idx)
    nv, nt, dev = verts_idx.shape[0], tris.shape[0], verts_idx.device
    ws, wsb = _scratch("o2345_mesh_simplify_workspace_bytes", (nv, nt), dev, "mesh_simplify")
    stats = torch.empty(ctypes.sizeof(_lib.STRUCTS["O2345SimplifyStats"]) + 8 * max_rounds, dtype=torch.uint8, device=dev)
    call("o2345_mesh_simplify_count", verts_idx, tris, ib, nv, nt, target, max_error, max_rounds, ws, wsb, stats)
    info = simplify_info(stats.cpu().numpy())
    verts = torch.empty(info["vertices"], 3, dtype=torch.float64, device=dev)
    tris_out = torch.empty(info["triangles"], 3, dtype=tris.dtype, device=dev)
    source = torch.empty(info["vertices"], dtype=torch.int32, device=dev)
    merged = torch.empty(nv, dtype=torch.int32, device=dev)
    call("o2345_mesh_simplify_emit", verts_idx, ib, nv, nt, ws, verts, tris_out, source, merged)
    return verts, tris_out, source, merged, info


# ---------------------------------------------------------------------------------------------------------- mesh projection
@_on_device
def mesh_project(blob, vol_cl, verts_idx, resolution, iterations, level=0.0, tol=None, max_step=None, max_move=None, bound_min=(-1.0, -1.0, -1.0),
                 bound_max=(1.0, 1.0, 1.0), precision=None):
    """Newton projection of mesh vertices onto the level set ``sdf == level`` on the device (== mesh_io.project_vertices with
    ``ops.sdf_mlp(blob, vol_cl, pts, variant=2, precision=precision)`` as its field, to the last bit; definitions in csrc/mesh_project.hip).  verts_idx
    fp64 [N,3] index coordinates on a ``resolution``^3 grid over ``bound_min`` .. ``bound_max``; ``iterations`` in [0, 64] (None: the config default);
    ``tol`` / ``max_step`` / ``max_move`` None: the config defaults -> (verts fp64 [N,3], info = {"evaluated", "converged", "unconverged", "stalled",
    "clamped", "max_before", "max_after"}).  All rounds are queued at once; one small D2H copy of the counters and one synchronisation at the end.  The
    input is not written.  With 0 iterations nothing is launched: ``verts_idx`` itself is returned, and ``info`` is None."""
    iterations = config.mesh_project_iterations(iterations)
    if iterations == 0:
        return verts_idx, None
    tol, max_step, max_move = config.mesh_project_tol(tol), config.mesh_project_max_step(max_step), config.mesh_project_max_move(max_move)
    level = float(level)
    if not np.isfinite(level):
        raise ValueError(f"mesh_project: level must be finite, got {level!r}")
    resolution = _resolution(resolution, "mesh_project")
    _vertices(verts_idx)
    bmin, bmax = _bounds(bound_min, bound_max, "mesh_project")
    mode = 2 if config.sdf_precision(precision) == "f16x3" else 0
    nv, dev = verts_idx.shape[0], verts_idx.device
    ws, wsb = _scratch("o2345_mesh_project_workspace_bytes", (nv,), dev, "mesh_project")
    out = torch.empty(nv, 3, dtype=torch.float64, device=dev)
    stats = _stats_block("O2345ProjectStats", dev)
    call("o2345_mesh_project", blob, vol_cl, vol_cl.shape[0], mode, verts_idx, nv, int(resolution), bmin, bmax, iterations, level, tol, max_step, max_move,
         ws, wsb, out, stats)
    return out, project_info(stats.cpu().numpy(), iterations)


def project_info(stats, iterations):
    """The stats block of o2345_mesh_project (O2345ProjectStats, on the host) -> the info dict of mesh_io.project_vertices; raises on a non-finite coordinate."""
    st = _lib.read_struct("O2345ProjectStats", stats)
    if st.n_nonfinite:
        raise RuntimeError(f"o2345 mesh_project: {st.n_nonfinite} vertices have a non-finite coordinate")
    return {"evaluated": list(st.count[:iterations + 1]), "converged": st.converged, "unconverged": st.unconverged, "stalled": st.stalled,
            "clamped": st.clamped, "max_before": _double_of_bits(st.max_before), "max_after": _double_of_bits(st.max_after)}


def mesh_cleanup(verts_idx, tris, opts, blob, vol_cl, resolution, level=0.0, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), precision=None,
                 project=True):
    """What follows marching cubes, in its one order: component filter -> decimation (the cell in grid spacings) -> simplification (edge collapse down to
    ``opts.simplify_faces`` triangles, error limit and rounds from config) -> Newton projection onto ``sdf == level`` (the field: ``blob``, ``vol_cl``,
    ``precision``), so that a caller's gradient, colours, packing and copies run on the kept, decimated, simplified, projected vertices.  ``opts``: a
    config.MeshOptions; ``project=False`` withholds the projection.  A stage that is off launches nothing and leaves its entry None -> (verts_idx, tris,
    {"components", "components_kept", "decimate", "simplify", "project"})."""
    info = {"components": None, "components_kept": None, "decimate": None, "simplify": None, "project": None}
    if opts.min_component_faces or opts.keep_largest:
        verts_idx, tris, _, cc = mesh_filter_components(verts_idx, tris, opts.min_component_faces, opts.keep_largest)
        info.update(cc)
    if opts.decimate_cell:
        verts_idx, tris, _, info["decimate"] = mesh_decimate(verts_idx, tris, opts.decimate_cell)
    if opts.simplify_faces:
        verts_idx, tris, _, _, info["simplify"] = mesh_simplify(verts_idx, tris, opts.simplify_faces)
    if opts.project_iterations and project:
        verts_idx, info["project"] = mesh_project(blob, vol_cl, verts_idx, resolution, opts.project_iterations, level=level, max_move=opts.project_max_move,
                                                  bound_min=bound_min, bound_max=bound_max, precision=precision)
    return verts_idx, tris, info


# ---------------------------------------------------------------------------------------------------------- mesh-to-mesh distance
_DISTANCE_EXHAUSTIVE_BELOW = 64     # a target with fewer triangles is searched exhaustively: a grid costs more launches than it saves

# a target mesh's uniform grid (ops.mesh_distance_grid): the device buffer, the max_cells it was sized for, and what the count pass reported
MeshGrid = namedtuple("MeshGrid", "buffer max_cells entries dims cell degenerate")


def _distance_spacing(spacing):
    spacing = mesh_io._check_spacing(spacing)
    return 0.0 if spacing is None else spacing


@_on_device
def mesh_surface_samples(verts, tris, spacing=None):
    """Area-weighted samples of a mesh's surface on the device (== mesh_io.surface_samples, to the last bit; definitions in csrc/mesh_distance.hip).  verts
    fp64 [N,3], tris [M,3] int32 / int64, ``spacing`` None (one sample per triangle) or a finite float > 0 -> (points fp64 [n,3], weight fp64 [n], triangle
    int32 [n]), triangle-major.  One synchronisation, for the count; raises on 2^28 samples or more, a non-finite coordinate, an index out of range."""
    spacing = _distance_spacing(spacing)
    tris, ib = _triangles(tris, "mesh_surface_samples")
    _vertices(verts, "mesh_surface_samples")
    nv, nt, dev = verts.shape[0], tris.shape[0], verts.device
    ws, wsb = _scratch("o2345_mesh_samples_workspace_bytes", (nt,), dev, "mesh_samples")
    n = ctypes.c_longlong()
    call("o2345_mesh_samples_count", verts, tris, ib, nv, nt, spacing, ws, wsb, n)
    points = torch.empty(n.value, 3, dtype=torch.float64, device=dev)
    weight = torch.empty(n.value, dtype=torch.float64, device=dev)
    triangle = torch.empty(n.value, dtype=torch.int32, device=dev)
    call("o2345_mesh_samples_emit", verts, tris, ib, nv, nt, ws, n.value, points, weight, triangle)
    return points, weight, triangle


@_on_device
def mesh_distance_grid(verts, tris, cell=None, max_cells=None):
    """The uniform grid over a target mesh that ops.mesh_closest_triangle walks (definitions in csrc/mesh_distance.hip) -> MeshGrid.  ``cell``: the cell
    edge in the units of ``verts`` (None: about as many cells as triangles with an area); ``max_cells`` (None: max(2^20, 2 M), at most 2^24) bounds the
    number of cells, and with it the memory: an edge that would need more, or more than 256 cells along an axis, is enlarged -- ``MeshGrid.cell`` and
    ``.dims`` say what is in use.  The choice changes the speed of a query, never its result.  One synchronisation, for the count; raises on a non-finite
    coordinate, an index out of range, a target without a triangle that has an area."""
    if cell is not None and not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"mesh_distance_grid: cell must be None or a finite float > 0, got {cell!r}")
    tris, ib = _triangles(tris, "mesh_distance_grid")
    _vertices(verts, "mesh_distance_grid")
    nv, nt, dev = verts.shape[0], tris.shape[0], verts.device
    max_cells = min(2 ** 24, max(2 ** 20, 2 * nt)) if max_cells is None else int(max_cells)
    wsb = call("o2345_mesh_distance_grid_workspace_bytes", nt, max_cells)
    if not wsb:
        raise ValueError(f"mesh_distance_grid: bad sizes ({nt} triangles, max_cells = {max_cells}: 1 .. 2^24)")
    ws = _workspace(wsb, dev, "mesh_distance_grid")
    ne, ndeg, dims, edge = ctypes.c_longlong(), ctypes.c_longlong(), (ctypes.c_int * 3)(), ctypes.c_double()
    call("o2345_mesh_distance_grid_count", verts, tris, ib, nv, nt, 0.0 if cell is None else float(cell), max_cells, ws, wsb, ne, ndeg, dims, edge)
    nbytes = call("o2345_mesh_distance_grid_bytes", max_cells, ne.value)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("o2345_mesh_distance_grid_emit", verts, tris, ib, nv, nt, max_cells, ws, ne.value, buf, nbytes)
    return MeshGrid(buf, max_cells, ne.value, tuple(dims), edge.value, ndeg.value)


@_on_device
def mesh_closest_triangle(points, verts, tris, grid=None):
    """For every point its closest triangle of a target mesh on the device (== mesh_io.closest_triangles, to the last bit) -> (d2 fp64 [n], nearest int32
    [n]): the squared distance and the smallest index among the triangles that attain it; +inf and -1 where the target has no triangle with an area.
    points fp64 [n,3]; ``grid``: a MeshGrid of the same ``verts`` and ``tris`` (ops.mesh_distance_grid), or None for the exhaustive search -- the same
    bits either way.  No synchronisation."""
    tris, ib = _triangles(tris, "mesh_closest_triangle")
    _vertices(verts, "mesh_closest_triangle")
    _vertices(points, "mesh_closest_triangle")
    n, dev = points.shape[0], points.device
    d2 = torch.empty(n, dtype=torch.float64, device=dev)
    nearest = torch.empty(n, dtype=torch.int32, device=dev)
    gp, gb, gm = (grid.buffer, grid.buffer.numel(), grid.max_cells) if grid is not None else (None, 0, 0)
    call("o2345_mesh_distance_query", points, n, verts, tris, ib, verts.shape[0], tris.shape[0], gp, gb, gm, d2, nearest)
    return d2, nearest


@_on_device
def mesh_distance_stats(d2, nearest, weight, thresholds=(), target=None, out=None):
    """The summary of one direction on the device -> the stats block (O2345DistanceStats as uint8, or ``out``): sums, the largest d2 as its bit pattern, counts;
    ``target`` = (verts, tris) adds the target's counters.  The same bytes on every run; no synchronisation.  ops.distance_summary reads it on the host."""
    th = np.ascontiguousarray(mesh_io._check_thresholds(thresholds), np.float64)
    n, dev = d2.shape[0], d2.device
    ws, wsb = _scratch("o2345_mesh_distance_reduce_workspace_bytes", (n,), dev, "mesh_distance_reduce")
    stats = _stats_block("O2345DistanceStats", dev) if out is None else out
    tv, (tt, ib), tnv, tnt = (None, (None, 4), 0, 0) if target is None else (target[0], _triangles(target[1], "mesh_distance_stats"), target[0].shape[0], target[1].shape[0])
    call("o2345_mesh_distance_reduce", d2, nearest, weight, n, th, len(th), tv, tt, ib, tnv, tnt, ws, wsb, stats)
    return stats


def distance_summary(stats, n_thresholds, target_triangles=None):
    """The stats block of o2345_mesh_distance_reduce (O2345DistanceStats, on the host) -> (the summary dict of mesh_io.distance_summary, the target's
    degenerate triangles); raises on a target without a usable triangle."""
    st = _lib.read_struct("O2345DistanceStats", stats)
    n, unmatched, degenerate, bad = st.n, st.n_unmatched, st.n_degenerate, st.n_bad
    if bad:
        raise RuntimeError(f"o2345 mesh_distance: {bad} target triangles have an index out of range or a non-finite coordinate")
    if unmatched:
        raise RuntimeError(f"o2345 mesh_distance: {unmatched} of {n} samples found no triangle: the target has no triangle with an area"
                           + (f" ({target_triangles} triangles, {degenerate} degenerate)" if target_triangles is not None else ""))
    W = st.sum_w
    div = lambda s: s / W if W > 0 else float("nan")
    return {"mean": div(st.sum_wd), "rms": float(np.sqrt(div(st.sum_wd2))) if W > 0 else float("nan"), "max": float(np.sqrt(_double_of_bits(st.max_d2_bits))),
            "within": [div(st.within[k]) for k in range(n_thresholds)], "samples": n, "area": W}, degenerate


@_on_device
def mesh_align_step(points, weights, transforms, target=None, grid=None, max_distance=None, pivot=(0.0, 0.0, 0.0), moments=None, want=()):
    """One step of the alignment on the device (o2345_mesh_align_step; definitions in csrc/mesh_align.hip, per pair == mesh_io.align_terms to the last bit)
    -> (moments fp64 [K,48] on the device, {name: tensor for name in ``want``}).  points fp64 [n,3], weights fp64 [n] or None (1), transforms fp64
    [K,12] on the device; ``target`` = (verts, tris) or None (no target: the centroid / radius / transform-only form); ``grid``: a MeshGrid of the target
    or None for the exhaustive search; ``want``: any of "moved" [K,n,3], "d2" [K,n], "nearest" [K,n] -- nothing of that size is written otherwise.  One
    synchronisation, for the library's check of the transforms."""
    tau = mesh_io._check_max_distance(max_distance)
    _vertices(points, "mesh_align_step")
    n, dev = points.shape[0], points.device
    if transforms.dtype != torch.float64 or transforms.dim() != 2 or transforms.shape[1] != 12:
        raise ValueError(f"mesh_align_step: expected transforms [K,12] float64, got {tuple(transforms.shape)} {transforms.dtype}")
    K = transforms.shape[0]
    if not 1 <= K <= mesh_io.ALIGN_MAX_TRANSFORMS:
        raise ValueError(f"mesh_align_step: {K} transforms; between 1 and {mesh_io.ALIGN_MAX_TRANSFORMS}")
    tv, (tt, ib), nv, nt = (None, (None, 4), 0, 0) if target is None else (target[0], _triangles(target[1], "mesh_align_step"), target[0].shape[0], target[1].shape[0])
    if tv is not None:
        _vertices(tv, "mesh_align_step")
    ws, wsb = _scratch("o2345_mesh_align_workspace_bytes", (n, K), dev, "mesh_align")
    moments = torch.empty(K, mesh_io.ALIGN_COLUMNS, dtype=torch.float64, device=dev) if moments is None else moments
    shapes = {"moved": ((K, n, 3), torch.float64), "d2": ((K, n), torch.float64), "nearest": ((K, n), torch.int32)}
    extra = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
    gp, gb, gm = (grid.buffer, grid.buffer.numel(), grid.max_cells) if grid is not None else (None, 0, 0)
    c = [float(x) for x in np.asarray(pivot, np.float64).reshape(3)]
    call("o2345_mesh_align_step", points, weights, n, transforms, K, tv, tt, ib, nv, nt, gp, gb, gm, tau, c[0], c[1], c[2], ws, wsb, moments,
         extra.get("moved"), extra.get("d2"), extra.get("nearest"))
    return moments, extra


@_on_device
def mesh_transform(verts, T):
    """Vertices fp64 [N,3] under the transform T (3 x 4 or 4 x 4, host) on the device -> fp64 [N,3] (== mesh_io.transform_vertices to the last bit): the
    alignment step without a target, with its ``moved`` output"""
    _vertices(verts, "mesh_transform")
    T = torch.from_numpy(mesh_io._align_matrix(T, "transform").reshape(1, 12).copy()).to(verts.device)
    return mesh_align_step(verts.contiguous(), None, T, want=("moved",))[1]["moved"][0]


def mesh_align_stepper(va, ta, vb, tb, spacing=None, cell=None):
    """The supplier of moments rows that mesh_io.align_run asks for, on the device: the samples of both meshes are taken once (mesh_surface_samples at
    ``spacing``) and B's grid is built once (mesh_distance_grid with ``cell``; a target of fewer than 64 triangles is searched exhaustively); a call is
    ONE o2345_mesh_align_step over all its transforms and one read-back of [K,48] doubles."""
    dev = va.device
    sets = {"a": mesh_surface_samples(va, ta, spacing)[:2], "b": mesh_surface_samples(vb, tb, spacing)[:2]}
    grid = mesh_distance_grid(vb, tb, cell) if tb.shape[0] >= _DISTANCE_EXHAUSTIVE_BELOW else None

    def step(side, transforms, pivot, tau, target):
        pts, w = sets[side]
        T = torch.from_numpy(np.ascontiguousarray(transforms, np.float64)).to(dev)
        rows, _ = mesh_align_step(pts, w, T, (vb, tb) if target else None, grid if target else None, tau, pivot)
        return rows.cpu().numpy()
    return step


def mesh_align(va, ta, vb, tb, spacing=None, iterations=30, tol=1e-9, max_distance=None, scale=True, candidates=None, search_iterations=5, init=None,
               cell=None):
    """The similarity transform that moves mesh A onto mesh B, on the device -> the dict of mesh_io.align_meshes (its host twin; the loop and the 7 x 7
    solve are mesh_io.align_run's, shared with it, over the rows of mesh_align_stepper).  va / vb fp64 [N,3], ta / tb [M,3] int32 / int64 on one device."""
    step = mesh_align_stepper(va, ta, vb, tb, spacing, cell)
    return mesh_io.align_run(step, iterations, tol, max_distance, scale, candidates, search_iterations, init)


def mesh_distance(va, ta, vb, tb, spacing=None, thresholds=(), return_samples=False, cell=None, align=None):
    """Distance between mesh A (under test) and mesh B (the reference) as surfaces, on the device -> the dict of mesh_io.mesh_distance (its host twin):
    one-sided summaries "a_to_b" / "b_to_a" (mean, rms, max, within, samples, area), "chamfer", "hausdorff", "precision" / "recall" / "fscore" per
    threshold, "degenerate_targets".  va / vb fp64 [N,3], ta / tb [M,3] int32 / int64 on one device.  Per direction: samples at ``spacing``
    (mesh_surface_samples), the target's grid (mesh_distance_grid with ``cell``; a target of fewer than 64 triangles is searched exhaustively), the query,
    the summary; ONE read-back of the two stats blocks at the end (the counts of the samples and grids synchronise before it).  d2 and nearest equal the
    twin's to the last bit, the sums to 1e-12.  ``return_samples`` adds "samples": {"a", "b"} -> {"points", "weight", "triangle", "d2", "nearest"},
    device tensors.  ``align`` (None: nothing new is launched and the dict is as it always was): True or a dict of mesh_align arguments
    (mesh_io.align_arguments) -- A is moved onto B first (mesh_align, mesh_transform), and "alignment" holds mesh_align's result."""
    th = mesh_io._check_thresholds(thresholds)
    alignment = None
    if align is not None and align is not False:
        alignment = mesh_align(va, ta, vb, tb, cell=cell, **mesh_io.align_arguments(align, spacing))
        va = mesh_transform(va, alignment["transform"])
    stats = _stats_block("O2345DistanceStats", va.device, 2)
    samples = {}
    for k, (name, (v, t), (tv, tt)) in enumerate((("a", (va, ta), (vb, tb)), ("b", (vb, tb), (va, ta)))):
        points, weight, triangle = mesh_surface_samples(v, t, spacing)
        grid = mesh_distance_grid(tv, tt, cell) if tt.shape[0] >= _DISTANCE_EXHAUSTIVE_BELOW else None
        d2, nearest = mesh_closest_triangle(points, tv, tt, grid)
        mesh_distance_stats(d2, nearest, weight, th, target=(tv, tt), out=stats[k])
        samples[name] = {"points": points, "weight": weight, "triangle": triangle, "d2": d2, "nearest": nearest}
    host = stats.cpu().numpy()
    a_to_b, deg_b = distance_summary(host[0], len(th), tb.shape[0])
    b_to_a, deg_a = distance_summary(host[1], len(th), ta.shape[0])
    out = mesh_io.distance_report(a_to_b, b_to_a, th, deg_a, deg_b)
    if return_samples:
        out["samples"] = samples
    if alignment is not None:
        out["alignment"] = alignment
    return out


# ---------------------------------------------------------------------------------------------------------- mesh audit
def audit_info(stats, nv, components):
    """The stats block of o2345_mesh_audit (O2345AuditStats, on the host) and the number of components that own a triangle -> the report of
    mesh_io.mesh_audit (mesh_io.audit_report, shared with the twin).  ``components``: a number, or a function that returns it -- called after the two
    refusals.  Raises on a triangle index out of range or a non-finite coordinate."""
    st = _lib.read_struct("O2345AuditStats", stats)
    if st.bad_index:
        raise RuntimeError(f"o2345 mesh_audit: {st.bad_index} triangles index outside 0 .. {nv - 1}")
    if st.nonfinite:
        raise RuntimeError(f"o2345 mesh_audit: {st.nonfinite} vertices have a non-finite coordinate")
    return mesh_io.audit_report({k: getattr(st, k) for k in mesh_io.AUDIT_COUNTS}, list(st.histogram), st.area, st.volume6, st.quality_sum, st.quality_min,
                                st.edge2_min, st.edge2_max, components() if callable(components) else components)


@_on_device
def mesh_audit(verts, tris, return_elements=False):
    """Audit of a mesh on the device (== mesh_io.mesh_audit, its host twin and the definition: counts, flags, quality, minima and maxima to the last bit,
    the three sums to 1e-12; csrc/mesh_audit.hip): is it a closed, oriented 2-manifold, and how good are its triangles.  verts fp64 [N,3], tris [M,3]
    int32 / int64, both only read -> the twin's dict (counts of used vertices, edges, faces, of repeated and zero-area triangles, of boundary,
    non-manifold, inconsistent and creased edges, of boundary, non-manifold, bow-tie and unused vertices; "histogram", "area", "volume", "quality_mean",
    "quality_min", "edge_min", "edge_max", "euler", "components", "oriented", "watertight", "genus").  One device-to-host copy, of the stats block;
    "components" comes from the component unit (ops.mesh_component_labels' pass, which synchronises once more).  ``return_elements`` adds the device
    tensors "vertex_flags" uint8 [N], "face_flags" uint8 [M] and "quality" fp64 [M].  Raises on an index out of range or a non-finite coordinate."""
    tris, ib = _triangles(tris, "mesh_audit")
    _vertices(verts, "mesh_audit")
    nv, nt, dev = verts.shape[0], tris.shape[0], verts.device
    ws, wsb = _scratch("o2345_mesh_audit_workspace_bytes", (nv, nt), dev, "mesh_audit")
    if not wsb:
        raise ValueError(f"mesh_audit: bad sizes ({nv} vertices, {nt} triangles; the tables are int32)")
    stats = _stats_block("O2345AuditStats", dev)
    vf, ff, q = (torch.empty(n, dtype=dt, device=dev) for n, dt in ((nv, torch.uint8), (nt, torch.uint8), (nt, torch.float64))) if return_elements else (None,) * 3
    call("o2345_mesh_audit", verts, tris, ib, nv, nt, ws, wsb, stats, vf, ff, q)
    # the components with at least one triangle: the selection count of the component unit at min_faces = 1
    out = audit_info(stats.cpu().numpy(), nv, lambda: _mesh_components_count(tris, nv, 1, False, None)[2])
    if return_elements:
        out.update(vertex_flags=vf, face_flags=ff, quality=q)
    return out


# ---------------------------------------------------------------------------------------------------------- self-intersections
def intersect_info(counts, nv):
    """The eight counts of o2345_mesh_intersect_count, on the host -> the report of mesh_io.mesh_intersections; raises on a triangle index out of range
    or a non-finite coordinate (the rest is void then)."""
    out = mesh_io.intersect_report(counts)
    if out["bad_index"]:
        raise RuntimeError(f"o2345 mesh_intersections: {out['bad_index']} triangles index outside 0 .. {nv - 1}")
    if out["nonfinite"]:
        raise RuntimeError(f"o2345 mesh_intersections: {out['nonfinite']} triangles have a non-finite vertex coordinate")
    return out


@_on_device
def mesh_intersections(verts, tris, return_pairs=False, cell=None, grid=True):
    """The self-intersections of a mesh on the device (== mesh_io.mesh_intersections, its host twin and the definition, to the last bit;
    csrc/mesh_intersect.hip): which pairs of triangles cross.  verts fp64 [N,3], tris [M,3] int32 / int64, both only read -> the twin's dict: "faces"
    (that take part), "skipped", "candidates" (boxes overlap, at most one shared index), "pairs", "faces_hit", "max_hits" ("bad_index" and "nonfinite"
    are 0: they raise).  The broad phase walks the grid of mesh_distance_grid(verts, tris, cell); a mesh of fewer than 64 triangles, or ``grid=False``
    (at most 2^16 triangles), is searched exhaustively -- the same result either way, whatever the cell edge.  A mesh without a triangle that has an
    area gives the all-zero report.  The grid's count synchronises once; the report is ONE copy of the eight counts.  ``return_pairs`` adds the device
    tensors "pairs_list" int32 [n,2] (t < u, sorted lexicographically; the same bytes on every run) and "face_hits" int32 [M].  Not counted: coplanar
    overlap, contacts that only touch, nested components, coincident vertices with different indices."""
    tris, ib = _triangles(tris, "mesh_intersections")
    _vertices(verts, "mesh_intersections")
    nv, nt, dev = verts.shape[0], tris.shape[0], verts.device
    ws, wsb = _scratch("o2345_mesh_intersect_workspace_bytes", (nv, nt), dev, "mesh_intersect")
    if not wsb:
        raise ValueError(f"mesh_intersections: bad sizes ({nv} vertices, {nt} triangles; the tables are int32)")
    g = None
    if grid and nt >= _DISTANCE_EXHAUSTIVE_BELOW:
        try:
            g = mesh_distance_grid(verts, tris, cell)
        except RuntimeError as e:
            if "no triangle with an area" not in str(e):
                raise                                                     # a bad index and a non-finite coordinate are the grid's refusals too
            g = None                                                      # nothing takes part: the exhaustive kernel finds that out per face
            if nt > mesh_io.INTERSECT_EXHAUSTIVE_MAX:
                out = mesh_io.intersect_report((0, 0, 0, nt, 0, 0, 0, 0))
                if return_pairs:
                    out.update(pairs_list=torch.zeros(0, 2, dtype=torch.int32, device=dev), face_hits=torch.zeros(nt, dtype=torch.int32, device=dev))
                return out
    gp, gb, gm = (g.buffer, g.buffer.numel(), g.max_cells) if g is not None else (None, 0, 0)
    counts = torch.empty(len(mesh_io.INTERSECT_COUNTS), dtype=torch.int64, device=dev)
    face_hits = torch.empty(nt, dtype=torch.int32, device=dev) if return_pairs else None
    call("o2345_mesh_intersect_count", verts, tris, ib, nv, nt, gp, gb, gm, ws, wsb, counts, face_hits)
    out = intersect_info(counts.tolist(), nv)
    if return_pairs:
        pairs = torch.empty(out["pairs"], 2, dtype=torch.int32, device=dev)
        call("o2345_mesh_intersect_emit", verts, tris, ib, nv, nt, gp, gb, gm, ws, out["pairs"], pairs)
        out.update(pairs_list=pairs, face_hits=face_hits)
    return out


# ---------------------------------------------------------------------------------------------------------- ray cast and ambient occlusion
def _raycast_grid(verts, tris, grid):
    """The grid argument of the two ray cast calls -> (buffer, bytes, max_cells, the mesh has no triangle with an area): a MeshGrid of the same mesh as it is; None: ops.mesh_distance_grid
    unless the mesh is tiny (fewer than 64 triangles) or has no triangle with an area; False: the exhaustive path (at most 2^16 triangles)."""
    if grid is None and tris.shape[0] >= _DISTANCE_EXHAUSTIVE_BELOW:
        try:
            grid = mesh_distance_grid(verts, tris)
        except RuntimeError as e:
            if "no triangle with an area" not in str(e):
                raise
            return None, 0, 0, True                                       # nothing can be hit
    return (grid.buffer, grid.buffer.numel(), grid.max_cells, False) if grid else (None, 0, 0, False)


@_on_device
def mesh_ray_cast(origins, directions, verts, tris, max_distance, grid=None, any_hit=False):
    """What rays hit on a mesh, on the device (== mesh_io.ray_cast, its host twin and the definition, to the last bit; csrc/mesh_raycast.hip).  origins,
    directions fp64 [n,3] (directions of any length), verts fp64 [N,3], tris [M,3] int32 / int64, all only read; the segment of ray i ends at origin +
    max_distance direction -> (distance fp64 [n] in direction lengths, inf without a hit; tri int32 [n], -1 without a hit), the nearest hit; ``any_hit``:
    bool [n] instead.  ``grid``: a MeshGrid of the same mesh (ops.mesh_distance_grid), None to build one (a mesh of fewer than 64 triangles is searched
    exhaustively), False for the exhaustive search (at most 2^16 triangles) -- the same result either way.  A ray through a shared edge or vertex hits
    neither neighbour.  The grid's count synchronises once; the cast itself does not."""
    L = mesh_io._check_ray_length("mesh_ray_cast", max_distance)
    tris, ib = _triangles(tris, "mesh_ray_cast")
    for x in (verts, origins, directions):
        _vertices(x, "mesh_ray_cast")
    if origins.shape != directions.shape:
        raise ValueError(f"mesh_ray_cast: {origins.shape[0]} origins and {directions.shape[0]} directions")
    n, dev = origins.shape[0], origins.device
    gp, gb, gm, empty = _raycast_grid(verts, tris, grid)
    t = None if any_hit else torch.empty(n, dtype=torch.float64, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev)
    call("o2345_mesh_ray_cast", origins, (origins + L * directions).contiguous(), n, verts, tris, ib, verts.shape[0], 0 if empty else tris.shape[0], gp, gb, gm,
         1 if any_hit else 0, t, tri)                                     # empty: no triangle has an area, nothing is hit
    return tri != 0 if any_hit else (t * L, tri)


def _occlusion_table(samples, dev):
    return torch.from_numpy(mesh_io.occlusion_directions(samples)).to(dev)


@_on_device
def mesh_occlusion(points, verts, tris, normals=None, owners=None, samples=64, max_distance=None, bias=None, grid=None, counters=None, validate=True):
    """Ambient occlusion of points against a mesh on the device (== mesh_io.mesh_occlusion, its host twin and the definition, to the last bit;
    csrc/mesh_raycast.hip): how many of ``samples`` cosine-weighted rays about the normal of each point are blocked within ``max_distance``.  points fp64
    [n,3]; the normal is ``normals`` fp64 [n,3], or the face normal of triangle ``owners`` int32 [n], turned to the side of ``normals`` when both are
    given -> (hits int32 [n], counts {"bad_points", "bad_frames", "rays"}); the exposure is (samples - hits) / samples (ops.mesh_occlusion_values).
    Defaults (mesh_io.occlusion_defaults): max_distance the diagonal of the vertices' box, bias 1e-6 of it; they read the box back (one synchronisation
    more).  ``grid`` as for ops.mesh_ray_cast.  ``validate=False`` returns the device counters int64 [4] in place of the dict and does not wait
    (mesh_io.occlusion_report reads them)."""
    if normals is None and owners is None:
        raise ValueError("mesh_occlusion: a point needs a direction (normals) or an owner triangle (owners)")
    tris, ib = _triangles(tris, "mesh_occlusion")
    for x in (verts, points) + (() if normals is None else (normals,)):
        _vertices(x, "mesh_occlusion")
    n, dev = points.shape[0], points.device
    if normals is not None and normals.shape[0] != n:
        raise ValueError(f"mesh_occlusion: {n} points and {normals.shape[0]} normals")
    if owners is not None and (owners.dtype != torch.int32 or tuple(owners.shape) != (n,)):
        raise ValueError(f"mesh_occlusion: expected owners int32 [{n}], got {tuple(owners.shape)} {owners.dtype}")
    table = _occlusion_table(samples, dev)
    if max_distance is None or bias is None:
        ok = torch.isfinite(verts).all(1)
        box = torch.stack([verts[ok].amin(0), verts[ok].amax(0)]).tolist() if bool(ok.any()) else [[0.0] * 3] * 2
        max_distance, bias = mesh_io.occlusion_defaults(box[0], box[1], max_distance, bias)
    else:
        max_distance, bias = mesh_io.occlusion_defaults((0, 0, 0), (0, 0, 0), max_distance, bias)
    gp, gb, gm, empty = _raycast_grid(verts, tris, grid)
    hits = torch.empty(n, dtype=torch.int32, device=dev)
    if counters is None:
        counters = torch.empty(len(mesh_io.OCCLUSION_COUNTS), dtype=torch.int64, device=dev)
    if empty:
        tris = tris[:0]                                                   # no triangle has an area: nothing is hit, and every owner is unusable
    call("o2345_mesh_occlusion", points, normals, owners, n, table, table.shape[0], max_distance, bias, verts, tris, ib, verts.shape[0], tris.shape[0], gp, gb, gm,
         hits, counters)
    return hits, (mesh_io.occlusion_report(counters.tolist()) if validate else counters)


def mesh_occlusion_values(hits, samples):
    """hits int32 [n] of ``samples`` rays, on the device -> the exposure fp32 [n,3] (== mesh_io.occlusion_values, exactly): float32((S - hits) / S) in every
    channel, what ops.mesh_texture_pack turns into the occlusion image"""
    v = ((float(samples) - hits.to(torch.float64)) / float(samples)).to(torch.float32)
    return v.reshape(-1, 1).expand(-1, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------- texture atlas
# ---------------------------------------------------------------------------------------------------------- hole filling
@_on_device
def mesh_fill_holes(verts_idx, tris, max_edges=None):
    """Closes the boundary loops of a mesh on the device (== mesh_io.fill_holes, to the last bit; definitions in csrc/mesh_fill.hip and include/o2345.h).
    verts_idx fp64 [N,3], tris [M,3] int32 / int64, ``max_edges``: the longest hole, in edges, that is filled (None: the config default,
    config.MESH_FILL_HOLES_ALL: every hole) -> (verts fp64 [N + c,3], tris [M + k,3] of the same dtype, hole int32 [k]: for every new triangle the number
    of its hole among the filled holes, info = the counts of mesh_io.FILL_COUNTS: {"boundary", "holes", "filled", "too_long", "open", "longest",
    "vertices", "triangles"}).  The input's vertices and triangles come first, bit for bit; a hole of three edges gets one triangle, a longer one a new
    vertex at the mean of its rim and a fan.  The inputs are not written; the count synchronises once, and the 64-byte copy of the counts behind it finds the stream idle.  With no boundary half-edge the inputs themselves are
    returned.  With ``max_edges == 0`` the stage is off: no kernel is launched, the inputs are returned as they are, ``hole`` and ``info`` are None."""
    max_edges = config.mesh_fill_holes(max_edges)
    if max_edges == 0:
        return verts_idx, tris, None, None
    tris, ib = _triangles(tris, "mesh_fill_holes")
    _vertices(verts_idx, "mesh_fill_holes")
    nv, nt, dev = verts_idx.shape[0], tris.shape[0], verts_idx.device
    ws, wsb = _scratch("o2345_mesh_fill_workspace_bytes", (nv, nt), dev, "mesh_fill")
    if wsb == 0:
        raise ValueError(f"mesh_fill_holes: bad sizes ({nv} vertices, {nt} triangles; the tables are int32)")
    counts = torch.empty(len(mesh_io.FILL_COUNTS), dtype=torch.int64, device=dev)
    call("o2345_mesh_fill_count", tris, ib, nv, nt, max_edges, ws, wsb, counts)
    info = dict(zip(mesh_io.FILL_COUNTS, counts.tolist()))
    hole = torch.empty(info["triangles"] - nt, dtype=torch.int32, device=dev)
    if info["boundary"] == 0:
        return verts_idx, tris, hole, info
    verts = torch.empty(info["vertices"], 3, dtype=torch.float64, device=dev)
    tris_out = torch.empty(info["triangles"], 3, dtype=tris.dtype, device=dev)
    call("o2345_mesh_fill_emit", verts_idx, tris, ib, nv, nt, ws, verts, tris_out, hole)
    return verts, tris_out, hole, info


def _texture_mesh(verts_idx, tris, what):
    t = _triangles(tris, what)
    _vertices(verts_idx, what)
    if verts_idx.shape[0] < 1:
        raise ValueError(f"{what}: a mesh with triangles has vertices")
    return t


def texture_check(stats):
    """The stats block of o2345_mesh_texture_points (O2345TextureStats, on the host): raises on a non-finite coordinate or a triangle index out of range."""
    st = _lib.read_struct("O2345TextureStats", stats)
    if st.n_bad:
        raise RuntimeError(f"o2345 mesh_texture_points: {st.n_bad} triangles index outside the vertex array")
    if st.n_nonfinite:
        raise RuntimeError(f"o2345 mesh_texture_points: {st.n_nonfinite} triangles have a non-finite vertex coordinate")


@_on_device
def mesh_texture_points(verts_idx, tris, texel, resolution, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), validate=True):
    """The surface point of every texel of the atlas (== mesh_io.texture_points, to the last bit; definitions in csrc/mesh_texture.hip).  verts_idx fp64
    [N,3] index coordinates on a ``resolution``^3 grid, tris [M,3] int32 / int64, ``texel`` in [4, 64] -> (points fp64 [cells c^2, 3] index coordinates,
    world fp32 [cells c^2, 3], stats uint8 [sizeof O2345TextureStats]), cell-major; the inputs are not written.  ``validate`` copies the counters to the host (one
    synchronisation) and raises on a non-finite coordinate or a triangle index out of range; a caller that queues more work passes False and hands the
    counters to texture_check after its own copy."""
    tris, ib = _texture_mesh(verts_idx, tris, "mesh_texture_points")
    lay = mesh_io.texture_layout(tris.shape[0], texel)
    resolution = _resolution(resolution, "mesh_texture_points")
    bmin, bmax = _bounds(bound_min, bound_max, "mesh_texture_points")
    dev, n = verts_idx.device, lay["texels"]
    assert call("o2345_mesh_texture_texels", tris.shape[0], lay["texel"], None, None) == n
    pts = torch.empty(n, 3, dtype=torch.float64, device=dev)
    world = torch.empty(n, 3, dtype=torch.float32, device=dev)
    stats = _stats_block("O2345TextureStats", dev)
    call("o2345_mesh_texture_points", verts_idx, verts_idx.shape[0], tris, ib, tris.shape[0], lay["texel"], int(resolution), bmin, bmax, pts, world, stats)
    if validate:
        texture_check(stats.cpu().numpy())
    return pts, world, stats


@_on_device
def mesh_texture_pack(rgb, nt, texel):
    """Cell-major texel colours fp32 [cells c^2, 3] -> the atlas image uint8 [H, W, 4] on the device (== mesh_io.pack_texture, exactly)."""
    lay = mesh_io.texture_layout(nt, texel)
    if rgb.dim() != 2 or tuple(rgb.shape) != (lay["texels"], 3):
        raise ValueError(f"mesh_texture_pack: expected colours [{lay['texels']}, 3], got {tuple(rgb.shape)}")
    image = torch.empty(lay["height"], lay["width"], 4, dtype=torch.uint8, device=rgb.device)
    call("o2345_mesh_texture_pack", rgb, int(nt), lay["texel"], image)
    return image


@_on_device
def mesh_texture_corners(verts_idx, tris, texel, grid_R, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None, grad=None):
    """The unwelded vertices of the textured asset (== mesh_io.texture_corners, to the last bit): (positions float32 [3M,3] in the asset frame, uv float32
    [3M,2], normals float32 [3M,3] or None, indices uint32-valued int32 storage [M,3] = 0, 1, 2, ..., bounds float32 [2,3]), all on the device.
    ``grad`` fp32 [N,3]: the SDF gradient at the (welded) vertices."""
    tris, ib = _texture_mesh(verts_idx, tris, "mesh_texture_corners")
    lay = mesh_io.texture_layout(tris.shape[0], texel)
    dev, m = verts_idx.device, tris.shape[0]
    if grad is not None and tuple(grad.shape) != (verts_idx.shape[0], 3):
        raise ValueError(f"mesh_texture_corners: expected gradients [{verts_idx.shape[0]}, 3], got {tuple(grad.shape)}")
    frame = _mesh_frame(bound_min, bound_max, scale_mat, trans_mat)
    pos = torch.empty(3 * m, 3, dtype=torch.float32, device=dev)
    uv = torch.empty(3 * m, 2, dtype=torch.float32, device=dev)
    nrm = None if grad is None else torch.empty(3 * m, 3, dtype=torch.float32, device=dev)
    idx = torch.empty(m, 3, dtype=torch.int32, device=dev)
    bounds = torch.empty(2, 3, dtype=torch.float32, device=dev)
    ws, wsb = _scratch("o2345_mesh_bounds_workspace_bytes", (3 * m,), dev, "mesh_bounds")
    call("o2345_mesh_texture_corners", verts_idx, verts_idx.shape[0], tris, ib, m, lay["texel"], int(grid_R), *frame, grad, pos, uv, nrm, idx, bounds, ws, wsb)
    return pos, uv, nrm, idx, bounds


def normal_map_counts(counters):
    """The counters block of the two normal-map entries on the host (int64 [4]) -> {"degenerate", "bad_gradient", "back_facing"}; none is an error."""
    c = np.asarray(counters).reshape(-1)
    if c.shape[0] != len(mesh_io.NORMAL_MAP_COUNTS):
        raise ValueError(f"normal_map_counts: expected {len(mesh_io.NORMAL_MAP_COUNTS)} counters, got {c.shape[0]}")
    return {k: int(v) for k, v in zip(mesh_io.NORMAL_MAP_COUNTS[:3], c)}


def _corner_buffers(positions, uv, what):
    if positions.dim() != 2 or positions.shape[1] != 3 or positions.shape[0] < 3 or positions.shape[0] % 3 or tuple(uv.shape) != (positions.shape[0], 2):
        raise ValueError(f"{what}: expected positions [3 M, 3] and uv [3 M, 2] of M >= 1 triangles, got {tuple(positions.shape)} and {tuple(uv.shape)}")
    return positions.shape[0] // 3


def _normal_map_counters(counters, dev, what):
    if counters is None:
        return torch.empty(len(mesh_io.NORMAL_MAP_COUNTS), dtype=torch.int64, device=dev)
    if not torch.is_tensor(counters) or counters.dtype != torch.int64 or tuple(counters.shape) != (len(mesh_io.NORMAL_MAP_COUNTS),):
        raise ValueError(f"{what}: counters are int64 [{len(mesh_io.NORMAL_MAP_COUNTS)}] on the device, got {counters!r}")
    return counters


@_on_device
def mesh_texture_frames(positions, uv):
    """One tangent frame per triangle of the textured asset from the buffers of mesh_texture_corners (== mesh_io.texture_frames, to the last bit;
    definitions in include/o2345.h): positions fp32 [3M,3], uv fp32 [3M,2] -> (normals fp32 [3M,3], the flat unit normal of the file's winding, tangents fp32
    [3M,4] = (T, w), counters int64 [4] on the device: mesh_io.NORMAL_MAP_COUNTS, the first written here).  A degenerate triangle gets (0, 1, 0) and
    (1, 0, 0, 1) and is counted; nothing synchronises: the caller reads the counters with its own copy (normal_map_counts)."""
    m = _corner_buffers(positions, uv, "mesh_texture_frames")
    dev = positions.device
    nrm = torch.empty(3 * m, 3, dtype=torch.float32, device=dev)
    tan = torch.empty(3 * m, 4, dtype=torch.float32, device=dev)
    counters = _normal_map_counters(None, dev, "mesh_texture_frames")
    call("o2345_mesh_texture_frames", positions, uv, m, nrm, tan, counters)
    return nrm, tan, counters


def _rotation(rotation, dev, what):
    """None, a device fp32 tensor of 9 elements, or the 3x3 / the 4x4 trans_mat on the host (uploaded) -> device fp32 [9] or None"""
    if rotation is None:
        return None
    if torch.is_tensor(rotation) and rotation.is_cuda:
        if rotation.dtype != torch.float32 or rotation.numel() != 9:
            raise ValueError(f"{what}: a rotation on the device is float32 [9] or [3,3], got {tuple(rotation.shape)} {rotation.dtype}")
        return rotation.contiguous().view(9)
    r = host_f32(rotation)
    if r.size != 9 and (r.size == 0 or r.size % 16):
        raise ValueError(f"{what}: rotation is a 3x3 or the 4x4 trans_mat, got {r.shape}")
    return torch.from_numpy(np.ascontiguousarray(r if r.size == 9 else r.reshape(-1, 4, 4)[0, :3, :3]).reshape(9)).to(dev)


@_on_device
def mesh_texture_normal_pack(grad, normals, tangents, nt, texel, rotation=None, counters=None):
    """Cell-major raw SDF gradients at the texel points fp32 [cells c^2, 3] and the frames of mesh_texture_frames -> the tangent-space normal map uint8
    [H, W, 4] on the device (== mesh_io.pack_normal_map, exactly).  ``rotation``: the 3x3 of trans_mat (a device fp32 [9] / [3,3], or a host 3x3 / 4x4,
    uploaded) or None.  ``counters``: the block of mesh_texture_frames, whose first entry is kept, or None (a block of its own, not returned); entries 1
    and 2 count bad gradients and back-facing texels.  Nothing synchronises."""
    lay = mesh_io.texture_layout(nt, texel)
    nt = int(nt)
    if grad.dim() != 2 or tuple(grad.shape) != (lay["texels"], 3):
        raise ValueError(f"mesh_texture_normal_pack: expected gradients [{lay['texels']}, 3], got {tuple(grad.shape)}")
    if tuple(normals.shape) != (3 * nt, 3) or tuple(tangents.shape) != (3 * nt, 4):
        raise ValueError(f"mesh_texture_normal_pack: expected normals [{3 * nt}, 3] and tangents [{3 * nt}, 4], got {tuple(normals.shape)} and {tuple(tangents.shape)}")
    dev = grad.device
    image = torch.empty(lay["height"], lay["width"], 4, dtype=torch.uint8, device=dev)
    call("o2345_mesh_texture_normal_pack", grad, _rotation(rotation, dev, "mesh_texture_normal_pack"), normals, tangents, nt, lay["texel"], image,
         _normal_map_counters(counters, dev, "mesh_texture_normal_pack"))
    return image


@_on_device
def obj_texture_text(positions, uv, normals=None, K=None, bounds=None):
    """The buffers of mesh_texture_corners -> the records of the textured Wavefront OBJ (uint8 tensor on the device; == mesh_io.obj_texture_text_numpy):
    "v", "vt", ["vn",] "f a/a b/b c/c" (include/o2345.h).  ``K`` as for obj_text."""
    n = positions.shape[0]
    K = _obj_digits(K, bounds, n, "obj_texture_text")
    if n % 3 or tuple(uv.shape) != (n, 2):
        raise ValueError(f"obj_texture_text: expected 3 M unwelded vertices and uv [3 M, 2], got {n} and {tuple(uv.shape)}")
    text = torch.empty(call("o2345_obj_texture_text_bytes", n, K, int(normals is not None)), dtype=torch.uint8, device=positions.device)
    call("o2345_obj_texture_text", positions, uv, normals, n, K, text)
    return text


# ---------------------------------------------------------------------------------------------------------- surface render
def _surface_lattice(u, what):
    if u.dim() != 3 or len(set(u.shape)) != 1 or not 2 <= u.shape[0] <= 2048:
        raise ValueError(f"{what}: the lattice is float32 [R,R,R] with 2 <= R <= 2048, got {tuple(u.shape)}")
    return int(u.shape[0])


@_on_device
def surface_bricks(u, level=0.0, inside_positive=False):
    """Brick flags of the surface trace (== surface.brick_flags, exactly): u float32 [R,R,R] on the device -> uint8 [nb,nb,nb], nb = ceil((R - 1) / 8);
    1 iff a node of the brick fails g > 0, g = u - level (level - u with ``inside_positive``)."""
    R = _surface_lattice(u, "surface_bricks")
    nb = (R - 1 + 7) // 8
    flags = torch.empty(nb, nb, nb, dtype=torch.uint8, device=u.device)
    call("o2345_surface_bricks", u, R, float(level), int(bool(inside_positive)), flags)
    return flags


def surface_info(stats, n_rays):
    """The stats block of o2345_surface_trace (O2345SurfaceStats, on the host) -> the info dict of surface.trace_rays: its 64-bit counters, in its order"""
    st = _lib.read_struct("O2345SurfaceStats", stats)
    return {"rays": int(n_rays), **{k: getattr(st, k) for k, t in st._fields_ if t is ctypes.c_ulonglong}}


@_on_device
def surface_trace(u, rays_o, rays_d, near, far, stride=None, refine=None, level=0.0, inside_positive=False, bound_min=(-1.0, -1.0, -1.0),
                  bound_max=(1.0, 1.0, 1.0), skip=True, flags=None, image_hw=None, want_info=True):
    """March rays through the trilinear lattice u (== surface.trace_rays, to the last bit; definitions in csrc/surface_trace.hip).  u float32 [R,R,R],
    rays_o / rays_d float32 [n,3], all on the device; ``stride`` / ``refine`` None: the config defaults -> dict(depth f32 [n], kind u8 [n] (0 none, 1
    hit, 2 the ray enters inside), point f32 [n,3], hits int32 [n] (the slots with kind != 0 in its first ``n_hits`` entries, in an arbitrary order),
    n_hits int32 [1] on the device (for ``index=`` / ``n_dev=`` of the network ops), stats uint8 [sizeof O2345SurfaceStats], info).  ``skip``: the empty-space skip over
    ``flags`` (ops.surface_bricks of the same lattice, level and sign; computed here when None); the result does not depend on it.  ``image_hw`` = (H, W)
    with H W = n: waves take 8 x 8 pixel tiles.  ``info`` (surface.trace_rays' exact counts) costs one small copy and a synchronisation; a caller that
    queues more work passes ``want_info=False`` and reads ``stats`` later (ops.surface_info)."""
    stride, refine = config.surface_stride(stride), config.surface_refine(refine)
    R = _surface_lattice(u, "surface_trace")
    near, far, level = float(near), float(far), float(level)
    if not (np.isfinite(near) and np.isfinite(far) and np.isfinite(level)):
        raise ValueError(f"surface_trace: near, far and level must be finite, got {near!r}, {far!r}, {level!r}")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_d.shape != rays_o.shape:
        raise ValueError(f"surface_trace: rays_o / rays_d must both be [n,3] (got {tuple(rays_o.shape)}, {tuple(rays_d.shape)})")
    bmin, bmax = _bounds(bound_min, bound_max, "surface_trace")
    n, dev = rays_o.shape[0], u.device
    H, W = (0, 0) if image_hw is None else (int(image_hw[0]), int(image_hw[1]))
    if image_hw is not None and (H < 1 or W < 1 or H * W != n):
        raise ValueError(f"surface_trace: image_hw {image_hw!r} does not hold {n} rays")
    if skip and flags is None:
        flags = surface_bricks(u, level, inside_positive)
    nb = (R - 1 + 7) // 8
    if skip and tuple(flags.shape) != (nb, nb, nb):
        raise ValueError(f"surface_trace: flags must be uint8 [{nb},{nb},{nb}] for R = {R}, got {tuple(flags.shape)}")
    wsb = call("o2345_surface_trace_workspace_bytes", n)
    if wsb == 0:
        raise ValueError(f"surface_trace: {n} rays are too many (n < 2^31)")
    hits = torch.empty(wsb // 4, dtype=torch.int32, device=dev)                # the workspace IS the hit list: owned by the result, not by the stream's cache
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    point = torch.empty(n, 3, dtype=torch.float32, device=dev)
    stats = _stats_block("O2345SurfaceStats", dev)
    at = _lib.STRUCTS["O2345SurfaceStats"].n_list.offset
    call("o2345_surface_trace", u, R, flags if skip else None, rays_o, rays_d, n, H, W, near, far, stride, refine, level, int(bool(inside_positive)), bmin, bmax,
         hits, wsb, depth, kind, point, stats)
    out = dict(depth=depth, kind=kind, point=point, hits=hits[:n], n_hits=stats[at:at + 4].view(torch.int32), stats=stats, info=None)
    if want_info:
        out["info"] = surface_info(stats.cpu().numpy(), n)
    return out


def _camera(K, c2w, what):
    K, M = host_f32(K), host_f32(c2w)
    if K.shape != (3, 3) or M.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"{what}: K [3,3] and c2w [3,4] or [4,4] expected, got {K.shape} and {M.shape}")
    from . import surface
    surface._pinhole(K, M)                                 # the twin's refusals: skew, a zero focal length, non-finite entries
    return K, np.ascontiguousarray(M[:3])


def camera_rays(K, c2w, H, W, device):
    """Rays through the pixel grid of a pinhole camera without skew (== surface.camera_rays, exactly): K [3,3], c2w [4,4] or [3,4] on the host (or tensors:
    copied) -> (rays_o, rays_d) float32 [H W, 3] on ``device``, raster order."""
    K, M = _camera(K, c2w, "camera_rays")
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"camera_rays: bad image size {H} x {W}")
    device = torch.device(device)
    with torch.cuda.device(device):
        o = torch.empty(H * W, 3, dtype=torch.float32, device=device)
        d = torch.empty(H * W, 3, dtype=torch.float32, device=device)
        call("o2345_camera_rays", K, M, H, W, o, d)
    return o, d


@_on_device
def surface_pack(kind, depth, rgb, grad, H, W, background=(0, 0, 0, 0)):
    """Per-ray results in raster order -> (color u8 [H,W,4], normal u8 [H,W,4], depth f32 [H,W]) on the device (== surface.pack_images, exactly): kind u8
    [H W], depth f32 [H W], rgb / grad f32 [H W, 3], read at hits only; ``background``: four integers in [0, 255], the colour image without a hit."""
    H, W = int(H), int(W)
    bg = np.asarray(background)
    if bg.shape != (4,) or not np.array_equal(bg, bg.astype(np.uint8)):
        raise ValueError(f"surface_pack: background is four integers in [0, 255], got {background!r}")
    bg = np.ascontiguousarray(bg, np.uint8)
    n = H * W
    if H < 1 or W < 1 or kind.numel() != n or depth.numel() != n or tuple(rgb.shape) != (n, 3) or tuple(grad.shape) != (n, 3):
        raise ValueError(f"surface_pack: kind / depth [{n}] and rgb / grad [{n},3] expected for {H} x {W}")
    dev = kind.device
    color = torch.empty(H, W, 4, dtype=torch.uint8, device=dev)
    normal = torch.empty(H, W, 4, dtype=torch.uint8, device=dev)
    out = torch.empty(H, W, dtype=torch.float32, device=dev)
    call("o2345_surface_pack", kind, depth, rgb, grad, H, W, bg, color, normal, out)
    return color, normal, out


# ---------------------------------------------------------------------------------------------------------- mesh rasterizer
def _raster_camera(K, c2w, near, cull, what):
    """the twin's refusals (raster.camera) -> (K float32 [3,3], the 3 x 4 of c2w float32: the two host arrays of the C ABI), near, cull"""
    from . import raster
    K, M = _camera(K, c2w, what)
    cam = raster.camera(K, M, near, cull)
    return (K, M), cam["near"], cam["cull"]


def raster_info(counts):
    """The counts of o2345_mesh_raster_count / _emit, on the host -> the info dict of raster.rasterize, by O2345_RASTER_*"""
    from . import raster
    return dict(zip(raster.COUNTS, (int(c) for c in counts)))


def _raster_visibility(verts, tris, ib, cam, H, W, near, cull, ray_depth, what):
    """count, one copy of the counts for the size of the tile lists, emit -> face int32 [H,W], depth float32 [H,W], bary float32 [H,W,3], the counts (device)"""
    from . import raster
    nv, nt, dev = verts.shape[0], tris.shape[0], verts.device
    ws, wsb = _scratch("o2345_mesh_raster_workspace_bytes", (nv, nt, H, W), dev, "mesh_raster")
    if not wsb:
        raise ValueError(f"{what}: bad sizes ({nv} vertices, {nt} triangles; the tables are int32)")
    counts = torch.empty(len(raster.COUNTS), dtype=torch.int64, device=dev)
    call("o2345_mesh_raster_count", verts, tris, ib, nv, nt, *cam, H, W, near, cull, ws, wsb, counts)
    n_pairs = raster_info(counts.tolist())["pairs"]
    if n_pairs >= 2 ** 31:
        raise ValueError(f"{what}: {n_pairs} (tile, face) pairs; the tile lists hold fewer than 2^31")
    lists = _workspace(4 * max(n_pairs, 1), dev, "mesh_raster_lists").view(torch.int32) if n_pairs else None
    face, depth, bary = (torch.empty(H, W, *s, dtype=d, device=dev) for s, d in (((), torch.int32), ((), torch.float32), ((3,), torch.float32)))
    call("o2345_mesh_raster_emit", nv, nt, *cam, H, W, near, cull, int(bool(ray_depth)), ws, wsb, n_pairs, lists, face, depth, bary, counts)
    return face, depth, bary, counts


@_on_device
def mesh_raster(verts, tris, K, c2w, H, W, near=1e-3, cull=0, ray_depth=False, vertex_colors=None, vertex_normals=None):
    """Rasterize a triangle mesh on the device (== raster.rasterize, its host twin and the definition, to the last bit; csrc/mesh_raster.hip).  verts fp64
    [N,3] in the world frame, tris [M,3] int32 / int64, vertex_colors / vertex_normals float32 [N,3] or None, all on the device and only read; K [3,3]
    without skew (fx, fy > 0) and c2w [4,4] or [3,4] (a rotation) on the host -> dict(face int32 [H,W] (-1: no hit), depth float32 [H,W] (along the
    camera's axis, or with ``ray_depth`` along the pixel's ray: the t of surface_trace), bary float32 [H,W,3], kind uint8 [H W], rgb float32 [H W,3], nrm
    float32 [H W,3] (the inputs of surface_pack), info: the counts by raster.COUNTS).  ``cull``: 0 none, 1 back faces, 2 front faces.  One
    synchronisation, for the size of the tile lists; the counts are read once more at the end."""
    from . import raster
    cam, near, cull = _raster_camera(K, c2w, near, cull, "mesh_raster")
    H, W = raster._image_size(H, W)
    tris, ib = _triangles(tris, "mesh_raster")
    _vertices(verts, "mesh_raster")
    nv, nt, dev = verts.shape[0], tris.shape[0], verts.device
    for a, what in ((vertex_colors, "vertex_colors"), (vertex_normals, "vertex_normals")):
        if a is not None and (a.dtype != torch.float32 or tuple(a.shape) != (nv, 3) or a.device != dev or not a.is_contiguous()):
            raise ValueError(f"mesh_raster: {what} must be contiguous float32 [{nv},3] on {dev}, got {a.dtype} {tuple(a.shape)} on {a.device}")
    face, depth, bary, counts = _raster_visibility(verts, tris, ib, cam, H, W, near, cull, ray_depth, "mesh_raster")
    kind = torch.empty(H * W, dtype=torch.uint8, device=dev)
    rgb = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    nrm = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    call("o2345_mesh_raster_shade", verts, tris, ib, nv, nt, face, bary, H, W, vertex_colors, vertex_normals, kind, rgb, nrm)
    return dict(face=face, depth=depth, bary=bary, kind=kind, rgb=rgb, nrm=nrm, info=raster_info(counts.tolist()))


def texture_raster_info(counters):
    """The counters of o2345_mesh_raster_shade_textured, on the host (int64 [4]) -> {"bad_uv", "flat_frame", "back_lit"}; none is an error."""
    from . import raster
    c = np.asarray(counters).reshape(-1)
    if c.shape[0] != len(raster.TEX_COUNTS):
        raise ValueError(f"texture_raster_info: expected {len(raster.TEX_COUNTS)} counters, got {c.shape[0]}")
    return {k: int(v) for k, v in zip(raster.TEX_COUNTS[:3], c)}


@_on_device
def mesh_raster_textured(positions, uv, image, K, c2w, H, W, near=1e-3, cull=0, ray_depth=False, normals=None, tangents=None, normal_image=None, ambient=0.25):
    """Rasterize a textured asset on the device (== raster.rasterize_textured, its host twin and the definition, to the last bit): positions float32
    [3M,3] in the asset's frame (widened to fp64 once; the triangles are 0, 1, 2, ...), uv float32 [3M,2], image uint8 [Ht,Wt,4], and with the normal map
    normals float32 [3M,3], tangents float32 [3M,4] and normal_image uint8 [Ht,Wt,4] -- the buffers of mesh_io.textured_asset_buffers or of a ``.glb``, all on
    the device and only read; K and c2w (asset_camera's, or any camera in the asset's frame) on the host -> mesh_raster's dict with rgb = the atlas's
    albedo and nrm = the shading normal, plus lit float32 [H W,3] and tex_info (raster.TEX_COUNTS by name).  ``cull`` 1 drops what is seen from behind
    whatever the camera's handedness.  Runs count, emit and the textured shade; mesh_raster's synchronisations, and one more copy for the counters."""
    from . import raster
    cull = raster.mirrored_cull(cull, host_f32(c2w))
    cam, near, cull = _raster_camera(K, c2w, near, cull, "mesh_raster_textured")
    H, W = raster._image_size(H, W)
    ambient = raster._ambient(ambient)
    dev = positions.device
    m = _corner_buffers(positions, uv, "mesh_raster_textured")
    if positions.dtype != torch.float32 or uv.dtype != torch.float32:
        raise ValueError(f"mesh_raster_textured: positions and uv are float32, got {positions.dtype} and {uv.dtype}")

    def atlas(a, what):
        if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1 or a.device != dev:
            raise ValueError(f"mesh_raster_textured: {what} is uint8 [Ht,Wt,4] on {dev}, got {a.dtype} {tuple(a.shape)} on {a.device}")
        if max(a.shape[:2]) > raster.TEX_MAX_SIDE:
            raise ValueError(f"mesh_raster_textured: {what} of {a.shape[1]} x {a.shape[0]}: a side is limited to {raster.TEX_MAX_SIDE}")
        return a.contiguous()
    image = atlas(image, "the atlas")
    mapped = normal_image is not None
    if (normals is None) != (tangents is None) or (normals is None) == mapped:
        raise ValueError("mesh_raster_textured: a normal map is normals, tangents and a normal image together")
    if mapped:
        normal_image = atlas(normal_image, "the normal image")
        if normal_image.shape != image.shape:
            raise ValueError(f"mesh_raster_textured: the normal image has the atlas's size {tuple(image.shape[:2])}, got {tuple(normal_image.shape[:2])}")
        if normals.dtype != torch.float32 or tuple(normals.shape) != (3 * m, 3) or tangents.dtype != torch.float32 or tuple(tangents.shape) != (3 * m, 4):
            raise ValueError(f"mesh_raster_textured: normals are float32 [{3 * m},3] and tangents float32 [{3 * m},4], got {tuple(normals.shape)} and {tuple(tangents.shape)}")
    verts = positions.contiguous().to(torch.float64)
    tris = torch.arange(3 * m, dtype=torch.int32, device=dev).view(m, 3)
    nv, nt, ib = 3 * m, m, 4
    face, depth, bary, counts = _raster_visibility(verts, tris, ib, cam, H, W, near, cull, ray_depth, "mesh_raster_textured")
    kind = torch.empty(H * W, dtype=torch.uint8, device=dev)
    rgb, nrm, lit = (torch.empty(H * W, 3, dtype=torch.float32, device=dev) for _ in range(3))
    counters = torch.empty(len(raster.TEX_COUNTS), dtype=torch.int64, device=dev)
    call("o2345_mesh_raster_shade_textured", verts, tris, ib, nv, nt, face, bary, uv.contiguous(), image, image.shape[0], image.shape[1], normal_image,
         normals, tangents, *cam, H, W, ambient, kind, rgb, nrm, lit, counters)
    return dict(face=face, depth=depth, bary=bary, kind=kind, rgb=rgb, nrm=nrm, lit=lit, info=raster_info(counts.tolist()),
                tex_info=texture_raster_info(counters.tolist()))
