"""Plain references of the sparse cost-regularisation network's units, and the seeded families their tests share -- TEST INFRASTRUCTURE ONLY.

torch and numpy on the CPU; neither the product package nor oracle/recon.py is imported here.  Every reference is written from the DEFINITION of its
operation: a level's index grid is the row of every cell; the next-coarser level is a 3 x 3 x 3 max-pool of the occupancy read at the even cells (less
the cells below the input's per-axis minimum, the rule of torchsparse's spdownsample); a sparse convolution is ATen's DENSE convolution of the
zero-filled lattice read at the output sites.  The float32 yardstick and the split-f16 model need the 27 per-offset products one by one, so they walk
a neighbour map built from the index grid; tests/test_sparse_ref_cpu.py checks that walk in float64 against the dense convolutions and everything
here against the oracle, and asserts that the families reach the edges they were chosen for; tests/test_gpu_sparse_units.py compares the HIP kernels
with these references on the very same inputs.

Conventions: a coordinate list is [n,3] int64 in CELLS, x-major sorted unless a test reorders it; `coords4(xyz, ts)` makes the [n,4] int32 list the
kernels take (cells * ts, batch 0).  A kernel K is [27,cin,cout], offset k = (oz+1)*9 + (oy+1)*3 + (ox+1)."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import frontend_ref as FR

F64 = torch.float64
ULP = 2.0 ** -23


def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else abs(int(k)) for k in key])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ levels
def coords4(xyz, ts):
    """[n,3] cells -> the kernels' coordinate list [n,4] int32: (x, y, z) * ts, batch 0."""
    xyz = torch.as_tensor(xyz).long().reshape(-1, 3)
    return torch.cat([xyz * ts, torch.zeros(len(xyz), 1, dtype=torch.long)], 1).int().contiguous()


def index_grid(xyz, cells):
    """The row of every cell of the lattice, or -1: int32 [nx*ny*nz], x-major."""
    g = torch.full(tuple(cells), -1, dtype=torch.int32)
    xyz = torch.as_tensor(xyz).long().reshape(-1, 3)
    if len(xyz):
        g[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = torch.arange(len(xyz), dtype=torch.int32)
    return g.reshape(-1)


def coarse_cells(cells):
    """The lattice ops.sparse_downsample allocates for the next level."""
    return tuple((int(c) + 1) // 2 + 1 for c in cells)


def coarse_level(xyz, cells):
    """The next-coarser level of the cells `xyz` of a lattice of `cells` cells -> (xyz_c [m,3] in coarse cells, x-major, its index grid on coarse_cells(cells)).
    Ones on the dense lattice, max-pooled 3 x 3 x 3, read at the even cells; cells below the per-axis minimum of the input dropped.  (Tensor strides do
    not enter: the list at stride ts is cells * ts, its coarse list is coarse cells * 2 ts.)"""
    nc = coarse_cells(cells)
    xyz = torch.as_tensor(xyz).long().reshape(-1, 3)
    if not len(xyz):
        return torch.zeros(0, 3, dtype=torch.long), index_grid(xyz, nc)
    ext = tuple(int(c) + 2 for c in cells)                 # room for the even cell behind an odd last cell
    occ = torch.zeros((1, 1) + ext, dtype=F64)
    occ[0, 0, xyz[:, 0], xyz[:, 1], xyz[:, 2]] = 1.0
    pooled = F.max_pool3d(occ, 3, stride=1, padding=1)[0, 0]
    even = torch.nonzero(pooled[::2, ::2, ::2] > 0) * 2    # fine-cell coordinates of the kept even cells, x-major
    even = even[(even >= xyz.min(0).values[None]).all(1)]
    xyz_c = even // 2
    assert all(int(xyz_c[:, a].max()) < nc[a] for a in range(3))
    return xyz_c, index_grid(xyz_c, nc)


def level_chain(xyz, cells, n=3):
    """-> [(xyz, cells, grid)] of the level itself and its n coarser levels."""
    out = [(torch.as_tensor(xyz).long().reshape(-1, 3), tuple(cells), index_grid(xyz, cells))]
    for _ in range(n):
        x, c, _ = out[-1]
        xc, gc = coarse_level(x, c)
        out.append((xc, coarse_cells(c), gc))
    return out


# ------------------------------------------------------------------------------------------------ convolutions
def dense_weight(K):
    """K [27,ci,co] (x fastest) -> conv3d weight [co,ci,3,3,3] indexed (dx, dy, dz)."""
    ci, co = K.shape[1:]
    return K.reshape(3, 3, 3, ci, co).permute(4, 3, 2, 1, 0).contiguous()


def dense_weight_transposed(K):
    """K [27,ci,co] -> conv_transpose3d weight [ci,co,3,3,3]."""
    ci, co = K.shape[1:]
    return K.reshape(3, 3, 3, ci, co).permute(3, 4, 2, 1, 0).contiguous()


def _dense(xyz, x, ext):
    g = torch.zeros((1, x.shape[1]) + tuple(ext), dtype=x.dtype)
    if len(xyz):
        g[0, :, xyz[:, 0], xyz[:, 1], xyz[:, 2]] = x.T
    return g


def conv_dense(mode, x, in_xyz, in_cells, out_xyz, K):
    """The convolution as ATen's dense one, in the precision of x (float64: the truth): zero-filled input lattice, read at the output cells."""
    K = K.to(x.dtype)
    if mode == 2:
        y = F.conv_transpose3d(_dense(in_xyz, x, in_cells), dense_weight_transposed(K), stride=2, padding=1, output_padding=1)[0]
    else:
        ext = tuple(int(c) + 2 + int(c) % 2 for c in in_cells)            # even extents with a free plane behind the last cell
        y = F.conv3d(_dense(in_xyz, x, ext), dense_weight(K), stride=1 + mode, padding=1)[0]
    assert not len(out_xyz) or all(int(out_xyz[:, a].max()) < y.shape[1 + a] for a in range(3))
    return y[:, out_xyz[:, 0], out_xyz[:, 1], out_xyz[:, 2]].T.contiguous()


def neighbour_map(mode, in_grid, in_cells, out_xyz):
    """[n_out,27] int64: the input row that offset k pairs with every output cell, or -1.  mode 0: cell + o; 1: 2 cell + o on the finer level;
    2: (cell - o) / 2 on the coarser level, only where all three of cell - o are even."""
    g = torch.as_tensor(in_grid).long().reshape(tuple(in_cells))
    q = torch.as_tensor(out_xyz).long().reshape(-1, 3)
    lim = torch.tensor(tuple(in_cells))
    nb = torch.full((len(q), 27), -1, dtype=torch.long)
    for k in range(27):
        o = torch.tensor([k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1])
        if mode == 0:
            c, ok = q + o, torch.ones(len(q), dtype=torch.bool)
        elif mode == 1:
            c, ok = 2 * q + o, torch.ones(len(q), dtype=torch.bool)
        else:
            d = q - o
            c, ok = torch.div(d, 2, rounding_mode="floor"), (d % 2 == 0).all(1)
        ok = ok & (c >= 0).all(1) & (c < lim).all(1)
        c = c[ok]
        nb[ok, k] = g[c[:, 0], c[:, 1], c[:, 2]]
    return nb


def conv_offsets(x, nbr, K):
    """out[q] = sum over k of x[nbr[q, k]] @ K[k]: 27 per-offset products, accumulated in the precision of x (float32: the yardstick -- ATen's own
    float32 convolution may accumulate otherwise and understate it)."""
    K = K.to(x.dtype)
    out = torch.zeros(nbr.shape[0], K.shape[2], dtype=x.dtype)
    for k in range(27):
        idx = nbr[:, k]
        v = idx >= 0
        if v.any():
            out[v] += x[idx[v]] @ K[k]
    return out


def _f16_rtz(v):
    """float32 -> the nearest float16 toward zero (v_cvt_pkrtz_f16_f32), returned as float32."""
    v = np.ascontiguousarray(v, np.float32)
    h = v.astype(np.float16)
    h = np.where(np.abs(h.astype(np.float32)) > np.abs(v), np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def split_activations(x):
    """csrc/split_f16.h, C form: hi = f16(x) toward zero, lo = f16(x - hi) toward zero of the exact float32 difference -> float32 arrays."""
    x = np.ascontiguousarray(x, np.float32)
    hi = _f16_rtz(x)
    return hi, _f16_rtz(x - hi)


def split_weights(K):
    """weights.pack_sparse_conv_x3: both halves rounded to nearest -> float32 arrays."""
    K = np.ascontiguousarray(K, np.float32)
    hi = K.astype(np.float16).astype(np.float32)
    return hi, (K - hi).astype(np.float16).astype(np.float32)


def conv_split_model(x, nbr, K):
    """The split-f16 form's value without the device's accumulation order: sum of x_hi W_hi + x_hi W_lo + x_lo W_hi in float64."""
    xh, xl = (torch.from_numpy(a).double() for a in split_activations(x.numpy()))
    wh, wl = (torch.from_numpy(a).double() for a in split_weights(K.numpy()))
    return conv_offsets(xh, nbr, wh + wl) + conv_offsets(xl, nbr, wh)


def rule_e_bound(e_yard, ref64):
    """Rule E on a yardstick error: 4 e + 4 ulp of the output's magnitude."""
    mag = ref64.abs().max().item() if ref64.numel() else 0.0
    return 4 * e_yard + 4 * ULP * mag


# ------------------------------------------------------------------------------------------------ the network
NET_LAYERS = [("conv0", 32, 16, 0), ("conv1", 16, 16, 1), ("conv2", 16, 16, 0), ("conv3", 16, 32, 1), ("conv4", 32, 32, 0), ("conv5", 32, 64, 1),
              ("conv6", 64, 64, 0), ("conv7", 64, 32, 2), ("conv9", 32, 16, 2), ("conv11", 16, 16, 2)]
NET_TS_OUT = dict(conv0=1, conv1=2, conv2=2, conv3=4, conv4=4, conv5=8, conv6=8, conv7=4, conv9=2, conv11=1)
CONV_COMBOS = [(ci, co, m) for _, ci, co, m in NET_LAYERS] + [(48, 16, 0)]                       # (48, 16): the lod-1 network's input width
COMBO_TS_OUT = [NET_TS_OUT[n] for n, _, _, _ in NET_LAYERS] + [1]


def draw_kernel(g, cin, cout, mode, kind="uniform"):
    """uniform(+-1/sqrt(27 fan)) as init_costreg_state_dict draws it (fan = cout for a transposed layer), or normal(0, 0.2)."""
    if kind == "normal":
        return _t(g.normal(0.0, 0.2, (27, cin, cout)))
    b = 1.0 / np.sqrt((cout if mode == 2 else cin) * 27)
    return _t(g.uniform(-b, b, (27, cin, cout)))


@functools.lru_cache(maxsize=None)
def net_weights(seed=0, random_affine=True):
    """name -> (kernel [27,ci,co], gamma, beta): gamma uniform in [0.5, 1.5] and beta normal(0, 0.2) in every layer, or 1 and 0."""
    g = _rng("net", seed)
    w = {}
    for name, ci, co, mode in NET_LAYERS:
        K = draw_kernel(g, ci, co, mode)
        gamma, beta = _t(g.uniform(0.5, 1.5, co)), _t(g.normal(0.0, 0.2, co))
        w[name] = (K, gamma, beta) if random_affine else (K, torch.ones(co), torch.zeros(co))
    return w


def state_dict_of(w):
    sd = {}
    for name, (K, gamma, beta) in w.items():
        sd[f"{name}.net.0.kernel"], sd[f"{name}.net.1.weight"], sd[f"{name}.net.1.bias"] = K.numpy(), gamma.numpy(), beta.numpy()
    return sd


def net_forward(feat, xyz, cells, w):
    """The U-net of costreg.py in float64 -> (rows [n,16], dict(levels = the four (xyz, cells, grid), blocks = every block's output by name)).
    conv0; conv1 down, conv2; conv3 down, conv4; conv5 down, conv6; conv7 up + conv4; conv9 up + conv2; conv11 up + conv0; every block is the
    convolution, batch normalisation with the batch's own statistics and ReLU; the skip is added after the activation."""
    L = level_chain(xyz, cells, 3)
    modes = {name: mode for name, _, _, mode in NET_LAYERS}
    blocks = {}

    def blk(name, x, lin, lout, skip=None):
        K, gamma, beta = w[name]
        nbr = neighbour_map(modes[name], L[lin][2], L[lin][1], L[lout][0])
        y = FR.bn_rows(conv_offsets(x.double(), nbr, K.double()), gamma, beta, eps=1e-5, slope=0.0, skip=skip)[0] if len(L[lout][0]) else \
            torch.zeros(0, K.shape[2], dtype=F64)
        blocks[name] = y
        return y

    c0 = blk("conv0", feat, 0, 0)
    c2 = blk("conv2", blk("conv1", c0, 0, 1), 1, 1)
    c4 = blk("conv4", blk("conv3", c2, 1, 2), 2, 2)
    x = blk("conv6", blk("conv5", c4, 2, 3), 3, 3)
    x = blk("conv7", x, 3, 2, skip=c4)
    x = blk("conv9", x, 2, 1, skip=c2)
    x = blk("conv11", x, 1, 0, skip=c0)
    return x, dict(levels=L, blocks=blocks)


# ------------------------------------------------------------------------------------------------ the seeded families
LATTICES = {"9x14x11": (9, 14, 11), "5x6x7": (5, 6, 7), "16x16x16": (16, 16, 16), "5x6x33": (5, 6, 33)}      # 5x6x33: three z-bricks of the brick
#                                                                        form with 1 cell in the last, two x-bricks with 1 cell in the last
COUNTS_9x14x11 = (1, 31, 32, 33, 127, 129, 511, 513)        # one lane | ragged wave | one tile | a second tile | around the streaming form's block of
#                                                             128 rows | around one round (512 rows) of the persistent form
COUNTS_16 = (3585, 3970)     # persistent grid 8 for both: the XCD-contiguous schedule.  3,585 rows = 113 tiles, chunks of 15: the last eighth has 8 tiles
#                              and the last tile one row; 3,970 rows also give the streaming form a grid of 32


def _box(lo, size):
    ax = [np.arange(l, l + s) for l, s in zip(lo, size)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def _sample(name, cells, n=None, p=None):
    g = _rng("set", name)
    ncell = cells[0] * cells[1] * cells[2]
    lin = np.sort(g.choice(ncell, n, replace=False)) if n is not None else np.flatnonzero(g.random(ncell) < p)
    return np.stack(np.unravel_index(lin, cells), -1)


def _family_table():
    f = {"blob": ("9x14x11", lambda c: _box((3, 4, 5), (4, 5, 3))),
         "blob3": ("9x14x11", lambda c: _box((1, 1, 1), (3, 3, 3))),
         "voxel": ("9x14x11", lambda c: np.array([[5, 6, 7]])),
         "two": ("9x14x11", lambda c: np.array([[1, 1, 1], [7, 12, 9]])),
         "full": ("5x6x7", lambda c: _box((0, 0, 0), c)),
         "random": ("9x14x11", lambda c: _sample("random", c, p=0.3)),
         "random5x6x7": ("5x6x7", lambda c: _sample("random5x6x7", c, p=0.3)),
         "random16": ("16x16x16", lambda c: _sample("random16", c, p=0.3)),
         "random5x6x33": ("5x6x33", lambda c: _sample("random5x6x33", c, p=0.3)),
         "full5x6x33": ("5x6x33", lambda c: _box((0, 0, 0), c))}
    for n in COUNTS_9x14x11:
        f[f"n{n}"] = ("9x14x11", lambda c, n=n: _sample(f"n{n}", c, n=n))
    for n in COUNTS_16:
        f[f"n{n}"] = ("16x16x16", lambda c, n=n: _sample(f"n{n}", c, n=n))
    return f


_FAMILIES = _family_table()
FAMILIES = tuple(_FAMILIES)
COUNT_FAMILIES = tuple(f"n{n}" for n in COUNTS_9x14x11 + COUNTS_16)
SHAPE_FAMILIES = ("blob", "blob3", "voxel", "two", "full", "random")
NET_FAMILIES = SHAPE_FAMILIES                                # the families the whole network runs on
BRICK_FAMILIES = COUNT_FAMILIES + ("full", "random5x6x7", "random", "random16", "random5x6x33", "full5x6x33")      # all four lattices
TENSOR_STRIDES = (1, 2, 4)


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (cells, xyz [n,3] int64 in cells, x-major)."""
    lat, make = _FAMILIES[name]
    cells = LATTICES[lat]
    xyz = torch.from_numpy(np.ascontiguousarray(make(cells))).long()
    key = (xyz[:, 0] * cells[1] + xyz[:, 1]) * cells[2] + xyz[:, 2]
    assert (key[1:] > key[:-1]).all() and (xyz >= 0).all() and (xyz < torch.tensor(cells)).all()
    return cells, xyz


def features(name, n, c):
    return _t(_rng("x", name, c).normal(0.0, 1.0, (n, c)))


@functools.lru_cache(maxsize=None)
def conv_case(fam, cin, cout, mode, kind="uniform", ts_out=1):
    """One convolution on a family, with all its references.  The family is the level the OUTPUT lives on for modes 0 and 2 (the input of mode 2 is its
    coarser level) and the level the INPUT lives on for mode 1 (the output is its coarser level); `ts_out` is the tensor stride of the output level.
    -> dict: in_xyz, in_cells, in_grid, ts_in, out_xyz, ts_out, x, K, nbr, ref64 (dense ATen, the truth), ref32 (27 float32 products), split (the
    split-f16 model), e_ref, e_split."""
    cells, xyz = family(fam)
    if mode == 0:
        in_xyz, in_cells, out_xyz, ts_in = xyz, cells, xyz, ts_out
    elif mode == 1:
        in_xyz, in_cells, out_xyz, ts_in = xyz, cells, coarse_level(xyz, cells)[0], ts_out // 2
        assert ts_out % 2 == 0
    else:
        in_xyz, in_cells, out_xyz, ts_in = coarse_level(xyz, cells)[0], coarse_cells(cells), xyz, ts_out * 2
    x = features(f"{fam}/{mode}", len(in_xyz), cin)
    K = draw_kernel(_rng("K", fam, cin, cout, mode, kind), cin, cout, mode, kind)
    in_grid = index_grid(in_xyz, in_cells)
    nbr = neighbour_map(mode, in_grid, in_cells, out_xyz)
    ref64 = conv_dense(mode, x.double(), in_xyz, in_cells, out_xyz, K)
    ref32 = conv_offsets(x, nbr, K)
    split = conv_split_model(x, nbr, K)
    e = lambda a: (a.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    return dict(in_xyz=in_xyz, in_cells=in_cells, in_grid=in_grid, ts_in=ts_in, out_xyz=out_xyz, ts_out=ts_out, x=x, K=K, nbr=nbr, ref64=ref64,
                ref32=ref32, split=split, e_ref=e(ref32), e_split=e(split))


LEVEL_CASES = [(fam, ci, co, m, ts * shift) for fam in ("blob", "random") for (ci, co, m), ts in zip(CONV_COMBOS, COMBO_TS_OUT) for shift in (1, 2)]
LEVEL_KIND = {"blob": "uniform", "random": "normal"}         # the random family carries the normal(0, 0.2) kernels

FP32_COUNT_PAIRS = [(16, 16, 0), (64, 32, 2)]               # the thread-per-row kernel: its guard is q < n_out in every instantiation
LDS_PAIRS = [(16, 16, 0), (16, 32, 0), (32, 16, 0), (32, 32, 0)]          # x3, operands resident in LDS, persistent workgroups of 16 tiles
STREAM_PAIRS = [(32, 64, 0), (64, 64, 0), (64, 32, 2), (48, 16, 0)]       # x3, operands streamed from L2, blocks of 128 rows


@functools.lru_cache(maxsize=None)
def net_case(fam, random_affine=True):
    cells, xyz = family(fam)
    feat = features(f"{fam}/net", len(xyz), 32)
    w = net_weights(0, random_affine)
    out, extra = net_forward(feat, xyz, cells, w)
    return dict(cells=cells, xyz=xyz, feat=feat, w=w, out=out, levels=extra["levels"], blocks=extra["blocks"])
