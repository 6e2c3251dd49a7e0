"""The sparse cost-regularisation network unit by unit: ops.build_index_grid, ops.sparse_downsample, ops.sparse_conv3d (fp32 VALU kernel),
ops.sparse_conv3d_x3 (gather form with the operands in LDS, gather form streaming them, brick form) and costreg.CostRegNet.forward, each entry alone,
against the references of tests/sparse_ref.py (checked on the CPU by tests/test_sparse_ref_cpu.py, which also asserts what the seeded families reach).

Integer work -- index grids, coarse lists and their order, counts, lattice sizes -- is compared bit for bit.  Convolutions are compared with the
float64 dense ATen convolution under rule E: max |gpu - ref64| <= 4 e + 4 ulp of the output's magnitude, where e is, for the
fp32 kernel, e_ref = max |ref32 - ref64| of the same case (ref32: 27 per-offset float32 products accumulated in float32) and, for the split-f16 forms,
max(e_ref, e_split), e_split = max |split model - ref64| (the model: x_hi W_hi + x_hi W_lo + x_lo W_hi summed in float64, i.e. the error the form has
by construction without the device's accumulation order).  Every comparison prints e_ref, e_split, the device error and its share of the bound.
The network is compared with the float64 network at the tolerance of test_gpu_parity.py::test_sparse_cnn_and_scatter, 1e-4 * max(1, max |ref|).

Shapes: every (cin, cout, mode) of COSTREG_LAYERS and (48, 16, 0), each at the level it has in the network and one level coarser (ts_out 1 ... 16:
the division c / ts); 1, 31, 32, 33, 127, 129, 511, 513 rows (a lane, a ragged wave, a tile, the streaming form's block of 128 rows, one round of the
persistent form); 3,585 and 3,970 rows of a 16^3 lattice (persistent grid 8: the XCD-contiguous schedule with a ragged last eighth and a last tile of
one row); lattices 9 x 14 x 11, 5 x 6 x 7, 16^3 and 5 x 6 x 33 (one-cell last bricks); blobs with odd per-axis minima, isolated voxels, single-row levels.

Measured on the MI355X (yardsticks computed on the CPU; DESIGN.md section 4, "Sparse network units: what pins what"), as device error (share of the bound):
fp32 kernel e_ref <= 5.5e-6, device <= 4.5e-6 (0.09 ... 0.19); gather form with operands in LDS e_ref <= 6.5e-6, e_split <= 4.7e-6, device <= 2.0e-5
(0.11 ... 0.63); streaming gather form e_ref <= 1.0e-5, e_split <= 7.6e-6, device <= 3.8e-5 (0.14 ... 0.68); brick form device <= 1.1e-5 (0.10 ... 0.33);
network f16x3 <= 1.3e-5 (0.024 of 1e-4 * |ref|), fp32 <= 2.3e-6 (0.004); blocks on a single row 0 ... 1.5e-8.  Before this file the fp32 kernel summed all
27 * cin products of an output in one chain and measured up to 2.6e-5 and up to 1.06 of its bound (64 -> 64 on the random family, 32 -> 16 on 5 x 6 x 33); it
now sums each offset's products on their own, as the yardstick does."""
import importlib

import pytest
import torch

import sparse_ref as R

pytestmark = pytest.mark.gpu
Wn = importlib.import_module("one-2-3-45_amd.weights")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    importlib.import_module("one-2-3-45_amd._lib").lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("one-2-3-45_amd.ops")


def rule_e(got, c, what, x3, ref64=None):
    """Rule E of one conv_case: the fp32 kernel on e_ref, the split-f16 forms on max(e_ref, e_split)."""
    ref64 = c["ref64"] if ref64 is None else ref64
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    yard = max(c["e_ref"], c["e_split"]) if x3 else c["e_ref"]
    bound = R.rule_e_bound(yard, c["ref64"])
    err = (got - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f"{what} [{'x3' if x3 else 'fp32'}]: e_ref {c['e_ref']:.2e}, e_split {c['e_split']:.2e}, device err {err:.2e}, bound {bound:.2e} "
          f"({err / bound if bound else 0:.2f})")
    assert err <= bound, f"{what}: device err {err:.3e} > 4 * {yard:.3e} + 4 ulp = {bound:.3e}"


def conv_args(c, dev):
    return (c["x"].to(dev), c["in_grid"].to(dev), c["in_cells"], R.coords4(c["out_xyz"], c["ts_out"]).to(dev), c["ts_out"])


def blob_of(c, dev):
    return torch.from_numpy(Wn.pack_sparse_conv_x3(c["K"].numpy())).to(dev)


# ------------------------------------------------------------------------------------------------ ops.build_index_grid
@pytest.mark.parametrize("ts", R.TENSOR_STRIDES)
@pytest.mark.parametrize("fam", [None, "random", "full", "random5x6x7", "random16", "n3970", "random5x6x33", "full5x6x33", "voxel", "n513"])
def test_build_index_grid(dev, ops, fam, ts):
    for lat in (R.LATTICES.values() if fam is None else [R.family(fam)[0]]):                         # fam None: n = 0 on all four lattices
        xyz = torch.zeros(0, 3, dtype=torch.long) if fam is None else R.family(fam)[1]
        got = ops.build_index_grid(R.coords4(xyz, ts).to(dev), ts, lat)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), R.index_grid(xyz, lat))


# ------------------------------------------------------------------------------------------------ ops.sparse_downsample
@pytest.mark.parametrize("ts", R.TENSOR_STRIDES)
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_sparse_downsample(dev, ops, fam, ts):
    cells, xyz = R.family(fam)
    want_xyz, want_grid = R.coarse_level(xyz, cells)
    grid, co, n, nc = ops.sparse_downsample(R.coords4(xyz, ts).to(dev), ts, cells)
    assert n == len(want_xyz) and tuple(nc) == R.coarse_cells(cells)
    assert torch.equal(co.cpu(), R.coords4(want_xyz, 2 * ts))                                        # the list, its order, batch column 0
    assert torch.equal(grid.cpu(), want_grid)


@pytest.mark.parametrize("fam", R.SHAPE_FAMILIES + ("n1", "n33", "n513", "n3585", "random5x6x33"))
def test_sparse_downsample_chain(dev, ops, fam):
    """The three calls of CostRegNet.forward, each on the previous call's own output."""
    cells, xyz = R.family(fam)
    want = R.level_chain(xyz, cells, 3)
    co, c = R.coords4(xyz, 1).to(dev), cells
    for lvl in (1, 2, 3):
        grid, co, n, c = ops.sparse_downsample(co, 1 << (lvl - 1), c)
        wx, wc, wg = want[lvl]
        assert n == len(wx) and tuple(c) == wc, f"level {lvl}"
        assert torch.equal(co.cpu(), R.coords4(wx, 1 << lvl)) and torch.equal(grid.cpu(), wg), f"level {lvl}"


def test_sparse_downsample_of_nothing(dev, ops):
    for ts in R.TENSOR_STRIDES:
        grid, co, n, nc = ops.sparse_downsample(torch.zeros(0, 4, dtype=torch.int32, device=dev), ts, (9, 14, 11))
        assert n == 0 and tuple(co.shape) == (0, 4) and tuple(nc) == (6, 8, 7) and grid.shape == (6 * 8 * 7,) and bool((grid == -1).all())


# ------------------------------------------------------------------------------------------------ ops.sparse_conv3d, ops.sparse_conv3d_x3
@pytest.mark.parametrize("fam,cin,cout,mode,ts_out", R.LEVEL_CASES)
def test_conv_at_its_level_and_one_coarser(dev, ops, fam, cin, cout, mode, ts_out):
    """Every (cin, cout, mode) the two networks launch, at the tensor stride it has there and at twice that: fp32 kernel and gather form; for
    (32, 16, 0) the brick form as well."""
    c = R.conv_case(fam, cin, cout, mode, R.LEVEL_KIND[fam], ts_out)
    args, what = conv_args(c, dev), f"{fam} {cin}->{cout} mode {mode} ts_out {ts_out}"
    rule_e(ops.sparse_conv3d(mode, *args, c["K"].to(dev)), c, what, False)
    rule_e(ops.sparse_conv3d_x3(mode, *args, blob_of(c, dev), cout), c, what + " gather", True)
    if (cin, cout, mode) == (32, 16, 0):
        rule_e(ops.sparse_conv3d_x3(mode, *args, blob_of(c, dev), cout, identity_rows=True), c, what + " brick", True)


@pytest.mark.parametrize("fam", R.COUNT_FAMILIES)
@pytest.mark.parametrize("cin,cout,mode", R.FP32_COUNT_PAIRS)
def test_conv_row_counts_fp32(dev, ops, fam, cin, cout, mode):
    c = R.conv_case(fam, cin, cout, mode, "normal", 1)
    rule_e(ops.sparse_conv3d(mode, *conv_args(c, dev), c["K"].to(dev)), c, f"{fam} {cin}->{cout} mode {mode}", False)


@pytest.mark.parametrize("fam", R.COUNT_FAMILIES)
@pytest.mark.parametrize("cin,cout,mode", R.LDS_PAIRS + R.STREAM_PAIRS)
def test_conv_row_counts_gather_forms(dev, ops, fam, cin, cout, mode):
    """LDS-resident form (16/32 -> 16/32: persistent workgroups of 16 tiles; 3,585 and 3,970 rows take the XCD-contiguous schedule) and streaming form
    (the others: blocks of 4 tiles).  identity_rows stays False, so (32, 16) runs the gather form here."""
    c = R.conv_case(fam, cin, cout, mode, "normal", 1)
    rule_e(ops.sparse_conv3d_x3(mode, *conv_args(c, dev), blob_of(c, dev), cout), c, f"{fam} {cin}->{cout} mode {mode}", True)


@pytest.mark.parametrize("fam", R.BRICK_FAMILIES)
def test_conv_brick_form(dev, ops, fam):
    """The brick form on all four lattices (5 x 6 x 33: one-cell last bricks on x and z), and the same layer without the identity-row guarantee on a
    reversed subset of the sites."""
    c = R.conv_case(fam, 32, 16, 0, "normal", 1)
    args, blob = conv_args(c, dev), blob_of(c, dev)
    out = ops.sparse_conv3d_x3(0, *args, blob, 16, identity_rows=True)
    rule_e(out, c, f"{fam} brick", True)
    sub = torch.arange(len(c["out_xyz"]) - 1, -1, -3)
    x, grid, cells, coords, ts = args
    got = ops.sparse_conv3d_x3(0, x, grid, cells, coords[sub.to(dev)].contiguous(), ts, blob, 16)
    rule_e(got, c, f"{fam} gather, reversed subset", True, ref64=c["ref64"][sub])
    rule_e(ops.sparse_conv3d(0, x, grid, cells, coords[sub.to(dev)].contiguous(), ts, c["K"].to(dev)), c, f"{fam} reversed subset", False, ref64=c["ref64"][sub])


@pytest.mark.parametrize("fam", ["voxel", "two"])
def test_conv_isolated_rows_are_the_centre_tap(dev, ops, fam):
    c = R.conv_case(fam, 32, 16, 0, "uniform", 1)
    centre = c["x"].double() @ c["K"][13].double()
    args = conv_args(c, dev)
    rule_e(ops.sparse_conv3d(0, *args, c["K"].to(dev)), c, f"{fam} centre tap", False, ref64=centre)
    rule_e(ops.sparse_conv3d_x3(0, *args, blob_of(c, dev), 16), c, f"{fam} centre tap, gather", True, ref64=centre)
    rule_e(ops.sparse_conv3d_x3(0, *args, blob_of(c, dev), 16, identity_rows=True), c, f"{fam} centre tap, brick", True, ref64=centre)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv_of_nothing(dev, ops, mode):
    c = R.conv_case("blob", 16, 16, mode, "uniform", 2 if mode == 1 else 1)
    x, grid, cells, coords, ts = conv_args(c, dev)
    K, blob = c["K"].to(dev), blob_of(c, dev)
    none4, nox = torch.zeros(0, 4, dtype=torch.int32, device=dev), torch.zeros(0, 16, device=dev)
    empty_grid = torch.full_like(grid, -1)
    for got in (ops.sparse_conv3d(mode, x, grid, cells, none4, ts, K), ops.sparse_conv3d_x3(mode, x, grid, cells, none4, ts, blob, 16)):
        assert tuple(got.shape) == (0, 16)
    for got in (ops.sparse_conv3d(mode, nox, empty_grid, cells, coords, ts, K), ops.sparse_conv3d_x3(mode, nox, empty_grid, cells, coords, ts, blob, 16)):
        assert tuple(got.shape) == (len(coords), 16) and bool((got == 0).all())


# ------------------------------------------------------------------------------------------------ costreg.CostRegNet.forward
def net_close(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    bound = 1e-4 * max(1.0, ref.abs().max().item() if ref.numel() else 1.0)
    print(f"{what}: device err {err:.2e}, bound {bound:.2e} ({err / bound:.3f})")
    assert err <= bound, f"{what}: device err {err:.3e} > {bound:.3e}"


@pytest.fixture(scope="module")
def nets(dev):
    costreg = importlib.import_module("one-2-3-45_amd.costreg")
    sd = R.state_dict_of(R.net_weights(0, True))
    return {p: costreg.CostRegNet(sd, dev, precision=p) for p in ("f16x3", "fp32")}


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("fam", R.NET_FAMILIES)
def test_network(dev, nets, fam, precision):
    """gamma in [0.5, 1.5], beta normal(0, 0.2) in every layer: a single-row level gives relu(beta), not 0, so its rows are checked at all."""
    n, net = R.net_case(fam), nets[precision]
    out = net.forward(n["feat"].to(dev), R.coords4(n["xyz"], 1).to(dev), None, n["cells"])
    assert list(net.level_sizes) == [len(x) for x, _, _ in n["levels"]]
    for lvl, (co, (x, _, _)) in enumerate(zip(net.levels, n["levels"])):
        assert torch.equal(co.cpu(), R.coords4(x, 1 << lvl)), f"level {lvl}"
    net_close(out, n["out"], f"network {fam} {precision}, levels {list(net.level_sizes)}")


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("fam", ["blob", "blob3", "voxel"])
def test_network_single_row_levels(dev, nets, fam, precision):
    """The blocks that run on a level of one row, each alone on the float64 network's own inputs: batch statistics of one row leave relu(beta), plus
    the skip where the block has one."""
    n, net = R.net_case(fam), nets[precision]
    L, B = n["levels"], n["blocks"]
    f32 = lambda t: t.float().to(dev)
    lv = lambda i: (L[i][2].to(dev), L[i][1], R.coords4(L[i][0], 1 << i).to(dev), 1 << i)
    g3, c3, co3, ts3 = lv(3)
    assert len(L[3][0]) == 1
    beta = lambda name: torch.relu(n["w"][name][2].double())[None]
    net_close(net._blk("conv5", f32(B["conv4"]), 1, *lv(2)[:2], co3, ts3), beta("conv5"), f"{fam} {precision} conv5 onto one row")
    net_close(net._blk("conv6", f32(B["conv5"]), 0, g3, c3, co3, ts3), beta("conv6"), f"{fam} {precision} conv6 on one row")
    if len(L[2][0]) == 1:
        g2, c2, co2, ts2 = lv(2)
        net_close(net._blk("conv4", f32(B["conv3"]), 0, g2, c2, co2, ts2), beta("conv4"), f"{fam} {precision} conv4 on one row")
        net_close(net._blk("conv7", f32(B["conv6"]), 2, g3, c3, co2, ts2, skip=f32(B["conv4"])), beta("conv7") + B["conv4"],
                  f"{fam} {precision} conv7 one row up to one row, with the skip")
        assert torch.equal(B["conv7"], beta("conv7") + B["conv4"])


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_network_of_nothing(dev, nets, precision):
    out = nets[precision].forward(torch.zeros(0, 32, device=dev), torch.zeros(0, 4, dtype=torch.int32, device=dev), None, (9, 14, 11))
    assert tuple(out.shape) == (0, 16) and list(nets[precision].level_sizes) == [0, 0, 0, 0]
