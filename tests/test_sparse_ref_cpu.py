"""tests/sparse_ref.py on the CPU: its references equal the oracle (oracle/recon.py: downsample_coords, build_kmap + sparse_conv, sparse_costreg) on
every seeded family -- lists and grids exactly, float64 values to 1e-10 --, its two operand splits equal the product's packers, and the families
reach the edges tests/test_gpu_sparse_units.py relies on.  Prints, per case, e_ref = max |float32 reference - float64| and e_split = max |split-f16
model - float64|: the two yardsticks of the GPU test.  No GPU."""
import importlib

import numpy as np
import pytest
import torch

import sparse_ref as R
from oracle import recon as O

Wn = importlib.import_module("one-2-3-45_amd.weights")


def _level(xyz, ts):
    return O.SparseLevel(xyz * ts, ts)


def _oracle_chain(xyz, ts, n=3):
    out = [_level(xyz, ts)]
    for _ in range(n):
        out.append(O.downsample_coords(out[-1]))
    return out


# ------------------------------------------------------------------------------------------------ the pieces against the product's packers
def test_splits_and_layer_table_match_the_package():
    x = np.concatenate([np.random.default_rng(0).normal(0, 1, 4096), [0.0, 1.0, -1.0, 2.0 ** -15, -2.0 ** -20, 1 + 2.0 ** -11, 1000.25]]).astype(np.float32)
    for a, b in zip(R.split_activations(x), Wn.f16_split_device(x)):
        assert np.array_equal(a, b)
    hi, lo = R.split_activations(x)
    assert (np.abs(hi) <= np.abs(x)).all() and (np.abs(hi + lo) <= np.abs(x)).all()                  # both halves toward zero
    assert np.abs(hi.astype(np.float64) + lo - x).max() <= 2.0 ** -20 * np.abs(x).max()
    for a, b in zip(R.split_weights(x), Wn.f16_split(x)):
        assert np.array_equal(a, b.astype(np.float32))
    assert [(n, ci, co) for n, ci, co, _ in R.NET_LAYERS] == list(Wn.COSTREG_LAYERS)
    # the blob of pack_sparse_conv_x3 holds exactly these halves: lane (i, h) of block nb, step (k, u), element t = W[k][16u + 8h + t][32 nb + i]
    K = R.draw_kernel(np.random.default_rng(1), 32, 16, 0).numpy()
    blob = Wn.pack_sparse_conv_x3(K).view(np.float16).reshape(27, 2, 1, 2, 2, 32, 8)               # [k][u][nb][hi|lo][h][i][t]
    wh, wl = R.split_weights(K)
    for half, want in ((0, wh), (1, wl)):
        got = blob[:, :, 0, half].transpose(0, 1, 2, 4, 3).reshape(27, 32, 32)[:, :, :16]          # [k][u][h][t][i] -> [k][ci][co]
        assert np.array_equal(got.astype(np.float32), want)
    # the network's kernels are drawn like init_costreg_state_dict's: inside +-1/sqrt(27 fan), and filling that range
    for name, ci, co, mode in R.NET_LAYERS:
        K = R.net_weights()[name][0]
        b = 1.0 / np.sqrt((co if mode == 2 else ci) * 27)
        ref = Wn.init_costreg_state_dict(0)[f"{name}.net.0.kernel"]
        assert K.shape == ref.shape and K.abs().max() <= b and K.abs().max() > 0.99 * b and np.abs(ref).max() <= b


# ------------------------------------------------------------------------------------------------ levels
@pytest.mark.parametrize("ts", R.TENSOR_STRIDES)
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_levels_equal_the_oracle(fam, ts):
    cells, xyz = R.family(fam)
    chain = R.level_chain(xyz, cells, 3)
    want = _oracle_chain(xyz, ts, 3)
    for i, ((x, c, g), L) in enumerate(zip(chain, want)):
        assert L.ts == ts << i
        assert torch.equal(x * L.ts, L.xyz), f"level {i}: list / order"
        # the grid is the oracle's lookup of every cell
        allc = torch.from_numpy(np.stack(np.unravel_index(np.arange(c[0] * c[1] * c[2]), c), -1)).long()
        assert torch.equal(g.long(), L.lookup(allc * L.ts)), f"level {i}: index grid"
        assert torch.equal(R.coords4(x, L.ts)[:, :3].long(), L.xyz) and (R.coords4(x, L.ts)[:, 3] == 0).all()
        if i:
            assert c == tuple((p + 1) // 2 + 1 for p in chain[i - 1][1])


def test_empty_level():
    xc, g = R.coarse_level(torch.zeros(0, 3, dtype=torch.long), (9, 14, 11))
    assert xc.shape == (0, 3) and g.shape == (6 * 8 * 7,) and (g == -1).all()
    assert (R.index_grid(torch.zeros(0, 3), (5, 6, 7)) == -1).all()


# ------------------------------------------------------------------------------------------------ convolutions
def _conv_cases():
    cases = [(fam, ci, co, m, R.LEVEL_KIND[fam], ts) for fam, ci, co, m, ts in R.LEVEL_CASES]
    cases += [(fam, ci, co, m, "normal", 1) for fam in R.COUNT_FAMILIES for ci, co, m in R.FP32_COUNT_PAIRS + R.LDS_PAIRS + R.STREAM_PAIRS]
    cases += [(fam, 32, 16, 0, "normal", 1) for fam in R.BRICK_FAMILIES]
    cases += [(fam, 32, 16, 0, "uniform", 1) for fam in ("voxel", "two")]
    return sorted(set(cases))


@pytest.mark.parametrize("fam,cin,cout,mode,kind,ts_out", _conv_cases())
def test_convolutions_equal_the_oracle(fam, cin, cout, mode, kind, ts_out):
    c = R.conv_case(fam, cin, cout, mode, kind, ts_out)
    Lin, Lout = _level(c["in_xyz"], c["ts_in"]), _level(c["out_xyz"], c["ts_out"])
    x64, K64 = c["x"].double(), c["K"].double()
    if mode == 2:
        kmap = O.build_kmap(Lout, Lin)                       # the down map with the roles swapped: [coarse row, k] -> fine row
        want = O.sparse_conv(x64, kmap, K64, transposed=True, n_out=len(c["out_xyz"]))
        q, k = torch.nonzero(kmap >= 0, as_tuple=True)
        assert int((c["nbr"] >= 0).sum()) == len(q) and torch.equal(c["nbr"][kmap[q, k], k], q)
    else:
        kmap = O.build_kmap(Lin, Lout)
        want = O.sparse_conv(x64, kmap, K64)
        assert torch.equal(c["nbr"], kmap)
    scale = max(1.0, c["ref64"].abs().max().item())
    assert c["ref64"].shape == (len(c["out_xyz"]), cout) and c["ref64"].dtype == torch.float64
    assert (c["ref64"] - want).abs().max().item() <= 1e-10 * scale                                   # dense ATen = the oracle's sparse convolution
    assert (R.conv_offsets(x64, c["nbr"], K64) - c["ref64"]).abs().max().item() <= 1e-10 * scale       # and = the per-offset walk the yardsticks use
    print(f"{fam} {cin}->{cout} mode {mode} ts_out {ts_out} {kind}: rows {len(c['out_xyz'])}, e_ref {c['e_ref']:.2e}, e_split {c['e_split']:.2e}, "
          f"max |ref| {c['ref64'].abs().max().item():.3g}")
    # both yardsticks are float32-class: a model that dropped a term or an offset would sit far above this
    assert c["e_ref"] <= 1e-6 * scale and c["e_split"] <= 2e-6 * scale


def test_isolated_rows_are_the_centre_tap():
    for fam in ("voxel", "two"):
        c = R.conv_case(fam, 32, 16, 0, "uniform", 1)
        assert ((c["nbr"] >= 0).sum(1) == 1).all() and (c["nbr"][:, 13] == torch.arange(len(c["x"]))).all()
        assert (c["ref64"] - c["x"].double() @ c["K"][13].double()).abs().max().item() <= 1e-12


# ------------------------------------------------------------------------------------------------ the whole network
@pytest.mark.parametrize("random_affine", [True, False])
@pytest.mark.parametrize("fam", R.NET_FAMILIES)
def test_network_equals_the_oracle(fam, random_affine):
    n = R.net_case(fam, random_affine)
    coords = R.coords4(n["xyz"], 1)
    w64 = {k: tuple(t.double() for t in v) for k, v in n["w"].items()}
    want, extra = O.sparse_costreg(n["feat"].double(), coords, w64)
    for (x, _, _), L in zip(n["levels"], extra["levels"]):
        assert torch.equal(x * L.ts, L.xyz)
    scale = max(1.0, n["out"].abs().max().item())
    assert (n["out"] - want).abs().max().item() <= 1e-10 * scale
    got32, _ = O.sparse_costreg(n["feat"], coords, n["w"])
    e32 = (got32.double() - n["out"]).abs().max().item()
    print(f"{fam} affine {'random' if random_affine else '1, 0'}: levels {[len(x) for x, _, _ in n['levels']]}, oracle float32 - float64 {e32:.2e}, "
          f"max |ref| {n['out'].abs().max().item():.3g} (bound {1e-5 * scale:.2e})")
    assert e32 <= 1e-5 * scale                              # a tenth of the GPU test's tolerance: the families that it runs stay inside


def test_single_row_levels_give_relu_beta():
    for fam, sizes in (("blob", [60, 12, 4, 1]), ("blob3", [27, 8, 1, 1]), ("voxel", [1, 1, 1, 1])):
        n = R.net_case(fam)
        assert [len(x) for x, _, _ in n["levels"]] == sizes
        for name, lvl in (("conv5", 3), ("conv6", 3)) + ((("conv3", 2), ("conv4", 2)) if sizes[2] == 1 else ()):
            beta = n["w"][name][2].double()
            assert torch.equal(n["blocks"][name], torch.relu(beta)[None]) and (beta > 0).any() and (beta < 0).any()
        if sizes[2] == 1:                                    # conv7 up from one row to one row: relu(beta) + the skip
            assert torch.equal(n["blocks"]["conv7"], torch.relu(n["w"]["conv7"][2].double())[None] + n["blocks"]["conv4"])


# ------------------------------------------------------------------------------------------------ what the families reach
def test_minimum_rule_reach():
    """Per axis: an odd and an even minimum among the families (the same cells serve every tensor stride, so this holds at ts 1 and ts 2 alike, and
    test_levels_equal_the_oracle runs both); a candidate dropped by the rule on each axis; an odd minimum at a coarse level; mixed parities."""
    mins = {fam: R.family(fam)[1].min(0).values.tolist() for fam in R.FAMILIES}
    for a in range(3):
        assert any(m[a] % 2 == 1 for m in mins.values()) and any(m[a] % 2 == 0 for m in mins.values())
    assert any(len({v % 2 for v in m}) == 2 for m in mins.values())                                 # another parity on one axis than on the others
    for ts in (1, 2):                                        # ... of the lists the kernels are given at that stride, in cells
        for a in range(3):
            par = {int(R.coords4(R.family(fam)[1], ts)[:, a].min()) // ts % 2 for fam in R.SHAPE_FAMILIES}
            assert par == {0, 1}
    dropped = [0, 0, 0]
    coarse_odd = False
    for fam in R.SHAPE_FAMILIES:
        cells, xyz = R.family(fam)
        for lvl, (x, c, _) in enumerate(R.level_chain(xyz, cells, 2)):
            if not len(x):
                continue
            mn = x.min(0).values
            coarse_odd |= lvl > 0 and bool((mn % 2 == 1).any())
            for a in range(3):                               # a cell at the odd minimum has the even candidate minimum - 1 below it: dropped
                dropped[a] += int(mn[a] % 2 == 1)
            # without the rule the level would be larger exactly when some axis has an odd minimum
            free = torch.unique(torch.cat([torch.div(x + torch.tensor(o), 2, rounding_mode="floor")[((x + torch.tensor(o)) % 2 == 0).all(1)]
                                           for o in R._box((-1, -1, -1), (3, 3, 3)).tolist()]), dim=0)
            assert (len(free) > len(R.coarse_level(x, c)[0])) == bool((mn % 2 == 1).any())
    assert all(dropped) and coarse_odd


def test_neighbourhood_reach():
    cnt = (R.conv_case("blob", 32, 16, 0, "uniform", 1)["nbr"] >= 0).sum(1)
    assert (cnt == 27).any()
    assert ((R.conv_case("two", 32, 16, 0, "uniform", 1)["nbr"] >= 0).sum(1) == 1).all()
    up = R.conv_case("blob", 64, 32, 2, "uniform", 4)
    assert len({tuple(p) for p in (up["out_xyz"] % 2).tolist()}) == 8                               # all eight parity classes of output cells
    assert ((up["nbr"] >= 0).sum(1) <= 8).all()
    # a 32-row tile with an offset that exactly one of its rows has: the wave-uniform skip must not decide on one lane's behalf
    lone = 0
    for fam, args in (("random", (32, 16, 0, "normal", 1)), ("n513", (16, 16, 0, "normal", 1)), ("n3585", (64, 64, 0, "normal", 1))):
        has = R.conv_case(fam, *args)["nbr"] >= 0
        for t in range(0, len(has), 32):
            lone += int((has[t:t + 32].sum(0) == 1).sum())
    assert lone > 0
    # ... and a tile where the one row is not the first of its wave half (lane 0 / lane 32 are where a per-lane decision would be read from)
    has = R.conv_case("random", 32, 16, 0, "normal", 1)["nbr"] >= 0
    assert any(((has[t:t + 32].sum(0) == 1) & ~has[t]).any() for t in range(0, len(has), 32))


def test_last_cell_and_brick_reach():
    cells, xyz = R.family("full")                            # 5 x 6 x 7: the last plane of an odd and of an even extent
    xc, _ = R.coarse_level(xyz, cells)
    nc = R.coarse_cells(cells)
    for a in range(3):
        assert int(xc[:, a].max()) == cells[a] // 2
    assert int(xc[:, 1].max()) == nc[1] - 1                  # even extent: the last cell the allocation has room for
    cells, xyz = R.family("random5x6x33")
    assert (xyz[:, 2] == 32).any() and (xyz[:, 0] == 4).any()                                        # the one-cell bricks are occupied
    assert cells[2] % 16 == 1 and cells[0] % 4 == 1
    for n in R.COUNTS_16:                                    # persistent grid of 8 -> the XCD-contiguous schedule
        want = -(-n // 512)
        assert want == 8 and len(R.family(f"n{n}")[1]) == n
    ntiles = -(-3585 // 32)
    chunk = (ntiles + 7) // 8
    assert ntiles == 113 and 7 * chunk < ntiles < 8 * chunk and ntiles - 7 * chunk == 8 and 3585 % 32 == 1
    assert -(-3970 // 128) == 32
    for n in R.COUNTS_9x14x11:
        assert len(R.family(f"n{n}")[1]) == n
