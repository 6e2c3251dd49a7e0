"""Trained-like weights for the SDF and colour networks, the seeded inputs their tests share, and the float64 truth -- TEST INFRASTRUCTURE ONLY.

torch and numpy on the CPU.  The initialisers (weights.init_sdf_weights, weights.init_color_state_dict, the golden networks) give b0 = b1 = 0, one
constant in b2, one constant in the w2 row and zero biases in four of the five colour heads: on such values every indexing of a bias vector gives
the same answer.  The families here have what a trained checkpoint has -- distinct non-zero biases, a spread w2 row with both signs, PE and latent
columns of O(0.1), weight-norm gains g != ||v||, a negative s -- so that a bias read at the wrong lane, block or scale moves the output by orders of
magnitude more than the tolerance (tests/test_trained_weights_cpu.py holds that as a gate: ten times the bound or more).

The truth is oracle/recon.py (sdf, sdf_grad, rendering_network) on .double() inputs and weights: the functions are dtype-generic.  The float32
call of the same functions gives e_ref, the accuracy class of a float32 evaluation, for rule E (tests/sampler_ref.py: rule_e_bound).  Nothing here
is derived from a kernel's output.

Bounds (sdf_bounds, color_bound), per case and output:
  fp32 forms        rule E: 4 e_ref + 4 ulp of the output's magnitude
  split-f16 forms   rule E + 2e-6 max(1, |sdf|max) for the SDF (as test_sdf_mlp_x3 grants), + 5e-6 for the colour (test_weights_packing.py), rule E alone
                    for the gradient
  ceiling           never looser than close()'s tolerance of that output in tests/test_gpu_parity.py: 2e-5 max(1, magnitude) for SDF, features and latent,
                    1e-4 max(1, magnitude) for the gradient and the colour."""
import functools
import importlib

import numpy as np
import torch

from oracle import recon as O
from sampler_ref import rule_e_bound

Wn = importlib.import_module("one-2-3-45_amd.weights")
F32, F64 = torch.float32, torch.float64

SDF_BIAS_KEYS = ("b0", "b1", "b2")
COLOR_BIAS_VECTORS = ("ray_dir_fc.0", "ray_dir_fc.2", "base_fc.0", "base_fc.2", "vis_fc.0", "vis_fc.2", "vis_fc2.0", "rgb_fc.0", "rgb_fc.2")
# the single-output heads: vis_fc.2's row 32, vis_fc2.2, rgb_fc.4 -- the three scalars behind CM_S (weights.CM_LAYOUT["S_SCALAR"])
COLOR_BIAS_SCALARS = (("vis_fc.2", 32), ("vis_fc2.2", 0), ("rgb_fc.4", 0))
# per-vector sigma where the sensitivity gate asks for more than 0.1: vis_fc.2, for its row 32 -- at 0.1 zeroing that scalar moves the colour by 4e-5
# to 8e-5, 7 to 12 times the bound; vis_fc2.0, the weakest vector, passes at 0.1 (1e-3 to 3e-3)
COLOR_BIAS_SIGMA = {"vis_fc.2": 0.5}
COLOR_S = -0.37


# ------------------------------------------------------------------------------------------------ families
@functools.lru_cache(maxsize=None)
def trained_sdf_weights(seed=0):
    """A dict like weights.init_sdf_weights: b0, b1 ~ N(0, 0.1), b2 ~ -0.5 + N(0, 0.1) (384 distinct non-zero values), PE and latent columns at
    sigma 0.1, every hidden entry of w2 (all 128 rows: variant 1 writes every row) times U(0.25, 1.75) with its sign flipped with probability 0.2."""
    W = Wn.init_sdf_weights(seed, latent_scale=0.1, pe_scale=0.1)
    rng = np.random.default_rng(7000 + seed)
    W["b0"] = rng.normal(0, 0.1, 128).astype(np.float32)
    W["b1"] = rng.normal(0, 0.1, 128).astype(np.float32)
    W["b2"] = (-0.5 + rng.normal(0, 0.1, 128)).astype(np.float32)
    scale = rng.uniform(0.25, 1.75, (128, 128)) * np.where(rng.uniform(0, 1, (128, 128)) < 0.2, -1.0, 1.0)
    W["w2"] = W["w2"].copy()
    W["w2"][:, :128] = (W["w2"][:, :128] * scale).astype(np.float32)
    for v in W.values():
        v.setflags(write=False)
    return W


def trained_sdf_state_dict(W, seed=0):
    """W under the reference's names lin{0,1,2}.{bias,weight_g,weight_v}: weight_v = W's rows times a random factor, weight_g = the float32 row
    norm of W, so that g v / ||v|| gives W back and g != ||v|| in every row.  The factors are drawn from {1/2, 2}, the powers of two inside [0.3, 3]:
    then v and ||v|| are exact multiples of W and ||W||, the fold is fl(fl(g w) / g) and returns W to 1 ulp.  With any other factor v = fl(w f)
    carries a rounding of its own and 3 to 6 % of the folded entries are 2 or 3 ulp from W (measured), which no fold could undo."""
    rng = np.random.default_rng(7100 + seed)
    sd = {}
    for i in range(3):
        w = torch.from_numpy(np.array(W[f"w{i}"], np.float32))
        f = torch.from_numpy(rng.choice(np.array([0.5, 2.0], np.float32), (w.shape[0], 1)))
        sd[f"lin{i}.weight_v"] = (w * f).contiguous()
        sd[f"lin{i}.weight_g"] = w.norm(dim=1, keepdim=True).contiguous()
        sd[f"lin{i}.bias"] = torch.from_numpy(np.array(W[f"b{i}"], np.float32))
    return sd


@functools.lru_cache(maxsize=None)
def trained_color_state_dict(seed=0):
    """weights.init_color_state_dict plus N(0, 0.1) on every bias (COLOR_BIAS_SIGMA for the vectors that take another sigma), s = -0.37"""
    sd = Wn.init_color_state_dict(seed)
    rng = np.random.default_rng(7200 + seed)
    for k in sorted(sd):
        if k.endswith(".bias"):
            sigma = COLOR_BIAS_SIGMA.get(k[:-len(".bias")], 0.1)
            sd[k] = (sd[k] + rng.normal(0, sigma, sd[k].shape)).astype(np.float32)
    sd["s"] = np.float32(COLOR_S)
    for v in sd.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sd


def sdf_t(W, dtype=F32):
    return {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in W.items()}


def color_t(sd, dtype=F32):
    return {k: torch.as_tensor(np.array(v), dtype=F32).to(dtype) for k, v in sd.items()}


def swap_extremes(vec):
    """a copy of the vector with its largest and smallest entry exchanged: the reference-side stand-in of a bias read at the wrong place"""
    v = np.array(vec)
    i, j = int(np.argmax(v)), int(np.argmin(v))
    v[i], v[j] = v[j], v[i]
    return v


def sdf_perturbations(W):
    """-> [(name, weights with one vector perturbed, the outputs that depend on it)]: what the sensitivity gate exchanges.  b0, b1 and the two parts
    of the w2 row reach SDF, features and gradient; b2 the features (variant 1 reads all 128 entries), and b2[0] <-> b2[1] the SDF of the kernels
    that read entry 0 alone; b2 drops out of the gradient, and the latent depends on no weight."""
    w2h, w2l, b2x = np.array(W["w2"]), np.array(W["w2"]), np.array(W["b2"])
    w2h[0, :128] = swap_extremes(w2h[0, :128])
    w2l[0, 128:] = swap_extremes(w2l[0, 128:])
    b2x[[0, 1]] = b2x[[1, 0]]
    every = ("sdf", "feat", "grad")
    return [("b0", dict(W, b0=swap_extremes(W["b0"])), every), ("b1", dict(W, b1=swap_extremes(W["b1"])), every),
            ("b2", dict(W, b2=swap_extremes(W["b2"])), ("feat",)), ("b2[1] for b2[0]", dict(W, b2=b2x), ("sdf", "feat")),
            ("w2 hidden row", dict(W, w2=w2h), every), ("w2 latent row", dict(W, w2=w2l), every)]


def color_perturbations(sd):
    """-> [(name, state dict with one bias vector's extremes exchanged / one scalar zeroed / s = 0.2, pinned)]; pinned: "yes", "V>=5" (s: with two
    views the pooling weights are 1 and 0 whatever s is) or "never" (rgb_fc.4.bias shifts every view's score alike and cancels in the softmax)"""
    out = []
    for name in COLOR_BIAS_VECTORS:
        v = np.array(sd[name + ".bias"])
        if name == "vis_fc.2":
            v[:32] = swap_extremes(v[:32])                       # the 32 rows that are a vector in the blob; row 32 is one of the scalars
        else:
            v = swap_extremes(v)
        out.append((name, dict(sd, **{name + ".bias": v}), "yes"))
    for name, idx in COLOR_BIAS_SCALARS:
        v = np.array(sd[name + ".bias"])
        v[idx] = 0.0
        out.append((f"{name}[{idx}] zeroed", dict(sd, **{name + ".bias": v}), "never" if name == "rgb_fc.4" else "yes"))
    out.append(("s = 0.2", dict(sd, s=np.float32(0.2)), "V>=5"))
    return out


# ------------------------------------------------------------------------------------------------ rule E and the ceilings
def bounded(ref32, ref64, extra=0.0, ceiling=2e-5):
    """-> (e_ref, bound): rule E plus ``extra``, never above ``ceiling`` * max(1, magnitude) (close() of tests/test_gpu_parity.py)"""
    e_ref, bound = rule_e_bound(ref32, ref64)
    mag = ref64.abs().max().item() if ref64.numel() else 0.0
    return e_ref, min(bound + extra, ceiling * max(1.0, mag))


# ------------------------------------------------------------------------------------------------ SDF inputs
SDF_DS = (2, 3, 17, 20)            # 2: the smallest side the entry accepts; 17: lattice nodes exactly representable; 20: the small scene's side
SDF_NS = (1, 33, 257, 2048)        # one live lane; two tiles; two workgroups; eight workgroups = the smallest launch on the per-XCD tile schedule
# every D and every n at least twice, n = 257 (the index + n_dev run) with the two sides that have interior cells, n = 2048 with them and with the
# volume that is all boundary
SDF_CASES = [(2, 33), (3, 257), (17, 2048), (20, 1), (17, 257), (20, 2048), (2, 1), (3, 33), (2, 2048)]
PLANT_BOTH = ("minus_one", "above_minus_one", "plus_one", "corner_band", "beyond")      # compared for value AND gradient (see sdf_points)
LATTICE_CASES = [(9, 17), (33, 20)]                                                      # (R, D): R = 9 on D = 17 puts every lattice point on a node


@functools.lru_cache(maxsize=None)
def sdf_volume(D, seed=0):
    """dense N(0, 1) latent volume [16,D,D,D] float32"""
    g = torch.Generator().manual_seed(7300 + 10 * D + seed)
    return torch.randn(16, D, D, D, generator=g).contiguous()


def index_of(p, D, dtype):
    """the sampler's index computation i = (p + 1) / 2 (D - 1) in ``dtype`` -> (i, floor, ok)"""
    i = (p.to(dtype) + 1) / 2 * (D - 1)
    return i, torch.floor(i), ((i > 0) & (i < D)).all(-1)


def _first_beyond(D):
    """the first float32 coordinate at which the index i reaches D in float32 AND in float64 arithmetic (trilinear_ref: zero from there on)"""
    p = np.float32(-1.0 + 2.0 * D / (D - 1))
    for _ in range(8):
        p = np.nextafter(p, np.float32(-np.inf))
    for _ in range(64):
        t = torch.tensor([[float(p)] * 3], dtype=F32)
        if all(bool((index_of(t, D, dt)[0] >= D).all()) for dt in (F32, F64)):
            return float(p)
        p = np.nextafter(p, np.float32(np.inf))
    raise AssertionError("no coordinate found")


@functools.lru_cache(maxsize=None)
def sdf_points(D, n, seed=0):
    """-> (pts float32 [n,3], rows): U(-1.12, 1.12)^3; from n = 33 on the first rows are planted, one coordinate on the named edge, the other two
    random inside the volume.  rows: name -> row index.
      minus_one        exactly -1 on one axis: i = 0, the latent is zero          above_minus_one  the next float above -1: the first sampled point
      plus_one         exactly +1: i = D - 1, the last node                       corner_band      1 + 1 / (D - 1): inside D - 1 < i < D (clamped corner)
      beyond           the first float with i >= D in float32 and in float64: zero again
      node0..node3     D = 17 only: points exactly on volume nodes (weights 1 and 0), one of them on three nodes' planes at once
      nan, huge        a NaN row and a 1e30 row: the sampler promises a zero latent and no read outside the volume (geom_math.h trilinear_ref_taps); the
                       embedding of such a point is not finite, so their SDF is compared with nothing
    On every planted row both precisions take the same cell and the same side of ``ok`` (the CPU test asserts it): at -1 + ulp, +1 and the nodes the
    index is exact; the trilinear sample JUMPS at i = 0 and i = D (to zero), which is why `beyond` is chosen where float32 and float64 agree."""
    g = torch.Generator().manual_seed(7400 + 100 * D + n + seed)
    pts = (torch.rand(n, 3, generator=g, dtype=F64) * 2.24 - 1.12).float()
    rows = {}
    if n >= 33:
        inner = (torch.rand(16, 3, generator=g, dtype=F64) * 1.6 - 0.8).float()
        plant = [("minus_one", -1.0), ("above_minus_one", float(np.nextafter(np.float32(-1.0), np.float32(0.0)))), ("plus_one", 1.0),
                 ("corner_band", float(np.float32(1.0 + 1.0 / (D - 1)))), ("beyond", _first_beyond(D))]
        for k, (name, v) in enumerate(plant):
            pts[k] = inner[k]
            pts[k, k % 3] = v
            rows[name] = k
        k = len(plant)
        if D == 17:
            node = lambda j: -1.0 + 2.0 * j / 16.0               # exactly representable
            for name, p in (("node0", (node(5), inner[k, 1], inner[k, 2])), ("node1", (inner[k + 1, 0], node(16), inner[k + 1, 2])),
                            ("node2", (node(3), node(8), node(11))), ("node3", (inner[k + 3, 0], inner[k + 3, 1], node(1)))):
                pts[k] = torch.tensor([float(c) for c in p])
                rows[name] = k
                k += 1
        pts[k] = inner[k]
        pts[k, 1] = float("nan")
        rows["nan"] = k
        pts[k + 1] = inner[k + 1]
        pts[k + 1, 2] = 1e30
        rows["huge"] = k + 1
    return pts.contiguous(), rows


def compared_rows(n, rows):
    """bool [n]: the rows compared with the truth (all but nan / huge)"""
    keep = torch.ones(n, dtype=torch.bool)
    for name in ("nan", "huge"):
        if name in rows:
            keep[rows[name]] = False
    return keep


def sdf_eval(pts, vol, W, dtype):
    """the oracle in ``dtype`` -> dict(y [P,128], lat [P,16], grad [P,3])"""
    Wd = sdf_t(W, dtype)
    y, lat = O.sdf(pts.to(dtype), vol.to(dtype), Wd)
    return dict(y=y, lat=lat, grad=O.sdf_grad(pts.to(dtype), vol.to(dtype), Wd))


@functools.lru_cache(maxsize=None)
def sdf_case(D, n, seed=0):
    """-> dict(pts, rows, keep, vol, r32, r64): the case's inputs and the oracle's float32 / float64 results on the compared rows"""
    pts, rows = sdf_points(D, n, seed)
    keep = compared_rows(n, rows)
    vol = sdf_volume(D, seed)
    W = trained_sdf_weights(seed)
    return dict(D=D, n=n, pts=pts, rows=rows, keep=keep, vol=vol, r32=sdf_eval(pts[keep], vol, W, F32), r64=sdf_eval(pts[keep], vol, W, F64))


def sdf_bounds(r32, r64):
    """-> {(output, precision): (e_ref, bound)} for output in sdf / feat / lat / grad, precision in fp32 / f16x3 (module docstring)"""
    s32, s64 = r32["y"][:, 0], r64["y"][:, 0]
    x3 = 2e-6 * max(1.0, s64.abs().max().item() if s64.numel() else 0.0)
    return {("sdf", "fp32"): bounded(s32, s64), ("sdf", "f16x3"): bounded(s32, s64, extra=x3),
            ("feat", "fp32"): bounded(r32["y"], r64["y"]), ("lat", "fp32"): bounded(r32["lat"], r64["lat"]),
            ("grad", "fp32"): bounded(r32["grad"], r64["grad"], ceiling=1e-4), ("grad", "f16x3"): bounded(r32["grad"], r64["grad"], ceiling=1e-4)}


INDEX_DS = (3, 17)
INDEX_LISTED, INDEX_N_DEV = 150, 101


@functools.lru_cache(maxsize=None)
def index_case(D, seed=0):
    """sdf_case(D, 257) through an index list of 150 rows and a device-side count of 101 -> dict(idx int32 [150], listed: the 101 rows evaluated,
    rows: those of them compared with the truth, r32 / r64: the oracle on them)"""
    c = sdf_case(D, 257, seed)
    idx = torch.randperm(257, generator=torch.Generator().manual_seed(D + seed))[:INDEX_LISTED].to(torch.int32)
    listed = idx[:INDEX_N_DEV].long()
    rows = listed[c["keep"][listed]]
    pos = torch.cumsum(c["keep"].long(), 0) - 1                                      # row -> its place among the compared rows
    return dict(c, idx=idx, listed=listed, cmp_rows=rows, r32={k: v[pos[rows]] for k, v in c["r32"].items()},
                r64={k: v[pos[rows]] for k, v in c["r64"].items()})


@functools.lru_cache(maxsize=None)
def given_latents_case(D, seed=0):
    """get_sdf_volume's call: every voxel centre with the voxel's OWN latent row, about 30 % of the voxels kept -> dict(pts [D^3,3], vol, kept bool
    [D^3], r32 / r64: the SDF of the kept voxels from oracle.sdf_mlp)"""
    vol = sdf_volume(D, seed)
    pts = lattice_points(D)                                                          # voxel index * 2 / (D - 1) - 1
    kept = torch.rand(D ** 3, generator=torch.Generator().manual_seed(D + seed)) < 0.3
    return dict(D=D, pts=pts, vol=vol, kept=kept, **{name: given_latents_eval(pts[kept], vol, kept, trained_sdf_weights(seed), dt)
                                                      for name, dt in (("r32", F32), ("r64", F64))})


def given_latents_eval(pts, vol, kept, W, dtype):
    lat = vol.reshape(16, -1).T[kept]
    return O.sdf_mlp(pts.to(dtype), lat.to(dtype), sdf_t(W, dtype))[:, 0]


def lattice_points(R):
    lin = torch.linspace(-1, 1, R)
    return torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3).contiguous()


@functools.lru_cache(maxsize=None)
def kept_voxels(D):
    """bool [D,D,D]: a few kept voxels for the sparse lattice form -- a 3^3 block off centre, one voxel at the first corner, one at the last"""
    kept = torch.zeros(D, D, D, dtype=torch.bool)
    c = D // 2
    kept[c - 1:c + 2, c:c + 3, c - 2:c + 1] = True
    kept[0, 0, 0] = kept[D - 1, D - 1, D - 1] = True
    return kept


@functools.lru_cache(maxsize=None)
def lattice_case(R, D, masked=False, seed=0):
    """the extraction lattice linspace(-1, 1, R)^3 on the case's volume (masked: zeroed outside kept_voxels(D)) -> dict(pts, vol, r32, r64: sdf [R^3])"""
    pts = lattice_points(R)
    vol = sdf_volume(D, seed)
    if masked:
        vol = (vol * kept_voxels(D)[None].float()).contiguous()
    W = trained_sdf_weights(seed)
    ev = lambda dt: O.sdf(pts.to(dt), vol.to(dt), sdf_t(W, dt))[0][:, 0]
    return dict(R=R, D=D, pts=pts, vol=vol, r32=ev(F32), r64=ev(F64))


# ------------------------------------------------------------------------------------------------ colour inputs
COLOR_VS = (2, 5, 8, 19)
COLOR_PS = (1, 33, 257)
COLOR_CASES = [(V, P) for V in COLOR_VS for P in COLOR_PS]


@functools.lru_cache(maxsize=None)
def color_inputs(V, P, seed=0):
    """Materialised tensors in the reference's layout: geometry_feat [P,16] N(0,1); rgb_feat [V,P,59] (colours in [0,1], features N(0,1)); ray_diff
    [V,P,4] (difference of two unit directions, their dot product); mask [V,P] with about 30 % of the views hidden.  From P = 33 on, point 0 is
    seen by no view and point 1 by exactly one."""
    g = torch.Generator().manual_seed(7500 + 100 * V + P + seed)
    geo = torch.randn(P, 16, generator=g)
    rf = torch.cat([torch.rand(V, P, 3, generator=g), torch.randn(V, P, 56, generator=g)], -1)
    a = torch.nn.functional.normalize(torch.randn(V, P, 3, generator=g), dim=-1)
    b = torch.nn.functional.normalize(torch.randn(1, P, 3, generator=g), dim=-1).expand(V, P, 3)
    rd = torch.cat([b - a, (a * b).sum(-1, keepdim=True)], -1)
    mask = torch.rand(V, P, generator=g) > 0.3
    if P >= 33:
        mask[:, 0] = False
        mask[:, 1] = False
        mask[V // 2, 1] = True
    return dict(V=V, P=P, geo=geo.contiguous(), rf=rf.contiguous(), rd=rd.contiguous(), mask=mask.contiguous())


def color_eval(d, sd, dtype):
    """the oracle network in ``dtype`` -> (rgb [P,3], valid views [P])"""
    return O.rendering_network(color_t(sd, dtype), d["geo"].to(dtype), d["rf"].to(dtype), d["rd"].to(dtype), d["mask"])


@functools.lru_cache(maxsize=None)
def color_case(V, P, seed=0):
    d = color_inputs(V, P, seed)
    sd = trained_color_state_dict(seed)
    (r32, _), (r64, nv) = color_eval(d, sd, F32), color_eval(d, sd, F64)
    return dict(d, r32=r32, r64=r64, nviews=nv)


MANY_VS = (33, 64, 65, 255)                  # past the list sort's 32 views | the last count with the view skip | the first without | the uint8 maximum
MANY_CASES = [(V, P) for V in MANY_VS for P in COLOR_PS]
MASK_KINDS = ("tile_hidden", "tile_hidden_one_blind", "all_views", "one_view")
BLIND_POINT = 5


def many_view_mask(V, P, kind, seed=0):
    """The masks color_inputs' random 30 % never draws, on the first 32-point tile (one wave of k_color_pts; all P points when P < 32):
      tile_hidden            every view from 32 on -- view 32 at V = 33, view 63 at V = 64 -- hidden from the whole tile, every point of which keeps a
                             view below 32: the wave-uniform skip drops those views in both passes
      tile_hidden_one_blind  the same, and point BLIND_POINT (point 0 when P is smaller) seen by no view: the network pass may skip nothing
      all_views              every view valid for every point: the count reaches V
      one_view               point p seen by view (V - 1 - p) mod V alone: point 0 by the last view
    -> bool [V,P]"""
    mask = color_inputs(V, P, seed)["mask"].clone()
    n = min(P, 32)
    if kind in ("tile_hidden", "tile_hidden_one_blind"):
        mask[32:, :n] = False
        mask[torch.arange(n) % 32, torch.arange(n)] = True
        if kind == "tile_hidden_one_blind":
            mask[:, min(BLIND_POINT, P - 1)] = False
    elif kind == "all_views":
        mask[:] = True
    elif kind == "one_view":
        mask[:] = False
        mask[(V - 1 - torch.arange(P)) % V, torch.arange(P)] = True
    else:
        raise KeyError(kind)
    return mask.contiguous()


@functools.lru_cache(maxsize=None)
def many_view_case(V, P, kind=None, seed=0):
    """color_case(V, P) (kind None), or the same tensors under many_view_mask(V, P, kind) with the oracle's float32 / float64 colours for that mask"""
    if kind is None:
        return color_case(V, P, seed)
    d = dict(color_inputs(V, P, seed), mask=many_view_mask(V, P, kind, seed))
    sd = trained_color_state_dict(seed)
    (r32, _), (r64, nv) = color_eval(d, sd, F32), color_eval(d, sd, F64)
    return dict(d, r32=r32, r64=r64, nviews=nv)


def color_bound(r32, r64, x3):
    """-> (e_ref, bound): rule E (+ 5e-6 for the split-f16 form), never above 1e-4 max(1, magnitude)"""
    return bounded(r32, r64, extra=5e-6 if x3 else 0.0, ceiling=1e-4)
