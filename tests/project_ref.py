"""Plain torch references of the projecting stages (voxel -> view and point -> view projection, the 2-D and 3-D zero-padded gathers, ray_diff, the
cost-volume rows, the list sort's visibility signature), and the seeded scenes and point families their tests share -- TEST INFRASTRUCTURE ONLY.

Every reference takes a dtype and evaluates ONE expression in it: float64 is the truth, float32 the yardstick of what rounding alone does to that
expression (rule E of DESIGN.md section 4).  They are written from the definition of each operation (reference lines cited, paths relative to
reconstruction/), not from the kernels and not through oracle/recon.py: tests/test_project_ref_cpu.py pins them against the oracle, the oracle against
the reference modules, and asserts that the input families reach the borders they were built for; tests/test_gpu_project_units.py compares the HIP
entries with them on the same inputs.  Image height H and width W are separate everywhere; no scene here is square.

The border band.  A mask is a comparison, and a float32 evaluation may fall on the other side of it than the float64 one when the compared quantity
lies within rounding of its threshold.  A (point, view) pair is AMBIGUOUS when, in float64, |gx| or |gy| lies within BAND * max(1, |value|) of 1, or z
within that distance of 0 or of its clamp, WITHOUT being equal to it (an exactly representable border is decided by <= against <, not by rounding);
a point is ambiguous for the geometry mask when a volume coordinate (g + 1) / 2 * (D - 1) lies that close to an integer without being one; a voxel is
ambiguous when one of its pairs is.  Ambiguous items are left out of comparisons with a reference and stay in every device-versus-device comparison."""
import functools
import importlib

import numpy as np
import torch

synth = importlib.import_module("one-2-3-45_amd.synth")

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
ULP = 2.0 ** -23
BAND = 8 * U
Z_CLAMP_VOXEL = 1e-6                    # ops/back_project.py:57
Z_CLAMP_POINT = 1e-3                    # ops/back_project.py:104 (cam2pixel)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ references
def lattice(dims):
    """x-major voxel lattice [dx*dy*dz, 3] of integer coordinates (ops/generate_grids.py:4-19), int64."""
    ax = [torch.arange(int(d)) for d in dims]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def voxel_world(dims, voxel_size, origin, dtype):
    """coords * voxel_size + origin evaluated in dtype from the float32 voxel size and origin (ops/back_project.py:44)."""
    return lattice(dims).to(dtype) * torch.tensor(np.float32(voxel_size).item(), dtype=dtype) + origin.to(dtype)[None]


def project(world, P, H, W, dtype):
    """Cost-volume projection (ops/back_project.py:49-63).  world [N,3], P [V,4,4] -> dict of [N,V]: gx, gy, z (before the clamp) and
    mask = |gx| <= 1 & |gy| <= 1 & z > 0; z >= 0 is clamped to >= 1e-6 before the division, negative z is left alone."""
    world, P = world.to(dtype), P.to(dtype)
    p = (P[None, :, :3, :3] * world[:, None, None, :]).sum(-1) + P[None, :, :3, 3]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    zc = torch.where(z >= 0, z.clamp(min=Z_CLAMP_VOXEL), z)
    gx = 2 * (x / zc) / (W - 1) - 1
    gy = 2 * (y / zc) / (H - 1) - 1
    return dict(gx=gx, gy=gy, z=z, mask=(gx.abs() <= 1) & (gy.abs() <= 1) & (z > 0))


def project_pts(pts, proj, H, W, dtype):
    """Colour-path projection (cam2pixel, ops/back_project.py:89-129, padding 'zeros').  pts [P,3], proj [V,3,4] = K @ w2c[:3] -> dict of [V,P]:
    gx, gy (a coordinate outside [-1, 1] is replaced by 2; gx_raw, gy_raw: before that), z (before its clamp to >= 1e-3) and mask = |gx| < 1 & |gy| < 1 (projector.py:188-190)."""
    pts, proj = pts.to(dtype), proj.to(dtype)
    p = (proj[:, None, :, :3] * pts[None, :, None, :]).sum(-1) + proj[:, None, :, 3]
    z = p[..., 2]
    zc = z.clamp(min=Z_CLAMP_POINT)
    gx = 2 * (p[..., 0] / zc) / (W - 1) - 1
    gy = 2 * (p[..., 1] / zc) / (H - 1) - 1
    two = torch.full_like(gx, 2.0)
    raw = dict(gx_raw=gx, gy_raw=gy)
    gx = torch.where((gx > 1) | (gx < -1), two, gx)
    gy = torch.where((gy > 1) | (gy < -1), two, gy)
    return dict(raw, gx=gx, gy=gy, z=z, mask=(gx.abs() < 1) & (gy.abs() < 1))


def bilinear(maps, gx, gy, dtype):
    """F.grid_sample 2-D, bilinear, zero padding, align_corners=True.  maps [V,C,H,W], gx / gy [V,N] -> [V,N,C]: pixel = (g + 1) / 2 * (size - 1), the
    four neighbours weighted by (1 - |dx|)(1 - |dy|), a neighbour outside the image contributes nothing."""
    maps, gx, gy = maps.to(dtype), gx.to(dtype), gy.to(dtype)
    V, C, H, W = maps.shape
    ix, iy = (gx + 1) / 2 * (W - 1), (gy + 1) / 2 * (H - 1)
    x0, y0 = ix.floor(), iy.floor()
    v = torch.arange(V)[:, None].expand_as(gx)
    out = torch.zeros(V, gx.shape[1], C, dtype=dtype)
    for yy, wy in ((y0, y0 + 1 - iy), (y0 + 1, iy - y0)):
        for xx, wx in ((x0, x0 + 1 - ix), (x0 + 1, ix - x0)):
            inside = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
            w = torch.where(inside, wx * wy, torch.zeros_like(wx))
            out += w[..., None] * maps[v, :, yy.clamp(0, H - 1).long(), xx.clamp(0, W - 1).long()]
    return out


def trilinear(volume, pts, dtype):
    """F.grid_sample 3-D, trilinear, zero padding, align_corners=True (render_utils.py:54-85).  volume [C,dx,dy,dz] (axes x, y, z), pts [P,3] -> [P,C]."""
    volume, pts = volume.to(dtype), pts.to(dtype)
    size = torch.tensor(volume.shape[1:], dtype=dtype)
    f = (pts + 1) / 2 * (size - 1)
    f0 = f.floor()
    out = torch.zeros(pts.shape[0], volume.shape[0], dtype=dtype)
    for corner in range(8):
        d = torch.tensor([(corner >> 2) & 1, (corner >> 1) & 1, corner & 1], dtype=dtype)
        c = f0 + d
        w = torch.where(d > 0, f - f0, f0 + 1 - f)
        inside = ((c >= 0) & (c <= size - 1)).all(1)
        ci = torch.minimum(c.clamp(min=0), size - 1).long()
        out += torch.where(inside, w.prod(1), torch.zeros_like(w[:, 0]))[:, None] * volume[:, ci[:, 0], ci[:, 1], ci[:, 2]].T
    return out


def geometry_mask(maskvol, pts, dtype):
    """projector.py:152-158: the point lies strictly inside the volume and the trilinear sample of the occupancy volume [dx,dy,dz] there is positive."""
    return (pts.abs() < 1).all(1) & (trilinear(maskvol[None], pts, dtype)[:, 0] > 0)


def query_dir(pts, dtype, query_cam=None, normals=None):
    """Direction a point is looked at from: (query_cam - p) / (|query_cam - p| + 1e-6) (projector.py:199-201), or its normal / max(|normal|, 1e-6)."""
    if normals is not None:
        n = normals.to(dtype)
        return n / n.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    q = query_cam.to(dtype)[None] - pts.to(dtype)
    return q / (q.norm(dim=-1, keepdim=True) + 1e-6)


def ray_diff(pts, qdir, cam_pos, dtype):
    """projector.py:65-94.  -> [V,P,4]: the normalised difference of the query direction and the direction to every source camera, and their dot product."""
    s = cam_pos.to(dtype)[:, None] - pts.to(dtype)[None]
    s = s / (s.norm(dim=-1, keepdim=True) + 1e-6)
    d = qdir.to(dtype)[None] - s
    return torch.cat([d / d.norm(dim=-1, keepdim=True).clamp(min=1e-6), (qdir.to(dtype)[None] * s).sum(-1, keepdim=True)], -1)


def project_features(s, pts, dtype, query_cam=None, normals=None):
    """Projector.compute / compute_view_independent on scene s -> dict(geo [P,16], rgb_feat [V,P,59] colour first, ray_diff [V,P,4], gmask [P],
    pmask [V,P], mask [V,P] = gmask & pmask, nviews [P])."""
    pr = project_pts(pts, s["proj"], s["H"], s["W"], dtype)
    gm = geometry_mask(s["maskvol"], pts, dtype)
    rf = torch.cat([bilinear(s["images"], pr["gx"], pr["gy"], dtype), bilinear(s["fmaps"], pr["gx"], pr["gy"], dtype)], -1)
    mask = gm[None] & pr["mask"]
    return dict(geo=trilinear(s["dense"], pts, dtype), rgb_feat=rf, ray_diff=ray_diff(pts, query_dir(pts, dtype, query_cam, normals), s["cam_pos"], dtype),
                gmask=gm, pmask=pr["mask"], mask=mask, nviews=mask.sum(0))


def costvol(feats, P, dims, voxel_size, origin, dtype, min_views=1, coords=None):
    """sparse_sdf_network.py:221-250, 286-362 on the whole lattice, or on the listed voxels coords [M,3].  feats [V,C,H,W] -> dict(cnt [M] valid views
    per voxel, keep [M] = cnt > min_views, coords [N,3] of the kept voxels in lattice order, inverse [M] (row of a kept voxel, else -1), rows [N,2C]
    = var | mean).  The sums run over ALL views, as in the reference (a view that does not see the voxel contributes its zero-padded sample, which is 0
    unless the voxel lies behind the camera); only the divisor, cnt + 1e-5, counts the valid ones."""
    xyz = lattice(dims) if coords is None else coords.long()
    world = xyz.to(dtype) * torch.tensor(np.float32(voxel_size).item(), dtype=dtype) + origin.to(dtype)[None]
    pr = project(world, P, feats.shape[2], feats.shape[3], dtype)
    cnt = pr["mask"].sum(1)
    keep = cnt > min_views
    f = bilinear(feats, pr["gx"][keep].T, pr["gy"][keep].T, dtype)              # [V,N,C]
    ic = 1.0 / (cnt[keep].to(dtype) + 1e-5)
    mean = f.sum(0) * ic[:, None]
    var = (f * f).sum(0) * ic[:, None] - mean * mean
    inverse = torch.full((xyz.shape[0],), -1, dtype=torch.long)
    inverse[keep] = torch.arange(int(keep.sum()))
    return dict(cnt=cnt, keep=keep, coords=xyz[keep], inverse=inverse, rows=torch.cat([var, mean], 1), pairs=pr)


def vis_signature(pts, proj, H, W, dtype):
    """Bit v of the key: the point projects STRICTLY inside view v's image, 0 < X / Z < W - 1 and 0 < Y / Z < H - 1 with Z clamped to >= 1e-3 -- the same
    set as project_pts' mask.  -> int64 [P]."""
    pr = project_pts(pts, proj, H, W, dtype)
    return (pr["mask"].long() << torch.arange(proj.shape[0])[:, None]).sum(0)


def rule_e_bound(ref32, ref64):
    """Rule E: e_ref = max |ref32 - ref64| -> (e_ref, 4 e_ref + 4 ulp of the output's magnitude)."""
    if not ref64.numel():
        return 0.0, 0.0
    e_ref = (ref32.double() - ref64).abs().max().item()
    return e_ref, 4 * e_ref + 4 * ULP * ref64.abs().max().item()


# ------------------------------------------------------------------------------------------------ the border band
def near(value, threshold, width=BAND):
    d = (value - threshold).abs()
    return (d < width * value.abs().clamp(min=1)) & (d != 0)


def ambiguous_pairs(pr64, z_clamp, width=BAND):
    """pr64: float64 output of project / project_pts -> bool, same shape: a compared quantity lies inside the band around its threshold (the image
    coordinates as they are before project_pts replaces those outside [-1, 1] by 2)."""
    gx, gy = pr64.get("gx_raw", pr64["gx"]), pr64.get("gy_raw", pr64["gy"])
    return near(gx.abs(), 1.0, width) | near(gy.abs(), 1.0, width) | near(pr64["z"], 0.0, width) | near(pr64["z"], z_clamp, width)


def ambiguous_geometry(pts, dims):
    f = (pts.to(F64) + 1) / 2 * (torch.tensor(dims, dtype=F64) - 1)
    return near(f, f.round()).any(1)


def ambiguous_points(s, pts, width=BAND):
    """-> (bool [P]: the point's view count is not compared with a reference, bool [V,P]: the pair's mask is not)."""
    pair = ambiguous_pairs(project_pts(pts, s["proj"], s["H"], s["W"], F64), Z_CLAMP_POINT, width)
    geo = ambiguous_geometry(pts, s["dims"])
    return pair.any(0) | geo, pair | geo[None]


# ------------------------------------------------------------------------------------------------ scenes
SHAPES = [(28, 44), (45, 24), (2, 3)]
NONDEGENERATE = SHAPES[:2]
VIEWS = (1, 3, 5)
SORT_VIEWS = 9                                                              # the list sort's second radix digit (views 8 ..) runs
NONCUBIC = (9, 14, 11)
SCENES = [(H, W, V, D) for (H, W) in SHAPES for V, D in ((5, 14), (3, 17), (1, 14))]
IMAGE_SEED = 3


def _finish(s):
    """Feature maps (standard normal; the compressed 16-channel ones leaky, like the compress layer's output), colour maps (uniform), and a latent volume
    with a seeded occupancy of 60 % that is zero where the occupancy is."""
    V, H, W, dims = s["V"], s["H"], s["W"], s["dims"]
    g = _rng(11, V, H, W, *dims)
    f16 = g.standard_normal((V, 16, H, W))
    s["f16"] = _t(np.where(f16 >= 0, f16, 0.01 * f16))
    s["fmaps"] = _t(g.standard_normal((V, 56, H, W)))
    s["images"] = _t(g.random((V, 3, H, W)))
    s["maskvol"] = _t(g.random(dims) < 0.6)
    s["dense"] = _t(g.standard_normal((16,) + tuple(dims))) * s["maskvol"][None]
    return s


@functools.lru_cache(maxsize=None)
def scene(H, W, V, D, dims=None):
    """synth.make_scene(V, hw=(H, W)) with a D^3 (or dims) lattice over [-1, 1]^3.  proj [V,3,4] and cam_pos [V,3] are formed once, in float64, and
    rounded: every reference and every kernel receives these very tensors."""
    sc = synth.make_scene(V, hw=(H, W), image_seed=IMAGE_SEED)
    dims = (D, D, D) if dims is None else tuple(dims)
    K, w2c = torch.from_numpy(sc["intrinsics"]).double(), torch.from_numpy(sc["w2cs"]).double()
    s = dict(sc=sc, H=H, W=W, V=V, D=D, dims=dims, voxel_size=2.0 / (D - 1), origin=_t(sc["partial_vol_origin"]), aff=_t(sc["affine_mats"]),
             proj=(K @ w2c[:, :3, :]).float().contiguous(), cam_pos=torch.inverse(w2c)[:, :3, 3].float().contiguous(),
             query_cam=_t(sc["query_c2w"][:3, 3]))
    return _finish(s)


SPHERE_RADIUS = 1.6
SPHERE_QUERY = np.array([0.4, -1.9, 0.7])
SPHERE_HW = (20, 28)
MANY_VIEWS = (33, 34, 64, 65, 255)


@functools.lru_cache(maxsize=None)
def sphere_scene(H, W, V, D, dims=None):
    """V distinct cameras for view counts the 32-view rig of synth.make_scene cannot give: centres on a Fibonacci spiral over the upper half (z > 0)
    of the sphere of radius SPHERE_RADIUS around the volume, each looking at its own seeded point within 0.1 of the origin, x to the right, y down, z
    forward; synth's intrinsics scaled to the image (f = 280 W / 256, principal point (W / 2, H / 2)).  At 20 x 28 a frustum's half angles are 18 and
    25 degrees: it holds the ball of radius 0.3 around the origin and, from 1.6 away, only part of [-1, 1]^3, so a point is seen by anything from
    none (low corners: every camera is above) to all of the views.  proj, aff and cam_pos are formed once in float64 and rounded once, as in
    scene(); K [V,3,3] and w2cs [V,4,4] are the same cameras for the entries that take those.  A query camera of the same kind at SPHERE_QUERY:
    query_cam [3], query_c2w [4,4], query_K [3,3]."""
    g = _rng(12, V, H, W)
    k = np.arange(V)
    z = 1.0 - (k + 0.5) / V
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    centre = np.concatenate([SPHERE_RADIUS * np.stack([r * np.cos(phi), r * np.sin(phi), z], 1), SPHERE_QUERY[None]])      # the query camera last
    target = g.uniform(-1.0, 1.0, (V + 1, 3)) * (0.1 / np.sqrt(3.0))
    fwd = target - centre
    fwd /= np.linalg.norm(fwd, axis=1, keepdims=True)
    up = np.where(np.abs(fwd[:, 2:3]) > 0.95, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 0.0, 1.0]]))
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    down = np.cross(fwd, right)
    c2w = np.tile(np.eye(4)[None], (V + 1, 1, 1))
    c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, down, fwd, centre
    w2c = np.linalg.inv(c2w[:V])
    f = 280.0 * W / 256.0
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    aff = np.tile(np.eye(4)[None], (V, 1, 1))
    aff[:, :3, :4] = K @ w2c[:, :3, :4]
    dims = (D, D, D) if dims is None else tuple(dims)
    s = dict(sc=None, H=H, W=W, V=V, D=D, dims=dims, voxel_size=2.0 / (D - 1), origin=_t([-1, -1, -1]), aff=_t(aff), proj=_t(aff[:, :3, :4]),
             cam_pos=_t(centre[:V]), query_cam=_t(SPHERE_QUERY), query_c2w=_t(c2w[V]), query_K=_t(K), K=_t(np.tile(K[None], (V, 1, 1))), w2cs=_t(w2c))
    return _finish(s)


SPHERE_TILES = dict(partial=0, none=1, all=2)            # the 32-point tiles the first 96 points of sphere_points are


@functools.lru_cache(maxsize=None)
def sphere_points(H, W, V, D, n=257):
    """n points of sphere_scene(H, W, V, D), picked by the float64 reference from a seeded pool in (-1, 1)^3, none of them inside the border band.  The
    first three 32-point tiles (one wave of the colour kernels each, SPHERE_TILES):
      partial   occupied points around the one that the last view and the fewest others see: every point is seen by 1 to V - 1 views, some view
                sees none of them
      none      occupied points that project into no view at all
      all       points seen by all V views
    then pool points in seeded order.  -> (pts [n,3], nviews int64 [n] of the float64 reference, mask bool [V,n])."""
    s = sphere_scene(H, W, V, D)
    pool = _t(_rng(27, V, H, W, D).uniform(-1.0, 1.0, (8192, 3)))
    pm = project_pts(pool, s["proj"], H, W, F64)["mask"]
    gm = geometry_mask(s["maskvol"], pool, F64)
    mask = pm & gm[None]
    nv = mask.sum(0)
    ok = ~ambiguous_points(s, pool)[0]
    part = torch.nonzero(ok & gm & (nv > 0) & (nv < V))[:, 0]
    last = part[mask[V - 1, part]]
    anchor = last[torch.argmin(nv[last])]
    near_anchor = part[torch.argsort((pool[part] - pool[anchor]).norm(dim=1))[:32]]
    none = torch.nonzero(ok & gm & (pm.sum(0) == 0))[:32, 0]
    every = torch.nonzero(ok & (nv == V))[:32, 0]
    assert len(near_anchor) == len(none) == len(every) == 32, (V, len(near_anchor), len(none), len(every))
    rest = torch.nonzero(ok)[:max(0, n - 96), 0]
    sel = torch.cat([near_anchor, none, every, rest])[:n]
    return pool[sel].contiguous(), nv[sel], mask[:, sel]


RIG_H, RIG_W, RIG_D = 13, 17, 17


@functools.lru_cache(maxsize=None)
def exact_rig():
    """Three axis-aligned cameras two units from the origin along -z, -x and -y (cyclic permutation rotations, translation (0, 0, 2)), focal length 16,
    principal point (8, 6) in a 13 x 17 image, over the D = 17 lattice of voxel size 1/8 and origin -1: every product, sum and quotient of the
    projection of a lattice node with a dyadic depth is exact in float32 and float64 alike.  gx = -1 on the plane X = 0, +1 on X = 16 Z (wx = Z / 2) and
    gy = +1 on Y = 12 Z (wy = 3 Z / 8, a division by 12), so whole rows of nodes lie on a border exactly."""
    perm = [np.eye(3), np.roll(np.eye(3), 1, axis=1), np.roll(np.eye(3), 2, axis=1)]
    K = np.array([[16.0, 0, 8], [0, 16, 6], [0, 0, 1]])
    w2c = np.tile(np.eye(4)[None], (3, 1, 1))
    for v in range(3):
        w2c[v, :3, :3], w2c[v, :3, 3] = perm[v], (0, 0, 2)
    aff = np.tile(np.eye(4)[None], (3, 1, 1))
    aff[:, :3, :4] = K @ w2c[:, :3, :4]
    s = dict(sc=None, H=RIG_H, W=RIG_W, V=3, D=RIG_D, dims=(RIG_D,) * 3, voxel_size=0.125, origin=_t([-1, -1, -1]), aff=_t(aff),
             proj=_t(aff[:, :3, :4]), cam_pos=_t(np.linalg.inv(w2c)[:, :3, 3]), query_cam=_t([0.5, -2.0, 0.25]))
    return _finish(s)


def rig_points():
    """The rig's lattice nodes strictly inside the volume, as points of the colour path."""
    s = exact_rig()
    p = voxel_world(s["dims"], s["voxel_size"], s["origin"], F32)
    return p[(p.abs() < 1).all(1)].contiguous()


# ------------------------------------------------------------------------------------------------ point families
POINT_COUNTS = (1, 31, 33, 257)
OFFSET_K = (0, 16, 64, 1024, 65536)
N_RANDOM = 4096


def random_points(n=N_RANDOM, seed=0):
    return _t(_rng(21, n, seed).uniform(-1.1, 1.1, (n, 3)))


def offset_points(s, k_min=0):
    """Per view and image side, points whose projection is aimed at g = +-(1 +- k 2^-24) on that side's axis: the other image coordinate uniform in
    (-1, 1), the depth uniform in [0.3, 3], back-projected through proj in float64, rounded to float32; those inside the volume are kept."""
    V, H, W = s["V"], s["H"], s["W"]
    g = _rng(22, V, H, W)
    per = max(48, 240 // V)
    Pm = s["proj"].double().numpy()
    out = []
    for v in range(V):
        Minv, t = np.linalg.inv(Pm[v, :, :3]), Pm[v, :, 3]
        for axis in (0, 1):
            for side in (-1.0, 1.0):
                for k in OFFSET_K:
                    if k < k_min:
                        continue
                    for sign in ((1.0,) if k == 0 else (-1.0, 1.0)):
                        gg = np.empty((per, 2))
                        gg[:, axis] = side * (1.0 + sign * k * U)
                        gg[:, 1 - axis] = g.uniform(-1, 1, per)
                        depth = g.uniform(0.3, 3.0, per)
                        pix = np.stack([(gg[:, 0] + 1) / 2 * (W - 1), (gg[:, 1] + 1) / 2 * (H - 1), np.ones(per)], 1) * depth[:, None]
                        out.append((pix - t[None]) @ Minv.T)
    p = np.concatenate(out).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(p[(np.abs(p) < 1).all(1)]))


FACE_VALUES = (1.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23)


def face_points(n_per=96, seed=0):
    """One coordinate exactly +-1 (outside: the volume is open), +-(1 - 2^-24) (the last float32 inside) or +-(1 + 2^-23); the others uniform in [-1, 1]."""
    g = _rng(23, n_per, seed)
    out = []
    for axis in range(3):
        for val in FACE_VALUES:
            for sign in (-1.0, 1.0):
                p = g.uniform(-1, 1, (n_per, 3))
                p[:, axis] = sign * val
                out.append(p)
    return _t(np.concatenate(out))


def node_points(s, n=3000):
    """Lattice nodes and edge midpoints (D = 17: multiples of 1/8 and 1/16, exact in float32) that touch an unoccupied voxel: at a node seven of the eight
    trilinear weights are exactly 0, at a midpoint six, and the mask sample is positive only through an occupied voxel of non-zero weight."""
    D = s["D"]
    m = s["maskvol"].numpy() > 0
    free = ~m
    touch = np.zeros_like(free)
    for ax in range(3):
        touch |= free | np.roll(free, 1, ax) | np.roll(free, -1, ax)
    nodes = np.argwhere(touch).astype(np.float64)
    mids = np.concatenate([nodes[nodes[:, ax] < D - 1] + 0.5 * np.eye(3)[ax] for ax in range(3)])
    p = np.concatenate([nodes, mids]) * s["voxel_size"] - 1.0
    g = _rng(24, D)
    p = p[g.choice(len(p), min(n, len(p)), replace=False)]
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    return _t(p)


def unit_normals(n, seed=0):
    v = _rng(25, n, seed).standard_normal((n, 3))
    return _t(v / np.linalg.norm(v, axis=1, keepdims=True))


def sort_list(n, P, seed=0):
    """n distinct slots into P points, ascending -> int32 [n]"""
    return torch.from_numpy(np.sort(_rng(26, n, P, seed).permutation(P)[:n]).astype(np.int32))
