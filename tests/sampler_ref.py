"""Plain references of the ray sampler's stages (csrc/render.hip, csrc/render_math.h), and the seeded inputs their tests share -- TEST
INFRASTRUCTURE ONLY.

torch on the CPU, nothing else: the product package is not imported here.  Every function restates oracle/recon.py (render, up_sample,
sample_pdf_det, cat_z, render_core) as whole-tensor expressions, RAY-MAJOR ([R,S]), once, for a dtype given by the caller: float64 is the truth
the kernels are compared with, float32 the accuracy class of the oracle's own arithmetic (tests/test_sampler_ref_cpu.py shows the float32 run equal
to the oracle bit for bit; the one deliberate difference, the summation order of inverse_cdf, is explained there).  Scalars and constants are rounded to float32 first (the kernels take them as float), so that both runs evaluate the
same function of the same numbers.  tests/test_gpu_sampler_units.py compares the HIP kernels with these references on the inputs generated below;
the CPU test asserts that those inputs exercise the edges they were chosen for and stay inside the caps of the tolerance rules."""
import functools

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23                       # of 1.0 in float32
EPS5 = float(np.float32(1e-5))         # the reference's 1e-5 / 1e-7 as the float32 kernels hold them
EPS7 = float(np.float32(1e-7))


def f32(x):
    """a python scalar as the float32 a kernel receives"""
    return float(np.float32(x))


def _c(t, dtype):
    return None if t is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------ references
def ray_points(rays_o, rays_d, z):
    """[R,3], [R,3], [R,S] -> [R,S,3]"""
    return rays_o[:, None] + rays_d[:, None] * z[..., None]


def occupancy(maskvol, pts):
    """F.grid_sample(mode='nearest', align_corners=False) of the mask volume [D,D,D]: index = round-half-even(((g + 1) D - 1) / 2) per axis,
    outside -> 0.  pts [...,3] -> [...] in pts.dtype."""
    D = maskvol.shape[0]
    idx = torch.round(((pts + 1) * D - 1) / 2)
    ok = ((idx >= 0) & (idx <= D - 1)).all(-1)
    ci = idx.clamp(0, D - 1).long()
    val = maskvol.to(pts.dtype)[ci[..., 0], ci[..., 1], ci[..., 2]]
    return torch.where(ok, val, torch.zeros((), dtype=pts.dtype))


def coarse(rays_o, rays_d, near, far, n_samples, t_rand=None, dtype=F64):
    """render()'s coarse samples: near + (far - near) * linspace(0, 1, S) (near / far: scalars, or [R] tensors -> the reference's [R,1] form), with
    the stratified jitter t_rand [R,S] when given.  -> (z [R,S], pts [R,S,3])"""
    o, d = _c(rays_o, dtype), _c(rays_d, dtype)
    R = o.shape[0]
    lin = torch.linspace(0, 1, n_samples, dtype=dtype)
    if torch.is_tensor(near):
        nr, fr = _c(near, dtype).reshape(R, 1), _c(far, dtype).reshape(R, 1)
        z = nr + (fr - nr) * lin[None, :]
    else:
        nr, fr = torch.tensor(f32(near), dtype=dtype), torch.tensor(f32(far), dtype=dtype)
        z = (nr + (fr - nr) * lin)[None].repeat(R, 1)
    if t_rand is not None:
        mids = 0.5 * (z[:, 1:] + z[:, :-1])
        upper = torch.cat([mids, z[:, -1:]], 1)
        lower = torch.cat([z[:, :1], mids], 1)
        z = lower + (upper - lower) * _c(t_rand, dtype)
    return z, ray_points(o, d, z)


def upsample_weights(z, sdf, m, inv_s, dtype=F64):
    """up_sample's section weights as sample_pdf takes them: alpha * T + 1e-5 [R,S-1].  m [R,S]: the samples' occupancy flags."""
    z, sdf, m = _c(z, dtype), _c(sdf, dtype), _c(m, dtype)
    inv_s = f32(inv_s)
    pm = m[:, :-1] * m[:, 1:]
    ps, ns, pz, nz = sdf[:, :-1], sdf[:, 1:], z[:, :-1], z[:, 1:]
    mid = (ps + ns) * 0.5
    dot = (ns - ps) / (nz - pz + EPS5)
    prev = torch.cat([torch.zeros_like(dot[:, :1]), dot[:, :-1]], 1)
    dot = torch.minimum(prev, dot).clip(-10.0, 0.0) * pm
    dist = nz - pz
    pc = torch.sigmoid((mid - dot * dist * 0.5) * inv_s)
    nc = torch.sigmoid((mid + dot * dist * 0.5) * inv_s)
    alpha = pm * ((pc - nc + EPS5) / (pc + EPS5))
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + EPS7], 1), 1)[:, :-1]
    return alpha * T + EPS5


def running_sum(x):
    """cumulative sum along the last axis, every partial sum rounded to x.dtype: the order and precision of a plain loop over a ray"""
    out = torch.empty_like(x)
    acc = torch.zeros_like(x[..., 0])
    for k in range(x.shape[-1]):
        acc = acc + x[..., k]
        out[..., k] = acc
    return out


def inverse_cdf(z, w, n, dtype=F64, serial_sum=True):
    """sample_pdf(det=True) on the section weights w [R,S-1] (the 1e-5 already added) over the bins z [R,S]: n new depths per ray.
    -> (new_z [R,n], bin [R,n] (index of the section the sample lands in; S-1: behind the last), mass [R,n] (that section's pdf mass),
    width [R,n] (its length)).
    serial_sum: the normaliser sum(w) and the cdf are accumulated section by section in `dtype` (running_sum), the order and precision of a plain
    loop over a ray and of the kernels.  ATen on the CPU, which the oracle runs on, adds w.sum(-1) pairwise and accumulates the float32 cumsum in
    DOUBLE (serial_sum=False: bit-equal with O.sample_pdf_det in float32): at S >= 64 that is an order of magnitude closer to the truth than any
    float32 accumulation, so a float32 run with it would understate the error of the float32 evaluation it stands for.  In float64 the two
    agree to 1e-15."""
    z, w = _c(z, dtype), _c(w, dtype)
    S = z.shape[1]
    if serial_sum:
        pdf = w / running_sum(w)[:, -1:]
        cdf = torch.cat([torch.zeros_like(pdf[:, :1]), running_sum(pdf)], -1)
    else:
        pdf = w / w.sum(-1, keepdim=True)
        cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    u = torch.linspace(0.5 / n, 1 - 0.5 / n, n, dtype=dtype).expand(cdf.shape[0], n).contiguous()
    ind = torch.searchsorted(cdf, u, right=True)
    lo = (ind - 1).clamp(min=0)
    hi = ind.clamp(max=S - 1)
    c0, c1 = cdf.gather(1, lo), cdf.gather(1, hi)
    b0, b1 = z.gather(1, lo), z.gather(1, hi)
    den = c1 - c0
    den = torch.where(den < EPS5, torch.ones_like(den), den)
    mass = pdf.gather(1, lo.clamp(max=S - 2))
    return b0 + (u - c0) / den * (b1 - b0), lo, mass, b1 - b0


def merge(z, sdf, new_z, new_sdf):
    """cat_z_vals' merge: stable sort of cat([z, new_z]) with the SDF gathered along (equal depths: existing samples first, then new ones in order)."""
    zz, idx = torch.sort(torch.cat([z, new_z], 1), dim=1, stable=True)
    return zz, torch.cat([sdf, new_sdf], 1).gather(1, idx)


def finalize(rays_o, rays_d, z, sample_dist, maskvol, dtype=F64):
    """render_core's head: section lengths (the last: sample_dist), mid depths, mid points, their nearest-voxel occupancy.  -> dict [R,S(,3)]"""
    o, d, z = _c(rays_o, dtype), _c(rays_d, dtype), _c(z, dtype)
    R = z.shape[0]
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), f32(sample_dist), dtype=dtype)], 1)
    mid = z + dists * 0.5
    pts = ray_points(o, d, mid)
    return dict(dists=dists, mid_z=mid, pts=pts, pm=occupancy(maskvol, pts))


COMPOSITE_OUTPUTS = ("color", "depth", "weights", "cdf", "weights_sum", "weights_max", "depth_var", "alpha_sum", "grad_err", "color_mask")


def composite_half(rays_d, grad, pm, dists, alpha_inter_ratio, dtype=F64):
    """the half-section SDF change icos * dist / 2 of render_core's opacity [R,S]"""
    d, grad, pm, dists = _c(rays_d, dtype), _c(grad, dtype), _c(pm, dtype), _c(dists, dtype)
    air = f32(alpha_inter_ratio)
    tdot = (d[:, None] * grad).sum(-1)
    icos = -(torch.relu(-tdot * 0.5 + 0.5) * (1 - air) + torch.relu(-tdot) * air) * pm
    return icos.clip(-10, 10) * dists * 0.5


def composite(rays_d, mid_z, dists, pm, sdf, grad, rgb, nviews, inv_s, alpha_inter_ratio, background, dtype=F64):
    """render_core's tail from given per-sample values ([R,S(,3)], nviews integer [R,S]) -> the ten outputs of o2345_ray_composite: color [R,3],
    depth, weights_sum, weights_max, depth_var, alpha_sum [R], grad_err [R,2] (sum pm (|g| - 1)^2, sum pm), color_mask bool [R], weights / cdf [R,S]"""
    mid_z, dists, pm, sdf, grad, rgb = (_c(t, dtype) for t in (mid_z, dists, pm, sdf, grad, rgb))
    inv_s, bg = f32(inv_s), f32(background)
    R = mid_z.shape[0]
    half = composite_half(rays_d, grad, pm, dists, alpha_inter_ratio, dtype)
    pc = torch.sigmoid((sdf - half) * inv_s)
    nc = torch.sigmoid((sdf + half) * inv_s)
    alpha = ((pc - nc + EPS5) / (pc + EPS5)).clip(0, 1) * pm
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=dtype), 1 - alpha + EPS7], 1), 1)[:, :-1]
    wts = alpha * T
    wsum = wts.sum(1, keepdim=True)
    color = (rgb * wts[..., None]).sum(1) + bg * (1 - wsum)
    depth = (mid_z * wts).sum(1, keepdim=True)
    gerr = (pm * (grad.norm(dim=-1) - 1) ** 2).sum(1)
    return dict(color=color, depth=depth[:, 0], weights=wts, cdf=pc, weights_sum=wsum[:, 0], weights_max=wts.max(1).values,
                depth_var=((mid_z - depth) ** 2 * wts).sum(1), alpha_sum=alpha.sum(1), grad_err=torch.stack([gerr, pm.sum(1)], 1),
                color_mask=(nviews >= 2).to(dtype).sum(1) > 8)


# ------------------------------------------------------------------------------------------------ tolerance rules
def rule_e_bound(ref32, ref64):
    """Rule E: e_ref = max |ref32 - ref64| -> (e_ref, bound = 4 e_ref + 4 ulp of the output's magnitude)"""
    e_ref = (ref32.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    mag = ref64.abs().max().item() if ref64.numel() else 0.0
    return e_ref, 4 * e_ref + 4 * ULP * mag


SWITCH_BAND = 1e-3                     # relative distance of a bin's mass from sample_pdf's 1e-5 switch inside which the placement is not compared finely


def rule_z(z, w):
    """Rule Z on the section weights w [R,S-1] over the bins z [R,S], for n new samples per ray: the float64 inverse CDF, and per sample
    sens = max over the landed bin and its two neighbours of width / den (den: the bin's pdf mass, 1 below 1e-5), the bin's width, and whether its
    mass lies in the switch band; dev32 = |float32 inverse CDF - float64 inverse CDF| / sens on these weights, the deviation rule Z's C is four times
    the maximum of (0 for switch-band samples: their bound is the bin's width).  -> callable n -> dict"""
    z64, w64 = z.double(), w.double()
    S = z64.shape[1]
    pdf = w64 / w64.sum(-1, keepdim=True)                                                   # [R,S-1]
    width = z64[:, 1:] - z64[:, :-1]
    ratio = width / torch.where(pdf < EPS5, torch.ones_like(pdf), pdf)
    pad = torch.zeros_like(ratio[:, :1])
    nb = torch.maximum(torch.maximum(torch.cat([pad, ratio[:, :-1]], 1), ratio), torch.cat([ratio[:, 1:], pad], 1))
    band = ((pdf - EPS5).abs() <= SWITCH_BAND * EPS5)

    def at(n):
        new64, lo, mass, wd = inverse_cdf(z64, w64, n, F64)
        new32 = inverse_cdf(z, w, n, F32)[0]
        k = lo.clamp(max=S - 2)
        sens = nb.gather(1, k)
        in_band = band.gather(1, k)
        dev = (new32.double() - new64).abs() / sens.clamp(min=1e-300)
        return dict(new_z=new64, new_z32=new32, sens=sens, width=width.gather(1, k), band=in_band, dev32=torch.where(in_band, torch.zeros_like(dev), dev))
    return at


def rule_z_bound(q, C, fine):
    """per-sample bound of rule Z: C * sens + 4 ulp(z); the bin's width (+ 4 ulp) for samples in the switch band.  fine [R] bool: the rays compared."""
    ulp_z = 4 * ULP * q["new_z"].abs()
    bound = torch.where(q["band"], q["width"], C * q["sens"]) + ulp_z
    return torch.where(fine[:, None], bound, torch.full_like(bound, float("inf")))


# ------------------------------------------------------------------------------------------------ shared inputs
MASK_D = 16
NEAR, FAR = 0.5, 2.75


@functools.lru_cache(maxsize=None)
def synthetic_mask():
    """[16,16,16] float32: occupied inside a border of two empty voxels, with a hole of 4^3 empty voxels off centre"""
    m = torch.zeros(MASK_D, MASK_D, MASK_D)
    m[2:14, 2:14, 2:14] = 1.0
    m[5:9, 6:10, 7:11] = 0.0
    return m


def rays(R, seed):
    """R rays from a sphere of radius 1.6 towards points inside the volume: every ray crosses the empty border, many the hole.  -> float32 [R,3] x 2"""
    g = torch.Generator().manual_seed(1000 + seed)
    o = torch.randn(R, 3, generator=g, dtype=F64)
    o = 1.6 * o / o.norm(dim=1, keepdim=True)
    tgt = torch.rand(R, 3, generator=g, dtype=F64) * 1.2 - 0.6
    d = tgt - o
    d = d / d.norm(dim=1, keepdim=True)
    return o.float().contiguous(), d.float().contiguous()


def sorted_depths(R, S, g, ties=0, stratified=False):
    """[R,S] float32 ascending in [NEAR, FAR]: uniform draws sorted, or (stratified) one draw per S-th of the range, like the jittered coarse samples
    (section lengths 0.2 .. 1.8 of the mean); ties: that many samples per ray repeat their predecessor (zero-length sections)"""
    if stratified:
        z = NEAR + (FAR - NEAR) * (torch.arange(S) + 0.1 + 0.8 * torch.rand(R, S, generator=g)) / S
    else:
        z = torch.sort(torch.rand(R, S, generator=g) * (FAR - NEAR) + NEAR, 1).values
    for _ in range(ties if S > 1 else 0):
        k = torch.randint(1, S, (R,), generator=g)
        z[torch.arange(R), k] = z[torch.arange(R), k - 1]
    return torch.sort(z, 1).values.contiguous()


# ---- coarse
COARSE_S = (2, 3, 64, 65)
COARSE_CASES = [(R, S, variant) for (R, S) in ((1, 64), (3, 65), (5, 3), (63, 2), (65, 3), (257, 2), (5, 65)) for variant in ("plain", "jitter", "per_ray")]


@functools.lru_cache(maxsize=None)
def coarse_inputs(R, S, variant):
    g = torch.Generator().manual_seed(R * 1000 + S)
    o, d = rays(R, R + S)
    t_rand = torch.rand(R, S, generator=g).contiguous() if variant != "plain" else None
    if variant == "per_ray":
        near = (0.3 + 0.4 * torch.rand(R, generator=g)).contiguous()
        far = (near + 1.0 + 1.5 * torch.rand(R, generator=g)).contiguous()
        t_rand = t_rand if (R + S) % 2 else None                # per-ray bounds with and without jitter
    else:
        near, far = NEAR, FAR
    return dict(rays_o=o, rays_d=d, near=near, far=far, t_rand=t_rand)


def coarse_bounds(d, z64, pts64):
    """Roundings of the expression, u = 2^-24 relative per float32 operation, M = max(|near|, |far|, |far - near|) of the ray:
      linspace: step = fl(1 / (S - 1)), one fused multiply-add -> |err| <= 2u;  fl(far - near): u;  the product: u;  fl(near + .): u |z|
        -> a coarse depth is within 4u |far - near| + u |z| <= 5u M of the truth;
      jitter: lower, upper = fl(0.5 (z + z')) -> 6u M each; fl(upper - lower) -> 12u M + u |.|; times t_rand in [0, 1), rounded, and the final sum
        rounded -> |err(z)| <= (6 + 12 + 3) u M = 21u M = 10.5 ulp(M);
      points o + d z: |d_c| err(z) + u |d_c z| + u |p| per component.
    -> (bound on z [R,1], bound on pts [R,S,3])"""
    near, far = d["near"], d["far"]
    if torch.is_tensor(near):
        M = torch.maximum(torch.maximum(near.abs(), far.abs()), (far - near).abs()).double()[:, None]
    else:
        M = torch.full((z64.shape[0], 1), max(abs(near), abs(far), abs(far - near)), dtype=F64)
    u = ULP / 2
    bz = (21 if d["t_rand"] is not None else 5) * u * M
    o, dd = d["rays_o"].double(), d["rays_d"].double()
    bp = dd[:, None].abs() * bz[..., None] + u * (dd[:, None] * z64[..., None]).abs() + u * pts64.abs() + u * o[:, None].abs()
    return bz, bp


# ---- up-sampling
FAMILIES = ("crossing", "no_crossing", "noisy", "defaults", "ties")
# (R, S, inv_s): every R and every S of the shared shapes once, every inv_s with all five families
UPSAMPLE_CASES = [(1, 2, 512.0), (3, 3, 1e6), (5, 9, 64.0), (63, 15, 512.0), (65, 16, 1e6), (257, 17, 64.0), (5, 64, 512.0), (3, 129, 1e6),
                  (5, 255, 64.0), (5, 129, 1e6)]
UPSAMPLE_NIMP = (1, 5, 16, 17, 64, 256)


@functools.lru_cache(maxsize=None)
def upsample_inputs(R, S, inv_s):
    """z / sdf [R,S] ray-major, the samples' occupancy m [R,S] (float32 arithmetic, as every float32 implementation evaluates it), family [R]: ray r
    belongs to family (r + S) % 5."""
    g = torch.Generator().manual_seed(R * 1000 + S)
    o, d = rays(R, R * 7 + S)
    fam = (torch.arange(R) + S) % len(FAMILIES)
    z = sorted_depths(R, S, g, stratified=True)
    tie = fam == FAMILIES.index("ties")
    if tie.any() and S > 2:
        z[tie] = sorted_depths(int(tie.sum()), S, g, ties=max(1, S // 8))
    m = occupancy(synthetic_mask(), ray_points(o, d, z))
    # the crossing depth: anywhere in [z_0, z_{S-1}]; rays 0 / 1 of a case inside the first / last section
    tc = z[:, :1] + (z[:, -1:] - z[:, :1]) * torch.rand(R, 1, generator=g)
    tc[0] = 0.5 * (z[0, 0] + z[0, 1])
    if R > 1:
        tc[1] = 0.5 * (z[1, -2] + z[1, -1])
    slope = 0.5 + torch.rand(R, 1, generator=g)
    clean = (tc - z) * slope
    sdf = clean.clone()
    k = fam == FAMILIES.index("no_crossing")
    sdf[k] = (0.05 + 0.3 * torch.rand(R, S, generator=g))[k]
    k = fam == FAMILIES.index("noisy")
    sdf[k] = (0.05 * torch.randn(R, S, generator=g))[k]
    k = fam == FAMILIES.index("defaults")
    sdf[k] = torch.where(m[k] > 0, clean[k], torch.full_like(clean[k], 100.0))
    return dict(rays_o=o, rays_d=d, z=z.contiguous(), sdf=sdf.contiguous(), m=m, family=fam, inv_s=inv_s)


def fine_rays(d):
    """rule Z compares the depths of families (a) and (b)"""
    return (d["family"] == FAMILIES.index("crossing")) | (d["family"] == FAMILIES.index("no_crossing"))


RULE_Z_DROPPED = set()                 # (S, n_imp) left to the bit-identity and weights checks: none -- on these inputs S = 255, n_imp = 256 meets the conditions too


# ---- merge
MERGE_CONTENT = ("sorted", "reversed", "shuffled", "ties", "duplicates", "front", "behind")
# (R, S, n_new): every S and every n_new once, 16 (the fused rank merge) at several S
MERGE_CASES = [(1, 1, 16), (3, 2, 1), (5, 15, 5), (63, 16, 16), (65, 17, 17), (257, 64, 16), (5, 127, 33), (3, 64, 80), (5, 17, 16), (5, 1, 33)]


@functools.lru_cache(maxsize=None)
def merge_inputs(R, S, n_new):
    """ray r's new block has content (r + S) % 7; the SDF values are distinct integers, so a gathered value names its source"""
    g = torch.Generator().manual_seed(R * 1000 + S * 7 + n_new)
    z = sorted_depths(R, S, g, ties=1 if S > 2 else 0)
    new_z = torch.rand(R, n_new, generator=g) * (FAR - NEAR) + NEAR
    content = (torch.arange(R) + S) % len(MERGE_CONTENT)
    for r in range(R):
        c = MERGE_CONTENT[int(content[r])]
        row = new_z[r]
        if c == "sorted":
            row = torch.sort(row).values
        elif c == "reversed":
            row = torch.sort(row, descending=True).values
        elif c == "ties":                                       # values copied from the list, in any order
            pick = torch.randint(0, S, (n_new,), generator=g)
            row = torch.where(torch.rand(n_new, generator=g) < 0.7, z[r, pick], row)
        elif c == "duplicates":
            pick = torch.randint(0, max(1, n_new // 2), (n_new,), generator=g)
            row = row[pick]
        elif c == "front":
            row = z[r, 0] - 0.01 - 0.2 * torch.rand(n_new, generator=g)
        elif c == "behind":
            row = z[r, -1] + 0.01 + 0.2 * torch.rand(n_new, generator=g)
        new_z[r] = row
    sdf = torch.arange(R * S, dtype=F32).reshape(R, S)
    new_sdf = -1.0 - torch.arange(R * n_new, dtype=F32).reshape(R, n_new)
    return dict(z=z, sdf=sdf, new_z=new_z.contiguous(), new_sdf=new_sdf, content=content)


# ---- finalize
FINALIZE_CASES = [(1, 256), (3, 17), (5, 2), (63, 1), (65, 2), (257, 17)]


@functools.lru_cache(maxsize=None)
def finalize_inputs(R, S):
    g = torch.Generator().manual_seed(R * 1000 + S + 5)
    o, d = rays(R, R * 3 + S)
    return dict(rays_o=o, rays_d=d, z=sorted_depths(R, S, g, ties=1 if S > 2 else 0), sample_dist=(FAR - NEAR) / 64)


def finalize_bounds(d, f64):
    """Roundings of render_core's head, u = 2^-24 relative per float32 operation, against the float64 expression on the float32 depths:
      dists = fl(z' - z): u |dists| (the last one is the given sample_dist: exact);
      mid_z = fl(z + dists / 2) (the halving is exact): its own rounding u |mid_z| plus half the error of dists;
      pts = fl(o + fl(d mid_z)) per component: |d_c| err(mid_z) + u |d_c mid_z| + u |p_c|;
      the factor 1 + 4u covers the second-order terms (a rounding is relative to the computed value, the bound is written on the true one).
    -> dict of bounds"""
    u = ULP / 2
    bd = u * f64["dists"].abs()
    bd[:, -1] = 0.0
    bm = (u * f64["mid_z"].abs() + 0.5 * bd) * (1 + 4 * u)
    dd = d["rays_d"].double()[:, None]
    bp = (dd.abs() * bm[..., None] + u * (dd * f64["mid_z"][..., None]).abs() + u * f64["pts"].abs()) * (1 + 4 * u)
    return dict(dists=bd, mid_z=bm, pts=bp)


def point_bound(rays_o, rays_d, z):
    """fl(o + fl(d z)) against the float64 o + d z on the float32 depths z [R,n]: u |d_c z| + u |p_c| per component (and second order).
    -> (pts64, bound) [R,n,3]"""
    u = ULP / 2
    dz = rays_d.double()[:, None] * z.double()[..., None]
    p64 = rays_o.double()[:, None] + dz
    return p64, (u * dz.abs() + u * p64.abs()) * (1 + 4 * u)


# ---- composite
# (R, S, alpha_inter_ratio, inv_s, background): every S, ratio, inv_s and background of the issue once or more
COMPOSITE_CASES = [(1, 256, 0.5, 30.0, 1.0), (3, 129, 1.0, 665.0, 0.0), (5, 17, 0.0, 1e6, 1.0), (63, 9, 0.5, 1e-6, 0.0), (65, 2, 1.0, 30.0, 1.0),
                   (257, 1, 0.0, 665.0, 0.0), (5, 129, 0.5, 1e6, 0.0), (3, 17, 1.0, 1e6, 1.0), (5, 9, 0.0, 30.0, 1.0)]
STEP_MARGIN = 1e-3                     # at inv_s = 1e6: |sdf +- half| >= this, i.e. both sigmoid arguments beyond +-1000 (saturated in either precision)


@functools.lru_cache(maxsize=None)
def composite_inputs(R, S, air, inv_s, bg):
    """Per-sample inputs ray-major.  Per ray (r + S) % 6: 0 pm all zero; 1 exactly 8 samples seen by >= 2 views (where S allows); 2 exactly 9, some of
    them with pm = 0; 3 zero / antiparallel gradients; 4 zero section lengths; 5 plain.  Unoccupied slots carry sdf = 100, grad = rgb = 0."""
    g = torch.Generator().manual_seed(R * 1000 + S * 3 + int(air * 2))
    o, d = rays(R, R * 5 + S)
    mid = sorted_depths(R, S, g)
    dists = torch.cat([mid[:, 1:] - mid[:, :-1], torch.full((R, 1), (FAR - NEAR) / 64)], 1)
    kind = (torch.arange(R) + S) % 6
    pm = (torch.rand(R, S, generator=g) > 0.3).float()
    pm[kind == 0] = 0.0
    grad = torch.randn(R, S, 3, generator=g)
    k3 = kind == 3
    sel = torch.rand(R, S, generator=g)
    grad = torch.where((k3[:, None] & (sel < 0.3))[..., None], torch.zeros_like(grad), grad)
    grad = torch.where((k3[:, None] & (sel > 0.6))[..., None], -d[:, None].expand(R, S, 3) * (0.5 + sel[..., None]), grad)
    k4 = kind == 4
    dists = torch.where(k4[:, None] & (torch.rand(R, S, generator=g) < 0.4), torch.zeros_like(dists), dists)
    sdf = 0.03 * torch.randn(R, S, generator=g)
    rgb = torch.rand(R, S, 3, generator=g)
    nv = torch.randint(0, 5, (R, S), generator=g)
    for r in range(R):
        want = {1: 8, 2: 9}.get(int(kind[r]))
        if want is not None:
            row = torch.zeros(S, dtype=torch.long)
            pick = torch.randperm(S, generator=g)[:min(want, S)]
            row[pick] = 2 + torch.randint(0, 3, (pick.numel(),), generator=g)
            row[row == 0] = torch.randint(0, 2, (int((row == 0).sum()),), generator=g)
            nv[r] = row
            if int(kind[r]) == 2:
                pm[r, pick[::2]] = 0.0
    if inv_s >= 1e5:                                            # the opacity is a step function of sdf +- half: stay away from the steps
        half = composite_half(d, grad, pm, dists, air, F64).abs()
        a = sdf.double().abs() - half
        sgn = torch.where(sdf >= 0, 1.0, -1.0).double()
        sdf = torch.where(a.abs() < 2 * STEP_MARGIN, sgn * (half + 2 * STEP_MARGIN), sdf.double()).float()
    occ = pm > 0
    sdf = torch.where(occ, sdf, torch.full_like(sdf, 100.0))
    grad = torch.where(occ[..., None], grad, torch.zeros_like(grad))
    rgb = torch.where(occ[..., None], rgb, torch.zeros_like(rgb))
    return dict(rays_o=o, rays_d=d, mid_z=mid, dists=dists.contiguous(), pm=pm, sdf=sdf.contiguous(), grad=grad.contiguous(), rgb=rgb.contiguous(),
                nviews=nv.to(torch.uint8), kind=kind, alpha_inter_ratio=air, inv_s=inv_s, background=bg)


def composite_refs(d):
    a = (d["rays_d"], d["mid_z"], d["dists"], d["pm"], d["sdf"], d["grad"], d["rgb"], d["nviews"], d["inv_s"], d["alpha_inter_ratio"], d["background"])
    return composite(*a, dtype=F32), composite(*a, dtype=F64)


def sm(t):
    """ray-major [R,S,...] -> SAMPLE-MAJOR contiguous [S,R,...] (the kernels' layout), and back"""
    return t.transpose(0, 1).contiguous()
