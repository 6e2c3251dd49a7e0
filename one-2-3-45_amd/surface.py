"""Host twin of the surface renderer (csrc/surface_trace.hip): depth, hit point and kind per ray by an exhaustive fixed-stride march through the
trilinear R^3 SDF lattice, with an exact empty-space skip; pinhole rays, look-at orbits and the image packer.  numpy only, no GPU.  This file is the
DEFINITION: the device equals it to the last bit.  All arithmetic is fp64, one operation at a time, in the order written; the trace has no square root.

What the image shows is the zero set of the trilinear lattice, the surface marching cubes meshes, not the network's own zero set."""
import numpy as np

BRICK = 8                       # cells per brick edge
MAX_STEPS = 1 << 20             # a ray with more strides than this is a bad ray
KIND_NONE, KIND_HIT, KIND_ENTRY = 0, 1, 2
INFO_KEYS = ("rays", "hits", "entry_hits", "box_misses", "misses", "stalled", "bad_rays", "samples", "lookups")


def _field(u, level, inside_positive):
    """g = double(u) - level, or level - double(u) for a lattice that is positive inside (the pipeline's extraction lattice is -sdf)"""
    u = np.asarray(u)
    if u.dtype != np.float32 or u.ndim != 3 or len(set(u.shape)) != 1 or u.shape[0] < 2:
        raise ValueError(f"surface: the lattice is float32 [R,R,R] with R >= 2, got {u.dtype} {u.shape}")
    level = float(level)
    if not np.isfinite(level):
        raise ValueError(f"surface: level must be finite, got {level!r}")
    g = u.astype(np.float64)
    return (level - g) if inside_positive else (g - level)


def _bounds(bound_min, bound_max):
    b0 = np.asarray(bound_min, np.float32).reshape(-1).astype(np.float64)
    b1 = np.asarray(bound_max, np.float32).reshape(-1).astype(np.float64)
    if b0.shape != (3,) or b1.shape != (3,) or not (np.isfinite(b0).all() and np.isfinite(b1).all() and (b1 > b0).all()):
        raise ValueError(f"surface: bound_max must be above bound_min on every axis, both finite, got {bound_min!r} and {bound_max!r}")
    return b0, b1, b1 - b0


def march_params(stride=1.0, refine=8):
    stride = float(stride)
    if not (0.0 < stride <= 8.0):
        raise ValueError(f"surface: stride must be in (0, 8], got {stride!r}")
    if isinstance(refine, (bool, np.bool_)) or int(refine) != refine or not 0 <= refine <= 32:
        raise ValueError(f"surface: refine must be an integer in [0, 32], got {refine!r}")
    return stride, int(refine)


def brick_flags(u, level=0.0, inside_positive=False):
    """uint8 [nb,nb,nb], nb = ceil((R - 1) / 8): flag[b] = 1 iff some node with index in [8 b_k, min(8 b_k + 8, R - 1)] on every axis fails g > 0 (a NaN
    node sets the flag).  A cell whose brick has flag 0 has eight strictly positive corners: every trilinear value inside it is > 0 in floating point."""
    a = ~(_field(u, level, inside_positive) > 0.0)
    R = a.shape[0]
    nb = (R - 1 + BRICK - 1) // BRICK
    for axis in range(3):
        a = np.stack([a.take(range(BRICK * b, min(BRICK * b + BRICK, R - 1) + 1), axis).any(axis) for b in range(nb)], axis)
    return np.ascontiguousarray(a, np.uint8)


def _cell(t, o, d, bmin, ext, R):
    """sample points o + t d -> (cell indices i_k <= R - 2, fractions f_k): x_k = (p_k - bmin_k) / ext_k * (R - 1), clamped to [0, R - 1] (a NaN clamps
    to 0: both clamps are `x if x > 0 else 0`, then `x if x < R - 1 else R - 1`)"""
    rm1 = float(R - 1)
    idx, frac = [], []
    for k in range(3):
        p = o[:, k] + t * d[:, k]
        x = (p - bmin[k]) / ext[k] * rm1
        x = np.where(x > 0.0, x, 0.0)
        x = np.where(x < rm1, x, rm1)
        i = np.minimum(np.floor(x), rm1 - 1.0)
        idx.append(i.astype(np.int64))
        frac.append(x - i)
    return idx, frac


def _value(g, idx, frac):
    """sum over the eight corners of ((wx wy) wz) g(corner); dx outer, dy, dz inner; accumulated left to right from 0"""
    v = np.zeros(idx[0].shape[0], np.float64)
    for dx in (0, 1):
        wx = frac[0] if dx else 1.0 - frac[0]
        for dy in (0, 1):
            wy = frac[1] if dy else 1.0 - frac[1]
            for dz in (0, 1):
                wz = frac[2] if dz else 1.0 - frac[2]
                v = v + ((wx * wy) * wz) * g[idx[0] + dx, idx[1] + dy, idx[2] + dz]
    return v


def trace_rays(u, rays_o, rays_d, near, far, stride=1.0, refine=8, level=0.0, inside_positive=False, bound_min=(-1.0, -1.0, -1.0),
               bound_max=(1.0, 1.0, 1.0), skip=True, want_t=False):
    """-> (depth f32 [n], kind u8 [n], point f32 [n,3], info[, t f64 [n] with ``want_t``: the depth before its rounding to float32, 0 without a hit]).  kind 0: no hit (depth and point 0), 1: a crossing from outside (g > 0) to not outside,
    2: the ray enters the box where it is already not outside (depth = t0).

    The ray o + t d is clipped to the box and [near, far] -> [t0, t1] (a slab test; an axis with d_k == 0 constrains nothing when bmin_k <= o_k <= bmax_k
    and otherwise the ray misses).  Samples t_j = t0 + j h, j = 0 .. n = floor((t1 - t0) / h), and one more at t1 when t_n < t1, with h = stride *
    min_k(ext_k) / (R - 1): `stride` lattice spacings for a unit direction -- h is a step in t, so a non-unit direction scales the spacing by |d|.  The first
    sample whose trilinear value is not > 0 ends the march; the bracket with its predecessor is narrowed `refine` times (even steps regula falsi, odd
    steps bisection) and the depth is the secant root of the final bracket.  ``skip``: samples whose cell lies in a brick without a flag (brick_flags)
    are outside without a lookup; a skipped predecessor is evaluated when the bracket needs it.  The result does not depend on ``skip``, only
    info["lookups"] does.
    Stalled (kind 0, counted): the first value that is not outside is NaN, or the final t is not finite (infinite lattice values).  Bad ray (kind 0, counted,
    never dereferenced): a non-finite origin or direction, or n > 2^20.
    info: exact counts -- rays = hits + entry_hits + box_misses + misses + stalled + bad_rays; samples = march samples visited + refinement evaluations;
    lookups = eight-corner evaluations (== samples when ``skip`` is off)."""
    g = _field(u, level, inside_positive)
    R = g.shape[0]
    stride, refine = march_params(stride, refine)
    near, far = float(near), float(far)
    if not (np.isfinite(near) and np.isfinite(far)):
        raise ValueError(f"surface: near and far must be finite, got {near!r} and {far!r}")
    bmin, bmax, ext = _bounds(bound_min, bound_max)
    o32, d32 = np.asarray(rays_o), np.asarray(rays_d)
    if o32.dtype != np.float32 or d32.dtype != np.float32 or o32.ndim != 2 or o32.shape[1] != 3 or d32.shape != o32.shape:
        raise ValueError(f"surface: rays_o and rays_d are float32 [n,3], got {o32.dtype} {o32.shape} and {d32.dtype} {d32.shape}")
    n_rays = o32.shape[0]
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    flags = brick_flags(u, level, inside_positive) if skip else None
    depth, kind, point = np.zeros(n_rays, np.float32), np.zeros(n_rays, np.uint8), np.zeros((n_rays, 3), np.float32)
    info = dict.fromkeys(INFO_KEYS, 0)
    info["rays"] = n_rays
    h = stride * float(ext.min()) / float(R - 1)
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1))
        # ---- the slab test
        t0, t1 = np.full(n_rays, near), np.full(n_rays, far)
        miss = np.zeros(n_rays, bool)
        for k in range(3):
            dk, ok = d[:, k], o[:, k]
            zero = dk == 0.0
            miss |= zero & ~((bmin[k] <= ok) & (ok <= bmax[k]))
            safe = np.where(zero | bad, 1.0, dk)
            a, b = (bmin[k] - ok) / safe, (bmax[k] - ok) / safe
            lo, hi = np.where(a < b, a, b), np.where(a < b, b, a)
            t0 = np.where(~zero & (lo > t0), lo, t0)
            t1 = np.where(~zero & (hi < t1), hi, t1)
        miss |= ~(t0 <= t1)
        miss &= ~bad
        q = np.floor((t1 - t0) / h)
        bad |= ~miss & ~bad & ~(q <= float(MAX_STEPS))
        miss &= ~bad
        info["bad_rays"], info["box_misses"] = int(bad.sum()), int(miss.sum())
        live = np.flatnonzero(~bad & ~miss)
        n = q[live].astype(np.int64)
        extra = (t0[live] + n.astype(np.float64) * h) < t1[live]
        m = n + 1 + extra                                             # samples of each live ray
        # ---- the march, all live rays at once, sample after sample
        L = live.shape[0]
        done = np.zeros(L, bool)
        pt, ps, pskip = np.zeros(L), np.zeros(L), np.zeros(L, bool)   # the predecessor: t, value, skipped
        bt_lo, bs_lo, bt_hi, bs_hi = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
        state = np.zeros(L, np.uint8)                                 # 0 marched through, 1 bracketed, 2 entry, 3 stalled
        ol, dl, t0l, t1l = o[live], d[live], t0[live], t1[live]
        for j in range(int(m.max()) if L else 0):
            act = np.flatnonzero(~done & (j < m))
            if act.size == 0:
                break
            t = np.where(j <= n[act], t0l[act] + float(j) * h, t1l[act])
            idx, frac = _cell(t, ol[act], dl[act], bmin, ext, R)
            info["samples"] += act.size
            ev = flags[idx[0] >> 3, idx[1] >> 3, idx[2] >> 3] != 0 if skip else np.ones(act.size, bool)
            v = np.full(act.size, np.nan)
            v[ev] = _value(g, [i[ev] for i in idx], [f[ev] for f in frac])
            info["lookups"] += int(ev.sum())
            outside = ~ev | (v > 0.0)
            e = ~outside
            if e.any():
                r, ve, te = act[e], v[e], t[e]
                nan = np.isnan(ve)
                state[r] = np.where(nan, 3, 2 if j == 0 else 1)
                done[r] = True
                bt_hi[r], bs_hi[r] = te, ve
                if j > 0:
                    need = r[~nan & pskip[r]]                          # a skipped predecessor is evaluated where the bracket needs it
                    if need.size:
                        pi, pf = _cell(pt[need], ol[need], dl[need], bmin, ext, R)
                        ps[need] = _value(g, pi, pf)
                        info["lookups"] += need.size
                    bt_lo[r], bs_lo[r] = pt[r], ps[r]
            keep = act[outside]
            pt[keep], ps[keep], pskip[keep] = t[outside], v[outside], ~ev[outside]
        # ---- refinement of the brackets
        br = np.flatnonzero(state == 1)
        lo, hi, s_lo, s_hi = bt_lo[br], bt_hi[br], bs_lo[br], bs_hi[br]
        for step in range(refine):
            tm = lo + (hi - lo) * (s_lo / (s_lo - s_hi)) if step % 2 == 0 else lo + (hi - lo) * 0.5
            idx, frac = _cell(tm, ol[br], dl[br], bmin, ext, R)
            v = _value(g, idx, frac)
            info["samples"] += br.size
            info["lookups"] += br.size
            out = v > 0.0
            lo, s_lo = np.where(out, tm, lo), np.where(out, v, s_lo)
            hi, s_hi = np.where(out, hi, tm), np.where(out, s_hi, v)
        tb = lo + (hi - lo) * (s_lo / (s_lo - s_hi))
        t_hit = np.zeros(L)
        t_hit[br] = tb
        t_hit[state == 2] = t0l[state == 2]
        state[(state == 1) & ~np.isfinite(t_hit)] = 3
        hit = (state == 1) | (state == 2)
        rows = live[hit]
        kind[rows] = state[hit]
        depth[rows] = t_hit[hit].astype(np.float32)
        point[rows] = (ol[hit] + t_hit[hit][:, None] * dl[hit]).astype(np.float32)
    info["hits"], info["entry_hits"] = int((state == 1).sum()), int((state == 2).sum())
    info["stalled"], info["misses"] = int((state == 3).sum()), int((state == 0).sum())
    if want_t:
        t64 = np.zeros(n_rays)
        t64[rows] = t_hit[hit]
        return depth, kind, point, info, t64
    return depth, kind, point, info


def _pinhole(K, c2w):
    K = np.asarray(K, np.float32).astype(np.float64)
    M = np.asarray(c2w, np.float32).astype(np.float64)
    if K.shape != (3, 3) or M.shape not in ((3, 4), (4, 4)) or not (np.isfinite(K).all() and np.isfinite(M).all()):
        raise ValueError(f"camera_rays: K [3,3] and c2w [3,4] or [4,4], both finite, expected; got {K.shape} and {M.shape}")
    if K[0, 1] != 0.0 or K[1, 0] != 0.0 or K[2, 0] != 0.0 or K[2, 1] != 0.0 or K[2, 2] != 1.0 or K[0, 0] == 0.0 or K[1, 1] == 0.0:
        raise ValueError("camera_rays: a pinhole camera without skew is [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with fx, fy != 0")
    return K, M[:3]


def unit_normal(g):
    """fp64 [n,3] -> (g / l, ok) with l = sqrt((gx gx + gy gy) + gz gz), as csrc/mesh_math.h does it; ok: l is finite and > 0, else the row is 0"""
    g = np.asarray(g, np.float64)
    with np.errstate(all="ignore"):
        l = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = (l > 0.0) & (l < np.inf)
        n = np.where(ok[:, None], g / np.where(ok, l, 1.0)[:, None], 0.0)
    return n, ok


def camera_rays(K, c2w, H, W):
    """Rays through the pixel grid of a pinhole camera without skew (any other K is refused) -> (rays_o, rays_d) float32 [H W, 3], raster order.  In fp64,
    from the float32 K and c2w: v = ((px - cx) / fx, (py - cy) / fy, 1), normalised by unit_normal, rotated by c2w's 3x3 with sums left to right, rounded to
    float32 once; the origin is c2w's translation.  (synth.gen_rays multiplies in float32: equal to 1e-6, not to the bit.)"""
    K, M = _pinhole(K, c2w)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"camera_rays: bad image size {H} x {W}")
    py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
    v = np.stack([(px.astype(np.float64) - K[0, 2]) / K[0, 0], (py.astype(np.float64) - K[1, 2]) / K[1, 1], np.ones(H * W)], 1)
    v, _ = unit_normal(v)
    d = np.stack([(M[r, 0] * v[:, 0] + M[r, 1] * v[:, 1]) + M[r, 2] * v[:, 2] for r in range(3)], 1).astype(np.float32)
    o = np.broadcast_to(M[:, 3].astype(np.float32), d.shape)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def orbit_c2w(n_views, elevation_deg=20.0, radius=2.0, up=(0.0, 0.0, 1.0)):
    """float32 [n,4,4]: look-at cameras on a circle around the origin, view i at azimuth 2 pi i / n about ``up`` and ``elevation_deg`` above the plane
    through the origin; camera axes as everywhere here (x right, y down, z forward: the ray through the principal point runs to the origin)."""
    n = int(n_views)
    e, radius = np.deg2rad(float(elevation_deg)), float(radius)
    if n < 1 or not (abs(float(elevation_deg)) < 90.0) or not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError(f"orbit_c2w: n_views >= 1, |elevation| < 90 degrees and a finite radius > 0 expected, got {n_views!r}, {elevation_deg!r}, {radius!r}")
    up = np.asarray(up, np.float64)
    up = up / np.linalg.norm(up)
    a0 = np.cross(up, [1.0, 0.0, 0.0]) if abs(up[0]) < 0.9 else np.cross(up, [0.0, 1.0, 0.0])
    a0 /= np.linalg.norm(a0)
    a1 = np.cross(up, a0)
    out = np.zeros((n, 4, 4), np.float64)
    for i in range(n):
        az = 2.0 * np.pi * i / n
        pos = radius * (np.cos(e) * (np.cos(az) * a0 + np.sin(az) * a1) + np.sin(e) * up)
        f = -pos / np.linalg.norm(pos)
        r = np.cross(f, up)
        r /= np.linalg.norm(r)
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2], out[i, :3, 3], out[i, 3, 3] = r, np.cross(f, r), f, pos, 1.0
    return out.astype(np.float32)


def _colour_u8(c):
    """csrc/mesh_math.h mesh_colour_u8: (uint8)(int)(c * 255.f), truncation in float32"""
    with np.errstate(all="ignore"):
        return (np.asarray(c, np.float32) * np.float32(255.0)).astype(np.int32).astype(np.uint8)


def pack_images(kind, depth, rgb, grad, H, W, background=(0, 0, 0, 0)):
    """Per-ray results in raster order -> (color u8 [H,W,4], normal u8 [H,W,4], depth f32 [H,W]).  kind u8 [H W]; depth f32 [H W]; rgb, grad f32 [H W, 3],
    read at hits (kind != 0) only.  Colour: the vertex colours' truncating quantisation, alpha 255; a miss gets ``background`` (four uint8).  Normal: the
    same quantisation of float32(n 0.5 + 0.5) with n = unit_normal(grad) in fp64 (0 for a zero or non-finite gradient), alpha 255; a miss is 0, 0, 0, 0.
    Depth: the ray's depth at a hit, 0 at a miss."""
    H, W = int(H), int(W)
    kind = np.asarray(kind, np.uint8).reshape(-1)
    bg = np.asarray(background)
    if kind.shape[0] != H * W or H < 1 or W < 1:
        raise ValueError(f"pack_images: {kind.shape[0]} rays do not fill {H} x {W}")
    if bg.shape != (4,) or not np.array_equal(bg, bg.astype(np.uint8)):
        raise ValueError(f"pack_images: background is four integers in [0, 255], got {background!r}")
    hit = kind != 0
    color = np.tile(bg.astype(np.uint8), (H * W, 1))
    normal = np.zeros((H * W, 4), np.uint8)
    out_depth = np.zeros(H * W, np.float32)
    color[hit, :3], color[hit, 3] = _colour_u8(np.asarray(rgb, np.float32).reshape(-1, 3)[hit]), 255
    n, _ = unit_normal(np.asarray(grad, np.float32).reshape(-1, 3)[hit].astype(np.float64))
    normal[hit, :3], normal[hit, 3] = _colour_u8((n * 0.5 + 0.5).astype(np.float32)), 255
    out_depth[hit] = np.asarray(depth, np.float32).reshape(-1)[hit]
    return color.reshape(H, W, 4), normal.reshape(H, W, 4), out_depth.reshape(H, W)
