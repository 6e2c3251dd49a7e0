"""Host twin of the mesh rasterizer (csrc/mesh_raster.hip, csrc/mesh_raster_math.h): depth, barycentrics, face id and the shading inputs per pixel of a
triangle mesh seen from a pinhole camera.  numpy only, no GPU.  This file is the DEFINITION: the device equals it to the last bit.  All real arithmetic is
fp64, one operation at a time, in the order written; coverage is decided in integers.  include/o2345.h carries the same text.

Camera      surface.camera_rays' one: K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] and c2w [12], host float32 widened to fp64; here fx, fy > 0 and the 3 x 3 of
            c2w is a rotation (|R^T R - I| <= 1e-5 in every entry).  x right, y down, z forward; the sample of pixel (px, py) is the integer point (px, py).
Corners     A face's corners are renumbered for the computation: corner 0 is the stored corner with the smallest vertex index, the others follow in
            stored (cyclic) order, so that the result does not depend on which corner a face is stored from.  Outputs are in STORED order.
Screen      q = p - t; x_c = (R00 q_x + R10 q_y) + R20 q_z, y_c with column 1, z_c with column 2; X = x_c / z_c * fx + cx, Y = y_c / z_c * fy + cy;
            sx = (int64) floor(X * 256 + 0.5), sy likewise.
Classes     a face is skipped under the first that applies: an index outside [0, nv) (never dereferenced); a non-finite coordinate; a corner that fails
            z_c >= near (no clipping); a corner that fails |X| <= 2^21 and |Y| <= 2^21; A2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) == 0 on the snapped
            integers; culled (cull 1 drops back faces, 2 front faces; a face is FRONT iff A2 < 0: with y down, a triangle whose (P1 - P0) x (P2 - P0)
            points at the camera runs clockwise on the screen's axes); the pixel box [ceil(min sx / 256), floor(max sx / 256)] x [.. sy ..] clipped
            to the image is empty.
Coverage    A2 < 0: corners 1 and 2 are exchanged (A2 > 0 afterwards).  With a = corner (i + 1) % 3, b = corner (i + 2) % 3, d = b - a and P = (256 px, 256 py):
            w_i = d_x (P_y - a_y) - d_y (P_x - a_x).  Covered iff for every i: w_i > 0, or w_i == 0 and (d_y > 0, or d_y == 0 and d_x < 0).
Depth       l_i = double(w_i) / double(A2); u_i = l_i / z_i (z_i: z_c of the unsnapped corner); iz = (u_0 + u_1) + u_2; z = 1 / iz; b_i = u_i * z.  A face
            whose z fails z < inf does not cover the pixel.
Visibility  the covering face with the smallest z; ties go to the smaller face index.
Outputs     face int32 (-1: none), depth float32 (z, or with ray_depth z * sqrt((vx vx + vy vy) + 1), v = ((px - cx) / fx, (py - cy) / fy, 1): the t of
            the ray through the pixel; 0 without a hit), bary float32 [H,W,3] in stored corner order (0 without a hit).
Shading     from face and the float32 bary widened to fp64, corners in stored order: rgb = (b0 c0 + b1 c1) + b2 c2 rounded to float32 once (0.5 without
            vertex colours), nrm likewise from vertex normals, or the flat (P1 - P0) x (P2 - P0) of the fp64 vertices; kind 1 at a hit.  pack_images of
            surface.py turns them into images.
Limits      no near clipping (a face with a corner in front of `near` is dropped whole), one sample per pixel, corners snapped to 1/256 pixel, corners beyond
            2^21 pixels drop the face.

Textured shading (shade_textured; csrc/mesh_raster_tex_math.h): a second shading stage behind the same visibility, on the buffers a textured asset
file holds, in the asset's own frame.  fp64, one operation at a time, in the order written; a dot product is (x x + y y) + z z; every result is rounded
to float32 once.  Inputs, only read: the soup verts fp64 [nv,3] and tris [nt,3] (a file: its positions widened, tris = 0, 1, 2, ...), face and bary of
the emit, uv float32 [nt,3,2] per stored corner (the file's TEXCOORD_0), image uint8 [Ht,Wt,4], optionally normal_image uint8 [Ht,Wt,4] with normals
float32 [3 nt,3] and tangents float32 [3 nt,4] (the file's NORMAL / TANGENT; the frame of triangle t is read at corner 3t), the camera and ambient in
[0, 1] (a float32).  Per pixel whose face is in [0, nt) and has its three indices in [0, nv) (any other pixel is a miss: kind 0, everything 0):
  uv        u = (b0 u0 + b1 u1) + b2 u2, v likewise, bary widened.  u or v not finite: rgb 0, lit 0, nrm the flat normal (N of corner 3t with a normal
            map), counted (bad_uv); the pixel is still a hit.
  fetch     mesh_io.sample_texture: x = u Wt - 0.5, y = v Ht - 0.5, x0 = floor(x), fx = x - x0, y0 and fy likewise; taps (0,0), (1,0), (0,1), (1,1) at
            column clamp(x0 + dx, 0, Wt - 1), row clamp(y0 + dy, 0, Ht - 1): the sum and the clamp are done in floating point, the conversion to an
            integer comes last, so that no uv overflows an index; weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; value = ((w00 c00 + w10
            c10) + w01 c01) + w11 c11 per channel on the bytes widened.  Albedo rgb = float32(value / 255.0), channels 0 - 2.
  normal    without a normal map: the unnormalised flat (P1 - P0) x (P2 - P0) of the fp64 vertices, as shade gives it.  With one: s = the same fetch of
            the normal image, (x, y, z) = s / 255.0 * 2.0 - 1.0; N, T, w of corner 3t promoted; B = w (N x T); m = (x T + y B) + z N; l = sqrt(m . m);
            nrm = float32(m / l).  A triangle with texture_frames' degenerate mark (TANGENT.y is a negative zero), or an l that is zero or not finite:
            nrm = N, counted (flat_frame).
  lit       d_k = (R_k0 vx + R_k1 vy) + R_k2 with v as in the depth, divided by sqrt(d . d): the pixel's ray in the mesh's frame; n = nrm widened,
            divided by sqrt(n . n), or 0 if that length is zero or not finite; c = n . d; s = -c if -c > 0, else 0; lit = float32(rgb (ambient + (1 -
            ambient) s)) per channel, rgb the float32 albedo widened.  c > 0 is counted (back_lit, informative).  Both vectors live in the mesh's
            frame: the term does not depend on the handedness of the camera matrix.
Counts: TEX_COUNTS, int64 [4] on the device.  A camera whose 3 x 3 has a negative determinant (asset_camera's: the asset frame is a reflection of the
reconstruction frame) shows a face from outside with A2 > 0; the textured front ends exchange cull 1 and 2 under such a camera, so that cull = 1 keeps
meaning "drop what is seen from behind".  Limits: one bilinear sample per pixel, no mip maps, CLAMP_TO_EDGE only, a Lambert headlight and nothing else."""
import numpy as np

from . import surface

TILE = 8
SUBPIXEL = 256
MAX_PIXELS = float(1 << 21)
CLASSES = ("ok", "bad_index", "nonfinite", "near", "range", "degenerate", "culled", "offscreen")
COUNTS = CLASSES[1:] + ("binned", "pairs", "pixels")            # the device's int64 counts, by O2345_RASTER_* in include/o2345.h
TEX_COUNTS = ("bad_uv", "flat_frame", "back_lit", "reserved")   # the textured stage's int64 [4]
TEX_MAX_SIDE = 16384


def camera(K, c2w, near, cull):
    """The checked camera of a call -> dict(R fp64 [3,3], t fp64 [3], fx, fy, cx, cy, near, cull)"""
    K, M = surface._pinhole(K, c2w)
    if not (K[0, 0] > 0.0 and K[1, 1] > 0.0):
        raise ValueError(f"raster: fx and fy must be > 0, got {K[0, 0]!r} and {K[1, 1]!r}")
    R = M[:, :3]
    if not (np.abs(R.T @ R - np.eye(3)) <= 1e-5).all():
        raise ValueError("raster: the 3 x 3 of c2w must be a rotation (|R^T R - I| <= 1e-5 in every entry)")
    near = float(near)
    if not (np.isfinite(near) and near > 0.0):
        raise ValueError(f"raster: near must be finite and > 0, got {near!r}")
    if isinstance(cull, (bool, np.bool_)) or cull not in (0, 1, 2):
        raise ValueError(f"raster: cull is 0 (none), 1 (back faces) or 2 (front faces), got {cull!r}")
    return dict(R=R, t=M[:, 3], fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near=near, cull=int(cull))


def _image_size(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"raster: bad image size {H} x {W}")
    return H, W


def _mesh(verts, tris):
    verts, tris = np.asarray(verts), np.asarray(tris)
    if verts.dtype != np.float64 or verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError(f"raster: vertices are float64 [nv,3], got {verts.dtype} {verts.shape}")
    if tris.dtype not in (np.int32, np.int64) or tris.ndim != 2 or tris.shape[1] != 3:
        raise ValueError(f"raster: triangles are int32 / int64 [nt,3], got {tris.dtype} {tris.shape}")
    if verts.shape[0] >= 2 ** 30 or 3 * tris.shape[0] >= 2 ** 31:
        raise ValueError(f"raster: bad sizes ({verts.shape[0]} vertices, {tris.shape[0]} triangles)")
    return verts, tris.astype(np.int64)


def face_setup(verts, tris, cam, H, W):
    """Per face -> dict(cls int [nt] (index into CLASSES), sx, sy int64 [nt,3] and z fp64 [nt,3] in computation order, corner int [nt,3] (the stored
    corner of computation corner j), box int64 [nt,4] = px0, py0, px1, py1 clipped to the image, a2 int64 [nt] (> 0 for a face that takes part)).  A face
    that fails one of the first four classes has zeros everywhere but in cls."""
    verts, tris = _mesh(verts, tris)
    H, W = _image_size(H, W)
    nv, nt = verts.shape[0], tris.shape[0]
    R, t = cam["R"], cam["t"]
    with np.errstate(all="ignore"):
        in_range = ((tris >= 0) & (tris < nv)).all(1)
        rot = np.argmin(tris, 1)                                            # the first smallest index
        corner = (rot[:, None] + np.arange(3)[None, :]) % 3
        idx = np.where(in_range[:, None], np.take_along_axis(tris, corner, 1), 0)
        P = verts[idx] if nv else np.zeros((nt, 3, 3))
        finite = np.isfinite(P).all((1, 2))
        q = P - t
        cc = [(R[0, k] * q[..., 0] + R[1, k] * q[..., 1]) + R[2, k] * q[..., 2] for k in range(3)]
        X = cc[0] / cc[2] * cam["fx"] + cam["cx"]
        Y = cc[1] / cc[2] * cam["fy"] + cam["cy"]
        near_ok = (cc[2] >= cam["near"]).all(1)
        range_ok = ((np.abs(X) <= MAX_PIXELS) & (np.abs(Y) <= MAX_PIXELS)).all(1)
        stage = in_range & finite & near_ok & range_ok
        s = stage[:, None]
        sx = np.floor(np.where(s, X, 0.0) * float(SUBPIXEL) + 0.5).astype(np.int64)
        sy = np.floor(np.where(s, Y, 0.0) * float(SUBPIXEL) + 0.5).astype(np.int64)
        z = np.where(s, cc[2], 0.0)
    corner = np.where(s, corner, 0)
    a2 = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sy[:, 1] - sy[:, 0]) * (sx[:, 2] - sx[:, 0])
    front = a2 < 0
    for a in (sx, sy, z, corner):
        a[front, 1], a[front, 2] = a[front, 2].copy(), a[front, 1].copy()
    a2 = np.abs(a2)
    culled = (front & (cam["cull"] == 2)) | (~front & (cam["cull"] == 1))
    box = np.stack([np.maximum(-((-sx.min(1)) // SUBPIXEL), 0), np.maximum(-((-sy.min(1)) // SUBPIXEL), 0),
                    np.minimum(sx.max(1) // SUBPIXEL, W - 1), np.minimum(sy.max(1) // SUBPIXEL, H - 1)], 1)
    box = np.where(s, box, 0)
    empty = (box[:, 0] > box[:, 2]) | (box[:, 1] > box[:, 3])
    cls = np.select([~in_range, ~finite, ~near_ok, ~range_ok, a2 == 0, culled, empty], [1, 2, 3, 4, 5, 6, 7], 0)
    return dict(cls=cls.astype(np.int64), sx=sx, sy=sy, z=z, corner=corner.astype(np.int64), box=box, a2=np.where(s[:, 0], a2, 0))


def pixel_terms(setup, f, px, py):
    """Face f (one that takes part) at the pixels (px, py), int64 arrays inside its box -> (w int64 [n,3], covered bool [n], z fp64 [n], b fp64 [n,3] in
    computation order; z and b are what the arithmetic gives wherever the edge functions cover, garbage elsewhere)"""
    sx, sy, zc, a2 = setup["sx"][f], setup["sy"][f], setup["z"][f], setup["a2"][f]
    Px, Py = SUBPIXEL * np.asarray(px, np.int64), SUBPIXEL * np.asarray(py, np.int64)
    w, inside = [], np.ones(Px.shape, bool)
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = int(sx[b] - sx[a]), int(sy[b] - sy[a])
        wi = dx * (Py - int(sy[a])) - dy * (Px - int(sx[a]))
        inside &= (wi > 0) | ((wi == 0) & (dy > 0 or (dy == 0 and dx < 0)))
        w.append(wi)
    w = np.stack(w, -1)
    with np.errstate(all="ignore"):
        lam = w.astype(np.float64) / float(a2)
        u = lam / zc
        iz = (u[..., 0] + u[..., 1]) + u[..., 2]
        z = 1.0 / iz
        b = u * z[..., None]
        covered = inside & (z < np.inf)
    return w, covered, z, b


def shade(verts, tris, face, bary, vertex_colors=None, vertex_normals=None):
    """face int32 [H,W] and bary float32 [H,W,3] -> (kind uint8 [H W], rgb float32 [H W,3], nrm float32 [H W,3]): the packer's inputs"""
    verts, tris = _mesh(verts, tris)
    face, bary = np.asarray(face, np.int32).reshape(-1), np.asarray(bary, np.float32).reshape(-1, 3).astype(np.float64)
    n = face.shape[0]
    hit = (face >= 0) & (face < tris.shape[0])
    kind, rgb, nrm = hit.astype(np.uint8), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    idx, b = tris[face[hit]], bary[hit]

    def attribute(a, what):
        a = np.asarray(a)
        if a.dtype != np.float32 or a.shape != verts.shape:
            raise ValueError(f"raster: {what} are float32 [nv,3], got {a.dtype} {a.shape}")
        c = a.astype(np.float64)[idx]                                      # [n,3 corners,3]
        return ((b[:, 0, None] * c[:, 0] + b[:, 1, None] * c[:, 1]) + b[:, 2, None] * c[:, 2]).astype(np.float32)

    with np.errstate(all="ignore"):
        rgb[hit] = np.float32(0.5) if vertex_colors is None else attribute(vertex_colors, "vertex colours")
        if vertex_normals is None:
            P = verts[idx]
            e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
            nrm[hit] = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                                 e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(np.float32)
        else:
            nrm[hit] = attribute(vertex_normals, "vertex normals")
    return kind, rgb, nrm


def rasterize(verts, tris, K, c2w, H, W, near=1e-3, cull=0, ray_depth=False, vertex_colors=None, vertex_normals=None):
    """verts float64 [nv,3] in the world frame, tris int32 / int64 [nt,3] -> dict(face int32 [H,W], depth float32 [H,W], bary float32 [H,W,3], kind uint8
    [H W], rgb float32 [H W,3], nrm float32 [H W,3], info: the counts by COUNTS).  The module's header is the definition."""
    cam = camera(K, c2w, near, cull)
    H, W = _image_size(H, W)
    S = face_setup(verts, tris, cam, H, W)
    cls, box = S["cls"], S["box"]
    info = {name: int((cls == k + 1).sum()) for k, name in enumerate(CLASSES[1:])}
    part = np.flatnonzero(cls == 0)
    tb = box[part] // TILE
    info["binned"] = int(part.shape[0])
    info["pairs"] = int(((tb[:, 2] - tb[:, 0] + 1) * (tb[:, 3] - tb[:, 1] + 1)).sum())
    best_z, best_f, best_b = np.full((H, W), np.inf), np.full((H, W), -1, np.int32), np.zeros((H, W, 3))
    for f in part:
        x0, y0, x1, y1 = (int(v) for v in box[f])
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        _, covered, z, b = pixel_terms(S, f, px, py)
        zz, ff = best_z[y0:y1 + 1, x0:x1 + 1], best_f[y0:y1 + 1, x0:x1 + 1]
        win = covered & ((z < zz) | ((z == zz) & (f < ff)))
        zz[win], ff[win] = z[win], f
        stored = np.empty_like(b)
        stored[..., S["corner"][f]] = b
        best_b[y0:y1 + 1, x0:x1 + 1][win] = stored[win]
    hit = best_f >= 0
    info["pixels"] = int(hit.sum())
    with np.errstate(all="ignore"):
        t = best_z
        if ray_depth:
            py, px = np.mgrid[0:H, 0:W]
            vx, vy = (px.astype(np.float64) - cam["cx"]) / cam["fx"], (py.astype(np.float64) - cam["cy"]) / cam["fy"]
            t = best_z * np.sqrt((vx * vx + vy * vy) + 1.0)
        depth = np.where(hit, t, 0.0).astype(np.float32)
    bary = np.where(hit[..., None], best_b, 0.0).astype(np.float32)
    kind, rgb, nrm = shade(verts, tris, best_f, bary, vertex_colors, vertex_normals)
    return dict(face=best_f, depth=depth, bary=bary, kind=kind, rgb=rgb, nrm=nrm, info=info)


def render(verts, tris, K, c2w, H, W, background=(0, 0, 0, 0), **kw):
    """rasterize + surface.pack_images -> dict(color u8 [H,W,4], normal u8 [H,W,4], depth f32 [H,W], face int32 [H,W], info)"""
    r = rasterize(verts, tris, K, c2w, H, W, **kw)
    color, normal, depth = surface.pack_images(r["kind"], r["depth"].reshape(-1), r["rgb"], r["nrm"], H, W, background)
    return dict(color=color, normal=normal, depth=depth, face=r["face"], info=r["info"])


# ---------------------------------------------------------------------------------------------------------- textured shading
def _ambient(ambient):
    a = float(np.float32(ambient))
    if not (0.0 <= a <= 1.0):
        raise ValueError(f"raster: ambient must be in [0, 1], got {ambient!r}")
    return a


def _atlas(image, what):
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 4 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"raster: {what} is uint8 [Ht,Wt,4], got {image.dtype} {image.shape}")
    if image.shape[0] > TEX_MAX_SIDE or image.shape[1] > TEX_MAX_SIDE or image.shape[0] * image.shape[1] >= 2 ** 31:
        raise ValueError(f"raster: {what} of {image.shape[1]} x {image.shape[0]}: a side is limited to {TEX_MAX_SIDE}")
    return image


def fetch_texture(image, u, v):
    """image uint8 [Ht,Wt,C], u and v fp64 [n], finite -> (value fp64 [n,C], taps: four (column int64 [n], row int64 [n], weight fp64 [n])): the header's
    fetch.  The tap's coordinate is summed and clamped in floating point and converted to an integer last."""
    Ht, Wt = image.shape[:2]
    x, y = u * float(Wt) - 0.5, v * float(Ht) - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    value, taps = None, []
    for dx, dy, w in ((0.0, 0.0, (1.0 - fx) * (1.0 - fy)), (1.0, 0.0, fx * (1.0 - fy)), (0.0, 1.0, (1.0 - fx) * fy), (1.0, 1.0, fx * fy)):
        xs, ys = x0 + dx, y0 + dy
        xi = np.where(xs < 0.0, 0.0, np.where(xs > float(Wt - 1), float(Wt - 1), xs)).astype(np.int64)
        yi = np.where(ys < 0.0, 0.0, np.where(ys > float(Ht - 1), float(Ht - 1), ys)).astype(np.int64)
        term = w[:, None] * image[yi, xi].astype(np.float64)
        value = term if value is None else value + term
        taps.append((xi, yi, w))
    return value, taps


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def texture_uv(b, c):
    """bary fp64 [m,3] and the triangles' uv fp64 [m,3,2] -> (u, v fp64 [m], good: both finite)"""
    with np.errstate(all="ignore"):
        u = (b[:, 0] * c[:, 0, 0] + b[:, 1] * c[:, 1, 0]) + b[:, 2] * c[:, 2, 0]
        v = (b[:, 0] * c[:, 0, 1] + b[:, 1] * c[:, 1, 1]) + b[:, 2] * c[:, 2, 1]
    return u, v, np.isfinite(u) & np.isfinite(v)


def tangent_normal(value, Nf, Tf):
    """The fetched normal texels fp64 [m,3] (0 .. 255) and the float32 frames N [m,3], (T, w) [m,4] -> (nrm float32 [m,3], ok [m]; N where not ok)"""
    with np.errstate(all="ignore"):
        s = value / 255.0 * 2.0 - 1.0
        N, T, w = Nf.astype(np.float64), Tf[:, :3].astype(np.float64), Tf[:, 3:].astype(np.float64)
        B = w * _cross(N, T)
        m = (s[:, 0:1] * T + s[:, 1:2] * B) + s[:, 2:3] * N
        l = np.sqrt(_dot(m, m))
        ok = ~((Tf[:, 1] == 0.0) & np.signbit(Tf[:, 1])) & (l > 0.0) & (l < np.inf)
        return np.where(ok[:, None], (m / l[:, None]).astype(np.float32), Nf), ok


def headlight(K, M, px, py, nrm, ambient):
    """The fp64 K and c2w [3,4], pixels int64 [m], nrm float32 [m,3] -> (the factor ambient + (1 - ambient) max(0, -(n . d)) fp64 [m], n . d fp64 [m])"""
    with np.errstate(all="ignore"):
        vx, vy = (px.astype(np.float64) - K[0, 2]) / K[0, 0], (py.astype(np.float64) - K[1, 2]) / K[1, 1]
        d = np.stack([(M[k, 0] * vx + M[k, 1] * vy) + M[k, 2] for k in range(3)], 1)
        d = d / np.sqrt(_dot(d, d))[:, None]
        g = nrm.astype(np.float64)
        l = np.sqrt(_dot(g, g))
        g = np.where(((l > 0.0) & (l < np.inf))[:, None], g / l[:, None], 0.0)
        cosine = _dot(g, d)
        return ambient + (1.0 - ambient) * np.where(-cosine > 0.0, -cosine, 0.0), cosine


def shade_textured(verts, tris, face, bary, uv, image, K, c2w, normals=None, tangents=None, normal_image=None, ambient=0.25):
    """The textured shading stage (the module's header is the definition): face int32 [H,W], bary float32 [H,W,3] of the emit -> (kind uint8 [H W], rgb
    float32 [H W,3] the albedo, nrm float32 [H W,3], lit float32 [H W,3], counts: TEX_COUNTS[:3] by name).  uv float32 [nt,3,2] (or [3 nt,2]), image
    uint8 [Ht,Wt,4]; normals float32 [3 nt,3], tangents float32 [3 nt,4] and normal_image uint8 [Ht,Wt,4] together or not at all."""
    verts, tris = _mesh(verts, tris)
    nv, nt = verts.shape[0], tris.shape[0]
    Kd, M = surface._pinhole(K, c2w)
    ambient = _ambient(ambient)
    image = _atlas(image, "the atlas")
    uv = np.asarray(uv)
    if uv.dtype != np.float32 or uv.size != 6 * nt:
        raise ValueError(f"raster: uv are float32 [{nt},3,2], got {uv.dtype} {uv.shape}")
    uv = uv.reshape(nt, 3, 2).astype(np.float64)
    mapped = normal_image is not None
    if (normals is None) != (tangents is None) or (normals is None) == mapped:
        raise ValueError("raster: a normal map is normals, tangents and a normal image together")
    if mapped:
        normal_image = _atlas(normal_image, "the normal image")
        normals, tangents = np.asarray(normals), np.asarray(tangents)
        if normal_image.shape != image.shape:
            raise ValueError(f"raster: the normal image has the atlas's size {image.shape[:2]}, got {normal_image.shape[:2]}")
        if normals.dtype != np.float32 or normals.shape != (3 * nt, 3) or tangents.dtype != np.float32 or tangents.shape != (3 * nt, 4):
            raise ValueError(f"raster: normals are float32 [{3 * nt},3] and tangents float32 [{3 * nt},4], got {normals.shape} and {tangents.shape}")
    face = np.asarray(face, np.int32)
    H, W = _image_size(*face.shape)
    face, bary = face.reshape(-1), np.asarray(bary, np.float32).reshape(-1, 3).astype(np.float64)
    n = face.shape[0]
    hit = (face >= 0) & (face < nt)
    hit[hit] = ((tris[face[hit]] >= 0) & (tris[face[hit]] < nv)).all(1)
    kind = hit.astype(np.uint8)
    rgb, nrm, lit = (np.zeros((n, 3), np.float32) for _ in range(3))
    at = np.flatnonzero(hit)
    t = face[at]
    u, v, good = texture_uv(bary[at], uv[t])
    us, vs = np.where(good, u, 0.0), np.where(good, v, 0.0)                      # a bad pixel fetches nothing; its values are replaced below
    with np.errstate(all="ignore"):
        albedo = np.where(good[:, None], (fetch_texture(image, us, vs)[0][:, :3] / 255.0).astype(np.float32), np.float32(0.0))
        flat_frame = np.zeros(at.shape[0], bool)
        if mapped:
            shading, ok = tangent_normal(fetch_texture(normal_image, us, vs)[0][:, :3], normals[3 * t], tangents[3 * t])
            flat_frame = good & ~ok
            shading = np.where(good[:, None], shading, normals[3 * t])
        else:
            P = verts[tris[t]]
            shading = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).astype(np.float32)
        py, px = np.divmod(at, W)
        factor, cosine = headlight(Kd, M, px, py, shading, ambient)
        lit_hit = np.where(good[:, None], (albedo.astype(np.float64) * factor[:, None]).astype(np.float32), np.float32(0.0))
        back = good & (cosine > 0.0)
    rgb[at], nrm[at], lit[at] = albedo, shading, lit_hit
    return kind, rgb, nrm, lit, {"bad_uv": int((~good).sum()), "flat_frame": int(flat_frame.sum()), "back_lit": int(back.sum())}


def is_mirrored(c2w):
    """whether the 3 x 3 of a camera matrix has a negative determinant (asset_camera's has): the textured front ends then exchange cull 1 and 2"""
    return bool(np.linalg.det(np.asarray(c2w, np.float32).astype(np.float64)[:3, :3]) < 0.0)


def mirrored_cull(cull, c2w):
    return {1: 2, 2: 1}.get(cull, cull) if not isinstance(cull, (bool, np.bool_)) and is_mirrored(c2w) else cull


def _soup(positions):
    p = np.asarray(positions)
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] != 3 or p.shape[0] % 3:
        raise ValueError(f"raster: the positions of a textured asset are float32 [3 M,3], got {p.dtype} {p.shape}")
    return p.astype(np.float64), np.arange(p.shape[0], dtype=np.int32).reshape(-1, 3)


def rasterize_textured(positions, uv, image, K, c2w, H, W, near=1e-3, cull=0, ray_depth=False, normals=None, tangents=None, normal_image=None, ambient=0.25):
    """The buffers of a textured asset (positions float32 [3 M,3], uv float32 [3 M,2], image uint8 [Ht,Wt,4]; with the normal map its NORMAL, TANGENT and
    second image) under a camera in the ASSET's frame (asset_camera's, or any proper one) -> rasterize's dict with rgb = the atlas's albedo, nrm = the
    shading normal, plus lit float32 [H W,3] and tex_info.  ``cull`` 1 drops what is seen from behind, whatever the camera's handedness."""
    verts, tris = _soup(positions)
    r = rasterize(verts, tris, K, c2w, H, W, near=near, cull=mirrored_cull(cull, c2w), ray_depth=ray_depth)
    kind, rgb, nrm, lit, counts = shade_textured(verts, tris, r["face"], r["bary"], uv, image, K, c2w, normals, tangents, normal_image, ambient)
    return dict(r, kind=kind, rgb=rgb, nrm=nrm, lit=lit, tex_info=counts)


def render_textured(positions, uv, image, K, c2w, H, W, background=(0, 0, 0, 0), **kw):
    """rasterize_textured + surface.pack_images -> dict(color, lit, normal u8 [H,W,4], depth f32 [H,W], face int32 [H,W], info, tex_info)"""
    r = rasterize_textured(positions, uv, image, K, c2w, H, W, **kw)
    color, normal, depth = surface.pack_images(r["kind"], r["depth"].reshape(-1), r["rgb"], r["nrm"], H, W, background)
    lit = surface.pack_images(r["kind"], r["depth"].reshape(-1), r["lit"], r["nrm"], H, W, background)[0]
    return dict(color=color, lit=lit, normal=normal, depth=depth, face=r["face"], info=r["info"], tex_info=r["tex_info"])


def asset_camera(c2w, scale_mat=None, trans_mat=None):
    """A camera of the reconstruction frame -> (c2w_asset float32 [3,4], depth_scale s, mirrored) for the asset file's frame, whose positions are P (T (s p +
    t_s) + t_t) with P the exchange of y and z (mesh_io.frame_positions, then columns 1 and 2 swapped): c2w_asset = [P T3 R | P (T3 (s c + t_s) + t_t)],
    computed in fp64 and rounded to float32 once.  The asset under it projects to the pixels of the reconstruction-frame mesh under ``c2w``, with depths
    (and so ``near``) multiplied by s.  Refused: a trans_mat whose 3 x 3 is not orthogonal (|T^T T - I| <= 1e-5 in every entry), a scale that is not
    positive, finite and the same on the three axes.  The matrix is a reflection unless trans_mat is one: ``mirrored`` says so (is_mirrored)."""
    M = np.asarray(c2w, np.float32).astype(np.float64)
    if M.shape not in ((3, 4), (4, 4)) or not np.isfinite(M).all():
        raise ValueError(f"asset_camera: c2w is a finite [3,4] or [4,4], got {M.shape}")
    from . import mesh_io
    S, T = mesh_io._mat44(scale_mat), mesh_io._mat44(trans_mat)
    s, ts, T3, tt = 1.0, np.zeros(3), np.eye(3), np.zeros(3)
    if S is not None:
        s, ts = float(S[0, 0]), S[:3, 3]
        if not (np.isfinite(S).all() and s > 0.0 and S[1, 1] == s and S[2, 2] == s and (S[:3, :3] == np.diag([s, s, s])).all()):
            raise ValueError("asset_camera: scale_mat must hold one positive scale for the three axes and nothing else in its 3 x 3")
    if T is not None:
        T3, tt = T[:3, :3], T[:3, 3]
        if not (np.isfinite(T).all() and (np.abs(T3.T @ T3 - np.eye(3)) <= 1e-5).all()):
            raise ValueError("asset_camera: the 3 x 3 of trans_mat must be orthogonal (|T^T T - I| <= 1e-5 in every entry)")
    R = (T3 @ M[:3, :3])[[0, 2, 1]]
    c = (T3 @ (s * M[:3, 3] + ts) + tt)[[0, 2, 1]]
    out = np.concatenate([R, c[:, None]], 1).astype(np.float32)
    return out, s, is_mirrored(out)
