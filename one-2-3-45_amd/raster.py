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
            2^21 pixels drop the face."""
import numpy as np

from . import surface

TILE = 8
SUBPIXEL = 256
MAX_PIXELS = float(1 << 21)
CLASSES = ("ok", "bad_index", "nonfinite", "near", "range", "degenerate", "culled", "offscreen")
COUNTS = CLASSES[1:] + ("binned", "pairs", "pixels")            # the device's int64 counts, by O2345_RASTER_* in include/o2345.h


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
