"""Synthetic inputs for the reconstruction hot path (no checkpoint / Zero123 output is available offline).

The camera rig and the scene normalisation follow the reference's data path so that the
tensors have the same geometry as a real run:

* rig: ``utils/utils.py:80-127`` (``calc_pose`` / ``get_poses``: radius 1.2, 8 stage-1 views,
  32 stage-2 views at +-10 deg), intrinsics ``utils/utils.py:133-135`` (f=280, c=128),
  near/far ``(0.5, 1.8)``.
* loader: ``reconstruction/data/One2345_eval_new_data.py:169-300`` (blender->opencv flip, poses
  relative to view 0, ``scale_mat`` from the union of the view frusta x1.1, ``affine_mats = K @ w2c``
  in the normalised frame, ``query_near_far = (0.95(d-1), 1.05(d+1))``) and
  ``reconstruction/data/scene.py:15-101`` (frustum corners / bounding box).

Everything here is plain numpy (host-side data prep, microseconds); the reference uses
``cv2.decomposeProjectionMatrix`` to recover the normalised pose, which for P = K [R|t] diag(r,r,r,1)
with a translation has the closed form  R' = R,  C' = (C - centre) / r.
"""
import numpy as np

BLENDER2OPENCV = np.diag([1.0, -1.0, -1.0, 1.0])


def _normalize(v):
    return v / (np.linalg.norm(v, axis=-1, keepdims=True) + 1e-10)


def rig_c2ws(init_polar_deg=60.0, radius=1.2, deg=10.0):
    """40 camera-to-world poses (8 stage-1 + 32 stage-2) in the rig frame, float32 like the reference."""
    mid = init_polar_deg
    if init_polar_deg <= 75:
        other = mid + 30
    else:
        other = mid - 30
    polar = np.radians(np.array([mid] * 4 + [other] * 4 + [mid - deg, mid + deg, mid, mid] * 4
                                + [other - deg, other + deg, other, other] * 4, dtype=np.float64)).astype(np.float32)
    overlook = [30 + 90 * k for k in range(4)]
    eyelevel = [60 + 90 * k for k in range(4)]
    delta = [0, 0, -deg, deg]
    azim = np.radians(np.array(overlook + eyelevel + [t + d for t in overlook for d in delta]
                               + [t + d for t in eyelevel for d in delta], dtype=np.float64)).astype(np.float32)
    centers = np.stack([radius * np.sin(azim) * np.sin(polar),
                        -radius * np.cos(azim) * np.sin(polar),
                        radius * np.cos(polar)], axis=-1).astype(np.float32)
    fwd = _normalize(centers)
    up = np.tile(np.array([[0, 0, 1]], np.float32), (len(centers), 1))
    right = _normalize(np.cross(up, fwd))
    up = _normalize(np.cross(fwd, right))
    poses = np.tile(np.eye(4, dtype=np.float32)[None], (len(centers), 1, 1))
    poses[:, :3, 0], poses[:, :3, 1], poses[:, :3, 2], poses[:, :3, 3] = right, up, fwd, centers
    return poses.astype(np.float64)


def _frustum_bounds(K, c2w, near, far, hw):
    h, w = hw
    xs = np.array([0, 0, w, w, 0, 0, w, w], np.float32)
    ys = np.array([0, h, 0, h, 0, h, 0, h], np.float32)
    ds = np.array([near] * 4 + [far] * 4, np.float32)
    pts = np.stack([(xs - K[0, 2]) * ds / K[0, 0], (ys - K[1, 2]) * ds / K[1, 1], ds, np.ones(8, np.float32)])
    return (c2w.astype(np.float32) @ pts.astype(np.float32))[:3]


def make_scene(n_views=8, image_seed=0, hw=(256, 256), polar=60.0, images="rand"):
    """Return the hot path's input contract as numpy arrays, batch dim dropped.

    n_views = 32 reproduces the reference configuration (all stage-2 views); n_views = 8 takes one
    stage-2 view per stage-1 view (files ``{k}_0.png``: source indices 0,4,...,28).  The rig has 32 source views: more raises.
    """
    if not 1 <= int(n_views) <= 32:
        raise ValueError(f"make_scene: n_views = {n_views}, but the rig has 32 source views (1 to 32 can be taken from it)")
    h, w = hw
    K4 = np.eye(4)
    f = 280.0 * w / 256.0                                # reference: 280 at 256^2
    K4[:3, :3] = [[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]]
    near_far = (1.2 - 0.7, 1.2 + 0.6)
    c2w_rig = rig_c2ws(polar) @ BLENDER2OPENCV
    w2c_rig = np.linalg.inv(c2w_rig)
    ref_inv = np.linalg.inv(w2c_rig[0])
    ids = [0] + list(range(8, 40))                       # target view + the 32 source views
    ext = np.stack([w2c_rig[i] @ ref_inv for i in ids])  # world = camera frame of view 0
    lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    for e in ext:
        p = _frustum_bounds(K4, np.linalg.inv(e.astype(np.float32)), near_far[0], near_far[1], (h, w))
        lo, hi = np.minimum(lo, p.min(1)), np.maximum(hi, p.max(1))
    center = ((hi + lo) / 2).astype(np.float32)
    radius = np.float32((hi - lo).max() / 2) * np.float32(1.1)
    scale_mat = np.diag([radius, radius, radius, 1.0]).astype(np.float32)
    scale_mat[:3, 3] = center

    def norm_pose(e):
        c2w_old = np.linalg.inv(e)
        c2w = np.eye(4)
        c2w[:3, :3] = c2w_old[:3, :3]
        c2w[:3, 3] = (c2w_old[:3, 3] - center) / radius
        return c2w

    c2ws = np.stack([norm_pose(e) for e in ext])
    w2cs = np.linalg.inv(c2ws)
    aff = np.tile(np.eye(4)[None], (len(ids), 1, 1))
    aff[:, :3, :4] = K4[:3, :3] @ w2cs[:, :3, :4]
    d = np.linalg.norm(c2ws[:, :3, 3], axis=-1)
    nf = np.stack([0.95 * (d - 1), 1.05 * (d + 1)], -1)
    src = np.arange(1, 33) if n_views == 32 else 1 + np.arange(n_views) * (32 // n_views)
    rng = np.random.default_rng(image_seed)
    if images == "rand":
        imgs = rng.random((len(src), 3, h, w), dtype=np.float32)
    else:
        imgs = np.ones((len(src), 3, h, w), np.float32)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(images=imgs, intrinsics=f32(np.tile(K4[None, :3, :3], (len(src), 1, 1))), w2cs=f32(w2cs[src]),
                c2ws=f32(c2ws[src]), affine_mats=f32(aff[src]), partial_vol_origin=f32([-1, -1, -1]),
                query_c2w=f32(c2ws[0]), query_w2c=f32(w2cs[0]), query_near_far=f32(nf[0]),
                query_intrinsic=f32(K4[:3, :3]), scale_mat=scale_mat, trans_mat=f32(ref_inv), img_wh=(w, h))


def gen_rays(K, c2w, H, W, scale=1):
    """Pixel-grid rays (``reconstruction/models/rays.py:11-54``); ``scale`` renders an (H*scale)x(W*scale)
    virtual camera with K scaled accordingly (BASELINE config 2: 512x512 rays from the 256^2 rig)."""
    Hs, Ws = H * scale, W * scale
    Ks = K.astype(np.float64).copy()
    Ks[:2] *= scale
    ys, xs = np.meshgrid(np.linspace(0, Hs - 1, Hs), np.linspace(0, Ws - 1, Ws), indexing="ij")
    p = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3).astype(np.float32)
    p = (np.linalg.inv(Ks).astype(np.float32) @ p.T).T
    v = p / np.linalg.norm(p, axis=-1, keepdims=True)
    v = (c2w[:3, :3].astype(np.float32) @ v.T).T
    o = np.broadcast_to(c2w[:3, 3].astype(np.float32), v.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(v, np.float32)
