"""What the normal-map tests share (tests/test_mesh_normal_map*.py, tests/test_gpu_mesh_normal_map.py): the marching-cubes ellipsoid and its analytic
gradient, small triangle strips with degenerate and bad inputs mixed in, the decoder that puts a texel back into the asset frame, and the bound it is
held to.  Everything here is written from the definition (include/o2345.h), never from the code under test."""
import importlib
import math

import numpy as np

mio = importlib.import_module("one-2-3-45_amd.mesh_io")

FLAT = np.array([128, 128, 255, 255], np.uint8)
# every channel is off by at most 1 / 255 (half a step of 2 / 255, and the clamp only moves values towards the true one), so the decoded vector is off by
# at most sqrt(3) / 255 against a unit vector, which turns it by at most asin(sqrt(3) / 255); 1e-6 for the float32 roundings of frame and reference
DECODE_BOUND = math.asin(math.sqrt(3.0) / 255.0) + 1e-6


def rotation():
    """trans_mat of tests/test_gpu_mesh_formats.py: a rotation about z and a translation, float32 [1,4,4] as the reference's sample dict carries it"""
    a = 0.6
    return np.array([[np.cos(a), -np.sin(a), 0, 0.3], [np.sin(a), np.cos(a), 0, -0.2], [0, 0, 1, 1.5], [0, 0, 0, 1]], np.float32)[None]


def ellipsoid(R=24):
    """-> (verts fp64 [N,3] index coordinates, faces int64 [M,3], grad_at: float32 world points -> the field's gradient float32) of the oracle's marching
    cubes on u = 0.8 - sqrt(x^2 + 1.3 y^2 + z^2): u = -sdf, so the gradient of the SDF points outwards"""
    from oracle import mc
    g = np.linspace(-1, 1, R, dtype=np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    v, f = mc.marching_cubes((0.8 - np.sqrt(X ** 2 + 1.3 * Y ** 2 + Z ** 2)).astype(np.float32), 0.0)

    def grad_at(world):
        w = np.asarray(world, np.float64)
        q = np.stack([w[:, 0], 1.3 * w[:, 1], w[:, 2]], 1)
        return (q / np.sqrt((q * q).sum(1))[:, None]).astype(np.float32)
    return v, f, grad_at


def owners(nt, c):
    """the owner triangle of every cell-major texel entry, from the A / B rule: local texel (i, j) belongs to 2k if i + j <= c - 1, else to min(2k + 1, nt - 1)"""
    cells = (nt + 1) // 2
    out = np.empty((cells, c, c), np.int64)
    for j in range(c):
        for i in range(c):
            out[:, j, i] = np.minimum(2 * np.arange(cells) + (1 if i + j >= c else 0), nt - 1)
    return out.reshape(-1)


def to_cells(image, nt, c):
    """image [H, W, C] -> its used cells in cell-major order [cells c^2, C], and the texels of the unused cells [n, C]"""
    L = mio.texture_layout(nt, c)
    G, cells = L["grid"], L["cells"]
    img = np.asarray(image)
    used, rest = [], []
    for k in range(L["rows"] * G):
        x0, y0 = (k % G) * c, (k // G) * c
        (used if k < cells else rest).append(img[y0:y0 + c, x0:x0 + c].reshape(c * c, -1))
    return np.concatenate(used), (np.concatenate(rest) if rest else np.zeros((0, img.shape[-1]), img.dtype))


def decode_angles(image, normals, tangents, nt, c, want):
    """the angle between x T + y B + z N, normalised, of every texel of a used cell and the unit vectors ``want`` [cells c^2, 3], in radians"""
    d = to_cells(mio.decode_normal_map(image), nt, c)[0]
    t = owners(nt, c)
    N = np.asarray(normals, np.float64)[3 * t]
    T = np.asarray(tangents, np.float64)[3 * t, :3]
    B = np.asarray(tangents, np.float64)[3 * t, 3:] * np.cross(N, T)
    v = d[:, :1] * T + d[:, 1:2] * B + d[:, 2:] * N
    v /= np.sqrt((v * v).sum(1))[:, None]
    w = np.asarray(want, np.float64)
    return np.arctan2(np.sqrt((np.cross(v, w) ** 2).sum(1)), (v * w).sum(1))


def strip(nt, c, seed, rot=None, bad=True):
    """nt small triangles (v, f: index coordinates on a 512^3 grid) through texture_corners -> dict(pos, uv float32 as the file holds them; grad float32
    [cells c^2, 3]; degenerate: the triangles made so; bad, back: the texel entries with a bad and with a backward gradient).  With ``bad`` and nt >= 3, triangle nt // 2 loses its area (three equal
    corners), and for any nt entries 1, 2 and 3 get a zero, a NaN and an inf gradient; entry 5 gets minus its triangle's normal."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(100.0, 400.0, 3) + rng.uniform(-3.0, 3.0, (nt + 2, 3))
    f = np.stack([np.arange(nt), np.arange(nt) + 1, np.arange(nt) + 2], 1)
    f[1::2] = f[1::2, ::-1]
    pos, uv, _, _ = mio.texture_corners(v, f, c, 512, trans_mat=rot)
    pos, uv = pos.copy(), uv.copy()
    L = mio.texture_layout(nt, c)
    grad = rng.normal(0.0, 1.0, (L["texels"], 3)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, (L["texels"], 1)).astype(np.float32)
    out = dict(pos=pos, uv=uv, grad=grad, degenerate=[], bad=[], back=[], nt=nt, c=c, rot=rot, v=v, f=f)
    if bad:
        if nt >= 3:
            t = nt // 2
            pos[3 * t + 1] = pos[3 * t]
            pos[3 * t + 2] = pos[3 * t]
            out["degenerate"] = [t]
        grad[1] = 0.0
        grad[2] = [1.0, np.nan, 0.0]
        grad[3] = [np.inf, 1.0, 0.0]
        out["bad"] = [1, 2, 3]
        t5 = int(owners(nt, c)[5])
        if t5 not in out["degenerate"]:
            e1, e2 = pos[3 * t5 + 1].astype(np.float64) - pos[3 * t5], pos[3 * t5 + 2].astype(np.float64) - pos[3 * t5]
            n = -np.cross(e1, e2)[[0, 2, 1]]                                           # minus the face normal, y and z exchanged back
            if rot is not None:
                n = np.asarray(rot, np.float64).reshape(-1, 4, 4)[0, :3, :3].T @ n          # and back through the rotation
            grad[5] = (n / np.linalg.norm(n) * 3.0).astype(np.float32)
            out["back"] = [5]
    return out


# ---- the definition once more, in plain Python floats (IEEE doubles), one triangle and one texel at a time: what the numpy twin is held to on small inputs
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _div(a, b):
    """IEEE division: Python raises where C gives an infinity or a NaN"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(x)))


def _usable(l):
    return l > 0.0 and l < math.inf


def ref_frame(p, uv):
    """p float32 [3,3], uv float32 [3,2] of one triangle -> (N [3], TANGENT [4]) as Python floats holding float32 values, degenerate: bool"""
    p, uv = [[float(x) for x in r] for r in p], [[float(x) for x in r] for r in uv]
    e1, e2 = [p[1][d] - p[0][d] for d in range(3)], [p[2][d] - p[0][d] for d in range(3)]
    c = _cross(e1, e2)
    l = _sqrt(_dot(c, c))
    du1, dv1, du2, dv2 = uv[1][0] - uv[0][0], uv[1][1] - uv[0][1], uv[2][0] - uv[0][0], uv[2][1] - uv[0][1]
    det = du1 * dv2 - du2 * dv1
    if not (_usable(l) and _usable(abs(det))):
        return [0.0, 1.0, 0.0], [1.0, -0.0, 0.0, 1.0], True
    n = [_div(x, l) for x in c]
    Pu = [_div(e1[d] * dv2 - e2[d] * dv1, det) for d in range(3)]
    Pv = [_div(e2[d] * du1 - e1[d] * du2, det) for d in range(3)]
    s = _dot(n, Pu)
    tv = [Pu[d] - n[d] * s for d in range(3)]
    lt = _sqrt(_dot(tv, tv))
    if not _usable(lt):
        return [0.0, 1.0, 0.0], [1.0, -0.0, 0.0, 1.0], True
    T = [_div(x, lt) for x in tv]
    w = 1.0 if _dot(_cross(n, T), [-x for x in Pv]) >= 0.0 else -1.0
    f32 = lambda x: float(np.float32(x) + np.float32(0.0))
    return [f32(x) for x in n], [f32(x) for x in T] + [w], False


def _channel(x):
    v = math.floor((x * 127.5 + 127.5) + 0.5)
    return 0 if v < 0 else 255 if v > 255 else int(v)


def ref_texel(g, R, N, TW):
    """g float32 [3], R = 3x3 (float32 values) or None, N [3] / TW [4] = the float32 frame -> (rgba, bad: bool, back: bool)"""
    g = [float(x) for x in g]
    l = _sqrt(_dot(g, g)) if all(math.isfinite(x) for x in g) else math.nan
    if not _usable(l):
        return [128, 128, 255, 255], True, False
    g = [_div(x, l) for x in g]
    if R is not None:
        R = [[float(x) for x in r] for r in R]
        g = [(R[r][0] * g[0] + R[r][1] * g[1]) + R[r][2] * g[2] for r in range(3)]
        l = _sqrt(_dot(g, g))
        if not _usable(l):
            return [128, 128, 255, 255], True, False
        g = [_div(x, l) for x in g]
    if TW[1] == 0.0 and math.copysign(1.0, TW[1]) < 0.0:
        return [128, 128, 255, 255], False, False
    n = [g[0], g[2], g[1]]
    N, T, w = [float(x) for x in N], [float(x) for x in TW[:3]], float(TW[3])
    B = [w * x for x in _cross(N, T)]
    z = _dot(n, N)
    return [_channel(_dot(n, T)), _channel(_dot(n, B)), _channel(z), 255], False, z < 0.0


def reference(case):
    """strip()'s case -> (normals float32 [3 nt,3], tangents float32 [3 nt,4], image uint8 [H,W,4], counts) by ref_frame / ref_texel and the raster order of
    the layout, texel by texel"""
    nt, c, rot = case["nt"], case["c"], case["rot"]
    R = None if rot is None else np.asarray(rot, np.float32).reshape(-1, 4, 4)[0, :3, :3]
    N, TW, deg = np.zeros((3 * nt, 3), np.float32), np.zeros((3 * nt, 4), np.float32), 0
    for t in range(nt):
        n, tw, d = ref_frame(case["pos"][3 * t:3 * t + 3], case["uv"][3 * t:3 * t + 3])
        N[3 * t:3 * t + 3], TW[3 * t:3 * t + 3], deg = n, tw, deg + d
    L = mio.texture_layout(nt, c)
    image = np.empty((L["height"], L["width"], 4), np.uint8)
    image[:] = FLAT
    own, bad, back = owners(nt, c), 0, 0
    for s in range(L["texels"]):
        k, r = divmod(s, c * c)
        j, i = divmod(r, c)
        t = int(own[s])
        rgba, b0, b1 = ref_texel(case["grad"][s], R, N[3 * t], TW[3 * t])
        image[(k // L["grid"]) * c + j, (k % L["grid"]) * c + i] = rgba
        bad, back = bad + b0, back + b1
    return N, TW, image, {"degenerate": deg, "bad_gradient": bad, "back_facing": back}
