"""CPU: the host twin of the surface renderer (one-2-3-45_amd/surface.py), which DEFINES what the device computes (tests/test_gpu_surface.py compares the
device with it byte for byte).  Expected values are closed forms, facts of the definition or hand-computed numbers, never the twin's own output."""
import functools
import importlib

import numpy as np
import pytest

S = importlib.import_module("one-2-3-45_amd.surface")
synth = importlib.import_module("one-2-3-45_amd.synth")

CENTRE, RADIUS, R_SPHERE = np.array([0.1, -0.05, 0.08]), 0.5, 48


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    pos, target, up = (np.asarray(a, np.float64) for a in (pos, target, up))
    f = (target - pos) / np.linalg.norm(target - pos)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, np.cross(f, r), f, pos
    return c2w


def lattice(fn, R):
    ax = np.linspace(-1.0, 1.0, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    u = fn(x, y, z).astype(np.float32)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def sphere_lattice(R=R_SPHERE):
    return lattice(lambda x, y, z: np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2) - RADIUS, R)


@functools.lru_cache(maxsize=None)
def sphere_rays():
    K = np.array([[60.0, 0, 20.0], [0, 60.0, 20.0], [0, 0, 1.0]])
    o, d = S.camera_rays(K, look_at((1.9, 0.9, 0.7), CENTRE), 40, 40)
    o.setflags(write=False); d.setflags(write=False)
    return o, d


def same(a, b):
    """two trace results carry the same bytes (depth, kind, point)"""
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def counts_add_up(info):
    assert set(info) == set(S.INFO_KEYS) and all(type(v) is int for v in info.values())
    assert info["rays"] == info["hits"] + info["entry_hits"] + info["box_misses"] + info["misses"] + info["stalled"] + info["bad_rays"]


# ---- the sphere against its closed form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1.0, 2.0])
@pytest.mark.parametrize("refine", [4, 8, 16])
def test_sphere_hits_and_depths_against_the_closed_form(stride, refine):
    o32, d32 = sphere_rays()
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    oc = o - CENTRE
    a, b, c = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - RADIUS ** 2
    disc = b * b - a * c
    analytic = disc > 0
    t_true = (-b - np.sqrt(np.where(analytic, disc, 0.0))) / a
    depth, kind, point, info = S.trace_rays(sphere_lattice(), o32, d32, 0.0, 10.0, stride=stride, refine=refine)
    counts_add_up(info)
    assert analytic.sum() > 500 and np.array_equal(kind != 0, analytic) and info["hits"] == int(analytic.sum()) and info["entry_hits"] == 0
    # Trilinear interpolation of a C2 field errs by <= (h^2 / 8) sum_k |d2f/dx_k^2| <= (h^2 / 8) * 2 / r for a distance field at radius r >= rho - h;
    # along a ray with incidence cos >= 0.5 that moves the zero crossing by at most twice as much in t.
    h = 2.0 / (R_SPHERE - 1)
    bound = h * h / (2.0 * (RADIUS - h)) + 1e-6
    assert abs(bound - 1.98e-3) < 1e-5
    normal = (o + t_true[:, None] * d - CENTRE) / RADIUS
    cos = np.abs((normal * d).sum(1))
    sel = analytic & (cos >= 0.5)
    err = np.abs(depth.astype(np.float64) - t_true)[sel].max()
    print(f"stride {stride} refine {refine}: {int(analytic.sum())} hits, {int(sel.sum())} with cos >= 0.5, worst depth error {err:.3e} (bound {bound:.3e})")
    assert sel.sum() >= 0.7 * analytic.sum()
    assert err <= bound
    assert np.abs(point[sel].astype(np.float64) - (o + t_true[:, None] * d)[sel]).max() <= bound * 1.01
    assert not depth[kind == 0].any() and not point[kind == 0].any()


# ---- the empty-space skip is exact ---------------------------------------------------------------------------------------------------------------------
def _speck(R):
    u = np.full((R, R, R), 0.5, np.float32)
    u[R // 2, R // 3, R // 2 + 1] = -0.3
    return u


def _slab(R):
    return lattice(lambda x, y, z: np.abs(z - 0.07) - 0.06, R)           # 0.12 thick: under three cells at R = 48, a brick is eight


def _with_nans(R):
    u = np.array(sphere_lattice(R))
    u[R // 2 - 3, R // 2, R // 2] = np.nan
    u[5, 6, 7] = np.nan
    return u


def _corner_ball(R):
    """a ball in the low corner: at R = 10 and 17 (two bricks per axis, the last one partial at R = 10) it lies in brick (0, 0, 0) alone"""
    return lattice(lambda x, y, z: np.sqrt((x + 0.55) ** 2 + (y + 0.55) ** 2 + (z + 0.55) ** 2) - 0.3, R)


SKIP_CASES = {"sphere": lambda: sphere_lattice(), "nan nodes": lambda: _with_nans(R_SPHERE), "speck": lambda: _speck(33), "slab": lambda: _slab(48),
              "R=9": lambda: _corner_ball(9), "R=9 empty": lambda: np.full((9, 9, 9), 0.25, np.float32), "R=10": lambda: _corner_ball(10),
              "R=17": lambda: _corner_ball(17)}


@pytest.mark.parametrize("case", list(SKIP_CASES))
def test_skip_on_equals_skip_off(case):
    u = SKIP_CASES[case]()
    o, d = sphere_rays()
    stride = 0.25 if case == "speck" else 1.0                           # the speck's zero set is 0.078 across, one stride at R = 33 is 0.0625
    on = S.trace_rays(u, o, d, 0.0, 10.0, stride=stride, skip=True)
    off = S.trace_rays(u, o, d, 0.0, 10.0, stride=stride, skip=False)
    assert same(on, off)
    counts_add_up(on[3]); counts_add_up(off[3])
    assert {k: v for k, v in on[3].items() if k != "lookups"} == {k: v for k, v in off[3].items() if k != "lookups"}
    assert off[3]["lookups"] == off[3]["samples"]
    if case == "R=9":                                                    # ONE brick, and it holds the surface: nothing can be skipped
        assert on[3]["lookups"] == off[3]["lookups"] and S.brick_flags(u).tolist() == [[[1]]]
    else:
        assert on[3]["lookups"] < off[3]["lookups"]
    if case == "R=9 empty":                                              # one brick without a flag: not one lookup
        assert on[3]["lookups"] == 0 and on[3]["misses"] == on[3]["rays"] - on[3]["box_misses"] > 0
    else:
        assert on[3]["hits"] + on[3]["stalled"] > 0


def test_brick_flags_by_brute_force():
    for R in (2, 9, 10, 17, 24):
        u = np.array(sphere_lattice(R))
        if R > 9:
            u[R - 1, 0, R - 1] = np.nan                                  # a NaN node sets its bricks' flags
        g = u.astype(np.float64)
        nb = (R - 1 + 7) // 8
        want = np.zeros((nb, nb, nb), np.uint8)
        for bx in range(nb):
            for by in range(nb):
                for bz in range(nb):
                    for x in range(8 * bx, min(8 * bx + 8, R - 1) + 1):
                        for y in range(8 * by, min(8 * by + 8, R - 1) + 1):
                            for z in range(8 * bz, min(8 * bz + 8, R - 1) + 1):
                                if not g[x, y, z] > 0:
                                    want[bx, by, bz] = 1
        got = S.brick_flags(u)
        assert got.dtype == np.uint8 and np.array_equal(got, want), R
        assert np.array_equal(S.brick_flags(-u, inside_positive=True), want)
    assert S.brick_flags(sphere_lattice(24), level=10.0).all() and not S.brick_flags(sphere_lattice(24), level=10.0, inside_positive=True).any()


# ---- classification, one case each ---------------------------------------------------------------------------------------------------------------------
def _one(o, d):
    return np.array([o], np.float32), np.array([d], np.float32)


def _only(info, key):
    counts_add_up(info)
    assert info[key] == 1 and info["rays"] == 1, info


def test_axis_parallel_ray_inside_the_slab_hits():
    depth, kind, point, info = S.trace_rays(sphere_lattice(), *_one((0.1, -0.05, -3.0), (0, 0, 1)), 0.0, 10.0)
    _only(info, "hits")
    assert kind[0] == 1 and abs(depth[0] - (3.0 + 0.08 - 0.5)) < 2e-3 and abs(point[0, 2] - (0.08 - 0.5)) < 2e-3 and point[0, 0] == np.float32(0.1)


def test_axis_parallel_ray_outside_the_slab_misses_the_box():
    for o in ((1.5, 0.0, -3.0), (0.0, -1.0000001, -3.0)):
        depth, kind, point, info = S.trace_rays(sphere_lattice(), *_one(o, (0, 0, 1)), 0.0, 10.0)
        _only(info, "box_misses")
        assert kind[0] == 0 and depth[0] == 0 and info["samples"] == 0
    # on the face itself the axis constrains nothing
    _only(S.trace_rays(sphere_lattice(), *_one((1.0, 0.0, -3.0), (0, 0, 1)), 0.0, 10.0)[3], "misses")


def test_ray_that_starts_inside_the_surface_is_an_entry_hit():
    depth, kind, point, info = S.trace_rays(sphere_lattice(), *_one(CENTRE, (0, 0, 1)), 0.0, 10.0)
    _only(info, "entry_hits")
    assert kind[0] == 2 and depth[0] == 0 and point[0].tobytes() == CENTRE.astype(np.float32).tobytes() and info["samples"] == 1
    depth, kind, _, info = S.trace_rays(sphere_lattice(), *_one(CENTRE - (0, 0, 3), (0, 0, 1)), 3.0 - 0.1, 10.0)          # near puts t0 inside
    _only(info, "entry_hits")
    assert depth[0] == np.float32(3.0 - 0.1)


def test_ray_through_a_nan_node_is_stalled():
    u = np.full((24, 24, 24), 0.5, np.float32)
    u[12, 12, 12] = np.nan
    ax = np.linspace(-1.0, 1.0, 24)
    for skip in (True, False):
        depth, kind, point, info = S.trace_rays(u, *_one((ax[12], ax[12], -3.0), (0, 0, 1)), 0.0, 10.0, skip=skip)
        _only(info, "stalled")
        assert kind[0] == 0 and depth[0] == 0 and not point.any()
    _only(S.trace_rays(u, *_one((ax[3], ax[3], -3.0), (0, 0, 1)), 0.0, 10.0)[3], "misses")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_ray_is_a_bad_ray(bad):
    for which in (0, 1):
        for k in range(3):
            od = [[0.1, -0.05, -3.0], [0.0, 0.0, 1.0]]
            od[which][k] = bad
            depth, kind, point, info = S.trace_rays(sphere_lattice(), *_one(*od), 0.0, 10.0)
            _only(info, "bad_rays")
            assert kind[0] == 0 and depth[0] == 0 and not point.any() and info["samples"] == 0 and info["lookups"] == 0


def test_a_ray_with_too_many_steps_is_a_bad_ray():
    _only(S.trace_rays(sphere_lattice(), *_one((0.1, -0.05, -3.0), (0, 0, 1e-6)), 0.0, 1e9)[3], "bad_rays")


def test_near_above_far_misses():
    o, d = sphere_rays()
    depth, kind, _, info = S.trace_rays(sphere_lattice(), o, d, 5.0, 1.0)
    counts_add_up(info)
    assert info["box_misses"] == o.shape[0] and not kind.any() and info["samples"] == 0


def test_refine_zero_is_the_secant_of_the_first_bracket():
    ax = np.linspace(-1.0, 1.0, R_SPHERE)
    i, j = 26, 22
    u = sphere_lattice()
    depth, kind, _, info = S.trace_rays(u, *_one((ax[i], ax[j], -2.0), (0, 0, 1)), 0.0, 10.0, refine=0)
    _only(info, "hits")
    line = u[i, j].astype(np.float64)
    k = int(np.flatnonzero(~(line > 0))[0])
    z = (k - 1) + line[k - 1] / (line[k - 1] - line[k])                 # along a lattice line the trilinear value is linear between two nodes
    assert abs(depth[0] - (2.0 + (z / (R_SPHERE - 1) * 2.0 - 1.0))) < 1e-6
    assert info["samples"] >= info["lookups"] > 0


def test_inside_positive_on_the_negated_lattice_gives_the_same_bytes():
    o, d = sphere_rays()
    for u in (sphere_lattice(), _with_nans(R_SPHERE)):
        a = S.trace_rays(u, o, d, 0.0, 10.0, level=0.02)
        b = S.trace_rays(-u, o, d, 0.0, 10.0, level=-0.02, inside_positive=True)
        assert same(a, b) and a[3] == b[3]


def test_arguments_are_checked():
    o, d = sphere_rays()
    u = sphere_lattice()
    for kw in (dict(stride=0.0), dict(stride=8.5), dict(stride=float("nan")), dict(refine=-1), dict(refine=33), dict(refine=1.5), dict(level=float("inf")),
               dict(bound_min=(1.0, -1.0, -1.0)), dict(bound_max=(1.0, float("nan"), 1.0))):
        with pytest.raises(ValueError):
            S.trace_rays(u, o, d, 0.0, 10.0, **kw)
    for args in ((u.astype(np.float64), o, d, 0.0, 10.0), (u[:, :, :5], o, d, 0.0, 10.0), (u[:1, :1, :1], o, d, 0.0, 10.0), (u, o.astype(np.float64), d, 0.0, 10.0),
                 (u, o[:5], d, 0.0, 10.0), (u, o, d, float("nan"), 10.0), (u, o, d, 0.0, float("inf"))):
        with pytest.raises(ValueError):
            S.trace_rays(*args)


def test_no_rays():
    z = np.zeros((0, 3), np.float32)
    depth, kind, point, info = S.trace_rays(sphere_lattice(), z, z, 0.0, 10.0)
    assert depth.shape == (0,) and kind.shape == (0,) and point.shape == (0, 3) and not any(info.values())


def test_other_bounds_scale_the_scene():
    """the same lattice over a box of twice the size, rays scaled with it: twice the depth"""
    o, d = sphere_rays()
    a = S.trace_rays(sphere_lattice(), o, d, 0.0, 10.0)
    b = S.trace_rays(sphere_lattice(), o * 2, d, 0.0, 20.0, bound_min=(-2, -2, -2), bound_max=(2, 2, 2))
    assert np.array_equal(a[1], b[1]) and a[3] == b[3] and np.abs(b[0] - 2 * a[0]).max() < 1e-5


# ---- rays, orbit, packer ----------------------------------------------------------------------------------------------------------------------------------
def test_camera_rays_agree_with_gen_rays():
    sc = synth.make_scene(n_views=8, hw=(32, 48))
    K, c2w = sc["query_intrinsic"], sc["query_c2w"]
    o, d = S.camera_rays(K, c2w, 32, 48)
    wo, wd = synth.gen_rays(K, c2w, 32, 48)
    assert o.dtype == d.dtype == np.float32 and o.shape == d.shape == (32 * 48, 3)
    assert o.tobytes() == wo.tobytes()
    assert np.abs(d.astype(np.float64) - wd).max() <= 1e-6                # gen_rays multiplies in float32: about ten float32 operations at O(1)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    # pixel (cx, cy) looks along the camera's z axis; raster order
    K2 = np.array([[50.0, 0, 7.0], [0, 40.0, 3.0], [0, 0, 1.0]], np.float32)
    o, d = S.camera_rays(K2, c2w, 9, 11)
    assert d[3 * 11 + 7].tobytes() == c2w[:3, 2].astype(np.float32).tobytes()
    v = np.array([(8 - 7.0) / 50.0, (5 - 3.0) / 40.0, 1.0])
    assert np.abs(d[5 * 11 + 8] - c2w[:3, :3].astype(np.float64) @ (v / np.linalg.norm(v))).max() < 1e-6


def test_camera_rays_refuse_what_is_not_a_pinhole_without_skew():
    c2w = np.eye(4, dtype=np.float32)
    good = np.array([[50.0, 0, 7.0], [0, 40.0, 3.0], [0, 0, 1.0]])
    for (r, c), v in (((0, 1), 0.1), ((1, 0), 0.1), ((2, 0), 0.1), ((2, 1), 1.0), ((2, 2), 2.0), ((0, 0), 0.0), ((1, 1), 0.0), ((0, 2), np.nan)):
        K = good.copy()
        K[r, c] = v
        with pytest.raises(ValueError):
            S.camera_rays(K, c2w, 4, 4)
    for args in ((good, c2w[:2], 4, 4), (good[:2], c2w, 4, 4), (good, c2w, 0, 4)):
        with pytest.raises(ValueError):
            S.camera_rays(*args)


@pytest.mark.parametrize("up", [(0.0, 0.0, 1.0), (0.0, -1.0, 0.0), (0.3, -0.5, 0.8)])
def test_orbit_frames_are_orthonormal_and_look_at_the_origin(up):
    n, elev, radius = 7, 25.0, 1.7
    c = S.orbit_c2w(n, elev, radius, up)
    assert c.dtype == np.float32 and c.shape == (n, 4, 4)
    upn = np.asarray(up) / np.linalg.norm(up)
    c = c.astype(np.float64)
    for i in range(n):
        Rm, pos = c[i, :3, :3], c[i, :3, 3]
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(Rm) - 1) < 1e-6
        assert abs(np.linalg.norm(pos) - radius) < 1e-6 and np.abs(pos / radius + Rm[:, 2]).max() < 1e-6          # z axis: from the camera to the origin
        assert abs(np.degrees(np.arcsin(pos @ upn / radius)) - elev) < 1e-4
        assert Rm[:, 1] @ upn < 0 and abs(Rm[:, 0] @ upn) < 1e-6                                                    # y down, x level
        assert np.array_equal(c[i, 3], [0, 0, 0, 1])
    e0 = c[0, :3, 3] - (c[0, :3, 3] @ upn) * upn
    e0 /= np.linalg.norm(e0)
    e1 = np.cross(upn, e0)
    az = np.unwrap(np.arctan2(c[:, :3, 3] @ e1, c[:, :3, 3] @ e0))
    assert np.abs(np.diff(az) - 2 * np.pi / n).max() < 1e-5                                                      # equal steps, one sense
    for bad in (dict(n_views=0), dict(n_views=3, elevation_deg=90.0), dict(n_views=3, radius=0.0)):
        with pytest.raises(ValueError):
            S.orbit_c2w(**bad)


def test_packer_quantisation_and_background_by_hand():
    kind = np.array([1, 0, 2, 1, 0, 1], np.uint8)
    depth = np.array([1.5, 9.0, 0.25, 2.0, 9.0, 3.0], np.float32)
    rgb = np.array([[0.0, 0.5, 1.0], [9, 9, 9], [0.999, 1 / 255, 0.2], [0.25, 0.75, 0.1], [9, 9, 9], [0.5, 0.5, 0.5]], np.float32)
    grad = np.array([[0, 0, 2.0], [9, 9, 9], [-3.0, 0, 0], [0, 0, 0], [9, 9, 9], [1.0, 1.0, 1.0]], np.float32)
    color, normal, d = S.pack_images(kind, depth, rgb, grad, 2, 3, background=(10, 20, 30, 40))
    assert color.dtype == normal.dtype == np.uint8 and d.dtype == np.float32 and color.shape == normal.shape == (2, 3, 4) and d.shape == (2, 3)
    # truncation of c * 255 in float32: 0.5 -> 127.5 -> 127, 0.999 -> 254.7 -> 254, 1 / 255 -> 1 (float32(1 / 255) * 255 == 1), 0.2 -> 51 (51.000004)
    assert color.reshape(6, 4).tolist() == [[0, 127, 255, 255], [10, 20, 30, 40], [254, 1, 51, 255], [63, 191, 25, 255], [10, 20, 30, 40], [127, 127, 127, 255]]
    # n 0.5 + 0.5: (0, 0, 1) -> 127, 127, 255; (-1, 0, 0) -> 0, 127, 127; a zero gradient -> n = 0 -> 127; (1, 1, 1) / sqrt 3 -> 0.7887 -> 201
    assert normal.reshape(6, 4).tolist() == [[127, 127, 255, 255], [0, 0, 0, 0], [0, 127, 127, 255], [127, 127, 127, 255], [0, 0, 0, 0], [201, 201, 201, 255]]
    assert d.reshape(6).tolist() == [1.5, 0.0, 0.25, 2.0, 0.0, 3.0]
    assert S.pack_images(kind, depth, rgb, grad, 3, 2)[0][0, 1].tolist() == [0, 0, 0, 0]
    for bad in ((1, 2, 3), (0, 0, 0, 256), (0, 0, 0, -1), (0.5, 0, 0, 0)):
        with pytest.raises(ValueError):
            S.pack_images(kind, depth, rgb, grad, 2, 3, background=bad)
    with pytest.raises(ValueError):
        S.pack_images(kind, depth, rgb, grad, 2, 2)


# ---- configuration and the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_ranges():
    config = importlib.import_module("one-2-3-45_amd.config")
    assert (config.SURFACE_STRIDE, config.SURFACE_REFINE, config.PREVIEW_VIEWS) == (1.0, 8, 0)      # the environment of the test run leaves them unset
    assert config.surface_stride() == 1.0 and config.surface_stride(0.5) == 0.5 and config.surface_stride(8) == 8.0
    assert config.surface_refine() == 8 and config.surface_refine(0) == 0 and config.surface_refine(32) == 32
    assert config.preview_views() == 0 and config.preview_views(3) == 3 and config.preview_views(0) == 0
    for fn, bad in ((config.surface_stride, (0.0, -1.0, 8.5, float("nan"), float("inf"))), (config.surface_refine, (-1, 33, 1.5, True)),
                    (config.preview_views, (-1, 1.5, True))):
        for x in bad:
            with pytest.raises(ValueError):
                fn(x)
    assert S.march_params() == (1.0, 8) and S.march_params(2, 0) == (2.0, 0)


def test_cabi_declares_the_surface_entries():
    L = importlib.import_module("one-2-3-45_amd._lib")
    protos = L.parse_header()
    for name in ("o2345_surface_bricks", "o2345_surface_trace_workspace_bytes", "o2345_surface_trace", "o2345_camera_rays", "o2345_surface_pack"):
        assert name in protos, name
    assert L.ABI_VERSION == 231 and len(protos["o2345_surface_trace"][1]) == 23
    build = importlib.import_module("one-2-3-45_amd.build")
    assert "surface_trace.hip" in build.SOURCES and "surface_trace.hip" not in build.EXTRA_FLAGS                # no extra flags
