"""The gate of tests/test_gpu_many_views.py, on the CPU and from the float64 references alone: the inputs of the view-count tests do reach the branches
they were built for.  The kernels fork on the view count V at 32 (the list sort and its 32-bit signature), at 64 (the wave-uniform view skip of
k_color_pts and its 64-bit mask of active views), at 255 (counts are uint8), at V mod 4 (the quad walk of costvol_row_quad16) and at multiples of 64
(the blocks of k_camera_terms); synth.make_scene's rig has 32 source views and cannot give more, so the scenes come from project_ref.sphere_scene.

  cameras    V pairwise different projection matrices and centres, all above the volume
  points     project_ref.sphere_points: a 32-point tile some views see and others do not (every point by at least one view, so that the network pass
             skips; a view that sees none of it, a view from 32 on that sees some of it), a tile no view sees, a tile every view sees -- the count
             V, 255 included, is reached and so is 0; no point lies in the border band
  voxels     the cost volume's counts reach V; the kept sets at min_views = 1, V - 2 and V - 1 differ, and the last keeps exactly the voxels every view sees
  masks      trained_weights.many_view_mask: each kind is what its name says, at every V and P of the GPU test
  the rig    synth.make_scene raises above 32 views and returns, for 4, 8, 19 and 32 views, the bytes it returned before it did"""
import hashlib
import importlib

import numpy as np
import pytest
import torch

import project_ref as R
import trained_weights as TW

synth = importlib.import_module("one-2-3-45_amd.synth")
F64 = torch.float64
H, W = R.SPHERE_HW
POINT_D, COST_D = 13, 11

# sha256 over the sorted (key, dtype, shape, bytes) of make_scene(V)'s dict, taken at the commit before the view-count check was added
RIG_SHA256 = {4: "00334d2247c94c2ca428f884b31de83edb37c52ecf8255761983a22034649ce8", 8: "b197c22c081c27062a68688407e292a7558c35f7740bf5bade8c867faf0c6be3",
              19: "4b2bbecf31123e402474365ae2c260aa30211169ce92b142667e840d1febfc0d", 32: "76133fc70e596014043de74b717389c8bff4712992d0dc1837a5649f94a8ec29"}


def scene_sha256(sc):
    h = hashlib.sha256()
    for k in sorted(sc):
        a = np.ascontiguousarray(np.asarray(sc[k]))
        for part in (k.encode(), str(a.dtype).encode(), str(a.shape).encode(), a.tobytes()):
            h.update(part)
    return h.hexdigest()


@pytest.mark.parametrize("V", sorted(RIG_SHA256))
def test_the_rig_returns_the_same_bytes(V):
    assert scene_sha256(synth.make_scene(V)) == RIG_SHA256[V]


@pytest.mark.parametrize("V", [33, 40, 64, 255])
def test_the_rig_refuses_more_than_32_views(V):
    with pytest.raises(ValueError, match="32 source views"):
        synth.make_scene(V)


@pytest.mark.parametrize("V", R.MANY_VIEWS)
def test_cameras_are_distinct(V):
    s = R.sphere_scene(H, W, V, POINT_D)
    assert tuple(s["proj"].shape) == (V, 3, 4) and tuple(s["aff"].shape) == (V, 4, 4) and tuple(s["cam_pos"].shape) == (V, 3) and H != W
    for name in ("proj", "cam_pos"):
        rows = s[name].reshape(V, -1).double()
        d = (rows[:, None] - rows[None]).abs().amax(-1) + torch.eye(V)
        assert float(d.min()) > 1e-3, f"{name}: two views closer than 1e-3 ({float(d.min()):.2e})"
    assert torch.equal(s["aff"][:, :3], s["proj"]) and bool((s["cam_pos"][:, 2] > 0).all())
    centre = torch.inverse(s["w2cs"].double())[:, :3, 3]
    assert float((centre - s["cam_pos"].double()).abs().max()) < 1e-6 and float((centre.norm(dim=1) - R.SPHERE_RADIUS).abs().max()) < 1e-6
    assert float((s["proj"].double() - s["K"].double() @ s["w2cs"].double()[:, :3]).abs().max()) < 1e-5      # K and w2cs are rounded on their own


@pytest.mark.parametrize("V", R.MANY_VIEWS)
def test_point_families_reach_their_tiles(V):
    s = R.sphere_scene(H, W, V, POINT_D)
    pts, nv, mask = R.sphere_points(H, W, V, POINT_D)
    assert tuple(pts.shape) == (257, 3) and not R.ambiguous_points(s, pts)[0].any()
    ref = R.project_features(s, pts, F64, query_cam=s["query_cam"])
    assert torch.equal(ref["nviews"], nv) and torch.equal(ref["mask"], mask)
    tile = lambda name: slice(32 * R.SPHERE_TILES[name], 32 * R.SPHERE_TILES[name] + 32)
    part = mask[:, tile("partial")]
    assert bool(((nv[tile("partial")] >= 1) & (nv[tile("partial")] < V)).all())
    seen_by = part.any(1)
    assert 0 < int(seen_by.sum()) < V, "no view sees none of the partly seen tile"
    assert bool(seen_by[32:].any()), "no view from 32 on sees the partly seen tile: the upper half of the active mask stays empty"
    assert bool((part.any(1) & ~part.all(1)).any()), "the tile's points agree about every view"
    assert not nv[tile("none")].any() and bool(ref["gmask"][tile("none")].all()) and not ref["pmask"][:, tile("none")].any()
    assert bool((nv[tile("all")] == V).all()) and int(nv.max()) == V and V <= 255
    print(f"V = {V}: partly seen tile: {int(seen_by.sum())} of {V} views see some of it, its points are seen by {int(nv[tile('partial')].min())} to "
          f"{int(nv[tile('partial')].max())}; counts of the 257 points: {int((nv == 0).sum())} zero, {int((nv == V).sum())} full")


@pytest.mark.parametrize("V", R.MANY_VIEWS)
def test_cost_volume_counts_reach_every_threshold(V):
    s = R.sphere_scene(H, W, V, COST_D)
    c = R.costvol(s["f16"], s["aff"], s["dims"], s["voxel_size"], s["origin"], F64, min_views=1)
    amb = R.ambiguous_pairs(c["pairs"], R.Z_CLAMP_VOXEL).any(1)
    cnt = c["cnt"][~amb]
    assert int(cnt.max()) == V and int((cnt == V).sum()) >= 8
    kept = [int((cnt > mv).sum()) for mv in (1, V - 2, V - 1)]
    assert kept[0] > kept[1] > kept[2] == int((cnt == V).sum()), kept
    assert int((cnt <= 1).sum()) > 0, "min_views = 1 drops nothing"
    print(f"V = {V} (V mod 4 = {V % 4}): {int(amb.sum())} ambiguous voxels of {COST_D ** 3}; kept at min_views 1, V - 2, V - 1: {kept}")


def test_every_quad_tail_occurs():
    assert {V % 4 for V in R.MANY_VIEWS} == {0, 1, 2, 3}


@pytest.mark.parametrize("V,P", TW.MANY_CASES)
def test_masks_are_what_their_names_say(V, P):
    base = TW.color_inputs(V, P)["mask"]
    n = min(P, 32)
    m = TW.many_view_mask(V, P, "tile_hidden")
    assert not m[32:, :n].any() and bool(m[:32, :n].any(0).all()) and torch.equal(m[:, n:], base[:, n:])
    assert bool((~m[:, :n].any(1))[[32, V - 1]].all()) and (V != 64 or not m[63, :n].any())
    b = TW.many_view_mask(V, P, "tile_hidden_one_blind")
    blind = min(TW.BLIND_POINT, P - 1)
    assert not b[:, blind].any() and torch.equal(b[:, [i for i in range(P) if i != blind]], m[:, [i for i in range(P) if i != blind]])
    assert bool(TW.many_view_mask(V, P, "all_views").all())
    o = TW.many_view_mask(V, P, "one_view")
    assert bool((o.sum(0) == 1).all()) and bool(o[V - 1, 0]) and len(set(o.long().argmax(0).tolist())) == min(P, V)
    # none of them is a mask the random draw gives
    for kind in TW.MASK_KINDS:
        assert not torch.equal(TW.many_view_mask(V, P, kind), base)
    c = TW.many_view_case(V, P, "all_views")
    assert bool((c["nviews"] == V).all()) and bool(torch.isfinite(c["r64"]).all())
