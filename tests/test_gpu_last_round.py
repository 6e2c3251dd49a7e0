"""GPU: the last up-sampling round of a render call (csrc/render.hip, o2345_render_rays).

The samples of round 3 are merged by the finalize round, which reads their DEPTHS only, and render_core evaluates the SDF again at the mid points -- as
in the reference, which deletes the SDF its last cat_z_vals returns unread (sparse_neus_renderer.py:540-547).  o2345_render_rays therefore does not
evaluate the SDF of round 3's samples: they keep cat_z_vals' default 100, which the finalize round's merge either does not read (16 samples per round:
the fused merge) or carries into a list that nobody reads (any other block size: k_ray_merge_any), and the "more than one point" rule that would have
emptied round 3's list has nothing left to decide.

What is pinned here, on the small scene with 16 coarse samples:
  1. no output depends on what the render workspace held before the call (filled with 0x00 and with 0xFF bytes: equal bit for bit, no NaN);
  2. render_rays == the stage path that still evaluates all four rounds (ray_coarse, sdf_mlp, 4 x (ray_upsample, sdf_mlp, ray_merge), render_core), bit
     for bit -- also under a mask with ONE occupied voxel, where round 3 has at most one sample inside the mask (the rule that is no longer applied
     to it would have fired);
  3. segment mode: 192 rays as three segments == three 64-ray calls, one segment with at most one sample inside the mask per round.
Shapes: 96 rays (sixteen-lane kernels, a partial wave) and 320 rays with O2345_RAY_STREAM_MIN = 64 (streaming kernels, a partial second block);
n_importance = 64 (16 per round: the fused merge) and 4 (one per round: k_ray_merge_any)."""
import functools

import numpy as np
import pytest
import torch

import sampler_ref as SR
from oracle import recon as O
from scene_util import rays_for, sdfW_t, small_scene
from test_gpu_parity import dev, dev_scene, ops  # noqa: F401  (fixtures)
from test_gpu_segments import _compare

pytestmark = pytest.mark.gpu

NS = 16
SHAPES = [(96, None), (320, "64")]                  # (rays, O2345_RAY_STREAM_MIN or the default 4096)
SCENE_KEYS = ("sdf_blob", "color_mfma_blob", "color_x3_blob", "vol_cl", "maskvol", "cmaps", "proj", "cam_pos")


def _use(lib_instance, stream_min):
    if stream_min is not None:
        assert ("ray_stream_min=" + stream_min).encode() in lib_instance({"O2345_RAY_STREAM_MIN": stream_min}).o2345_knobs()


@functools.lru_cache(maxsize=None)
def _one_voxel():
    """-> (mask [D,D,D] with ONE occupied voxel inside the surface, origin and direction of a ray through it, of a ray that misses the volume):
    tests/test_gpu_segments.py's construction"""
    s = small_scene()
    D = s["D"]
    c = (2 * torch.arange(D) + 1) / D - 1                                     # voxel centres of the nearest-mask lookup
    ctr = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    inside = torch.nonzero(O.sdf(ctr, s["dense"][0], sdfW_t(s["sdfW"]))[0][:, 0].reshape(D, D, D) < -0.05)
    ix, iy, iz = (int(v) for v in inside[inside.shape[0] // 3])
    mask = torch.zeros(D, D, D)
    mask[ix, iy, iz] = 1
    cross_o = torch.tensor([float(c[ix]) - 1.0 + 0.02, float(c[iy]), float(c[iz])])
    miss_d = torch.nn.functional.normalize(torch.tensor([1.0, 0.2, 0.1]), dim=0)
    return mask, cross_o, torch.tensor([1.0, 0.0, 0.0]), torch.tensor([5.0, 5.0, 5.0]), miss_d


def _one_voxel_rays(R, crossing):
    """R rays that miss the volume, the rays listed in ``crossing`` replaced by the ray through the occupied voxel"""
    _, co, cd, mo, md = _one_voxel()
    o, d = mo[None].repeat(R, 1), md[None].repeat(R, 1)
    o[crossing] = co
    d[crossing] = cd
    return o.contiguous(), d.contiguous()


def _setup(dev, ops, R, mask_kind):
    """-> (scene dict, rays_o, rays_d on the device, near, far, query camera)"""
    s = small_scene()
    d = dev_scene(s, dev, ops)
    scene = {k: d[k] for k in SCENE_KEYS}
    qcam = torch.from_numpy(s["sc"]["query_c2w"][:3, 3].copy()).to(dev)
    if mask_kind == "scene":
        ro, rd = (torch.from_numpy(a) for a in rays_for(s, R, seed=R, center=True))
        near, far = (float(v) for v in s["sc"]["query_near_far"][:2])
    else:
        scene["maskvol"] = _one_voxel()[0].reshape(-1).contiguous().to(dev)
        ro, rd = _one_voxel_rays(R, [R // 2])
        near, far = 0.1, 2.0
    return scene, ro.to(dev), rd.to(dev), near, far, qcam


@pytest.mark.parametrize("ni", [64, 4])
@pytest.mark.parametrize("R,stream_min", SHAPES)
def test_no_output_depends_on_stale_workspace(dev, ops, lib_instance, R, stream_min, ni):
    _use(lib_instance, stream_min)
    scene, ro, rd, near, far, qcam = _setup(dev, ops, R, "scene")
    outs = []
    for fill in (0x00, 0xFF):
        ws, nbytes = ops._scratch("o2345_render_workspace_bytes", (R, NS, ni, scene["cmaps"].shape[0]), dev, "render")
        assert ws.numel() >= nbytes
        ws.fill_(fill)
        outs.append(ops.render_rays(scene, ro, rd, near, far, NS, ni, 7.4, 1.0, 1.0, qcam, want_z=True, want_scalars=True))
    assert "z_vals" in outs[0] and "scalars" in outs[0]
    for k, v in outs[0].items():
        assert torch.equal(v, outs[1][k]), k
        if v.is_floating_point():
            assert not bool(torch.isnan(v).any()), k
    assert float(outs[0]["weights_sum"].max()) > 0.5


def _stage_path(ops, scene, ro, rd, near, far, ni, sample_dist, inv_s, qcam):
    """the render call from the public stage entries, the SDF of ALL four rounds' new samples evaluated and merged.
    -> (render_core's dict, the new samples of round 3 inside the mask)"""
    D = scene["vol_cl"].shape[0]
    R, NI = ro.shape[0], ni // 4
    maskvol = scene["maskvol"].reshape(-1)
    z, pts = ops.ray_coarse(ro, rd, near, far, NS)
    sdf = ops.sdf_mlp(scene["sdf_blob"], scene["vol_cl"], pts.view(-1, 3), variant=0)["sdf"].view(NS, R)
    for i in range(4):
        new_z, new_pts, lst = ops.ray_upsample(ro, rd, z, sdf, 64.0 * 2 ** i, maskvol, D, NI)
        new_sdf = torch.full((NI * R,), 100.0, device=z.device)              # cat_z_vals' default (:135); the list is empty when <= 1 sample is inside (:137)
        if lst.numel():
            ops.sdf_mlp(scene["sdf_blob"], scene["vol_cl"], new_pts.view(-1, 3), variant=0, index=lst.contiguous(), out={"sdf": new_sdf})
        z, sdf = ops.ray_merge(z, sdf, new_z, new_sdf.view(NI, R))
    inside = int((SR.occupancy(maskvol.view(D, D, D).cpu(), new_pts.cpu()) > 0).sum())
    return ops.render_core(scene, ro, rd, z, sample_dist, inv_s, 1.0, 1.0, qcam), inside


@pytest.mark.parametrize("mask_kind", ["scene", "one_voxel"])
@pytest.mark.parametrize("ni", [64, 4])
@pytest.mark.parametrize("R,stream_min", SHAPES)
def test_render_rays_equals_the_stage_path_with_four_evaluated_rounds(dev, ops, lib_instance, R, stream_min, ni, mask_kind):
    _use(lib_instance, stream_min)
    scene, ro, rd, near, far, qcam = _setup(dev, ops, R, mask_kind)
    inv_s = float(np.exp(2.0))
    sample_dist = float(np.float32(far - near) / np.float32(NS))
    got = ops.render_rays(scene, ro, rd, near, far, NS, ni, inv_s, 1.0, 1.0, qcam, want_z=True, sample_dist=sample_dist, weight_cull=0.0)
    want, inside = _stage_path(ops, scene, ro, rd, near, far, ni, sample_dist, inv_s, qcam)
    print(f"R={R} n_importance={ni} mask={mask_kind}: {inside} samples of round 3 inside the mask, {int((got['pm'] > 0).sum())} occupied mid points")
    if mask_kind == "one_voxel":
        assert inside <= 1, "round 3 must have at most one sample inside the mask"
        crossing = float(got["pm"][:, R // 2].sum())                         # only that ray can have occupied mid points; 80 samples are dense enough to have some
        assert float(got["pm"].sum()) == crossing and (crossing >= 1 or ni != 64)
    else:
        assert inside > 1 and float(got["weights_sum"].max()) > 0.5          # the rule does not fire: the stage path does evaluate round 3's samples
    for k in ("z_vals", "mid_z", "dists", "pm", "sdf", "grad", "weights", "color", "depth"):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("stream_min", [None, "64"])
def test_segments_equal_separate_calls_without_the_last_evaluation(dev, ops, lib_instance, stream_min):
    """192 rays as three 64-ray segments: one crossing ray (at most one sample inside the mask per round: cat_z_vals' rule fires in every round, round 3
    included), 64 crossing rays (it never fires), none.  Every output and the per-segment scalars equal the separate calls bit for bit."""
    _use(lib_instance, stream_min)
    G = 64
    scene, _, _, near, far, qcam = _setup(dev, ops, G, "one_voxel")
    segs = [_one_voxel_rays(G, [5]), _one_voxel_rays(G, list(range(G))), _one_voxel_rays(G, [])]
    ro = torch.cat([o for o, _ in segs]).contiguous().to(dev)
    rd = torch.cat([d for _, d in segs]).contiguous().to(dev)
    whole, parts = _compare(ops, scene, ro, rd, near, far, NS, 64, float(np.exp(2.0)), qcam, G, label=str(stream_min))
    # the lone crossing ray's samples differ from the crowd's (its new samples kept sdf = 100 in rounds 0 - 2), and the empty segment evaluated 100 points
    assert float((whole["z_vals"][:, 5] - whole["z_vals"][:, G]).abs().max()) > 1e-3
    assert float(parts[2]["pm"].sum()) == 0 and float(parts[2]["scalars"][3]) == 100.0
    want, inside = _stage_path(ops, scene, ro[:G].contiguous(), rd[:G].contiguous(), near, far, 64, float(np.float32(far - near) / np.float32(NS)),
                               float(np.exp(2.0)), qcam)
    assert inside <= 1, "the first segment must have at most one sample of round 3 inside the mask"
    assert torch.equal(want["z_vals"], whole["z_vals"][:, :G])
