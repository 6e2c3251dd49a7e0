"""The invariant o2345_render_rays rests on when it leaves the SDF of the LAST up-sampling round's samples unevaluated (csrc/render.hip): whatever SDF
the last merged block carries, cat_z_vals' merged depths and every output of render_core's head are the same -- the merge sorts by depth alone, and
finalize takes the depths alone (the reference deletes the SDF its last cat_z_vals returns unread, sparse_neus_renderer.py:540-547).  Shown on the
float64 / float32 references of tests/sampler_ref.py with the block's SDF replaced by NaN, on the merge cases the GPU tests use."""
import pytest
import torch

import sampler_ref as SR


@pytest.mark.parametrize("dtype", [SR.F64, SR.F32])
@pytest.mark.parametrize("R,S,n_new", SR.MERGE_CASES)
def test_nan_sdf_in_the_last_merged_block_changes_nothing_downstream(R, S, n_new, dtype):
    d = SR.merge_inputs(R, S, n_new)
    o, dd = SR.rays(R, R * 11 + S)
    z, sdf, new_z, new_sdf = (d[k].to(dtype) for k in ("z", "sdf", "new_z", "new_sdf"))
    zz, ss = SR.merge(z, sdf, new_z, new_sdf)
    zn, sn = SR.merge(z, sdf, new_z, torch.full_like(new_sdf, float("nan")))
    assert torch.equal(zz, zn) and torch.isfinite(zn).all()
    # the NaNs went where the new samples went and nowhere else: the only trace of the block's SDF is in the merged SDF list, which nothing reads
    lost = torch.isnan(sn)
    assert bool((lost.sum(1) == n_new).all()) and torch.equal(lost, ss < 0) and torch.equal(sn[~lost], ss[~lost])
    mask = SR.synthetic_mask()
    sample_dist = (SR.FAR - SR.NEAR) / 64
    want = SR.finalize(o, dd, zz, sample_dist, mask, dtype=dtype)
    got = SR.finalize(o, dd, zn, sample_dist, mask, dtype=dtype)
    assert set(got) == {"dists", "mid_z", "pts", "pm"}
    for k, v in want.items():
        assert torch.equal(got[k], v) and torch.isfinite(got[k]).all(), k
