"""CPU test: the register budget of the six SDF-network kernels, read from the compiler's resource-usage remarks at the product flags.

Every one of them runs 512-thread workgroups at two waves per SIMD, which leaves 256 registers per lane.  The split-f16 gradient kernel sits just below
that line: above it, it spills (224 bytes of scratch per lane, 9.9 -> 11.9 ms on 29.5 M points; csrc/sdf_common.h, MIXLO).  Only the exact fp32 gradient
kernel is allowed scratch: the 108 bytes per lane it has had since it was written.  LDS is all dynamic (layouts in csrc/sdf_common.h)."""
import pytest

from resource_usage import HAVE_HIPCC, kernel_usage

# scratch bytes per lane allowed, per kernel
SCRATCH = {
    "sdf_mlp.hip": (r"_ZN5o23459k_sdf_mlpILi([012])EEE", lambda m: "k_sdf_mlp<%s>" % m.group(1),
                    {"k_sdf_mlp<0>": 0, "k_sdf_mlp<1>": 0, "k_sdf_mlp<2>": 108}),
    "sdf_mlp_x3.hip": (r"_ZN5o23451(?:2k_sdf_mlp_x3ILb([01])EEE|3k_sdf_grad_x3E)", lambda m: "k_sdf_grad_x3" if m.group(1) is None else "k_sdf_mlp_x3<%s>" % m.group(1),
                       {"k_sdf_mlp_x3<0>": 0, "k_sdf_mlp_x3<1>": 0, "k_sdf_grad_x3": 0}),
}


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
@pytest.mark.parametrize("source", sorted(SCRATCH))
def test_sdf_kernels_fit_two_waves_per_simd(tmp_path, source):
    pattern, key, scratch = SCRATCH[source]
    use = kernel_usage(source, pattern, key, tmp_path)
    assert set(use) == set(scratch), sorted(use)
    for kernel, scratch_max in scratch.items():
        u = use[kernel]
        print(kernel, u)
        assert u["VGPRs"] + u["AGPRs"] <= 256, (kernel, u)
        assert u["Occupancy"] >= 2, (kernel, u)
        assert u["ScratchSize"] <= scratch_max, (kernel, u)
        assert u["LDS"] == 0, (kernel, u)                # all of it dynamic: sized by the launchers from the layouts in csrc/sdf_common.h
