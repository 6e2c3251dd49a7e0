"""CPU test: registers, occupancy and LDS of the ray-sampler kernels (csrc/render.hip), read from the compiler's resource-usage remarks at the product flags.

The kernels are built from shared per-sample stages (csrc/render.hip) and serial chains (csrc/render_math.h); a helper that costs a kernel its occupancy
or pushes it into scratch must show HERE.  The floor is what every kernel had at commit 306a2ce, where each stage was written out per kernel.  The 8 KB of
static LDS of the streaming kernels and of k_ray_cull is the compiler's placement of their per-lane validity masks (ValidBits), the 4 bytes of the round
kernels round_epilogue's flag, the 24 KB of k_ray_scalars its fp64 reduction tree; everything else is dynamic and sized by the launchers."""
import pytest

from resource_usage import HAVE_HIPCC, kernel_usage

# kernel: (occupancy [waves / SIMD] at least, static LDS [bytes] at most)
FLOOR = {
    "k_ray_stream<0,true>": (4, 8196), "k_ray_stream<0,false>": (5, 8196), "k_ray_stream<1,true>": (2, 8196), "k_ray_stream<1,false>": (2, 8196),
    "k_ray_stream<2,true>": (4, 0),
    "k_ray_group<0,true>": (8, 4), "k_ray_group<0,false>": (8, 4), "k_ray_group<1,true>": (8, 4), "k_ray_group<1,false>": (8, 4), "k_ray_group<2,true>": (8, 0),
    "k_ray_composite": (3, 0), "k_ray_composite_group": (8, 0), "k_ray_cull": (4, 8192), "k_ray_cull_group": (8, 0), "k_ray_merge_any": (2, 0),
    "k_ray_coarse": (8, 0), "k_ray_scalars": (8, 24576),
}
PATTERN = r"_ZN5o2345\d+(k_ray_[a-z_]+)(?:ILi([012])ELb([01])EEE|E)"


def _key(m):
    return m.group(1) if m.group(2) is None else "%s<%s,%s>" % (m.group(1), m.group(2), "true" if m.group(3) == "1" else "false")


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_ray_kernels_keep_their_occupancy_and_stay_out_of_scratch(tmp_path):
    use = kernel_usage("render.hip", PATTERN, _key, tmp_path)
    assert set(use) == set(FLOOR), sorted(use)             # a lost (or an unexpected) instantiation
    for kernel, (occupancy, lds) in FLOOR.items():
        u = use[kernel]
        print(kernel, u)
        assert u["ScratchSize"] == 0, (kernel, u)
        assert u["Occupancy"] >= occupancy, (kernel, u)
        assert u["LDS"] <= lds, (kernel, u)
