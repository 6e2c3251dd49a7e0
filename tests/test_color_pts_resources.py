"""CPU test: the register and LDS budget of k_color_pts, read from the compiler's resource-usage remarks at the product flags.

The f16x3 colour kernel runs 768-thread workgroups (3 waves per SIMD): that needs <= 168 VGPRs per lane, and its dynamic LDS (operand head, four
scalars, one 8 KB slot of shared rows per wave) must fit the 160 KiB of a CU -- the second is a static_assert in csrc/color_pts.hip, so a
successful compile checks it."""
import pytest

from resource_usage import HAVE_HIPCC, kernel_usage

# what the compiler reports for each form (template arguments <X3, FEATS>): VGPR ceiling and scratch bytes per lane allowed.  The f16x3 forms keep a
# few tile-level values (indices, addresses: written once per tile, read once at its end) in scratch; nothing inside a view loop.
BUDGET = {(True, False): (168, 64), (True, True): (168, 64), (False, False): (168, 0), (False, True): (168, 0)}


def _usage(tmp_path):
    return kernel_usage("color_pts.hip", r"_ZN5o234511k_color_ptsILb([01])ELb([01])E", lambda m: (m.group(1) == "1", m.group(2) == "1"), tmp_path)


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_color_pts_fits_three_waves_per_simd(tmp_path):
    use = _usage(tmp_path)
    assert set(use) == set(BUDGET), sorted(use)
    for form, (vgpr_max, scratch_max) in BUDGET.items():
        u = use[form]
        assert u["VGPRs"] + u["AGPRs"] <= vgpr_max, (form, u)
        assert u["Occupancy"] >= 3, (form, u)
        assert u["ScratchSize"] <= scratch_max, (form, u)
        assert u["LDS"] == 0, (form, u)                  # all of it dynamic: sized by color_pts_lds_bytes (static_assert <= 160 KiB)
