"""CPU test: the register and LDS budget of k_color_pts, read from the compiler's resource-usage remarks at the product flags.

The f16x3 colour kernel runs 768-thread workgroups (3 waves per SIMD): that needs <= 168 VGPRs per lane, and its dynamic LDS (operand head, four
scalars, one 8 KB slot of shared rows per wave) must fit the 160 KiB of a CU -- the second is a static_assert in csrc/color_pts.hip, so a
successful compile checks it."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

build = importlib.import_module("one-2-3-45_amd.build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# what the compiler reports for each form (template arguments <X3, FEATS>): VGPR ceiling and scratch bytes per lane allowed.  The f16x3 forms keep a
# few tile-level values (indices, addresses: written once per tile, read once at its end) in scratch; nothing inside a view loop.
BUDGET = {(True, False): (168, 64), (True, True): (168, 64), (False, False): (168, 0), (False, True): (168, 0)}


def _usage(tmp_path):
    src = os.path.join(build.CSRC, "color_pts.hip")
    cmd = [HIPCC] + build.FLAGS + build.EXTRA_FLAGS["color_pts.hip"] + ["--offload-device-only", "-c", src, "-o", str(tmp_path / "color_pts.o"),
                                                                       "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: _ZN5o234511k_color_ptsILb([01])ELb([01])E", line)
        if m:
            cur = (m.group(1) == "1", m.group(2) == "1")
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            out[cur].setdefault(m.group(1).split(" ")[0], int(m.group(2)))
        elif "Function Name:" in line:
            cur = None
    return out


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="needs hipcc")
def test_color_pts_fits_three_waves_per_simd(tmp_path):
    use = _usage(tmp_path)
    assert set(use) == set(BUDGET), sorted(use)
    for form, (vgpr_max, scratch_max) in BUDGET.items():
        u = use[form]
        assert u["VGPRs"] + u["AGPRs"] <= vgpr_max, (form, u)
        assert u["Occupancy"] >= 3, (form, u)
        assert u["ScratchSize"] <= scratch_max, (form, u)
        assert u["LDS"] == 0, (form, u)                  # all of it dynamic: sized by color_pts_lds_bytes (static_assert <= 160 KiB)
