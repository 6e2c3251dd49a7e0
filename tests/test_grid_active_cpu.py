"""CPU: the activity rule of the sparse lattice evaluation (csrc/geom_math.h grid_point_active / grid_tile_active, the source the pre-pass kernel of
csrc/sdf_mlp_x3.hip runs) against brute force over trilinear_ref_taps, in a stand-alone host program (tests/hostcheck/grid_active_check.hip).

(R, D) = (2, 2), (32, 32), (33, 16), (40, 24), (64, 16); masks: empty, full, one voxel at (0,0,0), one at (D-1,D-1,D-1), random 30 %.  The program
asserts that the point answer is exactly ``ok && any corner kept``, that the tile answer is its OR over the aligned 32 slots (the partial last tile and
tiles that straddle rows included) and that index 0 of any axis is inactive.  Also here: the budget rule of config.grid_background_allowed."""
import importlib
import os
import subprocess

import pytest

from resource_usage import HAVE_HIPCC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_grid_activity_rule_against_brute_force(tmp_path):
    exe = str(tmp_path / "grid_active_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off",
                           os.path.join(HERE, "hostcheck", "grid_active_check.hip"), "-o", exe], stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == "OK", r.stdout
    rows = [l for l in lines if l.startswith("R ")]
    assert len(rows) == 5 * 5                                                   # every (R, D) with every mask
    assert any(" partial 1 " in l for l in rows if l.startswith("R 33 "))       # 33^3 = 1123 * 32 + 1: the partial last tile was there
    assert all(" straddling 0 " in l for l in rows if l.startswith(("R 32 ", "R 64 ")))
    assert not any(" straddling 0 " in l for l in rows if l.startswith(("R 33 ", "R 40 ")))


def test_grid_background_budget(monkeypatch):
    config = importlib.import_module("one-2-3-45_amd.config")
    monkeypatch.setattr(config, "GRID_BACKGROUND_MB", 256)
    assert config.grid_background_allowed(256) and config.grid_background_allowed(406) and not config.grid_background_allowed(407)
    monkeypatch.setattr(config, "GRID_BACKGROUND_MB", 0)
    assert not config.grid_background_allowed(2)
    monkeypatch.setattr(config, "GRID_BACKGROUND_MB", 1 << 20)
    assert config.grid_background_allowed(1290) and not config.grid_background_allowed(1291)      # 1291^3 >= 2^31
