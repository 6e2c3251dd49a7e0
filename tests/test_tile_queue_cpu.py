"""CPU: the tile queue's index arithmetic (csrc/common.h: the static bound, the eight sub-ranges of the tail, the walk over the heads), compiled for
the host in a stand-alone program (tests/hostcheck/tile_queue_check.hip) that simulates the claims.

For a few thousand (n_tiles, grid, waves per workgroup) triples -- n_tiles = 0 and n_tiles < 8 included, both static schedules (one eighth of the list
per XCD, block-interleaved), tails of 1/16, 1/8, 1/4 and all of the list, 1 to 3 tiles per claim -- every wave walks its static share, then the waves claim
from eight heads in a random interleaving.  The program asserts that the static shares plus the claimed tiles cover [0, n_tiles) exactly once, that
every wave's static share has the same length, and that every sub-range was drained."""
import os
import re
import subprocess

import pytest

from resource_usage import HAVE_HIPCC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_static_shares_and_claims_cover_the_list_once(tmp_path):
    exe = str(tmp_path / "tile_queue_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(HERE, "hostcheck", "tile_queue_check.hip"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == "OK", r.stdout[-4000:]
    m = re.match(r"cases (\d+) empty (\d+) below8 (\d+) idle_heads (\d+) claims (\d+) queued_tiles (\d+) mismatches 0$", lines[-2])
    assert m, lines[-2]
    cases, empty, below8, idle_heads, claims, queued = map(int, m.groups())
    assert cases >= 3000 and empty > 0 and below8 > empty and idle_heads > 0            # the edge cases were there
    assert claims > queued > 0                                                          # every wave also saw each head exhausted
