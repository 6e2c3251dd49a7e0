"""GPU: the clean-up chain behind marching cubes (ops.mesh_cleanup, then smoothing) with EVERY option on at once, through the drop-in mirror: the
per-option files check one stage each, this one the order of all of them.  The expected value is the host twins composed in the documented order on
marching cubes of the returned lattice; every comparison is by bytes."""
import importlib

import numpy as np
import pytest
import torch

from mesh_scene_util import dev, golden_mirror, sdf_field  # noqa: F401 (dev: a fixture)

pytestmark = pytest.mark.gpu

ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")
config = importlib.import_module("one-2-3-45_amd.config")


def test_mirror_extract_geometry_with_every_option_on(dev, monkeypatch):
    ren, sdf, dense = golden_mirror(dev)
    R = 48
    monkeypatch.setattr(config, "MESH_KEEP_LARGEST", True)
    monkeypatch.setattr(config, "MESH_DECIMATE_CELL", 2.0)
    monkeypatch.setattr(config, "MESH_PROJECT_ITERATIONS", 4)
    monkeypatch.setattr(config, "MESH_SMOOTH_ITERATIONS", 3)
    assert config.MESH_PROJECT_MAX_MOVE is None                         # the environment of the test run leaves it unset: the limit is max(1, cell) = 2
    v, t, u = ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=R, threshold=0, device=dev,
                                   conditional_volume=dense, lod=0)
    # the twins, in the documented order, on marching cubes of the u the call returned
    vi, ti = ops.marching_cubes(torch.from_numpy(u).to(dev).contiguous(), 0.0)
    hv, hf = vi.cpu().numpy(), ti.cpu().numpy()
    assert hf.shape[0] > 0
    fv, ff, _, _, _, _ = mio.filter_components(hv, hf, keep_largest=True)
    dv, df, _, _, dinfo = mio.decimate_mesh(fv, ff, 2.0)
    field = sdf_field(sdf.sdf_layer.blob(), dense[0].permute(1, 2, 3, 0).contiguous(), None)
    pv, pinfo = mio.project_vertices(dv, field, R, 4, level=-0.0, max_move=2.0)
    sv = mio.smooth_vertices(pv, df, 3)
    # not vacuous: a chain that skips a stage cannot give these bytes
    assert 0 < dinfo["vertices"] < fv.shape[0] and df.shape[0] > 0
    assert pinfo["max_before"] > 1e-3 and pv.tobytes() != np.ascontiguousarray(dv).tobytes()
    assert sv.tobytes() != pv.tobytes()
    want = sv / (R - 1) * 2.0 + -1.0
    assert v.dtype == np.float64 and v.shape == want.shape and v.tobytes() == want.tobytes()
    assert t.dtype == hf.dtype and np.array_equal(t, df)
