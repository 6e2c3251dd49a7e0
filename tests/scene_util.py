"""Small seeded scenes for the tests, built with the ORACLE only (no reference, no GPU)."""
import functools
import importlib
import os

import numpy as np
import torch

from oracle import recon as O

pkg = importlib.import_module("one-2-3-45_amd")
SMALL_SCENE_DENSE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_scene_dense.npz")


def costreg_oracle_weights(sd):
    names = [n for n, _, _ in pkg.weights.COSTREG_LAYERS]
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    return {n: (t(sd[f"{n}.net.0.kernel"]), t(sd[f"{n}.net.1.weight"]), t(sd[f"{n}.net.1.bias"])) for n in names}


@functools.lru_cache(maxsize=4)
@torch.no_grad()
def small_scene(V=4, HW=48, D=20, seed=0):
    sc = pkg.synth.make_scene(V, hw=(HW, HW), image_seed=seed)
    rng = np.random.default_rng(seed + 1)
    fmaps = rng.standard_normal((V, 56, HW, HW)).astype(np.float32)
    f16 = rng.standard_normal((V, 16, HW, HW)).astype(np.float32)
    f16 = np.where(f16 >= 0, f16, 0.01 * f16).astype(np.float32)          # post-ABN-like statistics
    vs = 2.0 / (D - 1)
    aff = torch.from_numpy(sc["affine_mats"])
    origin = torch.from_numpy(sc["partial_vol_origin"])
    coords, vol, cnt = O.costvol(torch.from_numpy(f16), aff, [D, D, D], vs, origin)
    csd = pkg.weights.init_costreg_state_dict(seed)
    rows16, extra = O.sparse_costreg(vol, coords, costreg_oracle_weights(csd))
    dense, mask = O.scatter_dense(coords, rows16, [D, D, D])
    W = pkg.weights.init_sdf_weights(seed)
    rsd = pkg.weights.init_color_state_dict(seed)
    return dict(sc=sc, V=V, H=HW, W=HW, D=D, voxel_size=vs, fmaps=fmaps, f16=f16, coords=coords, vol=vol, cnt=cnt,
                costreg_sd=csd, rows16=rows16, levels=extra["levels"], dense=dense, mask=mask, sdfW=W, color_sd=rsd)


def sdfW_t(W):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in W.items()}


def color_t(sd):
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k, v in sd.items()}


def rays_for(scene, n, seed=0, center=True):
    sc = scene["sc"]
    ro, rd = pkg.synth.gen_rays(sc["query_intrinsic"], sc["query_c2w"], scene["H"], scene["W"])
    rng = np.random.default_rng(seed)
    H, W = scene["H"], scene["W"]
    if center:
        ys, xs = rng.integers(H // 4, 3 * H // 4, n), rng.integers(W // 4, 3 * W // 4, n)
        sel = ys * W + xs
    else:
        sel = rng.integers(0, H * W, n)
    return ro[sel].copy(), rd[sel].copy()


def stored_small_scene_dense():
    """small_scene()'s latent volume [1,16,20,20,20] as stored in tests/golden/small_scene_dense.npz (written by
    `PYTHONPATH=. python tests/scene_util.py`).  The CPU build of that volume (sparse convolutions) rounds differently on different host CPUs, by
    ~2e-6; a test whose result amplifies such differences takes the stored volume, so that it sees the same input on every host."""
    return torch.from_numpy(np.load(SMALL_SCENE_DENSE)["dense"])


if __name__ == "__main__":
    np.savez_compressed(SMALL_SCENE_DENSE, dense=small_scene()["dense"].numpy())
