"""Shared code of the nn.DataParallel tests (tests/test_dataparallel_cpu.py, tests/test_gpu_dataparallel.py).

* ``replicate_clones``: torch's own ``torch.nn.parallel.replicate`` with the parameter / buffer broadcast replaced by per-replica clones on the
  tensors' own device -- what ``DataParallel.forward`` builds on every forward, reproducible on a CPU or on ONE GPU (replicas on one device).
* ``MiniTrainer``: the reference trainer's call sequence of the mirror modules for --mode export_mesh (features -> conditional volume ->
  extract_geometry -> vertex colours through the projector and the rendering network, trainer_generic.py:827-979, :1309-1382) and --mode val
  (the 512-ray chunk loop of render(), :503-524), in an nn.Module with the reference's attribute names -- usable where the reference is not.
* ``reference_trainer``: the reference's UNCHANGED GenericTrainer through ``dropin.install()`` and tests/fake_ops.py (CPU only; same set-up as
  tests/test_trainer_dropin.py)."""
import contextlib
import importlib
import sys
import types
from unittest import mock

import numpy as np
import torch
import torch.nn as nn

pkg = importlib.import_module("one-2-3-45_amd")
recon = importlib.import_module("one-2-3-45_amd.recon")
featurenet = importlib.import_module("one-2-3-45_amd.featurenet")


def _clones(tensors, devices, detach=False):
    return [[t.detach().clone() if detach else t.clone() for t in tensors] for _ in devices]


def replicate_clones(module, n):
    """``n`` replicas of ``module`` made by torch's real replicate(), the broadcast patched to clones."""
    R = importlib.import_module("torch.nn.parallel.replicate")
    with mock.patch.object(R, "_broadcast_coalesced_reshape", _clones):
        return R.replicate(module, list(range(n)))


def pack_delta(before):
    """pack_stats() entries that grew since the snapshot ``before`` (preloads excluded)."""
    now = recon.pack_stats()
    return {k: v - before.get(k, 0) for k, v in now.items() if k[0] != "preload" and v != before.get(k, 0)}


class Conf(dict):
    def _get(self, k, default=None):
        if k in self:
            return self[k]
        if default is None:
            raise KeyError(k)
        return default

    def get_int(self, k, default=None):
        return int(self._get(k, default))

    def get_float(self, k, default=None):
        return float(self._get(k, default))

    def get_bool(self, k, default=None):
        return bool(self._get(k, default))


def make_networks(D, seed=3, tmp="/tmp"):
    """Seeded FeatureNet, SparseSdfNetwork (lod 0), GeneralRenderingNetwork, SingleVarianceNetwork (CPU; the latent columns of the SDF layers perturbed so
    that the volume matters)."""
    torch.manual_seed(seed)
    feat = featurenet.FeatureNet()
    sdf = recon.SparseSdfNetwork(lod=0, ch_in=56, voxel_size=2.0 / (D - 1), vol_dims=[D, D, D], hidden_dim=128, cost_type="variance_mean",
                                 d_pyramid_feature_compress=16, regnet_d_out=16, num_sdf_layers=4, multires=6)
    g = torch.Generator().manual_seed(seed)
    L = sdf.sdf_layer
    L.lin1.weight_v.data[:, 128:] += 0.03 * torch.randn(128, 16, generator=g)
    L.lin2.weight_v.data[:, 128:] += 0.03 * torch.randn(128, 16, generator=g)
    ren = recon.GeneralRenderingNetwork(in_geometry_feat_ch=16, in_rendering_feat_ch=56, anti_alias_pooling=True)
    var = recon.SingleVarianceNetwork(0.2)
    return feat, sdf, ren, var


class MiniTrainer(nn.Module):
    """The reference trainer's lod-0 use of the mirrors, forward(sample, mode="export_mesh" | "val") like GenericTrainer.forward."""

    def __init__(self, D, seed=3, tmp="/tmp", sink=None):
        super().__init__()
        self.sink = sink                 # dict: forward stores its outputs there under the scene's batch_idx (nn.DataParallel gathers tensors only)
        feat, sdf, ren, var = make_networks(D, seed)
        self.pyramid_feature_network_geometry_lod0 = feat
        self.sdf_network_lod0, self.rendering_network_lod0, self.variance_network_lod0 = sdf, ren, var
        self.sdf_renderer_lod0 = recon.SparseNeuSRenderer(None, sdf, var, ren, 64, 64, 0, 1.0, alpha_type="div", conf=Conf({"general.base_exp_dir": tmp}))

    @torch.no_grad()
    def _volume(self, sample):
        imgs = sample["images"][0]
        fm = featurenet.fused_pyramid(self.pyramid_feature_network_geometry_lod0, imgs)
        H, W = imgs.shape[-2:]
        cv = self.sdf_network_lod0.get_conditional_volume(feature_maps=fm[None], partial_vol_origin=sample["partial_vol_origin"],
                                                          proj_mats=sample["affine_mats"], sizeH=H, sizeW=W, lod=0)
        return imgs, fm, cv

    @torch.no_grad()
    def forward(self, sample, mode="export_mesh", resolution=32, chunk_size=512):
        out = self._forward(sample, mode, resolution, chunk_size)
        if self.sink is None:
            return out
        self.sink[(int(sample["batch_idx"][0]), mode)] = out
        return sample["batch_idx"].new_zeros(1)

    def _forward(self, sample, mode, resolution, chunk_size):
        imgs, fm, cv = self._volume(sample)
        vol, mask = cv["dense_volume_scale0"], cv["valid_mask_volume_scale0"]
        sdf, ren = self.sdf_network_lod0, self.sdf_renderer_lod0
        kw = dict(rendering_feature_maps=fm, color_maps=imgs, w2cs=sample["w2cs"][0], intrinsics=sample["intrinsics"][0], query_c2w=sample["query_c2w"])
        if mode == "export_mesh":
            v, t, _ = ren.extract_geometry(sdf, torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3), resolution=resolution, threshold=0,
                                           device=vol.device, conditional_volume=vol, lod=0)
            h = ren.rendering_projector.compute_view_independent(torch.tensor(v).to(vol), lod=0, geometryVolume=vol[0], geometryVolumeMask=mask[0],
                                                                 sdf_network=sdf, img_wh=list(imgs.shape[-2:]), **kw)
            rgb, _ = self.rendering_network_lod0(*h[:4])
            return {"vertices": torch.from_numpy(np.asarray(v)), "triangles": torch.from_numpy(np.asarray(t)), "colours": rgb.reshape(-1, 3).cpu()}
        rays_o, rays_d = sample["rays"]["rays_o"][0].reshape(-1, 3), sample["rays"]["rays_v"][0].reshape(-1, 3)
        near, far = sample["query_near_far"][0, :1], sample["query_near_far"][0, 1:]          # the same tensors for every chunk, as the trainer passes them
        out = []
        for ro, rd in zip(rays_o.split(chunk_size), rays_d.split(chunk_size)):
            r = ren.render(ro, rd, near, far, sdf, self.rendering_network_lod0, perturb_overwrite=0, alpha_inter_ratio=1.0, lod=0,
                           conditional_volume=vol, conditional_valid_mask_volume=mask, feature_maps=fm, color_maps=imgs, w2cs=kw["w2cs"],
                           intrinsics=kw["intrinsics"], img_wh=list(imgs.shape[-2:]), query_c2w=kw["query_c2w"], if_render_with_grad=False)
            out.append(r["color_fine"].detach().cpu())
        return {"image": torch.cat(out).reshape(imgs.shape[-2], imgs.shape[-1], 3)}


def make_sample(V, HW, seed=5, device="cpu", batch_idx=0):
    """The dict the reference's dataset hands to the trainer (data/One2345_eval_new_data.py:300-377), batch dimension 1."""
    sc = pkg.synth.make_scene(V, hw=(HW, HW), image_seed=seed)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None].to(device)
    ro, rd = pkg.synth.gen_rays(sc["query_intrinsic"], sc["query_c2w"], HW, HW)
    ys, xs = np.meshgrid(np.linspace(0, HW - 1, HW), np.linspace(0, HW - 1, HW), indexing="ij")
    uv = np.stack([2 * xs / (HW - 1) - 1, 2 * ys / (HW - 1) - 1], -1).reshape(-1, 2).astype(np.float32)
    return {"batch_idx": torch.tensor([batch_idx], device=device), "meta": ["synthetic_scene"], "img_wh": torch.tensor([[HW, HW]]), "partial_vol_origin": T(sc["partial_vol_origin"]),
            "query_near_far": T(sc["query_near_far"]), "rays": {"rays_o": T(ro), "rays_v": T(rd), "rays_ndc_uv": T(uv)},
            "images": T(sc["images"]), "intrinsics": T(sc["intrinsics"]), "w2cs": T(sc["w2cs"]), "c2ws": T(sc["c2ws"]),
            "affine_mats": T(sc["affine_mats"]), "scale_mat": T(sc["scale_mat"]), "trans_mat": T(sc["trans_mat"]),
            "query_c2w": T(sc["query_c2w"]), "query_w2c": T(sc["query_w2c"]), "query_image": T(sc["images"][0]),
            "scale_factor": torch.tensor([1.0], device=device)}, sc


def batch_samples(samples):
    """Scenes of batch size 1 -> one sample of batch size len(samples) (what nn.DataParallel scatters along dim 0, one scene per device)."""
    a = samples[0]
    if isinstance(a, dict):
        return {k: batch_samples([s[k] for s in samples]) for k in a}
    if torch.is_tensor(a):
        return torch.cat(samples, 0)
    return sum(samples, [])


@contextlib.contextmanager
def reference_trainer(monkeypatch, tmp):
    """-> (GenericTrainer class of the reference, namespace of the mirror modules + the images cv2.imwrite was given); every sys.modules / meta_path
    change is undone afterwards.  CPU only (the ops layer is tests/fake_ops.py)."""
    import fake_ops
    from oracle import ref_import as RI
    dropin = importlib.import_module("one-2-3-45_amd.dropin")
    mine = ("torchsparse", "inplace_abn", "mcubes", "trimesh", "models", "utils", "loss", "cv2", "torchvision", "icecream", "tsparse")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in mine}
    written = []

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("cv2", COLORMAP_JET=2, applyColorMap=lambda x, cmap: np.repeat(np.asarray(x)[..., None], 3, -1),
        imwrite=lambda path, img: written.append((path, np.array(img))) or True)
    tv = mod("torchvision")
    tv.utils = mod("torchvision.utils")
    tv.transforms = mod("torchvision.transforms")
    mod("icecream", ic=lambda *a, **k: None)
    old_path = list(sys.path)
    sys.path.insert(0, RI.REF)
    old_dwb = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        dropin.install()
        fake_ops.install(monkeypatch)
        from models.trainer_generic import GenericTrainer
        import models.featurenet as mf
        import models.rendering_network as mr
        import models.sparse_sdf_network as ms
        assert ms.SparseSdfNetwork.__module__.startswith("one-2-3-45_amd") and mf.FeatureNet.__module__.startswith("one-2-3-45_amd")
        yield GenericTrainer, types.SimpleNamespace(sdf=ms, ren=mr, feat=mf, written=written, tmp=str(tmp))
    finally:
        sys.meta_path[:] = [f for f in sys.meta_path if type(f).__name__ != "_AliasFinder"]
        for k in list(sys.modules):
            if k.split(".")[0] in mine:
                del sys.modules[k]
        sys.modules.update(saved)
        sys.path[:] = old_path
        sys.dont_write_bytecode = old_dwb


def build_reference_trainer(GenericTrainer, M, D, seed=3):
    feat, sdf, ren, var = make_networks(D, seed)
    conf = Conf({"model.num_lods": 1, "train.if_fix_lod0_networks": True, "train.sdf_igr_weight": 0.1, "train.val_mesh_freq": 1,
                 "general.base_exp_dir": M.tmp, "model.h_patch_size": 3})
    return GenericTrainer(None, feat, None, sdf, None, var, None, ren, None, n_samples_lod0=64, n_importance_lod0=64, n_samples_lod1=64,
                          n_importance_lod1=64, n_outside=0, perturb=1.0, alpha_type="div", conf=conf, timestamp="", base_exp_dir=M.tmp)
