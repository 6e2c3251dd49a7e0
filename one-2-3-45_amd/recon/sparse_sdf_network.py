"""SparseSdfNetwork on the HIP back end (mirror of models/sparse_sdf_network.py:35-499, lod 0 path)."""
import importlib
import threading

import numpy as np
import torch
import torch.nn as nn

from .. import config, ops, weights
from ..costreg import CostRegNet
from ..featurenet import ConvBnReLU
from ..weights import COSTREG_LAYERS
from .packs import PackCache, param, params_key

def _prepack_after_load(module, incompatible_keys):
    module.prepack(resolutions=config.prepack_resolutions())                      # (a load_state_dict post hook must return None)


_tsnn = None


def _spnn():
    global _tsnn
    if _tsnn is None:
        _tsnn = importlib.import_module("one-2-3-45_amd.shims.torchsparse.nn")
    return _tsnn


def _attr_cache(t, name, key, make):
    """A value derived from tensor ``t`` (and nothing that ``key`` does not capture), memoised ON the tensor object: valid while the same object has
    the same version counter (any in-place write bumps it).  The trainer hands the SAME tensors to every 512-ray chunk of an image
    (trainer_generic.py:365-416 slices the sample dict once, then loops), so per-image work is done once, not 128 times."""
    hit = getattr(t, name, None)
    k = (t._version,) + tuple(key)
    if hit is not None and hit[0] == k:
        return hit[1]
    val = make()
    try:
        setattr(t, name, (k, val))
    except Exception:                      # a tensor subclass without a __dict__: just do not cache
        pass
    return val


_CL_BY_STORAGE = {}        # (data_ptr, shape, device) -> (weakref of the channel-first volume get_conditional_volume returned, its version, channel-last copy)
_CL_LOCK = threading.Lock()


def _register_channel_last(cf, cl):
    """get_conditional_volume's two layouts of one volume, findable from ANY view of the channel-first tensor: the trainer hands `vol[0]` to the projector
    (trainer_generic.py:1330-1345), a new tensor object on the same storage and version counter -- without this its first use re-laid the volume out through
    an ATen copy kernel (12 ms on the first call of a process, inside the reference's "export mesh time" bracket)."""
    import weakref
    cf._o2345_cl = ((cf._version,), cl)
    with _CL_LOCK:                       # nn.DataParallel's device threads register volumes at once: the prune walks the dict while others insert
        for k in [k for k, (ref, _, _) in _CL_BY_STORAGE.items() if ref() is None]:
            del _CL_BY_STORAGE[k]
        _CL_BY_STORAGE[(cf.data_ptr(), tuple(cf.shape), str(cf.device))] = (weakref.ref(cf), cf._version, cl)


def _channel_last_of_view(volume):
    rec = _CL_BY_STORAGE.get((volume.data_ptr(), tuple(volume.shape), str(volume.device)))
    if rec is not None:
        src = rec[0]()
        # the source tensor is alive (so its memory was not handed to anybody else), this tensor shares its version counter, nothing was written since
        if src is not None and src._version == rec[1] and volume._version == rec[1] and volume.is_contiguous() and volume.dtype == src.dtype:
            return rec[2]
    return volume[0].permute(1, 2, 3, 0).contiguous()


def channel_last(volume):
    """[1,C,D,D,D] reference layout -> [D,D,D,C] sampler layout, memoised on the tensor object per version (get_conditional_volume registers the
    channel-last copy its scatter kernel wrote anyway, so the volumes the trainer passes around -- the returned object or views of it -- are never re-laid out)."""
    return _attr_cache(volume, "_o2345_cl", (), lambda: _channel_last_of_view(volume))


class LatentSDFLayer(nn.Module):
    """Parameter container with the reference's names (lin{0,1,2}.{bias,weight_g,weight_v}) and initialisation
    (sparse_sdf_network.py:57-103); evaluation happens in csrc/sdf_mlp.hip."""

    def __init__(self, d_in=3, d_out=129, d_hidden=128, n_layers=4, skip_in=(4,), multires=0, bias=0.5, geometric_init=True,
                 weight_norm=True, activation="softplus", d_conditional_feature=16):
        super().__init__()
        if not (d_in == 3 and d_hidden == 128 and n_layers == 4 and multires == 6 and weight_norm and activation == "softplus"
                and d_conditional_feature == 16):
            raise NotImplementedError("o2345 LatentSDFLayer: only the released configuration (3->PE(6)->128->128->128, softplus) is built")
        dims_in = [39, 144, 144]
        for l, din in enumerate(dims_in):
            lin = nn.Linear(din, 128)
            if geometric_init:
                if l == 2:
                    nn.init.normal_(lin.weight, mean=np.sqrt(np.pi) / np.sqrt(din), std=0.0001)
                    nn.init.constant_(lin.bias, -bias)
                    nn.init.constant_(lin.weight[:, -16:], 0.0)
                    nn.init.constant_(lin.bias[-16:], 0.0)
                elif l == 0:
                    nn.init.constant_(lin.bias, 0.0)
                    nn.init.constant_(lin.weight[:, 3:], 0.0)
                    nn.init.normal_(lin.weight[:, :3], 0.0, np.sqrt(2) / np.sqrt(128))
                else:
                    nn.init.constant_(lin.bias, 0.0)
                    nn.init.normal_(lin.weight, 0.0, np.sqrt(2) / np.sqrt(128))
                    nn.init.constant_(lin.weight[:, -16:], 0.0)
            setattr(self, f"lin{l}", nn.utils.weight_norm(lin))
        self._packs = PackCache(self)       # per-device blob / grid tables, shared with every nn.DataParallel replica (recon/packs.py)

    _NAMES = tuple(f"lin{l}.{n}" for l in range(3) for n in ("bias", "weight_g", "weight_v"))        # state-dict keys, in _params() order

    def _params(self):
        """The parameters in a fixed order without walking the module tree (named_parameters() costs 0.2 ms, and render() asks per 512-ray chunk)."""
        return [param(m, n) for m in (self.lin0, self.lin1, self.lin2) for n in ("bias", "weight_g", "weight_v")]

    def weights_key(self):
        """Identity of the current parameters (objects, storages, version counters): changes with any load / assignment / in-place update."""
        return params_key(self._params())

    def _source_key(self):
        """weights_key() of the SOURCE module (this one, or the module this nn.DataParallel replica was made from): what the pack cache is keyed by."""
        return params_key(self._packs.source(self)._params())

    def _packed(self):
        """(blob on the parameters' device, folded weights W) of the current parameters; packed once per device and source parameters."""
        ps = self._params()
        dev = ps[0].device
        src = self._packs.source(self)
        key = params_key(ps if src is self else src._params())

        def make():
            W = weights.sdf_weights_from_state_dict({k: p.detach() for k, p in zip(self._NAMES, ps)}, "")
            return torch.from_numpy(weights.packed_sdf_blob(W)).to(dev), W
        return self._packs.get("sdf_blob", dev, key, make)

    def blob(self):
        return self._packed()[0]

    def grid_tables(self, resolution):
        """Layer 0 tabulated for the extraction lattice (csrc/sdf_mlp_x3.hip TAB form; rebuilt when a parameter changes)."""
        if config.sdf_precision() != "f16x3":
            return None
        blob, W = self._packed()
        R = int(resolution)

        def make():
            axes, bias = weights.packed_sdf_grid_tables(W, R)
            return ops.sdf_grid_tables(torch.from_numpy(axes).to(blob.device), torch.from_numpy(bias).to(blob.device))
        return self._packs.get("sdf_grid", blob.device, self._source_key(), make, slot=R)


class _SparseCostRegNet(nn.Module):
    """Parameter container with the reference's key names (conv{0..11}.net.0.kernel, conv*.net.1.{weight,bias,...})."""

    def __init__(self, d_in, d_out=8):
        super().__init__()
        spnn = _spnn()
        self.d_in, self.d_out = d_in, d_out
        for name, ci, co in COSTREG_LAYERS:
            ci = d_in if name == "conv0" else (d_out if name == "conv1" else ci)
            co = d_out if name in ("conv0", "conv11") else co
            tr = name in ("conv7", "conv9", "conv11")
            blk = nn.Module()
            blk.net = nn.Sequential(spnn.Conv3d(ci, co, kernel_size=3, stride=1 if name in ("conv0", "conv2", "conv4", "conv6") else 2, transposed=tr),
                                    spnn.BatchNorm(co), spnn.ReLU(True))
            setattr(self, name, blk)


class SparseSdfNetwork(nn.Module):
    def __init__(self, lod, ch_in, voxel_size, vol_dims, hidden_dim=128, activation="softplus", cost_type="variance_mean",
                 d_pyramid_feature_compress=16, regnet_d_out=8, num_sdf_layers=4, multires=6):
        super().__init__()
        if lod not in (0, 1):
            raise NotImplementedError("o2345 SparseSdfNetwork: lod 0 and lod 1 only (as in the released configurations)")
        self.lod, self.ch_in, self.voxel_size = lod, ch_in, voxel_size
        self.vol_dims = torch.tensor(vol_dims)
        self.hidden_dim, self.cost_type = hidden_dim, cost_type
        self.d_pyramid_feature_compress, self.regnet_d_out, self.multires = d_pyramid_feature_compress, regnet_d_out, multires
        self.selected_views_num, self.gru_fusion = 2, None
        self.compress_layer = ConvBnReLU(ch_in, d_pyramid_feature_compress, 3, 1, 1)
        self.sparse_costreg_net = _SparseCostRegNet(d_in=d_pyramid_feature_compress * 2 + (16 if lod > 0 else 0), d_out=regnet_d_out)
        self.sdf_layer = LatentSDFLayer(d_in=3, d_out=hidden_dim + 1, d_hidden=hidden_dim, n_layers=num_sdf_layers, multires=multires,
                                        geometric_init=True, weight_norm=True, activation=activation, d_conditional_feature=16)
        self._packs = PackCache(self)       # packed sparse CNN + voxel lattice per device, shared with every nn.DataParallel replica (recon/packs.py)
        # weights are packed for the kernels when they are LOADED (the runner loads its checkpoint before the first timed call,
        # exp_runner_generic_blender_val.py:485-512), not inside the first query
        self.register_load_state_dict_post_hook(_prepack_after_load)

    def prepack(self, resolutions=()):
        """Pack every parameter for the kernels now (operand blobs, packed sparse CNN, convolution weights, optional layer-0 tables of the extraction
        lattice): a no-op while the parameters are on the CPU.  Called after load_state_dict; a deployment may also call it after .to(device)."""
        p = self.sdf_layer.lin0.bias
        if not p.is_cuda:
            return self
        ops.preload(p.device)                    # every code object of the library, once per device (not inside the first timed call)
        with torch.cuda.device(p.device):
            self.sdf_layer.blob()
            self._costreg(p.device)
            self.compress_layer.packed()
            for R in resolutions:
                self.sdf_layer.grid_tables(R)
                # extract_geometry returns the R^3 field as numpy through a pinned block (ops.to_host_numpy): the first hipHostMalloc of that size costs ~5 ms;
                # allocated, touched and handed back to torch's caching host allocator here, it is a cache hit inside the first "export mesh time" bracket
                torch.empty(R ** 3, dtype=torch.float32, pin_memory=True).zero_()
            self._voxel_lattice(tuple(int(d) for d in self.vol_dims.tolist()), p.device)
            # one tiny launch of each SDF kernel: the first launch of a kernel object costs ~10 ms in the HIP runtime (after its code object is loaded);
            # at load time it is a warm-up, inside the reference's "export mesh time" bracket of a fresh process it was a fifth of the bracket
            blob = self.sdf_layer.blob()
            vol = torch.zeros(2, 2, 2, 16, device=p.device)
            pts = torch.zeros(32, 3, device=p.device)
            for variant in (0, 2):
                ops.sdf_mlp(blob, vol, pts, variant=variant)
            if config.sdf_precision() == "f16x3":
                ops.sdf_mlp(blob, vol, None, variant=0, grid_R=2, sign=-1.0, grid_tables=self.sdf_layer.grid_tables(2))
                self.sdf_layer._packs.discard("sdf_grid", p.device, slot=2)
        return self

    def _voxel_lattice(self, D, device):
        """generate_grid (ops/generate_grids.py:4-19): the voxel-index lattice [1,3,D,D,D] only depends on the volume size -- built once per (size, device)
        (five launches; at prepack time for the configured vol_dims), returned read-only by contract."""
        D = tuple(D)
        return self._packs.get("lattice", device, D,
                               lambda: torch.stack(torch.meshgrid(*[torch.arange(d, dtype=torch.float32, device=device) for d in D], indexing="ij"))[None])

    def _costreg(self, device):
        """The packed sparse CNN of the current parameters (re-packed only when a parameter of the source module changes)."""
        # the CURRENT parameter objects on every call (10 blocks x (kernel, BN weight, BN bias): a cached list goes stale when load_state_dict(assign=True)
        # or a direct assignment replaces the Parameter objects); read from the modules' own tables, no walk over the module tree
        src = self._packs.source(self)
        sd = self._costreg_params(self)
        key = params_key((sd if src is self else self._costreg_params(src)).values()) + (config.color_precision(),)
        return self._packs.get("costreg", device, key, lambda: CostRegNet({k: v.detach() for k, v in sd.items()}, device))

    @staticmethod
    def _costreg_params(net):
        """{state-dict key (below sparse_costreg_net.): parameter} of the three parameters of each block that the packed network reads."""
        sd = {}
        for name, _, _ in COSTREG_LAYERS:
            blk = net.sparse_costreg_net._modules[name]._modules["net"]._modules
            sd[f"{name}.net.0.kernel"] = param(blk["0"], "kernel")
            sd[f"{name}.net.1.weight"] = param(blk["1"], "weight")
            sd[f"{name}.net.1.bias"] = param(blk["1"], "bias")
        return sd

    # ------------------------------------------------------------------------------------------------ cost volume
    @torch.no_grad()
    def get_conditional_volume(self, feature_maps, partial_vol_origin, proj_mats, sizeH=None, sizeW=None, lod=0, pre_coords=None,
                               pre_feats=None):
        """feature_maps [1,V,56,H,W], partial_vol_origin [1,3], proj_mats [1,V,4,4] -> dict with the reference's keys
        (sparse_sdf_network.py:395-398)."""
        if feature_maps.shape[0] != 1:
            raise NotImplementedError("batch size 1 only (as in the reference's runner)")
        fm = feature_maps[0].contiguous().float()
        V, _, H, W = fm.shape
        D = tuple(int(d) for d in self.vol_dims.tolist())
        if sizeH is not None and (int(sizeH) != H or int(sizeW) != W):
            raise NotImplementedError("feature maps must be at image resolution (the fused pyramid is)")
        feats_nhwc = self.compress_layer.forward_nhwc(fm)
        aff = proj_mats[0].contiguous().float()
        origin = partial_vol_origin[0]
        if self.lod == 0:
            cnt, row, coords, n = ops.costvol_index(aff, V, H, W, D, self.voxel_size, origin, min_views=min(1, V - 1))
            rows = ops.costvol_gather(feats_nhwc, aff, D, self.voxel_size, origin, cnt, coords)
            rows16 = self._costreg(rows.device).forward(rows, coords, row, D)
        else:
            # coarse-to-fine (:335-372): children of the voxels kept from lod 0, filtered by visibility, cost rows || parent feature
            assert pre_feats is not None and pre_coords is not None
            up_feat, up_coords = self.upsample(pre_feats, pre_coords, 1)
            coords = up_coords[:, [1, 2, 3, 0]].to(torch.int32).contiguous()
            cnt = ops.visible_count_list(aff, H, W, self.voxel_size, origin, coords)
            keep = cnt > 1
            coords, cnt, up_feat = coords[keep].contiguous(), cnt[keep].contiguous(), up_feat[keep]
            rows = ops.costvol_gather_list(feats_nhwc, aff, self.voxel_size, origin, cnt, coords)
            feat = torch.cat([rows, up_feat.float()], dim=1).contiguous()
            row = ops.build_index_grid(coords, 1, D)
            rows16 = self._costreg(rows.device).forward(feat, coords, row, D)
        cl, cf, mask = ops.scatter_dense(rows16, row, D, want_cf=True)
        _register_channel_last(cf, cl)               # channel_last()'s memo: the same data in the samplers' layout, written by the same kernel
        lod_ = self.lod
        lattice = self._voxel_lattice(D, cf.device)
        return {f"dense_volume_scale{lod_}": cf, f"valid_mask_volume_scale{lod_}": mask, f"visible_mask_scale{lod_}": mask,
                f"coords_scale{lod_}": lattice}

    def upsample(self, pre_feat, pre_coords, interval, num=8):
        """(N,C), (N,4: b,x,y,z) -> (8N,C), (8N,4): children in the reference's order base,+x,+y,+z,+xy,+xz,+yz,+xyz
        (sparse_sdf_network.py:198-219)."""
        with torch.no_grad():
            off = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 1, 0], [0, 1, 0, 1], [0, 0, 1, 1], [0, 1, 1, 1]],
                               dtype=pre_coords.dtype, device=pre_coords.device)[:num] * interval
            up_coords = (pre_coords[:, None, :] + off[None]).reshape(-1, 4)
            up_feat = pre_feat[:, None, :].expand(-1, num, -1).reshape(-1, pre_feat.shape[1])
        return up_feat, up_coords

    # ------------------------------------------------------------------------------------------------ SDF queries
    def sdf(self, pts, conditional_volume, lod):
        pts = pts.detach().contiguous().float()
        r = ops.sdf_mlp(self.sdf_layer.blob(), channel_last(conditional_volume), pts, variant=1, want_lat=True)
        return {f"sdf_pts_scale{lod}": r["feat"][:, :1], f"sdf_features_pts_scale{lod}": r["feat"][:, 1:],
                f"sampled_latent_scale{lod}": r["lat"]}

    def gradient(self, x, conditional_volume, lod):
        r = ops.sdf_mlp(self.sdf_layer.blob(), channel_last(conditional_volume), x.detach().contiguous().float(), variant=2)
        return r["grad"].unsqueeze(1)

    @torch.no_grad()
    def get_sdf_volume(self, conditional_volume, mask_volume, coords_volume, partial_origin):
        """SDF at the voxel centres using each voxel's OWN latent (sparse_sdf_network.py:441-474); invalid voxels = 1.
        One indexed launch of the MFMA kernel with the channel-last volume itself as the per-point latent table."""
        _, C, dX, dY, dZ = conditional_volume.shape
        cl = channel_last(conditional_volume)
        idx = torch.nonzero(mask_volume.reshape(-1) > 0)[:, 0].to(torch.int32).contiguous()
        pts = (coords_volume.reshape(3, -1).t() * self.voxel_size + partial_origin.reshape(1, 3)).contiguous().float()
        out = {"sdf": torch.ones(dX * dY * dZ, dtype=torch.float32, device=pts.device)}
        ops.sdf_mlp(self.sdf_layer.blob(), cl, pts, variant=0, index=idx, out=out, lat_in=cl.reshape(-1, C))
        return out["sdf"].view(1, 1, dX, dY, dZ)
