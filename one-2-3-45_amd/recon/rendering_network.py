"""GeneralRenderingNetwork (mirror of models/rendering_network.py:26-129): same parameters / state-dict keys; the forward
pass of projector outputs produced by our Projector runs fused in csrc/color_pts.hip."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import config, ops, weights
from .packs import PackCache, param, params_key


def _prepack_after_load(module, incompatible_keys):
    module.prepack()                      # (a load_state_dict post hook must return None)


class DeferredColour:
    """What our Projector returns in place of the four big tensors: everything csrc/color_pts.hip needs.  It is passed through
    the unchanged trainer code (trainer_generic.py:1330-1361) straight into GeneralRenderingNetwork.forward."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, *a, **k):
        return self

    def detach(self):
        return self

    def materialise(self):
        """The reference Projector's own four tensors for these points (models/projector.py:96-425): geometry_feat [R,S,16], rgb_feat [V,R,S,59],
        ray_diff [V,R,S,4], mask [V,R,S] -- for a caller that feeds a rendering network other than ours."""
        R, S = self.shape
        geo, rf, rd, m = ops.project_features(self.vol_cl, self.maskvol, self.cmaps, self.proj, self.cam_pos, self.pts,
                                              query_cam=getattr(self, "query_cam", None), normals=getattr(self, "normals", None))
        V = rf.shape[0]
        return geo.view(R, S, 16), rf.view(V, R, S, 59), rd.view(V, R, S, 4), m.view(V, R, S)


class GeneralRenderingNetwork(nn.Module):
    def __init__(self, in_geometry_feat_ch=8, in_rendering_feat_ch=56, anti_alias_pooling=True):
        super().__init__()
        if not (in_geometry_feat_ch == 16 and in_rendering_feat_ch == 56 and anti_alias_pooling):
            raise NotImplementedError("o2345 GeneralRenderingNetwork: only the released configuration (16 / 56 / pooling) is built")
        self.in_geometry_feat_ch, self.in_rendering_feat_ch, self.anti_alias_pooling = 16, 56, True
        self.s = nn.Parameter(torch.tensor(0.2), requires_grad=True)
        act = nn.ELU(inplace=True)
        self.ray_dir_fc = nn.Sequential(nn.Linear(4, 16), act, nn.Linear(16, 59), act)
        self.base_fc = nn.Sequential(nn.Linear(193, 64), act, nn.Linear(64, 32), act)
        self.vis_fc = nn.Sequential(nn.Linear(32, 32), act, nn.Linear(32, 33), act)
        self.vis_fc2 = nn.Sequential(nn.Linear(32, 32), act, nn.Linear(32, 1), nn.Sigmoid())
        self.rgb_fc = nn.Sequential(nn.Linear(37, 16), act, nn.Linear(16, 8), act, nn.Linear(8, 1))
        for seq in (self.base_fc, self.vis_fc2, self.vis_fc, self.rgb_fc):
            for m in seq:
                if isinstance(m, nn.Linear):
                    nn.init.kaiming_normal_(m.weight.data)
                    nn.init.zeros_(m.bias.data)
        self._packs = PackCache(self)       # per-device (x3, MFMA) blobs, shared with every nn.DataParallel replica (recon/packs.py)
        # packed for the kernels when the weights are LOADED (the runner loads its checkpoint before the first timed call), not inside the first query
        self.register_load_state_dict_post_hook(_prepack_after_load)

    _LINEARS = (("ray_dir_fc", (0, 2)), ("base_fc", (0, 2)), ("vis_fc", (0, 2)), ("vis_fc2", (0, 2)), ("rgb_fc", (0, 2, 4)))
    _NAMES = ("s",) + tuple(f"{name}.{i}.{n}" for name, idx in _LINEARS for i in idx for n in ("weight", "bias"))     # state-dict keys, in _params() order

    def _params(self):
        """The CURRENT Parameter objects in a fixed order, read from the modules' own tables on every call (no cached list: load_state_dict(assign=True),
        `m.weight = nn.Parameter(...)` and parametrisation removal REPLACE the objects) and without walking the module tree (named_parameters() costs
        0.2 ms, and render() asks per 512-ray chunk)."""
        ps = [param(self, "s")]
        for name, idx in self._LINEARS:
            seq = self._modules[name]._modules
            for i in idx:
                lin = seq[str(i)]
                ps.append(param(lin, "weight"))
                ps.append(param(lin, "bias"))
        return ps

    def weights_key(self):
        """Identity of the current parameters (objects, storages, version counters): changes with any load / assignment / in-place update."""
        return params_key(self._params())

    def _blobs(self):
        """(x3 blob, fp32-MFMA blob) of the current parameters; packed once per device, re-packed only when a parameter of the SOURCE module (this one, or
        the module this nn.DataParallel replica was made from) changed (object identity / data pointer / version counter)."""
        ps = self._params()
        src = self._packs.source(self)
        key = params_key(ps if src is self else src._params())
        dev = ps[0].device

        def make():
            sd = {k: p.detach() for k, p in zip(self._NAMES, ps)}
            return torch.from_numpy(weights.packed_color_x3_blob(sd)).to(dev), torch.from_numpy(weights.packed_color_mfma_blob(sd)).to(dev)
        return self._packs.get("colour", dev, key, make)

    def prepack(self):
        """Pack the parameters for the kernels now and run ONE tiny launch of the colour kernel (its first launch in a process costs ~10 ms in the HIP
        runtime: a warm-up here, a fifth of the reference's "export mesh time" bracket when it happened inside the first query)."""
        if self.s.is_cuda:
            dev = self.s.device
            ops.preload(dev)
            with torch.cuda.device(dev):
                blob, mfma = self.color_network()
                z = lambda *sh: torch.zeros(*sh, device=dev)
                eye = torch.eye(4, device=dev)[None]
                proj, cam = ops.camera_terms(torch.eye(3, device=dev)[None].contiguous(), eye.contiguous())
                ops.color_points(blob, z(2, 2, 2, 16), z(8), z(1, 2, 2, 64), proj, cam, z(32, 3), normals=z(32, 3) + 1.0, want_nviews=False, mfma=mfma)
        return self

    def color_network(self):
        """-> (blob, mfma): the weights as ops.color_points takes them in the configured colour precision"""
        xb, mb = self._blobs()
        return (xb, "x3") if config.color_precision() == "f16x3" else (mb, True)

    def mfma_blob(self):
        return self._blobs()[1]

    def x3_blob(self):
        return self._blobs()[0]

    @torch.no_grad()
    def forward(self, geometry_feat, rgb_feat=None, ray_diff=None, mask=None):
        """Either the reference's four tensors or a DeferredColour produced by our Projector.  Returns
        (rgb [n_rays, n_samples, 3], valid_mask [n_rays]) like rendering_network.py:122-129."""
        if isinstance(geometry_feat, DeferredColour):
            d = geometry_feat
            blob, mode = self.color_network()
            rgb, nv = ops.color_points(blob, d.vol_cl, d.maskvol, d.cmaps, d.proj, d.cam_pos, d.pts,
                                       query_cam=d.query_cam, normals=d.normals, want_nviews=True, mfma=mode)
            R, S = d.shape
            valid = ((nv.view(R, S) >= 2).float().sum(1) > 8)
            return rgb.view(R, S, 3), valid
        # the reference's own call form (rendering_network.py:75-83): geometry_feat [R,S,16], rgb_feat [V,R,S,59], ray_diff [V,R,S,4], mask [V,R,S]
        # -- any Projector's materialised tensors.  Same network kernel, inputs read instead of gathered (slower than the fused path, same results)
        if rgb_feat is None or ray_diff is None or mask is None:
            raise ValueError("o2345 GeneralRenderingNetwork.forward: pass a DeferredColour or the reference's four tensors")
        R, S = geometry_feat.shape[:2]
        V = rgb_feat.shape[0]
        blob, mode = self.color_network()
        rgb, nv = ops.color_from_features(blob, geometry_feat.reshape(R * S, -1), rgb_feat.reshape(V, R * S, -1),
                                          ray_diff.reshape(V, R * S, 4), mask.reshape(V, R * S).float(), x3=mode == "x3")
        valid = ((nv.view(R, S) >= 2).float().sum(1) > 8)
        return rgb.view(R, S, 3), valid
