"""Per-scene reconstruction on one MI355X: the hot path of export_mesh_step / val_step (trainer_generic.py:359-622,
827-979) as a sequence of HIP calls with no host synchronisation except the three size read-backs
(kept-voxel count, coarse-level sizes, mesh size)."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from . import config, ops, weights
from .costreg import CostRegNet
from .featurenet import ConvBnReLU, FeatureNet, fused_pyramid, set_precision


def _load_checked(module, sd, what):
    """load_state_dict that only tolerates absent BatchNorm running buffers (the reference runs in training mode and this back end
    never reads them): a renamed / missing parameter must not silently leave seeded stand-in weights in place."""
    res = module.load_state_dict(sd, strict=False)
    missing = [k for k in res.missing_keys if not ("running_" in k or "num_batches_tracked" in k)]
    if missing or res.unexpected_keys:
        raise KeyError(f"{what}: checkpoint does not match (missing {missing}, unexpected {list(res.unexpected_keys)})")


class SceneWeights:
    """All network parameters of one lod-0 model on the device (seeded stand-ins unless state dicts are given)."""

    def __init__(self, device, seed=0, sdf=None, color_sd=None, costreg_sd=None, variance=0.2, sdf_precision=None, color_precision=None):
        self.device = device
        sdf_precision = config.sdf_precision(sdf_precision)
        color_precision = config.color_precision(color_precision)
        self.color_precision = color_precision    # "f16x3" (default) | "fp32": see config.py
        self.sdf_precision = sdf_precision        # "f16x3" (default) | "fp32": see config.py
        with torch.random.fork_rng(devices=[]):         # seeded stand-in initialisation must not reset the caller's global RNG
            torch.manual_seed(seed)
            self.featurenet = set_precision(FeatureNet().to(device), color_precision)      # 2-D convolutions follow the same mode as the
            self.compress = set_precision(ConvBnReLU(56, 16).to(device), color_precision)   # sparse ones: strict fp32 means fp32 everywhere
        self.sdfW = sdf or weights.init_sdf_weights(seed)
        self.color_sd = color_sd or weights.init_color_state_dict(seed)
        self.costreg_sd = costreg_sd or weights.init_costreg_state_dict(seed)
        t = lambda a: torch.from_numpy(a).to(device)
        self.sdf_blob = t(weights.pack_sdf_blob(self.sdfW))
        self.color_mblob = t(weights.pack_color_mfma_blob(self.color_sd))
        self.color_xblob = t(weights.pack_color_x3_blob(self.color_sd))
        self.costreg = CostRegNet(self.costreg_sd, device, precision=color_precision)      # sparse convolutions follow the same mode
        self._grid_tabs = {}
        self._grid_bg = {}                # resolution -> background table (grid_background)
        self._grid_extractions = {}       # resolution -> extractions that asked for one
        self.variance = float(variance)
        self.inv_s = float(np.clip(np.exp(10.0 * variance), 1e-6, 1e6))

    def color_network(self):
        """-> (blob, mfma): the colour network's weights as ops.color_points takes them in this object's colour precision"""
        return (self.color_xblob, "x3") if self.color_precision == "f16x3" else (self.color_mblob, True)

    def grid_tables(self, resolution):
        """Layer 0 of the SDF network tabulated for the extraction lattice of this resolution (built once per resolution; f16x3 mode only)."""
        if self.sdf_precision != "f16x3":
            return None
        R = int(resolution)
        if R not in self._grid_tabs:
            axes, bias = weights.sdf_grid_tables(self.sdfW, R)
            dev = self.sdf_blob.device
            self._grid_tabs[R] = ops.sdf_grid_tables(torch.from_numpy(axes).to(dev), torch.from_numpy(bias).to(dev))
        return self._grid_tabs[R]

    def grid_background(self, resolution):
        """u of an EMPTY scene on the extraction lattice, [R^3] for sign +1: the lattice kernel itself on a volume of zeros, so that a point without a
        kept voxel among its trilinear corners has exactly this value in every scene these weights reconstruct (ops.sdf_mlp, ``grid_background``).
        Owned like the layer-0 tables, next to them; built and used on the caller's current stream.  Built at the SECOND extraction at a resolution,
        never at the first: a process that extracts one mesh pays nothing and allocates nothing.  None (= evaluate the whole lattice) for that first
        extraction, in fp32 mode, and wherever config.grid_background_allowed says no (O2345_GRID_BACKGROUND_MB)."""
        R = int(resolution)
        if self.sdf_precision != "f16x3" or not config.grid_background_allowed(R):
            return None
        if R not in self._grid_bg:
            seen = self._grid_extractions.get(R, 0)
            self._grid_extractions[R] = seen + 1
            if seen == 0:
                return None
            empty = torch.zeros(2, 2, 2, 16, dtype=torch.float32, device=self.sdf_blob.device)
            self._grid_bg[R] = ops.sdf_mlp(self.sdf_blob, empty, None, variant=0, grid_R=R, sign=1.0, precision="f16x3", grid_tables=self.grid_tables(R))["sdf"]
        return self._grid_bg[R]

    @classmethod
    def from_state_dicts(cls, device, sdf_network_sd, rendering_network_sd, variance, featurenet_sd=None, sdf_precision=None, color_precision=None):
        """Build from the reference checkpoint's per-network state dicts (exp_runner_generic_blender_val.py:485-512:
        keys ``sdf_network_lod0``, ``rendering_network_lod0``, ``variance_network_lod0``, ``pyramid_feature_network``)."""
        t = lambda v: torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v))
        sd = {k: t(v) for k, v in sdf_network_sd.items()}
        costreg = {k[len("sparse_costreg_net."):]: v for k, v in sd.items() if k.startswith("sparse_costreg_net.")}
        self = cls(device, seed=0, sdf=weights.sdf_weights_from_state_dict(sd, "sdf_layer."),
                   color_sd={k: t(v).numpy() for k, v in rendering_network_sd.items()}, costreg_sd=costreg, variance=float(variance),
                   sdf_precision=sdf_precision, color_precision=color_precision)
        comp = {k[len("compress_layer."):]: v for k, v in sd.items() if k.startswith("compress_layer.")}
        _load_checked(self.compress, comp, "compress_layer")
        if featurenet_sd is not None:
            _load_checked(self.featurenet, {k: t(v) for k, v in featurenet_sd.items()}, "pyramid_feature_network")
        return self

    @staticmethod
    def _read_checkpoint(path, names, allow_pickle=None):
        import os
        if allow_pickle is None:
            allow_pickle = os.environ.get("O2345_ALLOW_PICKLE", "0") not in ("", "0")
        try:                                   # only float tensors are kept, so the restricted unpickler is enough for a well-formed checkpoint
            ck = torch.load(path, map_location="cpu", weights_only=True)
        except Exception as e:                 # checkpoints that carry optimizer / numpy scalars need the full unpickler (the reference's own loader uses it)
            if not allow_pickle:
                raise RuntimeError(f"o2345 SceneWeights.from_checkpoint: {path!r} does not load with the restricted unpickler ({type(e).__name__}: {e}); "
                                   "pass allow_pickle=True (or O2345_ALLOW_PICKLE=1) only for a checkpoint you trust -- the full unpickler runs code "
                                   "from the file") from e
            import warnings
            warnings.warn(f"o2345: loading {path!r} with the FULL unpickler (allow_pickle): code in the file is executed")
            ck = torch.load(path, map_location="cpu", weights_only=False)
        return {n: {k: v for k, v in ck[n].items() if torch.is_tensor(v) and v.is_floating_point()} for n in names}

    @classmethod
    def from_checkpoint(cls, device, path, broadcast=False, sdf_precision=None, color_precision=None, allow_pickle=None):
        """Every rank builds its weights from ONE checkpoint file in the reference's format (exp_runner_generic_blender_val.py:514-541: keys
        ``sdf_network_lod0``, ``rendering_network_lod0``, ``variance_network_lod0``, ``pyramid_feature_network``).  Default: each rank reads the file
        (< 4 MB); ``broadcast=True``: rank 0 OF THE PROCESS GROUP reads it and the state dicts reach the other ranks through
        sharding.broadcast_state_dicts (one RCCL broadcast) -- ``path`` may then be None on the other ranks; needs an initialised process group.
        The file is read with torch's restricted unpickler.  A checkpoint that needs the full unpickler (optimizer state with numpy scalars, as the
        reference's own trainer writes) executes arbitrary code from the file when loaded: that is opt-in -- ``allow_pickle=True`` or O2345_ALLOW_PICKLE=1
        -- for files you trust, never a silent fallback."""
        import torch.distributed as dist
        from . import sharding
        names = ("sdf_network_lod0", "rendering_network_lod0", "variance_network_lod0", "pyramid_feature_network")
        if broadcast and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("SceneWeights.from_checkpoint(broadcast=True) needs an initialised torch.distributed process group (sharding.init)")
        state = None
        if not broadcast or dist.get_rank() == 0:
            try:
                state = cls._read_checkpoint(path, names, allow_pickle)
            except Exception as e:                 # with broadcast=True the other ranks are about to enter the collective: hand them the failure instead of a hang
                if not broadcast:
                    raise
                state = e
        if broadcast:
            state = sharding.broadcast_state_dicts(state, device)
        return cls.from_state_dicts(device, state["sdf_network_lod0"], state["rendering_network_lod0"], state["variance_network_lod0"]["variance"],
                                    featurenet_sd=state["pyramid_feature_network"], sdf_precision=sdf_precision, color_precision=color_precision)


@torch.no_grad()
def build_volume(wt, imgs, affine_mats, origin, D, voxel_size, fmaps=None):
    """imgs [V,3,H,W] cuda -> scene dict (dense latent volume, occupancy, colour maps...) -- steps (a),(b) of 3.2.
    ``fmaps`` [V,56,H,W] may be supplied to skip FeatureNet."""
    V, _, H, W = imgs.shape
    cmaps = None
    if fmaps is None:
        # the fused pyramid is written once, as the channel-last colour map [V,H,W,64] (rgb | 56 features | pad); the compress layer reads its
        # features from there (channel offset 3): the channel-first [V,56,H,W] tensor of the reference API is never materialised on this path
        _, cmaps = fused_pyramid(wt.featurenet, imgs, want_cmaps=True, want_nchw=False)
        feats_nhwc = wt.compress.forward_nhwc(cmaps, nhwc_offset=3)            # Conv3x3 56->16 + batch stats, then ABN + channel-last re-layout (HIP)
    else:
        feats_nhwc = wt.compress.forward_nhwc(fmaps)
    cnt, row, coords, n = ops.costvol_index(affine_mats, V, H, W, (D, D, D), voxel_size, origin)
    rows = ops.costvol_gather(feats_nhwc, affine_mats, (D, D, D), voxel_size, origin, cnt, coords)
    rows16 = wt.costreg.forward(rows, coords, row, (D, D, D))
    vol_cl, vol_cf, mask = ops.scatter_dense(rows16, row, (D, D, D), want_cf=False)
    if cmaps is None:
        cmaps = ops.pack_color_maps(fmaps, imgs.contiguous())
    return dict(vol_cl=vol_cl, maskvol=mask.view(-1), cmaps=cmaps, n_voxels=n, rows16=rows16, fmaps=fmaps, rows=rows, coords=coords,
                row_of_voxel=row, cnt=cnt, feats_nhwc=feats_nhwc)


def camera_terms(intrinsics, w2cs):
    """proj = intrinsics @ w2cs[:, :3, :] (render_utils.py:106), cam_pos = inverse(w2cs)[:, :3, 3]: one HIP launch (ops.camera_terms), no BLAS / solver library."""
    return ops.camera_terms(intrinsics, w2cs)


@torch.no_grad()
def render(wt, vol, proj, cam_pos, rays_o, rays_d, near, far, query_cam, n_samples=64, n_importance=64, want_z=False, t_rand=None):
    """One call renders all rays (no 512-ray chunks).  ``t_rand`` [R, n_samples]: the reference's perturb > 0 jitter (drawn by the caller).
    Note: the reference's per-512-ray-chunk quirks (cat_z_vals skipped when <= 1 new point of the CHUNK is valid; "first 100 points"
    when a chunk has no valid point) apply per CALL here -- identical when called per chunk, as the drop-in mirror does (or per segment of one
    call: ops.render_rays(segment_rays=...)).  The colour network skips occupied samples whose compositing weight is below config.WEIGHT_CULL
    (2^-24: a ray's colour moves by <= 7.6e-6, nothing else changes; O2345_WEIGHT_CULL=0 = every occupied sample, like the reference)."""
    scene = dict(sdf_blob=wt.sdf_blob, vol_cl=vol["vol_cl"], maskvol=vol["maskvol"],
                 cmaps=vol["cmaps"], proj=proj, cam_pos=cam_pos, color_mfma_blob=wt.color_mblob,
                 sdf_precision=wt.sdf_precision, color_precision=wt.color_precision,
                 color_x3_blob=wt.color_xblob)
    return ops.render_rays(scene, rays_o, rays_d, near, far, n_samples, n_importance, wt.inv_s, 1.0, 1.0, query_cam, want_z, t_rand=t_rand)


@torch.no_grad()
def render_scene_split(wt, imgs, affine_mats, origin, D, voxel_size, proj, cam_pos, rays_o, rays_d, near, far, query_cam, src=0,
                       keys=("color", "depth", "weights_sum", "color_mask"), **render_kw):
    """ONE image rendered by all ranks of the process group (intra-scene split; single-scene latency instead of scene throughput).
    ``imgs`` [V,3,H,W]: the scene's source images on rank ``src`` (None elsewhere) -- one broadcast; every rank builds the volume itself and renders a
    contiguous block of the rays (sharding.ray_block); one all-gather returns ``keys`` of pipeline.render for ALL rays on every rank.  A render call's
    results do not depend on how the rays are batched (tests/test_gpu_parity.py::test_chunked_render_equals_one_call), so the result equals the
    one-GPU call bit for bit wherever the reference's per-call rules cannot fire (a block without any occupied sample).  Without a process group this
    is build_volume + render."""
    from . import sharding as sh
    dev = rays_o.device
    imgs = sh.broadcast_tensor(imgs, src=src, device=dev)
    vol = build_volume(wt, imgs, affine_mats, origin, D, voxel_size)
    rank, world = (torch.distributed.get_rank(), torch.distributed.get_world_size()) if torch.distributed.is_initialized() else (0, 1)
    lo, hi, per = sh.ray_block(rays_o.shape[0], rank, world)
    R_all = rays_o.shape[0]
    per_ray = lambda a, b: {k: (v[a:b].contiguous() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == R_all else v)     # t_rand [R, n_samples] (perturb > 0)
                            for k, v in render_kw.items()}                                                                  # follows its rays
    if hi > lo:
        o = render(wt, vol, proj, cam_pos, rays_o[lo:hi].contiguous(), rays_d[lo:hi].contiguous(), near, far, query_cam, **per_ray(lo, hi))
        block = {k: o[k] for k in keys}
    else:                                                # more ranks than 64-ray blocks: this rank contributes nothing
        o = render(wt, vol, proj, cam_pos, rays_o[:1].contiguous(), rays_d[:1].contiguous(), near, far, query_cam, **per_ray(0, 1))
        block = {k: o[k][:0] for k in keys}
    return sh.gather_ray_blocks(block, rays_o.shape[0], per, device=dev), vol


def _index_to_world(idx, resolution):
    return idx / (resolution - 1.0) * 2.0 - 1.0                               # sparse_neus_renderer.py:936: index coordinates -> [-1, 1]


def _colours_at(wt, vol, proj, cam_pos, pts):
    """SDF gradient, and the colour network with it as the normal input, at float32 world points [N,3] -> (rgb, grad)"""
    g = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], pts, variant=2, precision=wt.sdf_precision)["grad"]
    blob, mfma = wt.color_network()
    rgb, _ = ops.color_points(blob, vol["vol_cl"], vol["maskvol"], vol["cmaps"], proj, cam_pos, pts, normals=g, want_nviews=False, mfma=mfma)
    return rgb, g


def _extraction_lattice(wt, vol, resolution):
    """u = -sdf on the resolution^3 lattice over [-1, 1]^3, float32 [R,R,R]: what marching cubes meshes and the surface render marches through"""
    bg = wt.grid_background(resolution)
    u = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], None, variant=0, grid_R=resolution, sign=-1.0, precision=wt.sdf_precision, grid_tables=wt.grid_tables(resolution),
                    maskvol=vol["maskvol"] if bg is not None else None, grid_background=bg)["sdf"]
    return u.view(resolution, resolution, resolution)


# _mesh_fields' result: verts fp64 [N,3] in [-1, 1], verts_idx the same in index coordinates, tris, rgb fp32 [N,3], the lattice u [R,R,R], grad (the SDF
# gradient at the vertices; None for an empty mesh), info (ops.mesh_cleanup's), texture (None, or mesh_io.export_asset's ``texture`` dict)
MeshFields = namedtuple("MeshFields", "verts verts_idx tris rgb u grad info texture")


def _mesh_fields(wt, vol, proj, cam_pos, resolution, opts, fill_holes=0, normal_map=False, ambient_occlusion=False):
    """The device work of extract_mesh, once -> MeshFields; ``opts``: a config.MeshOptions.  Marching cubes, then the clean-up chain (ops.mesh_cleanup),
    then gradient and colours at the resulting vertices: the asset export reuses that gradient, the colour network's normal input, for NORMAL.
    ``texture_texel`` = c in [4, 64]: ``texture`` is the baked atlas -- "rgb", the colour network at the surface point of every texel
    (ops.mesh_texture_points on the final unsmoothed mesh; with projection on, those points go through ops.mesh_project with the same limits first, so
    that the texture is taken on the surface and not on the chord planes of a coarse mesh), "stats" (the point op's error counters, still on the
    device: mesh_io.export_asset raises on them after its copy), "layout" (mesh_io.texture_layout), "project" (the texel projection's info) and "texel".
    ``smooth_iterations``: Taubin smoothing (ops.mesh_smooth; factors and pinning from config) as the LAST step: gradient, colours and texels are taken
    at the unsmoothed vertices, which lie on the zero set, so only ``verts`` and ``verts_idx`` differ; the result is not projected again.
    ``fill_holes`` = n >= 3 (a keyword of its own, not a field of ``opts``; 0 = off: nothing is launched and ``info`` keeps its keys): ops.mesh_fill_holes
    closes the boundary loops of at most n edges directly after the clean-up chain -- behind the projection, because a cap does not lie on the zero set
    and must not be moved onto it, and in front of gradient, colours and texture, so that the cap's vertices and triangles are coloured and textured like
    any other; ``info`` gains "fill", the counts of ops.mesh_fill_holes.  A filled rim is no boundary any more: the smoothing's pinning does not hold it.
    ``normal_map`` (a keyword of its own too; it needs ``texture_texel``): ``texture`` keeps "grad", the SDF gradient at the texel points -- the second
    result of the colour call that bakes the atlas, thrown away otherwise -- from which mesh_io.export_asset bakes the tangent-space normal map.  Nothing
    more is evaluated; the frames come from the exported (smoothed) positions, the gradients from the unsmoothed surface points.
    ``ambient_occlusion`` (a keyword of its own too; it needs ``texture_texel``): ``texture`` gains "occlusion_hits" int32 [cells c^2], "occlusion_samples"
    and "occlusion_counts" (device int64 [4]; mesh_io.export_asset reads them with its one copy into "occlusion_info") -- ops.mesh_occlusion at the texel points ON
    THE MESH, ops.mesh_texture_points' points before any projection (a projected point may lie under its own triangle), against the final unsmoothed
    mesh, about the face normal of the texel's owner triangle (mesh_io._texel_owners) on the side of the texel gradient the colour call returns anyway:
    that settles the side whatever the winding.  Samples, ray length and bias from config (64, resolution / 8 and 1e-3 index units).  No synchronisation
    beyond the grid's count."""
    if normal_map and not opts.texture_texel:
        raise ValueError("normal_map: the normal map belongs to the texture atlas; set texture_texel")
    if ambient_occlusion and not opts.texture_texel:
        raise ValueError("ambient_occlusion: the occlusion map belongs to the texture atlas; set texture_texel")
    prec = wt.sdf_precision
    # build_volume's pair: ops.scatter_dense writes zeros into vol_cl wherever maskvol is zero, which is what the sparse lattice evaluation needs (a
    # hand-made ``vol`` must keep that: points without a kept corner voxel get the empty scene's value from the second extraction on)
    u = _extraction_lattice(wt, vol, resolution)
    verts_idx, tris = ops.marching_cubes(u, 0.0)
    verts_idx, tris, info = ops.mesh_cleanup(verts_idx, tris, opts, wt.sdf_blob, vol["vol_cl"], resolution, precision=prec)
    if fill_holes:
        verts_idx, tris, _, info["fill"] = ops.mesh_fill_holes(verts_idx, tris, fill_holes)
    verts = _index_to_world(verts_idx, resolution)
    pts = verts.to(torch.float32).contiguous()
    if pts.shape[0] == 0:
        return MeshFields(verts, verts_idx, tris, torch.zeros(0, 3, device=pts.device), u, None, info, None)
    rgb, g = _colours_at(wt, vol, proj, cam_pos, pts)
    texture = None
    if opts.texture_texel and tris.shape[0]:
        tpts, tworld, tstats = ops.mesh_texture_points(verts_idx, tris, opts.texture_texel, resolution, validate=False)
        tpro, on_mesh = None, tpts
        if opts.project_iterations:
            tpts, tpro = ops.mesh_project(wt.sdf_blob, vol["vol_cl"], tpts, resolution, opts.project_iterations, max_move=opts.project_max_move, precision=prec)
            tworld = _index_to_world(tpts, resolution).to(torch.float32).contiguous()
        trgb, tgrad = _colours_at(wt, vol, proj, cam_pos, tworld)
        texture = dict(texel=opts.texture_texel, rgb=trgb, stats=tstats, project=tpro, layout=ops.mesh_io.texture_layout(tris.shape[0], opts.texture_texel))
        if normal_map:
            texture["grad"] = tgrad
        if ambient_occlusion:
            owners = torch.from_numpy(ops.mesh_io._texel_owners(texture["layout"], tris.shape[0]).reshape(-1).astype(np.int32)).to(on_mesh.device)
            hits, counts = ops.mesh_occlusion(on_mesh, verts_idx, tris, normals=tgrad.to(torch.float64), owners=owners, samples=config.MESH_OCCLUSION_SAMPLES,
                                              max_distance=config.mesh_occlusion_distance(resolution), bias=config.MESH_OCCLUSION_BIAS, validate=False)
            texture.update(occlusion_hits=hits, occlusion_samples=config.MESH_OCCLUSION_SAMPLES, occlusion_counts=counts)
    if opts.smooth_iterations:
        verts_idx = ops.mesh_smooth(verts_idx, tris, opts.smooth_iterations)
        verts = _index_to_world(verts_idx, resolution)
    return MeshFields(verts, verts_idx, tris, rgb, u, g, info, texture)


def _texture_block(texture):
    """-> the "texture" entry of a result dict: {width, height, texel, texels} or None; with a normal map also "normal_map": True, with an occlusion map
    "occlusion": True (a result without them keeps the keys it had)"""
    if not texture:
        return None
    return dict({k: texture["layout"][k] for k in ("width", "height", "texel", "texels")}, **({"normal_map": True} if "grad" in texture else {}),
                **({"occlusion": True} if "occlusion_hits" in texture else {}))


@torch.no_grad()
def extract_mesh(wt, vol, proj, cam_pos, resolution, return_index_verts=False, min_component_faces=None, keep_largest=None, smooth_iterations=None,
                 decimate_cell=None, project_iterations=None, simplify_faces=None, fill_holes=None):
    """extract_fields + marching cubes [+ component filter] [+ decimation] [+ simplification] [+ projection onto the zero set] [+ hole filling] + vertex
    colouring (trainer_generic.py:1309-1363) [+ smoothing], all on the device.  The options: None = the config default, off unless set
    (config.mesh_options; ``fill_holes``: config.mesh_fill_holes, the longest hole in edges that is closed)."""
    m = _mesh_fields(wt, vol, proj, cam_pos, resolution,
                     config.mesh_options(min_component_faces, keep_largest, decimate_cell, project_iterations, smooth_iterations, texture_texel=0,
                                         simplify_faces=simplify_faces), fill_holes=config.mesh_fill_holes(fill_holes))
    return (m.verts_idx if return_index_verts else m.verts), m.tris, m.rgb, m.u


@torch.no_grad()
def export_mesh_ply(path, wt, vol, proj, cam_pos, resolution, scale_mat=None, trans_mat=None, min_component_faces=None, keep_largest=None,
                    smooth_iterations=None, decimate_cell=None, project_iterations=None, simplify_faces=None, fill_holes=None):
    """validate_colored_mesh end to end (trainer_generic.py:1309-1382): SDF grid, marching cubes, vertex colours, frame transforms,
    uint8 colours and the binary PLY -- records packed on the device (csrc/mesh_pack.hip), one D2H copy, one file write.
    The options are extract_mesh's.  Returns (n_vertices, n_triangles)."""
    from . import mesh_io
    verts_idx, tris, rgb, _ = extract_mesh(wt, vol, proj, cam_pos, resolution, True, min_component_faces, keep_largest, smooth_iterations, decimate_cell,
                                           project_iterations, simplify_faces, fill_holes)
    return mesh_io.export_mesh(path, verts_idx, tris, resolution, scale_mat=scale_mat, trans_mat=trans_mat, vertex_colors=rgb if verts_idx.shape[0] else None)


@torch.no_grad()
def export_mesh_asset(path, wt, vol, proj, cam_pos, resolution, scale_mat=None, trans_mat=None, normals=False, min_component_faces=None, keep_largest=None,
                      smooth_iterations=None, decimate_cell=None, project_iterations=None, texture_texel=None, simplify_faces=None, fill_holes=None,
                      normal_map=None, ambient_occlusion=None):
    """export_mesh_ply followed by convert_mesh_format (utils/utils.py:31-47) without the PLY in between: the coloured mesh as ``.glb`` or ``.obj`` in the
    asset frame ((x, y, z) -> (x, z, y), faces reversed), buffers / text packed on the device (csrc/mesh_export.hip).  ``normals=True`` adds unit vertex
    normals from the SDF gradient the vertex colouring already computed (at the unsmoothed vertices when ``smooth_iterations`` is on, at the projected ones
    when ``project_iterations`` is).  A ``.ply`` path gives export_mesh_ply's file.  Returns (n_vertices, n_triangles).
    ``texture_texel`` (None: the config default, 0 = off) = c in [4, 64]: the textured asset instead -- the colour network baked into an atlas of one
    c x c cell per pair of triangles (_mesh_fields, ``texture``), 3 M unwelded vertices with texture coordinates and no vertex colours; the PNG sits inside
    the ``.glb``, or as ``.mtl`` + ``.png`` next to the ``.obj``.  A ``.ply`` path with a texture requested raises ValueError.  ``fill_holes``:
    extract_mesh's.  ``normal_map`` (None: the config default O2345_MESH_NORMAL_MAP, off: nothing is launched and the file keeps its bytes): the textured
    asset also carries a tangent-space normal map baked from the SDF gradient at the texel points (mesh_io.export_asset, ``texture["grad"]``), so that a
    decimated or simplified mesh is lit like the full surface; NORMAL is then the flat face normal whatever ``normals`` says.  With ``texture_texel`` off
    it raises ValueError.  ``ambient_occlusion`` (None: the config default O2345_MESH_OCCLUSION, off: nothing is launched and the file keeps its bytes): the
    textured asset also carries an ambient occlusion map baked by ray casting against the final mesh (_mesh_fields; csrc/mesh_raycast.hip), the
    occlusionTexture of the ``.glb`` and ``stem_occlusion.png`` next to the ``.obj``, so that a decimated mesh keeps the contact shading of its
    concavities.  With ``texture_texel`` off it raises ValueError."""
    from . import mesh_io
    opts = config.mesh_options(min_component_faces, keep_largest, decimate_cell, project_iterations, smooth_iterations, texture_texel, simplify_faces)
    if opts.texture_texel and mesh_io._asset_ext(path) == ".ply":
        raise ValueError("texture: a .ply has no texture coordinates; the output is .glb or .obj")
    m = _mesh_fields(wt, vol, proj, cam_pos, resolution, opts, fill_holes=config.mesh_fill_holes(fill_holes), normal_map=config.mesh_normal_map(normal_map),
                     ambient_occlusion=config.mesh_occlusion(ambient_occlusion))
    return mesh_io.export_asset(path, m.verts_idx, m.tris, resolution, scale_mat=scale_mat, trans_mat=trans_mat,
                                vertex_colors=m.rgb if m.verts_idx.shape[0] else None, normals=m.grad if normals else None, texture=m.texture)


def _device_mesh(mesh, dev):
    """(verts, tris) as device tensors or host arrays -> (verts fp64 [N,3], tris int32 / int64 [M,3]) contiguous on ``dev``"""
    v, t = mesh
    v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64)))
    if not torch.is_tensor(t):
        t = np.asarray(t)
        t = torch.from_numpy(np.ascontiguousarray(t if t.dtype in (np.int32, np.int64) else t.astype(np.int64)))
    return v.to(dev).contiguous(), t.to(dev).contiguous()


# reconstruct_folder's mesh_error report: samples every half grid spacing, F-score at a quarter, a half, one and two spacings
MESH_ERROR_SPACING = 0.5
MESH_ERROR_THRESHOLDS = (0.25, 0.5, 1.0, 2.0)


@torch.no_grad()
def mesh_distance(a, b, spacing=None, thresholds=(), return_samples=False, align=None):
    """Distance between two meshes as surfaces on the device (ops.mesh_distance; definitions in mesh_io.mesh_distance, its host twin): ``a`` (the mesh
    under test) and ``b`` (the reference) are (verts [N,3], tris [M,3]) pairs of device tensors or host arrays -- host arrays are uploaded, to the device
    of the first device tensor among the four, else the current one.  -> dict(a_to_b, b_to_a: {mean, rms, max, within, samples, area}; chamfer;
    hausdorff; thresholds, precision, recall, fscore; degenerate_targets).  ``spacing`` None: one sample per triangle.  ``align`` (None: the meshes share
    a frame; nothing else is launched and the dict is unchanged): True (an 8-azimuth search about z, then point-to-plane refinement) or a dict of
    mesh_align's arguments -- ``a`` is moved onto ``b`` first and the dict gains "alignment", mesh_align's result."""
    dev = next((x.device for x in (*a, *b) if torch.is_tensor(x) and x.is_cuda), None)
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    (va, ta), (vb, tb) = _device_mesh(a, dev), _device_mesh(b, dev)
    return ops.mesh_distance(va, ta, vb, tb, spacing, thresholds, return_samples, align=align)


@torch.no_grad()
def mesh_align(a, b, spacing=None, iterations=30, tol=1e-9, max_distance=None, scale=True, candidates=None, search_iterations=5, init=None):
    """The similarity transform (rotation, translation, uniform scale unless ``scale`` is off) that moves mesh ``a`` onto mesh ``b``, on the device
    (ops.mesh_align; definitions in mesh_io.align_meshes, its host twin): point-to-plane Gauss-Newton of a's surface samples against b, started from each
    rotation of ``candidates`` ([K,3,3], e.g. mesh_io.rotation_candidates(8); None: the identity alone) after matching centroids and rms radii, the best
    candidate after ``search_iterations`` steps refined to ``tol``.  Meshes as in mesh_distance.  -> dict(transform [4,4], scale, rotation, translation,
    score, rms, inlier_fraction, iterations, converged, candidate, candidate_scores, history)."""
    dev = next((x.device for x in (*a, *b) if torch.is_tensor(x) and x.is_cuda), None)
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    (va, ta), (vb, tb) = _device_mesh(a, dev), _device_mesh(b, dev)
    return ops.mesh_align(va, ta, vb, tb, spacing, iterations, tol, max_distance, scale, candidates, search_iterations, init)


@torch.no_grad()
def mesh_audit(mesh, return_elements=False):
    """Audit of a mesh on the device (ops.mesh_audit; definitions in mesh_io.mesh_audit, its host twin): ``mesh`` is a (verts [N,3], tris [M,3]) pair of
    device tensors or host arrays -- host arrays are uploaded, to the device of the first device tensor of the pair, else the current one.  -> the twin's
    dict: counts of open, non-manifold, inconsistent and creased edges, of bow-tie and unused vertices, "euler", "components", "watertight", "oriented",
    "genus", "area", "volume", the quality histogram, mean and minimum, the shortest and the longest edge."""
    dev = next((x.device for x in mesh if torch.is_tensor(x) and x.is_cuda), None)
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    return ops.mesh_audit(*_device_mesh(mesh, dev), return_elements)


@torch.no_grad()
def mesh_intersections(mesh, return_pairs=False):
    """The self-intersections of a mesh on the device (ops.mesh_intersections; definitions in mesh_io.mesh_intersections, its host twin): ``mesh`` is a
    (verts [N,3], tris [M,3]) pair of device tensors or host arrays -- host arrays are uploaded, to the device of the first device tensor of the pair,
    else the current one.  -> the twin's dict: "faces", "skipped", "candidates", "pairs", "faces_hit", "max_hits"; ``return_pairs`` adds the device
    tensors "pairs_list" int32 [n,2] and "face_hits" int32 [M]."""
    dev = next((x.device for x in mesh if torch.is_tensor(x) and x.is_cuda), None)
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    return ops.mesh_intersections(*_device_mesh(mesh, dev), return_pairs)


def _mesh_device(mesh):
    dev = next((x.device for x in mesh if torch.is_tensor(x) and x.is_cuda), None)
    return torch.device("cuda", torch.cuda.current_device()) if dev is None else dev


def _device_points(x, dev):
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3)))
    return x.to(dev, torch.float64).contiguous()


@torch.no_grad()
def mesh_ray_cast(mesh, origins, directions, max_distance, any_hit=False):
    """What rays hit on a mesh, on the device (ops.mesh_ray_cast; definitions in mesh_io.ray_cast, its host twin): ``mesh`` is a (verts [N,3], tris [M,3])
    pair, ``origins`` and ``directions`` [n,3], device tensors or host arrays -- host arrays are uploaded, to the device of the first device tensor of
    the pair, else the current one.  -> (distance fp64 [n] in direction lengths up to ``max_distance``, inf without a hit; tri int32 [n], -1 without a
    hit) on the device; ``any_hit``: bool [n]."""
    dev = _mesh_device(mesh)
    return ops.mesh_ray_cast(_device_points(origins, dev), _device_points(directions, dev), *_device_mesh(mesh, dev), max_distance, any_hit=any_hit)


@torch.no_grad()
def mesh_occlusion(mesh, samples=64, max_distance=None, bias=None, spacing=None, flip=False):
    """Ambient occlusion of a mesh against itself on the device (ops.mesh_occlusion; definitions in mesh_io.mesh_occlusion, its host twin), per face:
    ``mesh`` as in mesh_ray_cast.  The points are the triangle-major surface samples of ops.mesh_surface_samples at ``spacing`` (None: one per triangle,
    at the centroid), each about the face normal of its own triangle in stored order (``flip``: about its negative, for a mesh wound the other way).
    -> dict(exposure fp64 [M]: the mean of (samples - hits) / samples over a face's points, NaN for a face without a point; hits int32 [n], triangle
    int32 [n], points fp64 [n,3], on the device; mean: the area-weighted mean exposure; counts: {"bad_points", "bad_frames", "rays"}; samples,
    max_distance and bias as used)."""
    dev = _mesh_device(mesh)
    v, t = _device_mesh(mesh, dev)
    points, weight, triangle = ops.mesh_surface_samples(v, t, spacing)
    normals = None
    if flip:
        P = v[t.long()[triangle.long()]]                                  # [n,3 corners,3]
        normals = -torch.linalg.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ok = torch.isfinite(v).all(1)
    box = torch.stack([v[ok].amin(0), v[ok].amax(0)]).tolist() if bool(ok.any()) else [[0.0] * 3] * 2
    max_distance, bias = ops.mesh_io.occlusion_defaults(box[0], box[1], max_distance, bias)
    hits, counts = ops.mesh_occlusion(points, v, t, normals=normals, owners=triangle, samples=samples, max_distance=max_distance, bias=bias)
    value = (float(samples) - hits.to(torch.float64)) / float(samples)
    M = t.shape[0]
    total = torch.zeros(M, dtype=torch.float64, device=dev).index_add_(0, triangle.long(), value)
    count = torch.zeros(M, dtype=torch.float64, device=dev).index_add_(0, triangle.long(), torch.ones_like(value))
    wsum = float(weight.sum())
    return dict(exposure=total / count, hits=hits, triangle=triangle, points=points, mean=float((weight * value).sum()) / wsum if wsum > 0 else float("nan"),
                counts=counts, samples=int(samples), max_distance=max_distance, bias=bias)


def _surface_view(wt, vol, proj, cam_pos, u, flags, intrinsic, c2w, H, W, near, far, stride, refine, background):
    """one image of render_surface from a lattice and its brick flags"""
    dev = u.device
    rays_o, rays_d = ops.camera_rays(intrinsic, c2w, H, W, dev)
    tr = ops.surface_trace(u, rays_o, rays_d, near, far, stride=stride, refine=refine, inside_positive=True, flags=flags, image_hw=(H, W), want_info=False)
    pts, hits, n_hits = tr["point"], tr["hits"], tr["n_hits"]
    g = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], pts, variant=2, precision=wt.sdf_precision, index=hits, n_dev=n_hits)["grad"]
    blob, mfma = wt.color_network()
    cam = torch.as_tensor(ops.host_f32(c2w)[:3, 3].copy()).to(dev)
    rgb, _ = ops.color_points(blob, vol["vol_cl"], vol["maskvol"], vol["cmaps"], proj, cam_pos, pts, query_cam=cam, index=hits, n_dev=n_hits,
                              want_nviews=False, mfma=mfma)
    color, normal, depth = ops.surface_pack(tr["kind"], tr["depth"], rgb, g, H, W, background)
    return dict(color=color, normal=normal, depth=depth, kind=tr["kind"].view(H, W), point=pts.view(H, W, 3),
                info=ops.surface_info(tr["stats"].cpu().numpy(), H * W), u=u)


@torch.no_grad()
def render_surface(wt, vol, proj, cam_pos, intrinsic, c2w, H, W, resolution=256, near=0.0, far=1.0e6, stride=None, refine=None, u=None,
                   background=(0, 0, 0, 0)):
    """Depth, normal and colour image of the reconstruction's surface for the pinhole camera (intrinsic [3,3] without skew, c2w [4,4]), H x W pixels, by
    marching the extraction lattice (ops.surface_trace; definitions in surface.py, limits in DESIGN.md section 7): the image shows the zero set of the
    TRILINEAR resolution^3 lattice, the surface extract_mesh's marching cubes meshes, one sample per pixel.  The lattice is computed as _mesh_fields
    computes it, or taken from ``u`` (float32 [R,R,R] = -sdf, e.g. the one extract_mesh returned: no lattice kernel runs then).  Steps: brick flags,
    rays, trace, then on the hit list only the SDF gradient (the normal image) and the colour network as seen from the camera (ops.color_points with
    query_cam = the camera position), then the packer.  ``near`` / ``far`` bound t along the ray on top of the [-1, 1]^3 box; ``stride`` / ``refine``
    None: the config defaults (O2345_SURFACE_STRIDE, O2345_SURFACE_REFINE).  One synchronisation, for the counts.
    -> dict(color u8 [H,W,4], normal u8 [H,W,4], depth f32 [H,W], kind u8 [H,W], point f32 [H,W,3], info, u)."""
    if u is None:
        u = _extraction_lattice(wt, vol, int(resolution))
    flags = ops.surface_bricks(u, 0.0, True)
    return _surface_view(wt, vol, proj, cam_pos, u, flags, intrinsic, c2w, int(H), int(W), near, far, stride, refine, background)


@torch.no_grad()
def render_turntable(wt, vol, proj, cam_pos, intrinsic, H, W, n_views, elevation_deg=20.0, radius=2.0, resolution=256, near=0.0, far=1.0e6, stride=None,
                     refine=None, u=None, background=(0, 0, 0, 0), up=(0.0, 0.0, 1.0)):
    """render_surface from ``n_views`` look-at cameras on a circle around the origin (surface.orbit_c2w: ``elevation_deg`` above the plane normal to
    ``up``, at ``radius``); the lattice and the brick flags are computed once.  -> (list of render_surface results, c2w float32 [n,4,4])."""
    from . import surface
    c2ws = surface.orbit_c2w(n_views, elevation_deg, radius, up)
    if u is None:
        u = _extraction_lattice(wt, vol, int(resolution))
    flags = ops.surface_bricks(u, 0.0, True)
    return [_surface_view(wt, vol, proj, cam_pos, u, flags, intrinsic, c, int(H), int(W), near, far, stride, refine, background) for c in c2ws], c2ws


def _raster_mesh(mesh, vertex_colors, vertex_normals):
    """the camera-independent part of render_mesh: the mesh and its attributes on one device, in the dtypes ops.mesh_raster takes"""
    tensors = [x for x in (*mesh, vertex_colors, vertex_normals) if torch.is_tensor(x) and x.is_cuda]
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    verts, tris = _device_mesh(mesh, dev)
    if verts.dtype != torch.float64:
        verts = verts.to(torch.float64)
    attr = lambda a: None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))).to(dev, torch.float32).contiguous()
    return verts, tris, attr(vertex_colors), attr(vertex_normals)


def _mesh_view(verts, tris, colors, normals, intrinsic, c2w, H, W, near, cull, ray_depth, background):
    """one image of render_mesh from the prepared mesh"""
    r = ops.mesh_raster(verts, tris, intrinsic, c2w, H, W, near=near, cull=cull, ray_depth=ray_depth, vertex_colors=colors, vertex_normals=normals)
    color, normal, depth = ops.surface_pack(r["kind"], r["depth"].view(-1), r["rgb"], r["nrm"], H, W, background)
    return dict(color=color, normal=normal, depth=depth, face=r["face"], bary=r["bary"], info=r["info"])


@torch.no_grad()
def render_mesh(mesh, intrinsic, c2w, H, W, vertex_colors=None, vertex_normals=None, background=(0, 0, 0, 0), near=1e-3, cull=0, ray_depth=True):
    """Depth, normal, colour and face image of a triangle mesh for the pinhole camera (intrinsic [3,3] without skew, c2w [4,4]), H x W pixels, by
    rasterizing it on the device (ops.mesh_raster; definitions in raster.py, limits in DESIGN.md section 7).  ``mesh`` is a (verts [N,3], tris [M,3]) pair
    in the WORLD frame, device tensors or host arrays (uploaded); ``vertex_colors`` / ``vertex_normals`` float32 [N,3] or None (a 0.5 grey; the faces'
    flat normals).  The images are registered pixel for pixel with render_surface's: the same camera, the same sample point per pixel, the same packer
    (colour quantisation, normal encoding, ``background``), and with ``ray_depth`` (the default here) the same depth, the t along the pixel's ray.
    ``cull``: 0 none, 1 back faces, 2 front faces.  -> dict(color u8 [H,W,4], normal u8 [H,W,4], depth f32 [H,W], face int32 [H,W] (-1: no hit), bary f32
    [H,W,3], info: the counts of ops.mesh_raster)."""
    return _mesh_view(*_raster_mesh(mesh, vertex_colors, vertex_normals), intrinsic, c2w, int(H), int(W), near, cull, ray_depth, background)


@torch.no_grad()
def render_mesh_turntable(mesh, intrinsic, H, W, n_views, elevation_deg=20.0, radius=2.0, vertex_colors=None, vertex_normals=None, background=(0, 0, 0, 0),
                          near=1e-3, cull=0, ray_depth=True, up=(0.0, 0.0, 1.0)):
    """render_mesh from ``n_views`` look-at cameras on a circle around the origin (surface.orbit_c2w, render_turntable's cameras); the mesh and its
    attributes are uploaded and converted once.  -> (list of render_mesh results, c2w float32 [n,4,4])."""
    from . import surface
    c2ws = surface.orbit_c2w(n_views, elevation_deg, radius, up)
    prepared = _raster_mesh(mesh, vertex_colors, vertex_normals)
    return [_mesh_view(*prepared, intrinsic, c, int(H), int(W), near, cull, ray_depth, background) for c in c2ws], c2ws


_TEXTURED_KEYS = ("pos", "uv", "image", "nrm", "tan", "nimage")


def _textured_asset(asset):
    """render_textured_mesh's ``asset`` -> the buffers ops.mesh_raster_textured takes, contiguous on one device: a ``.glb`` path is read
    (mesh_io.read_textured_glb), host arrays are uploaded; NORMAL is used only beside TANGENT and the normal image"""
    from . import mesh_io
    if isinstance(asset, (str, bytes)) or hasattr(asset, "__fspath__"):
        asset = mesh_io.read_textured_glb(asset)
    missing = [k for k in _TEXTURED_KEYS[:3] if k not in asset]
    if missing:
        raise ValueError(f"render_textured_mesh: the asset lacks {missing}")
    mapped = "tan" in asset or "nimage" in asset
    if mapped and not all(k in asset for k in _TEXTURED_KEYS):
        raise ValueError("render_textured_mesh: a normal map is nrm, tan and nimage together")
    a = {k: asset[k] for k in (_TEXTURED_KEYS if mapped else _TEXTURED_KEYS[:3])}
    tensors = [x for x in a.values() if torch.is_tensor(x) and x.is_cuda]
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
    return {k: (x if torch.is_tensor(x) else torch.from_numpy(np.array(x, order="C"))).to(dev).contiguous() for k, x in a.items()}    # a copy: the array may be read-only


def _textured_view(a, intrinsic, c2w, H, W, near, cull, ray_depth, ambient, background):
    """one image of render_textured_mesh from the prepared buffers"""
    r = ops.mesh_raster_textured(a["pos"], a["uv"], a["image"], intrinsic, c2w, H, W, near=near, cull=cull, ray_depth=ray_depth, normals=a.get("nrm"),
                                 tangents=a.get("tan"), normal_image=a.get("nimage"), ambient=ambient)
    color, normal, depth = ops.surface_pack(r["kind"], r["depth"].view(-1), r["rgb"], r["nrm"], H, W, background)
    lit = ops.surface_pack(r["kind"], r["depth"].view(-1), r["lit"], r["nrm"], H, W, background)[0]
    return dict(color=color, lit=lit, normal=normal, depth=depth, face=r["face"], info=r["info"], tex_info=r["tex_info"])


@torch.no_grad()
def render_textured_mesh(asset, intrinsic, c2w, H, W, background=(0, 0, 0, 0), near=1e-3, cull=0, ray_depth=True, ambient=0.25):
    """The textured asset as a viewer shows it, rasterized on the device (ops.mesh_raster_textured; definitions in raster.py, limits in DESIGN.md section
    7): the atlas sampled bilinearly, the normal map through the file's tangent frames, a headlight.  ``asset``: the dict of
    mesh_io.textured_asset_buffers (device tensors), the same keys as host arrays, or the path of a ``.glb`` this package wrote with ``texture_texel`` --
    all three render through the same code, in the ASSET's frame: ``c2w`` is raster.asset_camera's (which also gives the factor for ``near`` and the
    depths), or any camera in that frame.  -> dict(color, lit, normal u8 [H,W,4], depth f32 [H,W], face int32 [H,W], info, tex_info); ``lit`` is the
    colour under the headlight with the ``ambient`` floor, ``normal`` the shading normal (the decoded map, or the flat normal without one)."""
    return _textured_view(_textured_asset(asset), intrinsic, c2w, int(H), int(W), near, cull, ray_depth, ambient, background)


@torch.no_grad()
def render_textured_turntable(asset, intrinsic, H, W, n_views, elevation_deg=20.0, radius=2.0, scale_mat=None, trans_mat=None, background=(0, 0, 0, 0),
                              near=1e-3, cull=0, ray_depth=True, ambient=0.25, up=(0.0, 0.0, 1.0)):
    """render_textured_mesh from render_turntable's ``n_views`` cameras of the RECONSTRUCTION frame (surface.orbit_c2w), each mapped into the asset's frame
    by raster.asset_camera with the export's ``scale_mat`` / ``trans_mat`` (``near`` is multiplied by its scale); the buffers are read or uploaded once.
    -> (list of render_textured_mesh results, c2w float32 [n,4,4] of the reconstruction frame)."""
    from . import raster, surface
    c2ws = surface.orbit_c2w(n_views, elevation_deg, radius, up)
    a = _textured_asset(asset)
    out = []
    for c in c2ws:
        M, s, _ = raster.asset_camera(c, scale_mat, trans_mat)
        out.append(_textured_view(a, intrinsic, M, int(H), int(W), near * s, cull, ray_depth, ambient, background))
    return out, c2ws


def _write_textured_previews(buffers, s, n, folder):
    """n views of a folder's textured asset (the device buffers of its export) as ``textured_XXX.png`` and ``textured_lit_XXX.png`` in ``folder``, from
    _write_previews' cameras mapped into the asset's frame"""
    import os
    from . import mesh_io, raster
    K, cams, H, W = _preview_cameras(s, n)
    a = _textured_asset(buffers)
    out = []
    for k, c in enumerate(cams):
        M, scale, _ = raster.asset_camera(c, s["scale_mat"], s["trans_mat"])
        r = _textured_view(a, K, M, H, W, 1e-3 * scale, 0, True, 0.25, (0, 0, 0, 0))
        color, lit, normal, depth, face = ops.to_host_numpy(r["color"], r["lit"], r["normal"], r["depth"], r["face"])
        path, lit_path = os.path.join(folder, f"textured_{k:03d}.png"), os.path.join(folder, f"textured_lit_{k:03d}.png")
        for p, image in ((path, color), (lit_path, lit)):
            with open(p, "wb") as f:
                f.write(mesh_io.png_bytes(image, config.mesh_texture_png_level()))
        out.append({"path": path, "lit_path": lit_path, "color": color, "lit": lit, "normal": normal, "depth": depth, "face": face,
                    "c2w": np.array(c, np.float32), "c2w_asset": M, "info": r["info"], "tex_info": r["tex_info"]})
    return out


def _preview_cameras(s, n):
    """the cameras of a folder's previews -> (K [3,3], list of n c2w [4,4], H, W): the query camera, then an orbit through it"""
    from . import surface
    K, c2w = s["query_intrinsic"].numpy()[:3, :3], s["query_c2w"].numpy()
    H, W = int(s["img_wh"][1]), int(s["img_wh"][0])
    pos = c2w[:3, 3].astype(np.float64)
    up = -c2w[:3, 1].astype(np.float64)                                   # the camera's y axis points down
    dist = float(np.linalg.norm(pos))
    elev = float(np.degrees(np.arcsin(np.clip(np.dot(pos, up) / dist, -0.99, 0.99))))
    return K, [c2w] + list(surface.orbit_c2w(n, elev, dist, up)[1:]), H, W


def _write_mesh_previews(verts, tris, rgb, s, n, folder):
    """n rasterized views of a folder's final mesh (world frame, the PLY's vertex colours) as PNGs in ``folder``, from _write_previews' cameras"""
    import os
    from . import mesh_io
    K, cams, H, W = _preview_cameras(s, n)
    prepared = _raster_mesh((verts, tris), rgb, None)
    out = []
    for k, c in enumerate(cams):
        r = _mesh_view(*prepared, K, c, H, W, 1e-3, 0, True, (0, 0, 0, 0))
        color, normal, depth, face = ops.to_host_numpy(r["color"], r["normal"], r["depth"], r["face"])
        path = os.path.join(folder, f"mesh_preview_{k:03d}.png")
        with open(path, "wb") as f:
            f.write(mesh_io.png_bytes(color, config.mesh_texture_png_level()))
        out.append({"path": path, "color": color, "normal": normal, "depth": depth, "face": face, "c2w": np.array(c, np.float32), "info": r["info"]})
    return out


def _write_previews(wt, vol, proj, cam_pos, u, s, n, folder):
    """n surface renders of a folder's scene as PNGs in ``folder``: the query camera, then an orbit through it"""
    import os
    from . import mesh_io
    K, cams, H, W = _preview_cameras(s, n)
    flags = ops.surface_bricks(u, 0.0, True)
    out = []
    for k, c in enumerate(cams):
        r = _surface_view(wt, vol, proj, cam_pos, u, flags, K, c, H, W, 0.0, 1.0e6, None, None, (0, 0, 0, 0))
        color, normal, depth = ops.to_host_numpy(r["color"], r["normal"], r["depth"])
        path = os.path.join(folder, f"preview_{k:03d}.png")
        with open(path, "wb") as f:
            f.write(mesh_io.png_bytes(color, config.mesh_texture_png_level()))
        out.append({"path": path, "color": color, "normal": normal, "depth": depth, "c2w": np.array(c, np.float32), "info": r["info"]})
    return out


@torch.no_grad()
def reconstruct_folder(root_dir, name, wt, out_ply, D=96, resolution=256, render_val_image=False, output_format=None, min_component_faces=None,
                       keep_largest=None, smooth_iterations=None, decimate_cell=None, project_iterations=None, texture_texel=None, preview_views=None, mesh_error=None,
                       simplify_faces=None, mesh_audit=None, fill_holes=None, mesh_intersections=None, mesh_preview_views=None, normal_map=None,
                       textured_preview_views=None, ambient_occlusion=None):
    """run.py's reconstruction stage without the reference tree: Zero123-style folder (dataset.SceneFolder) -> coloured mesh (binary PLY in
    the original frame), optionally the val image of the target view.  ``output_format`` ".obj" / ".glb" (run.py --output_format) also writes
    ``mesh<ext>`` next to ``out_ply`` in the asset frame, from the same device buffers.  The mesh options are extract_mesh's.  Returns
    dict(vertices, triangles, kept_voxels, ply, components, components_kept, smooth_iterations, decimate_cell, decimate, simplify_faces, simplify,
    project_iterations, project[, asset][, color, depth]); the two component counts are None when the filter is off, ``decimate`` (the counts of
    ops.mesh_decimate) when decimation is, ``simplify`` (the info of ops.mesh_simplify: rounds, counts, why it stopped) when simplification is, and
    ``project`` (the info of ops.mesh_project) when projection is.  ``texture_texel`` (None: the config default, 0 = off): the texture atlas of
    export_mesh_asset for the ``output_format`` asset only -- the PLY stays vertex-coloured; the result's "texture" is {width, height, texel, texels},
    or None when no textured asset was written.  ``preview_views`` (None: the config default O2345_PREVIEW_VIEWS, 0 = off: nothing is launched and the
    result keeps its keys) = n >= 1: n surface renders (render_surface on the lattice the mesh was extracted from) written as ``preview_000.png`` ... next to
    the PLY -- view 0 is the folder's query camera, the others an orbit around the origin at its distance and elevation about its up axis; the result's
    "previews" is the list of {path, color, normal, depth, c2w}.  ``mesh_error`` (None: the config default O2345_MESH_ERROR, off: nothing is launched and
    the result has no new key): the result gains "mesh_error", mesh_distance between the final mesh (A) and the raw marching-cubes mesh before the
    clean-up chain (B, extracted again from the same lattice), in index coordinates -- units of the extraction grid's spacing -- with samples every 0.5
    and thresholds 0.25, 0.5, 1 and 2.  "a_to_b" is the geometric error of what was kept; "b_to_a" also contains whatever the component filter dropped.
    ``mesh_audit`` (None: the config default O2345_MESH_AUDIT, off: nothing is launched and the result has no new key): the result gains "mesh_audit",
    the report of ops.mesh_audit on the final mesh in index coordinates -- is it a closed, oriented 2-manifold, and how good are its triangles; area and
    volume in units of the extraction grid's spacing.  ``fill_holes`` (None: the config default O2345_MESH_FILL_HOLES, 0 = off: nothing is launched, the
    result has no new key and every file keeps its bytes) = n >= 3: the boundary loops of at most n edges are closed after the clean-up chain
    (ops.mesh_fill_holes; config.MESH_FILL_HOLES_ALL: every one); the result gains "fill_holes", its counts.  ``mesh_intersections`` (None: the config
    default O2345_MESH_INTERSECTIONS, off: nothing is launched and the result has no new key): the result gains "mesh_intersections", the counts of
    ops.mesh_intersections on the final mesh in index coordinates -- how many pairs of its triangles cross, which the audit cannot say.
    ``mesh_preview_views`` (None: the config default O2345_MESH_PREVIEW_VIEWS, 0 = off: nothing is launched, the result gains no key and every file keeps
    its bytes) = n >= 1: n rasterized views (render_mesh) of the FINAL mesh -- after the clean-up chain and the hole filling, in the world frame, with the
    vertex colours the PLY gets -- from the cameras of ``preview_views``, written as ``mesh_preview_000.png`` ... next to the PLY; unlike the surface
    previews they show what the mesh options did.  The result's "mesh_previews" is the list of {path, color, normal, depth, face, c2w, info}, and
    "mesh_preview_mesh" the rendered mesh: {verts fp64 [N,3], tris, vertex_colors float32 [N,3] or None}, on the device.
    ``normal_map`` (None: the config default O2345_MESH_NORMAL_MAP, off: nothing is launched and every file keeps its bytes): export_mesh_asset's
    tangent-space normal map for the textured ``output_format`` asset; the result's "texture" block then has "normal_map": True.  With ``texture_texel`` off it
    raises ValueError.
    ``ambient_occlusion`` (None: the config default O2345_MESH_OCCLUSION, off: nothing is launched and every file keeps its bytes): export_mesh_asset's
    ambient occlusion map for the textured ``output_format`` asset; the result's "texture" block then has "occlusion": True.  With ``texture_texel`` off it
    raises ValueError.
    ``textured_preview_views`` (None: the config default O2345_TEXTURED_PREVIEW_VIEWS, 0 = off: nothing is launched, the result gains no key and every file
    keeps its bytes) = n >= 1: n views of the TEXTURED asset as a viewer shows it (render_textured_mesh on the buffers the file is written from: the atlas,
    and with ``normal_map`` the normal map) from the cameras of ``preview_views`` mapped into the asset's frame (raster.asset_camera), written as
    ``textured_000.png`` ... (the albedo) and ``textured_lit_000.png`` ... (under the headlight) next to the PLY.  The result's "textured_previews" is the
    list of {path, lit_path, color, lit, normal, depth, face, c2w, c2w_asset, info, tex_info}.  It needs ``texture_texel`` and an ``output_format`` asset,
    otherwise ValueError."""
    import os
    from . import dataset, mesh_io
    if output_format not in (None, ".ply", ".obj", ".glb"):
        raise ValueError(f"reconstruct_folder: output_format {output_format!r} is not one of '.ply', '.obj', '.glb'")
    nmap = config.mesh_normal_map(normal_map)
    if nmap and not config.mesh_texture_texel(texture_texel):
        raise ValueError("normal_map: the normal map belongs to the texture atlas; set texture_texel")
    occlusion = config.mesh_occlusion(ambient_occlusion)
    if occlusion and not config.mesh_texture_texel(texture_texel):
        raise ValueError("ambient_occlusion: the occlusion map belongs to the texture atlas; set texture_texel")
    textured_previews = config.textured_preview_views(textured_preview_views)
    if textured_previews and not (config.mesh_texture_texel(texture_texel) and output_format in (".obj", ".glb")):
        raise ValueError("textured_preview_views: the textured previews show the textured asset; set texture_texel and output_format '.glb' or '.obj'")
    s = dataset.SceneFolder(root_dir, "export_mesh", specific_dataset_name=name)[0]
    dev = wt.device
    T = lambda t: t.to(dev).contiguous().float()
    vol = build_volume(wt, T(s["images"]), T(s["affine_mats"]), s["partial_vol_origin"].numpy(), D, 2.0 / (D - 1))
    proj, cam_pos = camera_terms(T(s["intrinsics"]), T(s["w2cs"]))
    opts = config.mesh_options(min_component_faces, keep_largest, decimate_cell, project_iterations, smooth_iterations, texture_texel, simplify_faces)
    previews = config.preview_views(preview_views)
    fill = config.mesh_fill_holes(fill_holes)
    asset = output_format in (".obj", ".glb")
    m = _mesh_fields(wt, vol, proj, cam_pos, resolution, opts if asset else opts._replace(texture_texel=0), fill_holes=fill, normal_map=nmap and asset,
                     ambient_occlusion=occlusion and asset)                # the atlas is for the asset only
    rgb = m.rgb if m.verts_idx.shape[0] else None
    nv, nt = mesh_io.export_mesh(out_ply, m.verts_idx, m.tris, resolution, scale_mat=s["scale_mat"], trans_mat=s["trans_mat"], vertex_colors=rgb)
    out = {"vertices": nv, "triangles": nt, "kept_voxels": int(vol["n_voxels"]), "ply": str(out_ply), "components": m.info["components"],
           "components_kept": m.info["components_kept"], "smooth_iterations": opts.smooth_iterations, "decimate_cell": opts.decimate_cell,
           "decimate": m.info["decimate"], "simplify_faces": opts.simplify_faces, "simplify": m.info["simplify"], "project_iterations": opts.project_iterations, "project": m.info["project"], "texture": _texture_block(m.texture)}
    if fill:
        out["fill_holes"] = m.info["fill"]
    if asset:
        out["asset"] = os.path.join(os.path.dirname(str(out_ply)), "mesh" + output_format)
        mesh_io.export_asset(out["asset"], m.verts_idx, m.tris, resolution, scale_mat=s["scale_mat"], trans_mat=s["trans_mat"], vertex_colors=rgb,
                             texture=m.texture)
    if config.mesh_error(mesh_error):
        raw_verts, raw_tris = ops.marching_cubes(m.u, 0.0)                # what _mesh_fields meshed before its clean-up chain: the same lattice, the same bits
        out["mesh_error"] = ops.mesh_distance(m.verts_idx, m.tris, raw_verts, raw_tris, MESH_ERROR_SPACING, MESH_ERROR_THRESHOLDS)
    if config.mesh_audit(mesh_audit):
        out["mesh_audit"] = ops.mesh_audit(m.verts_idx, m.tris)
    if config.mesh_intersections(mesh_intersections):
        out["mesh_intersections"] = ops.mesh_intersections(m.verts_idx, m.tris)
    mesh_previews = config.mesh_preview_views(mesh_preview_views)
    if mesh_previews:
        out["mesh_preview_mesh"] = {"verts": m.verts, "tris": m.tris, "vertex_colors": rgb}
        out["mesh_previews"] = _write_mesh_previews(m.verts, m.tris, rgb, s, mesh_previews, os.path.dirname(str(out_ply)))
    if textured_previews and m.texture is not None and m.verts_idx.shape[0]:
        buffers = mesh_io.textured_asset_buffers(m.verts_idx, m.tris, resolution, scale_mat=s["scale_mat"], trans_mat=s["trans_mat"], texture=m.texture)
        out["textured_previews"] = _write_textured_previews(buffers, s, textured_previews, os.path.dirname(str(out_ply)))
    if previews:
        out["previews"] = _write_previews(wt, vol, proj, cam_pos, m.u, s, previews, os.path.dirname(str(out_ply)))
    if render_val_image:
        r = render(wt, vol, proj, cam_pos, T(s["rays"]["rays_o"]), T(s["rays"]["rays_v"]), float(s["query_near_far"][0]), float(s["query_near_far"][1]),
                   T(s["query_c2w"][:3, 3]))
        H, W = int(s["img_wh"][1]), int(s["img_wh"][0])
        out["color"], out["depth"] = r["color"].view(H, W, 3), r["depth"].view(H, W)
    return out
