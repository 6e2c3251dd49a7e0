"""What the mesh and surface GPU tests share: the device fixture, the stored small scene on the device, the mirror renderer on the golden scene, and
the small helpers around them.  A test module imports the ``dev`` fixture by name and wraps stored_scene() in its own module-scoped ``scene`` fixture,
where it adds its preconditions and precomputed twins: every module builds its scene once."""
import importlib

import numpy as np
import pytest
import torch

ops = importlib.import_module("one-2-3-45_amd.ops")
pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
_lib = importlib.import_module("one-2-3-45_amd._lib")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.lib()
    return torch.device("cuda:0")


def stored_scene(dev, R=64, extract=True):
    """The stored small scene (D = 20) on the device -> dict(wt, vol, proj, cam_pos, R, host = scene_util.small_scene()); with ``extract`` also its
    plain mesh: plain = extract_mesh(..., return_index_verts=True), hv / hf = its vertices and faces on the host."""
    from scene_util import small_scene, stored_small_scene_dense
    s = small_scene()
    sc = s["sc"]
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dev)
    wt = pipeline.SceneWeights(dev, seed=0)
    vol = dict(vol_cl=stored_small_scene_dense()[0].permute(1, 2, 3, 0).contiguous().to(dev), maskvol=s["mask"][0, 0].contiguous().to(dev).view(-1),
               cmaps=ops.pack_color_maps(t(s["fmaps"]).contiguous(), t(sc["images"]).contiguous()))
    proj, cam_pos = pipeline.camera_terms(t(sc["intrinsics"]).float(), t(sc["w2cs"]).float())
    S = dict(wt=wt, vol=vol, proj=proj, cam_pos=cam_pos, R=R, host=s)
    if extract:
        S["plain"] = pipeline.extract_mesh(wt, vol, proj, cam_pos, R, return_index_verts=True)
        S["hv"], S["hf"] = S["plain"][0].cpu().numpy(), S["plain"][1].cpu().numpy()
    return S


def args(S):
    return S["wt"], S["vol"], S["proj"], S["cam_pos"], S["R"]


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def colours_at(S, world):
    """gradient and colours of the pipeline's two networks at float32 world points -> (rgb, grad)"""
    wt, vol = S["wt"], S["vol"]
    g = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], world, variant=2, precision=wt.sdf_precision)["grad"]
    blob, mfma = wt.color_network()
    rgb, _ = ops.color_points(blob, vol["vol_cl"], vol["maskvol"], vol["cmaps"], S["proj"], S["cam_pos"], world, normals=g, want_nviews=False, mfma=mfma)
    return rgb, g


def fields_at(S, verts_idx):
    """colours_at given index coordinates -> (rgb, grad)"""
    return colours_at(S, (verts_idx / (S["R"] - 1.0) * 2.0 - 1.0).to(torch.float32).contiguous())


def sdf_field(blob, vol_cl, prec):
    """the field of mesh_io.project_vertices: the device's own SDF + gradient kernel at the given float32 world points"""
    def field(pts32):
        o = ops.sdf_mlp(blob, vol_cl, torch.from_numpy(pts32).to(vol_cl.device), variant=2, precision=prec)
        return o["sdf"].cpu().numpy(), o["grad"].cpu().numpy()
    return field


def dev_tris(f, dev, dtype):
    return torch.from_numpy(np.array(f)).to(dev).to(dtype).contiguous().view(-1, 3)          # a copy: the shared meshes are read-only


def mc(dev, field):
    """HIP marching cubes of a host field at level 0 -> dict(verts, tris on the device, hv, hf on the host)"""
    verts, tris = ops.marching_cubes(torch.from_numpy(np.array(field)).to(dev), 0.0)
    return dict(verts=verts, tris=tris, hv=verts.cpu().numpy(), hf=tris.cpu().numpy())


def golden_mirror(dev):
    """The drop-in mirror on the golden scene -> (renderer, its SDF network, the latent volume [1,16,D,D,D] on the device)"""
    from golden_util import load
    recon = importlib.import_module("one-2-3-45_amd.recon")
    G = load()
    D = G["cfg"]["D"]
    sdf = recon.SparseSdfNetwork(lod=0, ch_in=56, voxel_size=2.0 / (D - 1), vol_dims=[D, D, D], hidden_dim=128, cost_type="variance_mean",
                                 d_pyramid_feature_compress=16, regnet_d_out=16, num_sdf_layers=4, multires=6).to(dev)
    sdf.load_state_dict(G["sdf_sd"], strict=False)
    ren = recon.SparseNeuSRenderer(None, sdf, recon.SingleVarianceNetwork(0.2).to(dev), recon.GeneralRenderingNetwork(16, 56, True).to(dev), 64, 64, 0, 1.0,
                                   alpha_type="div", conf=None)
    return ren, sdf, torch.from_numpy(np.ascontiguousarray(G["g"]["dense"])).to(dev)[None]
