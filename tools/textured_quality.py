"""What the textured export keeps: on the stored small scene (the weights and the volume the mesh tests use), from one orbit camera at 64 x 64, the colour
and the normals of a decimated mesh against those of the full mesh, with and without the atlas and the normal map.

    python tools/textured_quality.py [--cell 2] [--texel 8] [--size 64] [--view 1]
    python tools/textured_quality.py --time [--lattice 183] [--texel 4] [--size 512] [--reps 9] [--warmup 3]

Renders, all on the device: the full mesh with its vertex colours and the SDF gradient at its vertices as normals (the reference); the mesh at
``decimate_cell`` with vertex colours and flat normals (pipeline.render_mesh's path); the same mesh as the textured asset with ``texture_texel`` and the
normal map (ops.mesh_raster_textured under raster.asset_camera).  Over the pixels hit in all three images it prints one JSON line: the PSNR of the two
decimated colour images against the reference's (on the float rgb arrays, peak 1), the mean angle in degrees between their normals and the reference's,
and the pixel counts.  The numbers are recorded in DESIGN.md section 6; they depend on the seeded weights and are not asserted anywhere.

``--time`` takes no scene: on the marching-cubes mesh of a sphere on a ``--lattice``^3 grid (about 200,000 triangles at 183) as a textured asset with a
normal map and random texels, from one orbit camera at ``--size``^2, it times with HIP events (median of --reps calls after --warmup) the three entries of
one image -- o2345_mesh_raster_count, o2345_mesh_raster_emit and o2345_mesh_raster_shade_textured, the last with and without the normal map -- and prints
one JSON line.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timings(a):
    import statistics
    import torch
    ops = importlib.import_module("one-2-3-45_amd.ops")
    raster = importlib.import_module("one-2-3-45_amd.raster")
    surface = importlib.import_module("one-2-3-45_amd.surface")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    build = importlib.import_module("one-2-3-45_amd.build")
    dev, R, c = torch.device("cuda:0"), a.lattice, a.texel
    g = torch.linspace(-1.0, 1.0, R, device=dev)
    u = 0.8 - torch.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    v_idx, tris = ops.marching_cubes(u.contiguous(), 0.0)
    nt = int(tris.shape[0])
    lay = mesh_io.texture_layout(nt, c)
    gen = torch.Generator(device=dev).manual_seed(0)
    texture = dict(texel=c, rgb=torch.rand(lay["texels"], 3, device=dev, generator=gen), grad=torch.randn(lay["texels"], 3, device=dev, generator=gen))
    b = mesh_io.textured_asset_buffers(v_idx, tris, R, texture=texture)
    H = W = a.size
    K = np.array([[0.9 * W, 0, (W - 1) / 2.0], [0, 0.9 * H, (H - 1) / 2.0], [0, 0, 1]], np.float32)
    M, _, _ = raster.asset_camera(surface.orbit_c2w(4, 25.0, 2.0)[1])
    cam, near, cull = ops._raster_camera(K, M, 1e-3, 0, "textured_quality")
    verts, idx = b["pos"].to(torch.float64), torch.arange(3 * nt, dtype=torch.int32, device=dev).view(nt, 3)
    nv = 3 * nt
    ws, wsb = ops._scratch("o2345_mesh_raster_workspace_bytes", (nv, nt, H, W), dev, "mesh_raster")
    counts = torch.empty(len(raster.COUNTS), dtype=torch.int64, device=dev)
    count = lambda: ops.call("o2345_mesh_raster_count", verts, idx, 4, nv, nt, *cam, H, W, near, cull, ws, wsb, counts)
    count()
    n_pairs = ops.raster_info(counts.tolist())["pairs"]
    lists = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
    face, depth, bary = torch.empty(H, W, dtype=torch.int32, device=dev), torch.empty(H, W, device=dev), torch.empty(H, W, 3, device=dev)
    kind, counters = torch.empty(H * W, dtype=torch.uint8, device=dev), torch.empty(len(raster.TEX_COUNTS), dtype=torch.int64, device=dev)
    rgb, nrm, lit = (torch.empty(H * W, 3, device=dev) for _ in range(3))
    emit = lambda: ops.call("o2345_mesh_raster_emit", nv, nt, *cam, H, W, near, cull, 1, ws, wsb, n_pairs, lists, face, depth, bary, counts)
    shade = lambda mapped: ops.call("o2345_mesh_raster_shade_textured", verts, idx, 4, nv, nt, face, bary, b["uv"], b["image"], lay["height"], lay["width"],
                                    b["nimage"] if mapped else None, b["nrm"] if mapped else None, b["tan"] if mapped else None, *cam, H, W, 0.25, kind, rgb, nrm, lit,
                                    counters)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        acc = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(acc), "min_ms": min(acc), "max_ms": max(acc)}
    out = {"sources_sha": build.sources_sha(), "lattice": R, "triangles": nt, "texel": c, "atlas": [lay["height"], lay["width"]], "size": [H, W], "reps": a.reps,
           "warmup": a.warmup, "count_entry_ms": timed(count), "emit_entry_ms": timed(emit), "shade_textured_entry_ms": timed(lambda: shade(False)),
           "shade_textured_normal_map_entry_ms": timed(lambda: shade(True)), "info": ops.raster_info(counts.tolist()),
           "tex_info": ops.texture_raster_info(counters.tolist())}
    print(json.dumps(out))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cell", type=int, default=2)
    ap.add_argument("--texel", type=int, default=None)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--view", type=int, default=1)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--lattice", type=int, default=183)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    a.texel = a.texel or (4 if a.time else 8)
    a.size = a.size or (512 if a.time else 64)
    if a.time:
        return timings(a)
    import torch
    from mesh_scene_util import args, stored_scene
    ops = importlib.import_module("one-2-3-45_amd.ops")
    config = importlib.import_module("one-2-3-45_amd.config")
    pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
    raster = importlib.import_module("one-2-3-45_amd.raster")
    surface = importlib.import_module("one-2-3-45_amd.surface")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    S = stored_scene(torch.device("cuda:0"), extract=False)
    H = W = a.size
    K = np.array([[0.9 * W, 0, (W - 1) / 2.0], [0, 0.9 * H, (H - 1) / 2.0], [0, 0, 1]], np.float32)
    c2w = surface.orbit_c2w(4, 25.0, 1.6)[a.view]
    fields = lambda cell, texel: pipeline._mesh_fields(*args(S), config.mesh_options(None, None, cell, None, None, texel, None), normal_map=bool(texel))
    full, dec = fields(0, 0), fields(a.cell, a.texel)
    host = lambda r: {k: r[k].cpu().numpy().reshape(H * W, -1) for k in ("face", "rgb", "nrm")}
    ref = host(ops.mesh_raster(full.verts, full.tris, K, c2w, H, W, near=0.05, vertex_colors=full.rgb, vertex_normals=full.grad.contiguous()))
    flat = host(ops.mesh_raster(dec.verts, dec.tris, K, c2w, H, W, near=0.05, vertex_colors=dec.rgb))
    b = mesh_io.textured_asset_buffers(dec.verts_idx, dec.tris, S["R"], texture=dec.texture)
    M, _, _ = raster.asset_camera(c2w)
    tex = host(ops.mesh_raster_textured(b["pos"], b["uv"], b["image"], K, M, H, W, near=0.05, normals=b["nrm"], tangents=b["tan"], normal_image=b["nimage"]))
    tex["nrm"] = tex["nrm"][:, [0, 2, 1]]                                       # the asset frame exchanges y and z
    both = (ref["face"][:, 0] >= 0) & (flat["face"][:, 0] >= 0) & (tex["face"][:, 0] >= 0)

    def psnr(x):
        return float(10.0 * np.log10(1.0 / np.mean((x["rgb"][both].astype(np.float64) - ref["rgb"][both].astype(np.float64)) ** 2)))

    def angle(x):
        u, v = (n[both].astype(np.float64) / np.linalg.norm(n[both].astype(np.float64), axis=1)[:, None] for n in (x["nrm"], ref["nrm"]))
        return float(np.degrees(np.nanmean(np.arctan2(np.linalg.norm(np.cross(u, v), axis=1), (u * v).sum(1)))))
    out = {"decimate_cell": a.cell, "texture_texel": a.texel, "size": [H, W], "view": a.view, "triangles_full": int(full.tris.shape[0]),
           "triangles_decimated": int(dec.tris.shape[0]), "pixels_full": int((ref["face"] >= 0).sum()), "pixels_decimated": int((flat["face"] >= 0).sum()),
           "pixels_textured": int((tex["face"] >= 0).sum()), "pixels_compared": int(both.sum()), "psnr_vertex_coloured_db": psnr(flat), "psnr_textured_db": psnr(tex),
           "normal_angle_flat_deg": angle(flat), "normal_angle_mapped_deg": angle(tex)}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
