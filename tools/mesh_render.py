"""Renders a mesh file to PNG images with the rasterizer (csrc/mesh_raster.hip; host twin one-2-3-45_amd/raster.py).

    python tools/mesh_render.py MESH OUT.png [--views n] [--size HxW] [--elevation deg] [--cull 0|1|2] [--normals] [--host] [--json]
    python tools/mesh_render.py MESH.glb OUT.png --textured [--lit] [--ambient a] [--views n] [--size HxW] [--cull 0|1|2] [--normals] [--host] [--json]
    python tools/mesh_render.py --time [--reps 9] [--warmup 3] [--volume 128] [--grid 256]

MESH is a ``.ply``, ``.glb`` or ``.obj`` as this package writes them (mesh_io's parsers); its vertex colours are used when it has them, else a grey.  The
cameras are an orbit (surface.orbit_c2w) around the centre of the mesh's bounding box at 2.5 times its half diagonal, the focal length such that the mesh
fills the image.  One view is written to OUT.png, n views to OUT_000.png ...; ``--normals`` writes the normal image instead of the colour image.  ``--json``
prints one JSON line with the counts of every view.  Runs on the GPU (pipeline.render_mesh); ``--host`` uses the numpy twin (raster.render), which needs no
GPU and gives the same bytes.

``--textured`` renders a ``.glb`` written with ``texture_texel`` the way a viewer shows it (pipeline.render_textured_mesh; ``--host``: raster.render_textured):
the atlas sampled bilinearly instead of vertex colours, with ``--normals`` the shading normal (the normal map through the file's tangent frames when the file
has one), with ``--lit`` the colour under a headlight with the ``--ambient`` floor (0.25).  The cameras are the same orbit, in the file's own frame; ``--cull 1``
drops what is seen from behind.  ``--json`` also prints the textured stage's counts.  Without the flag the tool does what it did before.

``--time`` takes no file: on BASELINE config 2's raw mesh at a 256^3 lattice and on the same mesh simplified to 5,000 faces, at 256^2 and 512^2 pixels from
the scene's query camera, it times with HIP events (median of --reps calls after --warmup) the three entries of one image -- o2345_mesh_raster_count (the
per-face set-up, the tile counts and their scan), o2345_mesh_raster_emit (the tile lists and the tile kernel) and o2345_mesh_raster_shade -- and the
packer; on the host clock the whole pipeline.render_mesh, and for orientation pipeline.render_surface on the lattice the mesh came from (another
algorithm with another cost model: it marches a lattice and runs two networks per hit).  A per-kernel split needs a kernel trace of this run
(rocprofv3 --kernel-trace --stats -- python tools/mesh_render.py --time).  Prints one JSON line.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timings(reps, warmup, volume, grid):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    ops = importlib.import_module("one-2-3-45_amd.ops")
    raster = importlib.import_module("one-2-3-45_amd.raster")
    build = importlib.import_module("one-2-3-45_amd.build")
    pipeline = bench.pipeline

    def timed(fn, events):
        for _ in range(warmup):
            fn()
        acc = []
        for _ in range(reps):
            torch.cuda.synchronize()
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(acc), "min_ms": min(acc), "max_ms": max(acc)}

    dev = torch.device("cuda:0")
    wt = pipeline.SceneWeights(dev, seed=0)
    inp = bench.make_inputs(dev, 8, 0, 1)
    vol = pipeline.build_volume(wt, inp["imgs"], inp["aff"], inp["origin"], volume, 2.0 / (volume - 1))
    scene = (wt, vol, inp["proj"], inp["cam_pos"])
    v, t, rgb, u = pipeline.extract_mesh(*scene, grid)
    sv, st, srgb, _ = pipeline.extract_mesh(*scene, grid, simplify_faces=5000)
    c2w = inp["sc"]["query_c2w"]
    res = {"sources_sha": build.sources_sha(), "volume": volume, "grid": grid, "reps": reps, "warmup": warmup}
    for scale in (1, 2):
        H = W = 256 * scale
        K = np.array(inp["sc"]["query_intrinsic"], np.float64)[:3, :3].copy()
        K[:2] *= scale
        size = {}
        for name, (mv, mt, mc) in (("raw", (v, t, rgb)), ("simplified_5000", (sv, st, srgb))):
            mv, mc = mv.contiguous(), mc.contiguous()
            nv, nt = mv.shape[0], mt.shape[0]
            ib = 8 if mt.dtype == torch.int64 else 4
            cam, near, cull = ops._raster_camera(K, c2w, 1e-3, 0, "mesh_render")
            ws, wsb = ops._scratch("o2345_mesh_raster_workspace_bytes", (nv, nt, H, W), dev, "mesh_raster")
            counts = torch.empty(len(raster.COUNTS), dtype=torch.int64, device=dev)
            count = lambda: ops.call("o2345_mesh_raster_count", mv, mt, ib, nv, nt, *cam, H, W, near, cull, ws, wsb, counts)
            count()
            n_pairs = ops.raster_info(counts.tolist())["pairs"]
            lists = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
            face, depth, bary = (torch.empty(H, W, *s, dtype=d, device=dev) for s, d in (((), torch.int32), ((), torch.float32), ((3,), torch.float32)))
            kind, c, n = torch.empty(H * W, dtype=torch.uint8, device=dev), torch.empty(H * W, 3, device=dev), torch.empty(H * W, 3, device=dev)
            emit = lambda: ops.call("o2345_mesh_raster_emit", nv, nt, *cam, H, W, near, cull, 1, ws, wsb, n_pairs, lists, face, depth, bary, counts)
            shade = lambda: ops.call("o2345_mesh_raster_shade", mv, mt, ib, nv, nt, face, bary, H, W, mc, None, kind, c, n)
            row = {"vertices": nv, "triangles": nt, "workspace_bytes": wsb, "count_entry_ms": timed(count, True), "emit_entry_ms": timed(emit, True),
                   "shade_entry_ms": timed(shade, True), "pack_ms": timed(lambda: ops.surface_pack(kind, depth.view(-1), c, n, H, W), True)}
            row["info"] = ops.raster_info(counts.tolist())
            row["render_mesh_ms"] = timed(lambda: pipeline.render_mesh((mv, mt), K, c2w, H, W, vertex_colors=mc), False)
            size[name] = row
        size["render_surface_given_lattice_ms"] = timed(lambda: pipeline.render_surface(*scene, K, c2w, H, W, u=u), False)
        res[f"{H}x{W}"] = size
    print(json.dumps(res))
    return res


def fit_cameras(v, n, H, W, elevation):
    """-> (K float32 [3,3], c2w float32 [n,4,4]): an orbit around the centre of the bounding box that holds the whole mesh in the image"""
    surface = importlib.import_module("one-2-3-45_amd.surface")
    v = v[np.isfinite(v).all(1)]
    lo, hi = (v.min(0), v.max(0)) if v.shape[0] else (np.zeros(3), np.ones(3))
    centre, half = 0.5 * (lo + hi), max(0.5 * float(np.linalg.norm(hi - lo)), 1e-6)
    c2w = surface.orbit_c2w(n, elevation, 2.5 * half)
    c2w[:, :3, 3] += centre.astype(np.float32)
    focal = 0.5 * min(H, W) * (2.5 ** 2 - 1.0) ** 0.5 * 0.95                # the bounding sphere's silhouette just inside the shorter side
    return np.array([[focal, 0, (W - 1) / 2.0], [0, focal, (H - 1) / 2.0], [0, 0, 1]], np.float32), c2w, half


def textured(a, H, W, mesh_io):
    """--textured: the views of a textured .glb"""
    if mesh_io._asset_ext(a.mesh) != ".glb":
        raise SystemExit("--textured takes a .glb written with texture_texel (the GLB is the defined form of the textured asset)")
    asset = mesh_io.read_textured_glb(a.mesh)
    K, c2ws, half = fit_cameras(asset["pos"].astype(np.float64), a.views, H, W, a.elevation)
    kw = dict(near=1e-3 * half, cull=a.cull, ambient=a.ambient)
    which = "normal" if a.normals else "lit" if a.lit else "color"
    stem, suffix = os.path.splitext(a.out)
    report = []
    if not a.host:
        pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
        asset = pipeline._textured_asset(asset)                                 # uploaded once
    for k, c2w in enumerate(c2ws):
        if a.host:
            r = importlib.import_module("one-2-3-45_amd.raster").render_textured(
                asset["pos"], asset["uv"], asset["image"], K, c2w, H, W, normals=asset.get("nrm"), tangents=asset.get("tan"), normal_image=asset.get("nimage"), **kw)
            image = r[which]
        else:
            r = pipeline.render_textured_mesh(asset, K, c2w, H, W, ray_depth=False, **kw)
            image = r[which].cpu().numpy()
        path = a.out if a.views == 1 else f"{stem}_{k:03d}{suffix or '.png'}"
        with open(path, "wb") as fh:
            fh.write(mesh_io.png_bytes(image))
        report.append({"path": path, **r["info"], **r["tex_info"]})
    if a.json:
        print(json.dumps(report))
    else:
        for row in report:
            print(row["path"], " ".join(f"{k}={row[k]}" for k in row if k != "path"))
    return report


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", nargs="?")
    ap.add_argument("out", nargs="?")
    ap.add_argument("--views", type=int, default=1)
    ap.add_argument("--size", default="512x512")
    ap.add_argument("--elevation", type=float, default=20.0)
    ap.add_argument("--cull", type=int, default=0)
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--textured", action="store_true")
    ap.add_argument("--lit", action="store_true")
    ap.add_argument("--ambient", type=float, default=0.25)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--volume", type=int, default=128)
    ap.add_argument("--grid", type=int, default=256)
    a = ap.parse_args(argv)
    if a.time:
        return timings(a.reps, a.warmup, a.volume, a.grid)
    if not a.mesh or not a.out:
        ap.error("a mesh file and an output PNG, or --time")
    try:
        H, W = (int(x) for x in a.size.lower().split("x"))
    except ValueError:
        ap.error(f"--size is HxW, got {a.size!r}")
    if a.views < 1 or H < 1 or W < 1:
        ap.error("--views and both sides of --size must be at least 1")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    if a.lit and not a.textured:
        ap.error("--lit belongs to --textured")
    if a.textured:
        return textured(a, H, W, mesh_io)
    ext = mesh_io._asset_ext(a.mesh)
    parsed = {".ply": mesh_io.read_ply, ".glb": mesh_io.read_glb, ".obj": mesh_io.read_obj}[ext](a.mesh)
    v, f, colours = np.ascontiguousarray(parsed[0], np.float64), np.ascontiguousarray(parsed[1]), parsed[2]
    rgb = None if colours is None else np.ascontiguousarray(np.asarray(colours)[:, :3].astype(np.float32) / np.float32(255.0))
    K, c2ws, half = fit_cameras(v, a.views, H, W, a.elevation)
    kw = dict(vertex_colors=rgb, near=1e-3 * half, cull=a.cull)
    stem, suffix = os.path.splitext(a.out)
    report = []
    for k, c2w in enumerate(c2ws):
        if a.host:
            r = importlib.import_module("one-2-3-45_amd.raster").render(v, f, K, c2w, H, W, **kw)
            image = r["normal" if a.normals else "color"]
        else:
            r = importlib.import_module("one-2-3-45_amd.pipeline").render_mesh((v, f), K, c2w, H, W, ray_depth=False, **kw)
            image = r["normal" if a.normals else "color"].cpu().numpy()
        path = a.out if a.views == 1 else f"{stem}_{k:03d}{suffix or '.png'}"
        with open(path, "wb") as fh:
            fh.write(mesh_io.png_bytes(image))
        report.append({"path": path, **r["info"]})
    if a.json:
        print(json.dumps(report))
    else:
        for row in report:
            print(row["path"], " ".join(f"{k}={row[k]}" for k in row if k != "path"))
    return report


if __name__ == "__main__":
    main()
