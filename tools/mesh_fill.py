"""Closes the holes of a mesh file: every boundary loop of at most --max-edges edges gets a cap (one triangle for three edges, else a fan around the
centroid of its rim).

    python tools/mesh_fill.py IN OUT [--max-edges n] [--host] [--json]
    python tools/mesh_fill.py --time [IN] [--max-edges n] [--reps 5] [--warmup 2] [--volume 128] [--grid 256]

IN is a ``.ply``, ``.glb`` or ``.obj`` as this package writes them (mesh_io's parsers), OUT a ``.ply``, ``.glb`` or ``.obj``, written as it stands: no
change of frame.  Runs on the GPU (ops.mesh_fill_holes); ``--host`` uses the numpy twin (mesh_io.fill_holes), which needs no GPU and gives the same
bytes.  A new vertex takes the mean colour of its rim.  Prints the counts: boundary half-edges, holes, filled, too long, left open on chains, the longest
hole and the sizes of the output; ``--json`` prints them as one JSON line instead.  Without --max-edges every hole is filled.

``--time`` writes no file: it times ops.mesh_fill_holes on the host clock (the call synchronises; median of --reps calls after --warmup) and, on the same
mesh in the same process, ops.mesh_audit -- the unit that builds the same edge table and, on top of it, a union-find over all corners and the fp64
reductions.  The mesh is IN, or without one BASELINE config 2's raw mesh at a 256^3 lattice cut open by dropping the faces of one lattice slab (those whose
centroid has grid / 2 <= z < grid / 2 + 1).  Prints one JSON line.
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


def rim_colors(colors, faces, nt, nv_out):
    """the colours of a filled mesh: those of the input, and for every new vertex the mean of its rim, rounded half up (mesh_io.fill_holes' rule); the rim
    of new vertex c is the second corner of the new triangles (o_{k+1}, o_k, c)"""
    if colors is None:
        return None
    colors = np.asarray(colors)
    nv = colors.shape[0]
    fan = faces[nt:][faces[nt:, 2] >= nv]
    total, count = np.zeros((nv_out - nv, colors.shape[1]), np.int64), np.zeros(nv_out - nv, np.int64)
    np.add.at(total, fan[:, 2] - nv, colors[fan[:, 1]].astype(np.int64))
    np.add.at(count, fan[:, 2] - nv, 1)
    return np.concatenate([colors, ((2 * total + count[:, None]) // (2 * count[:, None])).astype(np.uint8)])


def config2_mesh_cut_open(volume, grid):
    """BASELINE config 2's raw mesh on the device, without the faces of one lattice slab -> (verts fp64 index coordinates, tris)"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    pipeline = bench.pipeline
    dev = torch.device("cuda:0")
    wt = pipeline.SceneWeights(dev, seed=0)
    inp = bench.make_inputs(dev, 8, 0, 1)
    vol = pipeline.build_volume(wt, inp["imgs"], inp["aff"], inp["origin"], volume, 2.0 / (volume - 1))
    v, t, _, _ = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], grid, return_index_verts=True)
    z = v[t.long()].mean(1)[:, 2]
    return v, t[~((z >= grid // 2) & (z < grid // 2 + 1))].contiguous()


def timings(mesh, max_edges, reps, warmup, volume, grid):
    import torch
    ops = importlib.import_module("one-2-3-45_amd.ops")
    build = importlib.import_module("one-2-3-45_amd.build")
    pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
    v, t = pipeline._device_mesh(mesh, torch.device("cuda:0")) if mesh else config2_mesh_cut_open(volume, grid)

    def timed(fn):
        for _ in range(warmup):
            fn()
        acc = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(acc), "min_ms": min(acc), "max_ms": max(acc)}

    fv, ft, _, info = ops.mesh_fill_holes(v, t, max_edges)
    res = {"sources_sha": build.sources_sha(), "vertices": v.shape[0], "triangles": t.shape[0], "max_edges": max_edges,
           "workspace_bytes": ops.call("o2345_mesh_fill_workspace_bytes", v.shape[0], t.shape[0]), "fill": info,
           "boundary_edges_before": ops.mesh_audit(v, t)["boundary_edges"], "boundary_edges_after": ops.mesh_audit(fv, ft)["boundary_edges"],
           "ops_mesh_fill_holes_ms": timed(lambda: ops.mesh_fill_holes(v, t, max_edges)), "ops_mesh_audit_ms": timed(lambda: ops.mesh_audit(v, t))}
    print(json.dumps(res))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", nargs="?")
    ap.add_argument("out", nargs="?")
    ap.add_argument("--max-edges", type=int, default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--volume", type=int, default=128)
    ap.add_argument("--grid", type=int, default=256)
    a = ap.parse_args(argv)
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    max_edges = mesh_io._check_max_edges(a.max_edges)
    if a.time:
        return timings(mesh_io.read_mesh(a.mesh)[:2] if a.mesh else None, max_edges, a.reps, a.warmup, a.volume, a.grid)
    if not (a.mesh and a.out):
        ap.error("IN and OUT, or --time")
    ext = mesh_io._asset_ext(a.out)
    v, f, c = {".ply": mesh_io.read_ply, ".glb": mesh_io.read_glb, ".obj": mesh_io.read_obj}[mesh_io._asset_ext(a.mesh)](a.mesh)[:3]
    nt = f.shape[0]
    if a.host:
        wv, wf, _, _, _, info = mesh_io.fill_holes(np.asarray(v, np.float64), f, max_edges)
    else:
        import torch
        pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
        ops = importlib.import_module("one-2-3-45_amd.ops")
        dv, dt, _, info = ops.mesh_fill_holes(*pipeline._device_mesh((np.asarray(v, np.float64), f), torch.device("cuda:0")), max_edges)
        wv, wf = dv.cpu().numpy(), dt.cpu().numpy()
    wv, wf = np.asarray(wv, np.float32), np.asarray(wf)
    wc = rim_colors(c, wf, nt, wv.shape[0])
    if ext == ".ply":
        mesh_io.write_ply_numpy(a.out, wv, wf.astype(np.int32), wc)
    else:
        (mesh_io.write_glb if ext == ".glb" else mesh_io.write_obj_numpy)(a.out, wv, wf, wc)
    if a.json:
        print(json.dumps(info))
    else:
        for k in mesh_io.FILL_COUNTS:
            print(f"{k:12s} {info[k]}")
    return info


if __name__ == "__main__":
    main()
