"""Audit of a mesh file: is it a closed, oriented 2-manifold, and how good are its triangles.

    python tools/mesh_audit.py MESH [--host] [--json] [--require-watertight]
    python tools/mesh_audit.py --time [--reps 5] [--warmup 2] [--volume 128] [--grid 256]

MESH is a ``.ply``, ``.glb`` or ``.obj`` as this package writes them (mesh_io's parsers).  Prints the counts of open, non-manifold and inconsistent edges,
of bow-tie and unused vertices, the Euler characteristic, components, genus, area, volume and the quality histogram; ``--json`` prints the report as one
JSON line instead.  Runs on the GPU (pipeline.mesh_audit); ``--host`` uses the numpy twin (mesh_io.mesh_audit), which needs no GPU.
``--require-watertight`` exits with status 1 unless the mesh is watertight.

``--time`` takes no file: it times ops.mesh_audit with HIP events (median of --reps calls after --warmup) on BASELINE config 2's raw mesh at a 256^3
lattice and on its ``simplify_faces`` result (a fifth of the triangles), next to ops.mesh_vertex_adjacency on the same meshes -- the existing unit with
the closest access pattern, one atomic pass over the half-edges; its count synchronises, so that one is timed on the host clock.  Prints one JSON line.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHOWN = ("vertices", "edges", "faces", "euler", "components", "genus", "watertight", "oriented", "boundary_edges", "nonmanifold_edges", "inconsistent_edges",
         "creased_edges", "boundary_vertices", "nonmanifold_vertices", "bowtie_vertices", "unused_vertices", "repeated_faces", "zero_area_faces", "area",
         "volume", "quality_mean", "quality_min", "edge_min", "edge_max", "histogram")


def timings(reps, warmup, volume, grid):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    ops = importlib.import_module("one-2-3-45_amd.ops")
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
    v, t, _, _ = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], grid, return_index_verts=True)
    sv, st, _, _ = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], grid, return_index_verts=True, simplify_faces=t.shape[0] // 5)
    res = {"sources_sha": build.sources_sha()}
    for name, (mv, mt) in (("raw", (v, t)), ("simplified", (sv, st))):
        nv, nt = mv.shape[0], mt.shape[0]
        ws, wsb = ops._scratch("o2345_mesh_audit_workspace_bytes", (nv, nt), dev, "mesh_audit")
        stats = ops._stats_block("O2345AuditStats", dev)
        vf, ff, q = torch.empty(nv, dtype=torch.uint8, device=dev), torch.empty(nt, dtype=torch.uint8, device=dev), torch.empty(nt, dtype=torch.float64, device=dev)
        ib = 8 if mt.dtype == torch.int64 else 4
        report = ops.mesh_audit(mv, mt)
        res[name] = {"vertices": nv, "triangles": nt, "workspace_bytes": wsb, "report": report,
                     "audit_kernels_ms": timed(lambda: ops.call("o2345_mesh_audit", mv, mt, ib, nv, nt, ws, wsb, stats, vf, ff, q), True),
                     "ops_mesh_audit_ms": timed(lambda: ops.mesh_audit(mv, mt), False),
                     "ops_mesh_vertex_adjacency_ms": timed(lambda: ops.mesh_vertex_adjacency(mt, nv), False)}
    print(json.dumps(res))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", nargs="?")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--require-watertight", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--volume", type=int, default=128)
    ap.add_argument("--grid", type=int, default=256)
    a = ap.parse_args(argv)
    if a.time:
        return timings(a.reps, a.warmup, a.volume, a.grid)
    if not a.mesh:
        ap.error("a mesh file, or --time")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    v, f, _ = mesh_io.read_mesh(a.mesh)
    if a.host:
        out = mesh_io.mesh_audit(v, f)
    else:
        out = importlib.import_module("one-2-3-45_amd.pipeline").mesh_audit((v, f))
    if a.json:
        print(json.dumps(out))
    else:
        for k in SHOWN:
            print(f"{k:22s} {out[k]}")
    if a.require_watertight and not out["watertight"]:
        sys.exit(1)
    return out


if __name__ == "__main__":
    main()
