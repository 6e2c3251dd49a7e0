"""Self-intersections of a mesh file: how many pairs of its triangles cross.

    python tools/mesh_intersect.py MESH [--host] [--json] [--pairs] [--require-none]
    python tools/mesh_intersect.py --time [--reps 5] [--warmup 2] [--volume 128] [--grid 256]

MESH is a ``.ply``, ``.glb`` or ``.obj`` as this package writes them (mesh_io's parsers).  Prints the faces that take part, the skipped ones, the candidate
pairs (boxes overlap, at most one shared index), the intersecting pairs, the faces in at least one pair and the most pairs on one face; ``--pairs`` also
prints the pairs, one ``t u`` per line; ``--json`` prints the report as one JSON line instead (with ``--pairs``: "pairs_list").  Runs on the GPU
(pipeline.mesh_intersections); ``--host`` uses the numpy twin (mesh_io.mesh_intersections), which needs no GPU and is quadratic in the faces.
``--require-none`` exits with status 1 if any pair intersects.  Vertices are welded as the file has them: coincident vertices with different indices
share nothing.

``--time`` takes no file: on BASELINE config 2's raw mesh at a 256^3 lattice and on its ``simplify_faces`` results (a fifth and a tenth of the triangles;
the tenth is small enough for the path without a grid) it times, with HIP events (median of --reps calls after --warmup), the kernels of one
o2345_mesh_intersect_count call through the grid, those of o2345_mesh_intersect_emit, the same count without a grid where the mesh has at most 2^16
faces, and the kernels of one o2345_mesh_audit call on the same mesh; on the host clock, ops.mesh_distance_grid (its count synchronises) and the whole ops.mesh_intersections.  Prints one JSON line.
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


def timings(reps, warmup, volume, grid):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    ops = importlib.import_module("one-2-3-45_amd.ops")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
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
    tv, tt, _, _ = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], grid, return_index_verts=True, simplify_faces=t.shape[0] // 10)
    res = {"sources_sha": build.sources_sha()}
    for name, (mv, mt) in (("raw", (v, t)), ("simplified", (sv, st)), ("simplified_tenth", (tv, tt))):
        nv, nt = mv.shape[0], mt.shape[0]
        ib = 8 if mt.dtype == torch.int64 else 4
        ws, wsb = ops._scratch("o2345_mesh_intersect_workspace_bytes", (nv, nt), dev, "mesh_intersect")
        g = ops.mesh_distance_grid(mv, mt)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        hits = torch.empty(nt, dtype=torch.int32, device=dev)
        report = ops.mesh_intersections(mv, mt)
        pairs = torch.empty(max(report["pairs"], 1), 2, dtype=torch.int32, device=dev)
        count = lambda gp, gb, gm: ops.call("o2345_mesh_intersect_count", mv, mt, ib, nv, nt, gp, gb, gm, ws, wsb, counts, hits)
        row = {"vertices": nv, "triangles": nt, "workspace_bytes": wsb, "grid_dims": list(g.dims), "grid_entries": g.entries, "report": report,
               "count_kernels_ms": timed(lambda: count(g.buffer, g.buffer.numel(), g.max_cells), True)}
        if report["pairs"]:
            row["emit_kernels_ms"] = timed(lambda: ops.call("o2345_mesh_intersect_emit", mv, mt, ib, nv, nt, g.buffer, g.buffer.numel(), g.max_cells, ws,
                                                            report["pairs"], pairs), True)
        if nt <= mesh_io.INTERSECT_EXHAUSTIVE_MAX:
            row["exhaustive_count_kernels_ms"] = timed(lambda: count(None, 0, 0), True)
            assert ops.intersect_info(counts.tolist(), nv) == report
        row["ops_mesh_distance_grid_ms"] = timed(lambda: ops.mesh_distance_grid(mv, mt), False)
        row["ops_mesh_intersections_ms"] = timed(lambda: ops.mesh_intersections(mv, mt), False)
        aws, awsb = ops._scratch("o2345_mesh_audit_workspace_bytes", (nv, nt), dev, "mesh_audit")
        stats = ops._stats_block("O2345AuditStats", dev)
        row["audit_kernels_ms"] = timed(lambda: ops.call("o2345_mesh_audit", mv, mt, ib, nv, nt, aws, awsb, stats, None, None, None), True)
        res[name] = row
    print(json.dumps(res))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", nargs="?")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--pairs", action="store_true")
    ap.add_argument("--require-none", action="store_true")
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
        out = mesh_io.mesh_intersections(v, f, a.pairs)
    else:
        out = importlib.import_module("one-2-3-45_amd.pipeline").mesh_intersections((v, f), a.pairs)
    out.pop("face_hits", None)
    if a.pairs:
        pl = out["pairs_list"]
        out["pairs_list"] = (pl if hasattr(pl, "tolist") and not hasattr(pl, "cpu") else pl.cpu()).tolist()
    if a.json:
        print(json.dumps(out))
    else:
        for k in mesh_io.INTERSECT_COUNTS[2:]:
            print(f"{k:12s} {out[k]}")
        for t, u in out.get("pairs_list", ()):
            print(t, u)
    if a.require_none and out["pairs"]:
        sys.exit(1)
    return out


if __name__ == "__main__":
    main()
