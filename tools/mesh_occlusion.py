"""Ambient occlusion of a mesh file against itself: how open its faces are.

    python tools/mesh_occlusion.py MESH [--samples 64] [--distance d] [--bias b] [--spacing s] [--flip] [--host] [--json] [--time [--reps 5] [--warmup 2]]

MESH is a ``.ply``, ``.glb`` or ``.obj`` as this package writes them (mesh_io's parsers).  At the surface samples of every face (one at the centroid, or
every ``--spacing``), ``--samples`` cosine-weighted rays about the face normal in stored order (``--flip``: about its negative) are cast up to
``--distance`` (default: the diagonal of the mesh's box); a face's exposure is the share of them that hit nothing.  Prints the area-weighted mean
exposure, its smallest and largest per-face value, the faces that are fully closed and fully open, and the counters (points with a non-finite
coordinate, faces without a normal, rays cast); ``--json`` prints one JSON line instead.  Runs on the GPU (pipeline.mesh_occlusion); ``--host`` uses the
numpy twin (mesh_io.mesh_occlusion), which needs no GPU and tests every ray against every face.

``--time`` also times, with HIP events (median of --reps calls after --warmup), the kernel of one o2345_mesh_occlusion call at the same points through
the mesh's grid and, where the mesh has at most 2^16 faces, without a grid; on the host clock, ops.mesh_distance_grid (its count synchronises).
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


def host_report(mesh_io, v, f, samples, distance, bias, spacing, flip):
    """pipeline.mesh_occlusion's dict from the numpy twins"""
    import numpy as np
    points, weight, triangle = mesh_io.surface_samples(v, f, spacing)
    normals = None
    if flip:
        P = np.asarray(v, np.float64)[np.asarray(f)[triangle]]
        normals = -np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    box = np.asarray(v, np.float64).reshape(-1, 3)
    distance, bias = mesh_io.occlusion_defaults(box.min(0), box.max(0), distance, bias)
    hits, counts = mesh_io.mesh_occlusion(points, v, f, normals=normals, owners=triangle, samples=samples, max_distance=distance, bias=bias)
    value = (float(samples) - hits) / float(samples)
    with np.errstate(invalid="ignore"):
        exposure = np.bincount(triangle, value, len(f)) / np.bincount(triangle, minlength=len(f))
    return dict(exposure=exposure, points=points, triangle=triangle, mean=float((weight * value).sum() / weight.sum()) if weight.sum() > 0 else float("nan"),
                counts=counts, samples=int(samples), max_distance=distance, bias=bias)


def timings(out, v, f, reps, warmup):
    import torch
    ops = importlib.import_module("one-2-3-45_amd.ops")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    dev = out["points"].device
    verts, tris = importlib.import_module("one-2-3-45_amd.pipeline")._device_mesh((v, f), dev)
    n, nv, nt, S = out["points"].shape[0], verts.shape[0], tris.shape[0], out["samples"]
    ib = 8 if tris.dtype == torch.int64 else 4
    table = ops._occlusion_table(S, dev)
    hits, counters = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int64, device=dev)

    def kernel(gp, gb, gm):
        ops.call("o2345_mesh_occlusion", out["points"], None, out["triangle"], n, table, S, out["max_distance"], out["bias"], verts, tris, ib, nv, nt, gp, gb, gm,
                 hits, counters)

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

    g = ops.mesh_distance_grid(verts, tris)
    res = {"rays": n * S, "grid_dims": list(g.dims), "grid_entries": g.entries, "grid_kernel_ms": timed(lambda: kernel(g.buffer, g.buffer.numel(), g.max_cells), True)}
    through_grid = hits.clone()
    if nt <= mesh_io.RAYCAST_EXHAUSTIVE_MAX:
        res["exhaustive_kernel_ms"] = timed(lambda: kernel(None, 0, 0), True)
        assert torch.equal(hits, through_grid)
    res["ops_mesh_distance_grid_ms"] = timed(lambda: ops.mesh_distance_grid(verts, tris), False)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--distance", type=float, default=None)
    ap.add_argument("--bias", type=float, default=None)
    ap.add_argument("--spacing", type=float, default=None)
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    if a.time and a.host:
        ap.error("--time measures the device kernels; drop --host")
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    v, f, _ = mesh_io.read_mesh(a.mesh)
    if a.host:
        out = host_report(mesh_io, v, f, a.samples, a.distance, a.bias, a.spacing, a.flip)
        exposure = out["exposure"]
    else:
        out = importlib.import_module("one-2-3-45_amd.pipeline").mesh_occlusion((v, f), a.samples, a.distance, a.bias, a.spacing, a.flip)
        exposure = out["exposure"].cpu().numpy()
    seen = exposure[exposure == exposure]                                    # a face without a sample has no value
    report = {"faces": int(len(f)), "points": int(out["points"].shape[0]), "samples": out["samples"], "max_distance": out["max_distance"], "bias": out["bias"],
              "mean_exposure": out["mean"], "min_exposure": float(seen.min()) if seen.size else None, "max_exposure": float(seen.max()) if seen.size else None,
              "closed_faces": int((seen == 0.0).sum()), "open_faces": int((seen == 1.0).sum()), **out["counts"]}
    if a.time:
        report["time"] = timings(out, v, f, a.reps, a.warmup)
    if a.json:
        print(json.dumps(report))
    else:
        for k, x in report.items():
            print(f"{k:14s} {x}")
    return report


if __name__ == "__main__":
    main()
