"""Times the mesh distance (csrc/mesh_distance.hip) on the GPU on two inputs, each a mesh against its ``decimate_cell=2`` version: the stored small scene's
mesh (tests/golden, 64^3 lattice) and BASELINE config 2's scene at a 256^3 lattice.  A = the decimated mesh, B = the plain one; samples every 0.5 grid
spacings, as pipeline.reconstruct_folder's ``mesh_error`` report takes them.

  per direction   samples (count + emit, host clock: the count synchronises), grid (count + emit, host clock), grid query and summary (HIP events), the
                  exhaustive query (HIP events) on all samples where one launch stays under 10 s by the rate of a 4,096-sample launch, else on that
                  sub-sample, with the grid query on the same sub-sample next to it, and the host twin's brute force on a stated sub-sample, extrapolated
  whole           ops.mesh_distance, and marching cubes + ops.mesh_distance: what ``mesh_error=True`` adds to reconstruct_folder
  --align         instead of the above: the alignment (csrc/mesh_align.hip) of the decimated mesh A onto the plain mesh B moved by 170 degrees about z,
                  scale 0.8, shift (0.3, -0.2, 0.1): ops.mesh_align with 8 azimuth candidates as a whole (host clock), one o2345_mesh_align_step at K = 8
                  (the candidates' starting transforms) and at K = 1 (the result) (HIP events; the step's own check of the transforms synchronises
                  inside), and next to each the grid query (o2345_mesh_distance_query) on the same K n moved points, with the ratio step / query
Medians over --reps calls after --warmup calls.  Prints one JSON line.

    python tools/time_mesh_distance.py [--reps 5] [--warmup 2] [--volume 128] [--grid 256] [--skip-small] [--skip-large] [--align]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402

pipeline = bench.pipeline
ops = importlib.import_module("one-2-3-45_amd.ops")
mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
build = importlib.import_module("one-2-3-45_amd.build")
SUB = 4096


def timed(fn, reps, warmup, events):
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


def direction(src, dst, reps, warmup, twin_samples):
    """samples of mesh ``src`` against mesh ``dst``"""
    (sv, st), (tv, tt) = src, dst
    pts, w, _ = ops.mesh_surface_samples(sv, st, pipeline.MESH_ERROR_SPACING)
    grid = ops.mesh_distance_grid(tv, tt)
    n, nt = pts.shape[0], tt.shape[0]
    out = {"samples": n, "source_triangles": st.shape[0], "target_triangles": nt, "grid_dims": grid.dims, "grid_cell": grid.cell, "grid_entries": grid.entries}
    out["samples_ms"] = timed(lambda: ops.mesh_surface_samples(sv, st, pipeline.MESH_ERROR_SPACING), reps, warmup, False)
    out["grid_ms"] = timed(lambda: ops.mesh_distance_grid(tv, tt), reps, warmup, False)
    out["grid_query_ms"] = timed(lambda: ops.mesh_closest_triangle(pts, tv, tt, grid), reps, warmup, True)
    d2, nearest = ops.mesh_closest_triangle(pts, tv, tt, grid)
    out["summary_ms"] = timed(lambda: ops.mesh_distance_stats(d2, nearest, w, pipeline.MESH_ERROR_THRESHOLDS, target=(tv, tt)), reps, warmup, True)
    sub = pts[:SUB].contiguous()
    probe = timed(lambda: ops.mesh_closest_triangle(sub, tv, tt), 1, 1, True)["median_ms"]
    # the probe's 16 blocks run side by side; a full launch runs at least 256 blocks at a time: a pessimistic guess, good enough for the 10 s rule
    out["exhaustive_estimate_ms"] = probe * max(1.0, -(-n // 256) / 256.0)
    full = out["exhaustive_estimate_ms"] <= 10e3
    q = pts if full else sub
    out["exhaustive_query_ms"] = timed(lambda: ops.mesh_closest_triangle(q, tv, tt), max(1, reps // 2), 1, True)
    out["exhaustive_query_samples"] = q.shape[0]
    ex = ops.mesh_closest_triangle(q, tv, tt)
    gr = ops.mesh_closest_triangle(q, tv, tt, grid)
    out["grid_equals_exhaustive"] = bool(torch.equal(ex[0].view(torch.int64), gr[0].view(torch.int64)) and torch.equal(ex[1], gr[1]))
    if not full:
        out["grid_query_on_that_sub_sample_ms"] = timed(lambda: ops.mesh_closest_triangle(q, tv, tt, grid), reps, warmup, True)
    m = min(twin_samples, n)
    hp, hv, hf = pts[:m].cpu().numpy(), tv.cpu().numpy(), tt.cpu().numpy()
    t0 = time.perf_counter()
    mesh_io.closest_triangles(hp, hv, hf, chunk=max(1, min(256, (1 << 22) // max(1, nt))))
    ms = (time.perf_counter() - t0) * 1e3
    out["host_twin"] = {"samples": m, "ms": ms, "extrapolated_to_all_samples_ms": ms * n / max(1, m)}
    return out


def pair(plain, dec, u, reps, warmup, twin_samples):
    res = {"a_to_b": direction(dec, plain, reps, warmup, twin_samples), "b_to_a": direction(plain, dec, reps, warmup, twin_samples)}
    whole = lambda: ops.mesh_distance(dec[0], dec[1], plain[0], plain[1], pipeline.MESH_ERROR_SPACING, pipeline.MESH_ERROR_THRESHOLDS)
    res["report"] = {k: v for k, v in whole().items() if k not in ("a_to_b", "b_to_a")}
    res["mesh_distance_ms"] = timed(whole, reps, warmup, False)
    res["mesh_error_adds_ms"] = timed(lambda: (ops.marching_cubes(u, 0.0), whole()), reps, warmup, False)
    return res


def alignment(plain, dec, reps, warmup):
    """A = the decimated mesh, B = the plain mesh under the large move"""
    import numpy as np
    (av, at), (pv, pt) = dec, plain
    c, s = np.cos(np.deg2rad(170.0)), np.sin(np.deg2rad(170.0))
    move = np.array([[0.8 * c, -0.8 * s, 0.0, 0.3], [0.8 * s, 0.8 * c, 0.0, -0.2], [0.0, 0.0, 0.8, 0.1]])
    bv, bt = ops.mesh_transform(pv, move), pt
    cand = mesh_io.rotation_candidates(8)
    whole = lambda: ops.mesh_align(av, at, bv, bt, pipeline.MESH_ERROR_SPACING, candidates=cand)
    res = whole()
    out = {"source_triangles": at.shape[0], "target_triangles": bt.shape[0],
           "result": {k: res[k] for k in ("scale", "score", "rms", "inlier_fraction", "iterations", "converged", "candidate", "candidate_scores")}}
    out["mesh_align_ms"] = timed(whole, reps, warmup, False)
    calls = []                                                        # the transforms of every step of one run: the first is the K = 8 start
    step = ops.mesh_align_stepper(av, at, bv, bt, pipeline.MESH_ERROR_SPACING)

    def recording(side, T, pivot, tau, target):
        if target:
            calls.append((T.copy(), np.array(pivot)))
        return step(side, T, pivot, tau, target)
    mesh_io.align_run(recording, candidates=cand)
    out["steps_of_one_run"] = len(calls)
    pts, w, _ = ops.mesh_surface_samples(av, at, pipeline.MESH_ERROR_SPACING)
    grid = ops.mesh_distance_grid(bv, bt)
    out["samples"] = pts.shape[0]
    for name, (T, pivot) in (("k8_start", calls[0]), ("k1_result", calls[-1])):
        Td = torch.from_numpy(np.ascontiguousarray(T)).to(pts.device)
        moved = ops.mesh_align_step(pts, w, Td, (bv, bt), grid, None, pivot, want=("moved",))[1]["moved"].view(-1, 3).contiguous()
        t_step = timed(lambda: ops.mesh_align_step(pts, w, Td, (bv, bt), grid, None, pivot), reps, warmup, True)
        t_query = timed(lambda: ops.mesh_closest_triangle(moved, bv, bt, grid), reps, warmup, True)
        out[name] = {"transforms": int(T.shape[0]), "points": moved.shape[0], "step_ms": t_step, "query_ms": t_query,
                     "step_over_query": t_step["median_ms"] / t_query["median_ms"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--volume", type=int, default=128)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--skip-small", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--align", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"sources_sha": build.sources_sha(), "spacing": pipeline.MESH_ERROR_SPACING, "thresholds": list(pipeline.MESH_ERROR_THRESHOLDS)}
    if not a.skip_small:
        from mesh_scene_util import args, stored_scene
        S = stored_scene(dev)
        v, t, _, u = pipeline.extract_mesh(*args(S), return_index_verts=True)
        dv, dt, _, _ = pipeline.extract_mesh(*args(S), return_index_verts=True, decimate_cell=2)
        res["small_scene_64"] = alignment((v, t), (dv, dt), a.reps, a.warmup) if a.align else pair((v, t), (dv, dt), u, a.reps, a.warmup, twin_samples=4096)
    if not a.skip_large:
        wt = pipeline.SceneWeights(dev, seed=0)
        inp = bench.make_inputs(dev, 8, 0, 1)
        vol = pipeline.build_volume(wt, inp["imgs"], inp["aff"], inp["origin"], a.volume, 2.0 / (a.volume - 1))
        v, t, _, u = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], a.grid, return_index_verts=True)
        dv, dt, _, _ = pipeline.extract_mesh(wt, vol, inp["proj"], inp["cam_pos"], a.grid, return_index_verts=True, decimate_cell=2)
        res[f"bench_scene_{a.grid}"] = alignment((v, t), (dv, dt), a.reps, a.warmup) if a.align else pair((v, t), (dv, dt), u, a.reps, a.warmup, twin_samples=64)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
