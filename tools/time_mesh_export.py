"""Times the mesh export stage on the GPU: PLY (the baseline, unchanged code) against GLB and OBJ packed on the device, and against the host OBJ writers
fed the same arrays.  Two meshes: BASELINE config 2 (8 views, 128^3 volume, 256^3 grid) and the 512^3 grid of the config-5 shape (256^3 volume).

  stage_ms   fields on the device -> file on a tmpfs path: packing kernels + D2H copies + file write, host clock around a call that ends synchronised
  whole_ms   pipeline.export_mesh_ply / export_mesh_asset: SDF lattice + marching cubes + vertex colours + the stage above
  kernel_ms  the packing kernels alone, HIP events
Medians over --reps calls after --warmup calls; the ratio against the PLY of the SAME run is what to read.  Prints one JSON line.

    python tools/time_mesh_export.py [--reps 9] [--warmup 3] [--skip-512]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pipeline = bench.pipeline
ops = importlib.import_module("one-2-3-45_amd.ops")
mio = importlib.import_module("one-2-3-45_amd.mesh_io")


def med(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def med_events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def one_mesh(dev, wt, tmp, D, R, ray_scale, a, numpy_writer):
    inp = bench.make_inputs(dev, 8, 0, ray_scale)
    vol = pipeline.build_volume(wt, inp["imgs"], inp["aff"], inp["origin"], D, 2.0 / (D - 1))
    _, verts_idx, tris, rgb, _, g = pipeline._mesh_fields(wt, vol, inp["proj"], inp["cam_pos"], R)
    n, m = int(verts_idx.shape[0]), int(tris.shape[0])
    P = lambda e: os.path.join(tmp, "mesh" + e)
    res = {"volume": D, "grid": R, "vertices": n, "triangles": m}
    stage = {
        "ply": lambda: mio.export_mesh(P(".ply"), verts_idx, tris, R, vertex_colors=rgb),
        "glb": lambda: mio.export_asset(P(".glb"), verts_idx, tris, R, vertex_colors=rgb),
        "obj": lambda: mio.export_asset(P(".obj"), verts_idx, tris, R, vertex_colors=rgb),
        "glb_normals": lambda: mio.export_asset(P("_n.glb"), verts_idx, tris, R, vertex_colors=rgb, normals=g),
    }
    # alternate the variants inside one loop: drift of the shared host hits all of them alike
    for fn in stage.values():
        for _ in range(a.warmup):
            fn()
    acc = {k: [] for k in stage}
    for _ in range(a.reps):
        for k, fn in stage.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc[k].append((time.perf_counter() - t0) * 1e3)
    res["stage_ms"] = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in acc.items()}
    res["stage_ratio_to_ply"] = {k: res["stage_ms"][k]["median_ms"] / res["stage_ms"]["ply"]["median_ms"] for k in stage}
    res["file_bytes"] = {k: os.path.getsize(P(e)) for k, e in (("ply", ".ply"), ("glb", ".glb"), ("obj", ".obj"))}
    # host OBJ writers from the same arrays (already on the host: the copy is not part of their time)
    pos, rgba, _, idx, bounds = ops.mesh_asset_pack(verts_idx, tris, R, rgb=rgb)
    h_pos, h_rgba, h_idx = (t.cpu().numpy() for t in (pos, rgba, idx))
    res["host_write_obj_ms"] = med(lambda: mio.write_obj(P("_host.obj"), h_pos, h_idx.view(np.uint32), h_rgba), max(3, a.reps // 3), 1)
    if numpy_writer:
        t0 = time.perf_counter()
        mio.write_obj_numpy(P("_numpy.obj"), h_pos, h_idx.view(np.uint32), h_rgba)
        res["host_write_obj_numpy_ms_once"] = (time.perf_counter() - t0) * 1e3
        assert open(P("_numpy.obj"), "rb").read() == open(P(".obj"), "rb").read() == open(P("_host.obj"), "rb").read()
    # kernels alone
    K = mio.obj_coordinate_digits(bounds.cpu().numpy())
    res["kernel_ms"] = {
        "ply_pack": med_events(lambda: ops.mesh_pack(verts_idx, tris, R, rgb=rgb), a.reps, a.warmup),
        "asset_pack": med_events(lambda: ops.mesh_asset_pack(verts_idx, tris, R, rgb=rgb), a.reps, a.warmup),
        "asset_pack_normals": med_events(lambda: ops.mesh_asset_pack(verts_idx, tris, R, rgb=rgb, grad=g), a.reps, a.warmup),
        "obj_text": med_events(lambda: ops.obj_text(pos, idx, rgba, None, K=K), a.reps, a.warmup),
    }
    whole = {
        "ply": lambda: pipeline.export_mesh_ply(P(".ply"), wt, vol, inp["proj"], inp["cam_pos"], R),
        "glb": lambda: pipeline.export_mesh_asset(P(".glb"), wt, vol, inp["proj"], inp["cam_pos"], R),
        "obj": lambda: pipeline.export_mesh_asset(P(".obj"), wt, vol, inp["proj"], inp["cam_pos"], R),
    }
    res["whole_ms"] = {k: med(fn, max(3, a.reps // 3), 1) for k, fn in whole.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-512", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: nothing here can be timed without one"
    dev = torch.device("cuda:0")
    wt = pipeline.SceneWeights(dev, seed=0)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    out = {"tmp_is_tmpfs": shm is not None, "reps": a.reps, "warmup": a.warmup}
    with tempfile.TemporaryDirectory(dir=shm) as tmp:
        out["config2"] = one_mesh(dev, wt, tmp, 128, 256, 2, a, numpy_writer=True)
        if not a.skip_512:
            out["config5_grid"] = one_mesh(dev, wt, tmp, 256, 512, 4, a, numpy_writer=False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
