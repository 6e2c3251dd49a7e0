"""Times the surface render (csrc/surface_trace.hip) on the GPU: BASELINE config 2's scene (8 views, 128^3 volume, 256^3 lattice), the 512^2 rays of its
query camera.

  kernel_ms   HIP events around each piece alone: bricks (k_surface_bricks), rays (k_camera_rays), trace with the empty-space skip on and off
              (k_surface_trace; `lookups / samples` next to it), gradient + colours over the hit list, pack (k_surface_pack)
  whole_ms    host clock around pipeline.render_surface, with a fresh lattice and with the lattice passed in as ``u``, and around pipeline.render (the
              NeuS volume render, code this feature does not touch) on the same rays, all three alternated inside one loop
Medians over --reps calls after --warmup calls.  Prints one JSON line.

    python tools/time_surface_render.py [--reps 9] [--warmup 3] [--volume 128] [--grid 256] [--ray-scale 2]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pipeline = bench.pipeline
ops = importlib.import_module("one-2-3-45_amd.ops")


def alternated(variants, reps, warmup, events):
    """{name: fn} -> {name: median ms}: every variant once per round of one loop, so that drift of the shared host hits all of them alike"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    acc = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                acc[k].append(e0.elapsed_time(e1))
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--volume", type=int, default=128)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--ray-scale", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    wt = pipeline.SceneWeights(dev, seed=0)
    inp = bench.make_inputs(dev, 8, 0, a.ray_scale)
    D, R = a.volume, a.grid
    vol = pipeline.build_volume(wt, inp["imgs"], inp["aff"], inp["origin"], D, 2.0 / (D - 1))
    sc = inp["sc"]
    K = np.array(sc["query_intrinsic"], np.float64)
    K[:2] *= a.ray_scale
    c2w = sc["query_c2w"]
    H = W = 256 * a.ray_scale
    args = (wt, vol, inp["proj"], inp["cam_pos"], K, c2w, H, W)
    first = pipeline.render_surface(*args, resolution=R)
    u = first["u"]
    res = {"volume": D, "grid": R, "rays": H * W, "info": first["info"], "stride": pipeline.config.SURFACE_STRIDE, "refine": pipeline.config.SURFACE_REFINE}
    flags = ops.surface_bricks(u, 0.0, True)
    res["bricks_flagged"], res["bricks"] = int(flags.sum().item()), flags.numel()
    ro, rd = ops.camera_rays(K, c2w, H, W, dev)
    trace = lambda skip, hw=(H, W): ops.surface_trace(u, ro, rd, 0.0, 1.0e6, inside_positive=True, flags=flags, skip=skip, image_hw=hw, want_info=False)
    tr = trace(True)
    off = ops.surface_info(trace(False)["stats"].cpu().numpy(), H * W)
    assert {k: v for k, v in off.items() if k != "lookups"} == {k: v for k, v in first["info"].items() if k != "lookups"}
    res["lookups_per_sample"] = {"skip": first["info"]["lookups"] / max(1, first["info"]["samples"]), "no_skip": off["lookups"] / max(1, off["samples"])}
    x3 = wt.color_precision == "f16x3"
    cam = inp["qcam"]

    def shade():
        g = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], tr["point"], variant=2, precision=wt.sdf_precision, index=tr["hits"], n_dev=tr["n_hits"])["grad"]
        rgb, _ = ops.color_points(wt.color_xblob if x3 else wt.color_mblob, vol["vol_cl"], vol["maskvol"], vol["cmaps"], inp["proj"], inp["cam_pos"], tr["point"],
                                  query_cam=cam, index=tr["hits"], n_dev=tr["n_hits"], want_nviews=False, mfma="x3" if x3 else True)
        return rgb, g
    rgb, g = shade()
    res["kernel_ms"] = alternated({
        "bricks": lambda: ops.surface_bricks(u, 0.0, True),
        "rays": lambda: ops.camera_rays(K, c2w, H, W, dev),
        "trace_skip_tiles": lambda: trace(True),
        "trace_skip_rows": lambda: trace(True, None),
        "trace_no_skip_tiles": lambda: trace(False),
        "grad_color_hits": shade,
        "pack": lambda: ops.surface_pack(tr["kind"], tr["depth"], rgb, g, H, W),
    }, a.reps, a.warmup, events=True)
    res["whole_ms"] = alternated({
        "render_surface_fresh_lattice": lambda: pipeline.render_surface(*args, resolution=R),
        "render_surface_given_lattice": lambda: pipeline.render_surface(*args, u=u),
        "volume_render": lambda: pipeline.render(wt, vol, inp["proj"], inp["cam_pos"], inp["rays_o"], inp["rays_d"], inp["near"], inp["far"], inp["qcam"]),
    }, a.reps, a.warmup, events=False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
