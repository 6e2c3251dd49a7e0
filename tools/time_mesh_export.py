"""Times the mesh export stage on the GPU: PLY (the baseline, unchanged code) against GLB and OBJ packed on the device, and against the host OBJ writers
fed the same arrays.  Two meshes: BASELINE config 2 (8 views, 128^3 volume, 256^3 grid) and the 512^3 grid of the config-5 shape (256^3 volume).

  stage_ms   fields on the device -> file on a tmpfs path: packing kernels + D2H copies + file write, host clock around a call that ends synchronised
  whole_ms   pipeline.export_mesh_ply / export_mesh_asset: SDF lattice + marching cubes + vertex colours + the stage above
  kernel_ms  the packing kernels alone, HIP events
  components the component filter (csrc/mesh_components.hip, keep_largest) on the config's mesh: its kernels alone (HIP events around the two-call
             protocol, which synchronises once in the middle) next to marching cubes on the same field, the gradient + colour time with and without
             it, and the filtered stage / whole-export variants inside the same alternating loops as the unfiltered ones
  smooth     Taubin smoothing (csrc/mesh_smooth.hip), 10 iterations with the config's factors, on the config's mesh: the adjacency build alone (two-call
             protocol, one synchronisation), the 20 step launches alone on a table built before, the whole op, the host twin (mesh_io.smooth_vertices,
             host clock, one call) on the same mesh, and whole-export variants inside the same alternating loop as the unsmoothed ones
  decimate   vertex clustering (csrc/mesh_decimate.hip) at cell 2 on the config's mesh: the sizes out, bytes-equality with the host twin
             (mesh_io.decimate_mesh, host clock, one call), the op alone (HIP events around the two-call protocol, which synchronises once in the
             middle), the gradient + colour time on the decimated vertices next to grad_color_all, and whole-export variants inside the same
             alternating loop as the others
  project    Newton projection onto the SDF's zero set (csrc/mesh_project.hip), 4 iterations, on the config's mesh and on its cell-2 decimation (move
             limit 2): the op alone (HIP events around the queued rounds, the small D2H copy of the counters and its synchronisation), the active
             vertices per round, max |sdf| before -> after, and whole-export variants with and without it, with and without decimation, inside the
             same alternating loop as the others
  texture    the texture atlas (csrc/mesh_texture.hip) of the cell-2 decimation at texel 4 and 8 and of the config's full mesh at texel 4: the texel
             count and image size, the three kernels alone (HIP events), the gradient + colour calls over the texel points, the D2H copy of the
             textured GLB's buffers, mesh_io.png_bytes at zlib levels 0 and 1 (host clock), and whole-export variants textured against
             vertex-coloured inside the same alternating loop as the others
  normal map the tangent-space normal map next to the atlas (k_tex_frames, k_tex_normal_pack in the same unit): the two kernels alone in the texture
             block, and the whole export with the map next to the textured one (glb_decimate2_texture4_normal against glb_decimate2_texture4)
  simplify   quadric-error edge collapse (csrc/mesh_simplify.hip) of the config's mesh down to the face count clustering reached at cell 2: the rounds and
             the collapses of each, bytes-equality with the host twin (mesh_io.simplify_mesh, host clock, one call), the op as a whole (HIP events; it
             synchronises once per round), ops.mesh_distance of the result against the raw mesh in both directions next to the same numbers for the
             cell-2 clustering, each also after 4 projection rounds, and whole-export variants inside the same alternating loop as the others
Medians over --reps calls after --warmup calls; the ratio against the PLY of the SAME run is what to read.  Prints one JSON line.

    python tools/time_mesh_export.py [--reps 9] [--warmup 3] [--skip-512] [--whole glb_decimate2_texture4,glb_decimate2_texture4_normal]

--whole NAMES times only the named whole-export variants (those that need no simplification target) and skips every other block.
"""
import argparse
import ctypes
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
config = importlib.import_module("one-2-3-45_amd.config")
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
    if a.whole:
        whole = whole_variants(lambda e: os.path.join(tmp, "mesh" + e), (wt, vol, inp["proj"], inp["cam_pos"], R), None)
        return {"volume": D, "grid": R, "whole_ms": time_whole({k: whole[k] for k in a.whole.split(",")}, a.reps)}
    _, verts_idx, tris, rgb, u, g, _, _ = pipeline._mesh_fields(wt, vol, inp["proj"], inp["cam_pos"], R, config.mesh_options())
    n, m = int(verts_idx.shape[0]), int(tris.shape[0])
    _, f_verts, f_tris, f_rgb, _, _, cc, _ = pipeline._mesh_fields(wt, vol, inp["proj"], inp["cam_pos"], R, config.mesh_options(keep_largest=True))
    cc = {k: cc[k] for k in ("components", "components_kept")}
    P = lambda e: os.path.join(tmp, "mesh" + e)
    res = {"volume": D, "grid": R, "vertices": n, "triangles": m}
    stage = {
        "ply": lambda: mio.export_mesh(P(".ply"), verts_idx, tris, R, vertex_colors=rgb),
        "glb": lambda: mio.export_asset(P(".glb"), verts_idx, tris, R, vertex_colors=rgb),
        "obj": lambda: mio.export_asset(P(".obj"), verts_idx, tris, R, vertex_colors=rgb),
        "glb_normals": lambda: mio.export_asset(P("_n.glb"), verts_idx, tris, R, vertex_colors=rgb, normals=g),
        "ply_largest": lambda: mio.export_mesh(P("_l.ply"), f_verts, f_tris, R, vertex_colors=f_rgb),
        "glb_largest": lambda: mio.export_asset(P("_l.glb"), f_verts, f_tris, R, vertex_colors=f_rgb),
        "obj_largest": lambda: mio.export_asset(P("_l.obj"), f_verts, f_tris, R, vertex_colors=f_rgb),
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
    # the component filter: kernels alone next to marching cubes on the same field, and what it saves downstream (gradient + colours of dropped vertices)
    def grad_color(vi):
        pts = (vi / (R - 1.0) * 2.0 - 1.0).to(torch.float32).contiguous()
        gg = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], pts, variant=2, precision=wt.sdf_precision)["grad"]
        x3 = wt.color_precision == "f16x3"
        ops.color_points(wt.color_xblob if x3 else wt.color_mblob, vol["vol_cl"], vol["maskvol"], vol["cmaps"], inp["proj"], inp["cam_pos"], pts, normals=gg,
                         want_nviews=False, mfma="x3" if x3 else True)
    res["components"] = dict(cc, vertices_kept=int(f_verts.shape[0]), triangles_kept=int(f_tris.shape[0]), kernel_ms={
        "marching_cubes": med_events(lambda: ops.marching_cubes(u, 0.0), a.reps, a.warmup),
        "filter_keep_largest": med_events(lambda: ops.mesh_filter_components(verts_idx, tris, keep_largest=True), a.reps, a.warmup),
        "labels_only": med_events(lambda: ops.mesh_component_labels(tris, n), a.reps, a.warmup),
        "grad_color_all": med_events(lambda: grad_color(verts_idx), a.reps, a.warmup),
        "grad_color_kept": med_events(lambda: grad_color(f_verts), a.reps, a.warmup),
    })
    # Taubin smoothing, 10 iterations: table, steps, both; the host twin on the same arrays as the yardstick
    L = importlib.import_module("one-2-3-45_amd._lib").lib()
    offsets, neighbours, boundary = ops.mesh_vertex_adjacency(tris, n)
    s_tmp, s_out = torch.empty_like(verts_idx), torch.empty_like(verts_idx)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    def steps():
        rc = L.o2345_mesh_smooth(ptr(verts_idx), n, ptr(offsets), ptr(neighbours), ptr(boundary) if config.mesh_smooth_pin_boundary() else None, IT,
                                 config.mesh_smooth_lambda(), config.mesh_smooth_mu(), ptr(s_tmp), ptr(s_out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.o2345_last_error()
    hv, hf = verts_idx.cpu().numpy(), tris.cpu().numpy()
    t0 = time.perf_counter()
    mio.vertex_adjacency(hf, n)
    t1 = time.perf_counter()
    twin = mio.smooth_vertices(hv, hf, IT, config.mesh_smooth_lambda(), config.mesh_smooth_mu(), config.mesh_smooth_pin_boundary())
    t2 = time.perf_counter()
    deg = (offsets[1:] - offsets[:-1])
    res["smooth"] = {"iterations": IT, "entries": int(neighbours.shape[0]), "max_degree": int(deg.max()) if n else 0, "boundary_vertices": int(boundary.sum()),
                     "equals_host_twin": ops.mesh_smooth(verts_idx, tris, IT).cpu().numpy().tobytes() == twin.tobytes(),
                     "kernel_ms": {"adjacency": med_events(lambda: ops.mesh_vertex_adjacency(tris, n), a.reps, a.warmup),
                                   "steps": med_events(steps, a.reps, a.warmup),
                                   "mesh_smooth": med_events(lambda: ops.mesh_smooth(verts_idx, tris, IT), a.reps, a.warmup)},
                     "host_adjacency_ms_once": (t1 - t0) * 1e3, "host_twin_ms_once": (t2 - t1) * 1e3}
    # decimation at cell 2: the op alone, the host twin on the same arrays, and the gradient + colour work that is left
    d_verts, d_tris, _, d_info = ops.mesh_decimate(verts_idx, tris, CELL)
    t0 = time.perf_counter()
    twin = mio.decimate_mesh(hv, hf, CELL)
    t1 = time.perf_counter()
    res["decimate"] = dict(d_info, cell=CELL, largest_cluster=int(np.bincount(twin[3][twin[3] >= 0]).max()) if d_info["vertices"] else 0,
                           equals_host_twin=bool(d_verts.cpu().numpy().tobytes() == twin[0].tobytes() and np.array_equal(d_tris.cpu().numpy(), twin[1])
                                                 and d_info == twin[4]),
                           kernel_ms={"mesh_decimate": med_events(lambda: ops.mesh_decimate(verts_idx, tris, CELL), a.reps, a.warmup),
                                      "grad_color_all": med_events(lambda: grad_color(verts_idx), a.reps, a.warmup),
                                      "grad_color_decimated": med_events(lambda: grad_color(d_verts), a.reps, a.warmup)},
                           host_twin_ms_once=(t1 - t0) * 1e3)
    # projection onto the zero set, 4 rounds: the op alone on the marching-cubes vertices and on the decimated ones
    proj_op = lambda v, mm: ops.mesh_project(wt.sdf_blob, vol["vol_cl"], v, R, PIT, max_move=mm, precision=wt.sdf_precision)
    res["project"] = {"iterations": PIT}
    for key, v, mm in (("all", verts_idx, 1.0), ("decimated", d_verts, max(1.0, CELL))):
        res["project"][key] = dict(proj_op(v, mm)[1], vertices=int(v.shape[0]), max_move=mm, mesh_project_ms=med_events(lambda: proj_op(v, mm), a.reps, a.warmup))
    # edge collapse down to clustering's face count: the op, the twin, and both results as surfaces against the raw mesh
    TARGET = int(d_info["triangles"])
    s_verts, s_tris, _, _, s_info = ops.mesh_simplify(verts_idx, tris, TARGET)
    t0 = time.perf_counter()
    twin = mio.simplify_mesh(hv, hf, TARGET)
    t1 = time.perf_counter()

    def error_to_raw(v, t):
        d = ops.mesh_distance(v, t, verts_idx, tris, 0.5, (0.25, 0.5, 1.0, 2.0))
        return {"a_to_b": {k: d["a_to_b"][k] for k in ("mean", "max")}, "b_to_a": {k: d["b_to_a"][k] for k in ("mean", "max")}, "chamfer": d["chamfer"],
                "fscore": d["fscore"], "vertices": int(v.shape[0]), "triangles": int(t.shape[0])}
    res["simplify"] = dict(s_info, target=TARGET,
                           equals_host_twin=bool(s_verts.cpu().numpy().tobytes() == twin[0].tobytes() and np.array_equal(s_tris.cpu().numpy(), twin[1])
                                                 and s_info == twin[5]),
                           kernel_ms={"mesh_simplify": med_events(lambda: ops.mesh_simplify(verts_idx, tris, TARGET), a.reps, a.warmup),
                                      "mesh_decimate": med_events(lambda: ops.mesh_decimate(verts_idx, tris, CELL), a.reps, a.warmup),
                                      "adjacency": med_events(lambda: ops.mesh_vertex_adjacency(tris, n), a.reps, a.warmup),
                                      "grad_color_simplified": med_events(lambda: grad_color(s_verts), a.reps, a.warmup)},
                           host_twin_ms_once=(t1 - t0) * 1e3,
                           error_to_raw={"collapse": error_to_raw(s_verts, s_tris), "cluster": error_to_raw(d_verts, d_tris),
                                         "collapse_project4": error_to_raw(proj_op(s_verts, 1.0)[0], s_tris),
                                         "cluster_project4": error_to_raw(proj_op(d_verts, max(1.0, CELL))[0], d_tris)})
    # the texture atlas: kernels alone, the network calls over the texels, the copy and the PNG
    def grad_color_pts(pts):
        gg = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], pts, variant=2, precision=wt.sdf_precision)["grad"]
        x3 = wt.color_precision == "f16x3"
        return ops.color_points(wt.color_xblob if x3 else wt.color_mblob, vol["vol_cl"], vol["maskvol"], vol["cmaps"], inp["proj"], inp["cam_pos"], pts, normals=gg,
                                want_nviews=False, mfma="x3" if x3 else True)[0]
    res["texture"] = {}
    for key, tv, tt, c in (("decimated_texel4", d_verts, d_tris, 4), ("decimated_texel8", d_verts, d_tris, 8), ("all_texel4", verts_idx, tris, 4)):
        lay = mio.texture_layout(int(tt.shape[0]), c)
        _, tworld, _ = ops.mesh_texture_points(tv, tt, c, R)
        trgb = grad_color_pts(tworld)
        tgrad = ops.sdf_mlp(wt.sdf_blob, vol["vol_cl"], tworld, variant=2, precision=wt.sdf_precision)["grad"]
        image = ops.mesh_texture_pack(trgb, int(tt.shape[0]), c)
        bufs = [image] + [t for t in ops.mesh_texture_corners(tv, tt, c, R) if t is not None]
        t_pos, t_uv = bufs[1], bufs[2]
        t_nrm, t_tan, _ = ops.mesh_texture_frames(t_pos, t_uv)
        h_image = image.cpu().numpy()
        png = {}
        for level in (0, 1):
            r = med(lambda: mio.png_bytes(h_image, level), max(3, a.reps // 3), 1)
            png[f"level{level}"] = dict(r, bytes=len(mio.png_bytes(h_image, level)))
        res["texture"][key] = {
            "triangles": int(tt.shape[0]), "texel": c, "texels": lay["texels"], "width": lay["width"], "height": lay["height"],
            "kernel_ms": {"tex_points": med_events(lambda: ops.mesh_texture_points(tv, tt, c, R, validate=False), a.reps, a.warmup),
                          "tex_pack": med_events(lambda: ops.mesh_texture_pack(trgb, int(tt.shape[0]), c), a.reps, a.warmup),
                          "tex_corners": med_events(lambda: ops.mesh_texture_corners(tv, tt, c, R), a.reps, a.warmup),
                          "tex_frames": med_events(lambda: ops.mesh_texture_frames(t_pos, t_uv), a.reps, a.warmup),
                          "tex_normal_pack": med_events(lambda: ops.mesh_texture_normal_pack(tgrad, t_nrm, t_tan, int(tt.shape[0]), c), a.reps, a.warmup),
                          "grad_color_texels": med_events(lambda: grad_color_pts(tworld), a.reps, a.warmup)},
            "d2h_ms": med(lambda: ops.to_host_numpy(*bufs), a.reps, a.warmup), "png_ms": png}
        del trgb, tgrad, image, bufs, tworld, t_pos, t_uv, t_nrm, t_tan
    res["whole_ms"] = time_whole(whole_variants(P, (wt, vol, inp["proj"], inp["cam_pos"], R), TARGET), a.reps)
    return res


CELL, PIT, IT = 2.0, 4, 10            # one_mesh's decimation cell, projection rounds and smoothing iterations


def whole_variants(P, A, TARGET):
    """name -> call of every whole-export variant; TARGET: the face count of the simplification rows, None to leave them out"""
    whole = {
        "ply": lambda: pipeline.export_mesh_ply(P(".ply"), *A),
        "glb": lambda: pipeline.export_mesh_asset(P(".glb"), *A),
        "obj": lambda: pipeline.export_mesh_asset(P(".obj"), *A),
        "ply_largest": lambda: pipeline.export_mesh_ply(P("_l.ply"), *A, keep_largest=True),
        "glb_largest": lambda: pipeline.export_mesh_asset(P("_l.glb"), *A, keep_largest=True),
        "obj_largest": lambda: pipeline.export_mesh_asset(P("_l.obj"), *A, keep_largest=True),
        "ply_smooth10": lambda: pipeline.export_mesh_ply(P("_s.ply"), *A, smooth_iterations=IT),
        "glb_smooth10": lambda: pipeline.export_mesh_asset(P("_s.glb"), *A, smooth_iterations=IT),
        "obj_smooth10": lambda: pipeline.export_mesh_asset(P("_s.obj"), *A, smooth_iterations=IT),
        "ply_decimate2": lambda: pipeline.export_mesh_ply(P("_d.ply"), *A, decimate_cell=CELL),
        "glb_decimate2": lambda: pipeline.export_mesh_asset(P("_d.glb"), *A, decimate_cell=CELL),
        "obj_decimate2": lambda: pipeline.export_mesh_asset(P("_d.obj"), *A, decimate_cell=CELL),
        "ply_project4": lambda: pipeline.export_mesh_ply(P("_p.ply"), *A, project_iterations=PIT),
        "glb_project4": lambda: pipeline.export_mesh_asset(P("_p.glb"), *A, project_iterations=PIT),
        "ply_decimate2_project4": lambda: pipeline.export_mesh_ply(P("_dp.ply"), *A, decimate_cell=CELL, project_iterations=PIT),
        "glb_decimate2_project4": lambda: pipeline.export_mesh_asset(P("_dp.glb"), *A, decimate_cell=CELL, project_iterations=PIT),
        "glb_decimate2_texture4": lambda: pipeline.export_mesh_asset(P("_dt4.glb"), *A, decimate_cell=CELL, texture_texel=4),
        "glb_decimate2_texture4_normal": lambda: pipeline.export_mesh_asset(P("_dt4n.glb"), *A, decimate_cell=CELL, texture_texel=4, normal_map=True),
        "glb_decimate2_texture8": lambda: pipeline.export_mesh_asset(P("_dt8.glb"), *A, decimate_cell=CELL, texture_texel=8),
        "obj_decimate2_texture4": lambda: pipeline.export_mesh_asset(P("_dt4.obj"), *A, decimate_cell=CELL, texture_texel=4),
        "glb_decimate2_project4_texture4": lambda: pipeline.export_mesh_asset(P("_dpt4.glb"), *A, decimate_cell=CELL, project_iterations=PIT, texture_texel=4),
        "glb_texture4": lambda: pipeline.export_mesh_asset(P("_t4.glb"), *A, texture_texel=4),
    }
    if TARGET is not None:
        whole.update({
            "ply_simplify": lambda: pipeline.export_mesh_ply(P("_q.ply"), *A, simplify_faces=TARGET),
            "glb_simplify": lambda: pipeline.export_mesh_asset(P("_q.glb"), *A, simplify_faces=TARGET),
            "ply_simplify_project4": lambda: pipeline.export_mesh_ply(P("_qp.ply"), *A, simplify_faces=TARGET, project_iterations=PIT),
        })
    return whole


def time_whole(whole, reps):
    """alternated like the stage variants; the spread (min .. max) of each is what a difference between two of them has to exceed"""
    for fn in whole.values():
        fn()
    wacc = {k: [] for k in whole}
    for _ in range(max(3, reps)):
        for k, fn in whole.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wacc[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in wacc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-512", action="store_true")
    ap.add_argument("--whole", default="", help="comma-separated whole-export variants: time only these")
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
