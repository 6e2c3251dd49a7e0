"""Distance between two mesh files as surfaces: Chamfer, Hausdorff, and precision / recall / F-score at distance thresholds, printed as JSON.

    python tools/mesh_distance.py A B [--spacing s] [--threshold t ...] [--host]
                                      [--align] [--align-azimuths n] [--align-up x,y,z] [--align-no-scale] [--align-max-distance d] [--save-aligned PATH]

A is the mesh under test, B the reference; ``.ply``, ``.glb`` and ``.obj`` as this package writes them.  Where one file is a PLY and the other an asset,
the PLY's mesh is brought into the asset frame first (y and z exchanged, faces reversed: an isometry).  Distances are in the files' own units.
``--spacing``: a surface sample every s units (default: one per triangle); ``--threshold`` may be given up to 8 times.  Runs on the GPU
(pipeline.mesh_distance); ``--host`` uses the numpy twin (mesh_io.mesh_distance: brute force, for small meshes or a machine without a GPU).
``--align`` (implied by the other --align-* options and by --save-aligned): A is first moved onto B by a similarity transform (mesh_align: rotation,
translation, uniform scale unless ``--align-no-scale``), found from ``--align-azimuths`` n (default 8; 1: the identity alone) start rotations about
``--align-up`` (default 0,0,1) and refined point-to-plane; samples farther than ``--align-max-distance`` from B take no part.  The report gains
"alignment"; ``--save-aligned`` writes the moved A (.ply, .glb or .obj by its extension).
"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--spacing", type=float, default=None)
    ap.add_argument("--threshold", type=float, action="append", default=[])
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--align-azimuths", type=int, default=None)
    ap.add_argument("--align-up", type=lambda s: tuple(float(x) for x in s.split(",")), default=None)
    ap.add_argument("--align-no-scale", action="store_true")
    ap.add_argument("--align-max-distance", type=float, default=None)
    ap.add_argument("--save-aligned", default=None)
    a = ap.parse_args(argv)
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    align = None
    if a.align or a.align_azimuths is not None or a.align_up is not None or a.align_no_scale or a.align_max_distance is not None or a.save_aligned:
        n = mesh_io.ALIGN_DEFAULT_AZIMUTHS if a.align_azimuths is None else a.align_azimuths
        align = {"candidates": mesh_io.rotation_candidates(n, (0.0, 0.0, 1.0) if a.align_up is None else a.align_up), "scale": not a.align_no_scale,
                 "max_distance": a.align_max_distance}
    ma, mb = mesh_io.load_mesh_pair(a.a, a.b)
    if a.host:
        out = mesh_io.mesh_distance(*ma, *mb, a.spacing, a.threshold, align=align)
    else:
        pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
        out = pipeline.mesh_distance(ma, mb, a.spacing, a.threshold, align=align)
    if a.save_aligned:
        mesh_io.write_mesh(a.save_aligned, mesh_io.transform_vertices(ma[0], out["alignment"]["transform"]), ma[1])
    out = json.loads(json.dumps(out, default=lambda x: x.tolist()))          # the alignment holds arrays
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
