"""Distance between two mesh files as surfaces: Chamfer, Hausdorff, and precision / recall / F-score at distance thresholds, printed as JSON.

    python tools/mesh_distance.py A B [--spacing s] [--threshold t ...] [--host]

A is the mesh under test, B the reference; ``.ply``, ``.glb`` and ``.obj`` as this package writes them.  Where one file is a PLY and the other an asset,
the PLY's mesh is brought into the asset frame first (y and z exchanged, faces reversed: an isometry).  Distances are in the files' own units.
``--spacing``: a surface sample every s units (default: one per triangle); ``--threshold`` may be given up to 8 times.  Runs on the GPU
(pipeline.mesh_distance); ``--host`` uses the numpy twin (mesh_io.mesh_distance: brute force, for small meshes or a machine without a GPU).
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
    a = ap.parse_args(argv)
    mesh_io = importlib.import_module("one-2-3-45_amd.mesh_io")
    if a.host:
        out = mesh_io.compare_mesh_files(a.a, a.b, a.spacing, a.threshold)
    else:
        pipeline = importlib.import_module("one-2-3-45_amd.pipeline")
        ma, mb = mesh_io.load_mesh_pair(a.a, a.b)
        out = pipeline.mesh_distance(ma, mb, a.spacing, a.threshold)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
