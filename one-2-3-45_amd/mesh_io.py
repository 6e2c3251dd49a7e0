"""Mesh serialisation: binary little-endian PLY in the layout trimesh's exporter produces for
``trimesh.Trimesh(vertices, faces[, vertex_colors]).export('x.ply')`` (the reference's models/trainer_generic.py:1302-1303,
1377-1382): vertex = 3 x float32 [+ 4 x uint8 rgba], face = uint8 count + 3 x int32.

``export_mesh`` is the device path: marching-cubes index coordinates, the frame transforms and the uint8 colours are turned into
the two record arrays by csrc/mesh_pack.hip, copied to the host once and written with a single ``write``.
``write_ply`` / ``read_ply`` are the host-side (numpy) file layer, also used by the ``trimesh`` shim.
trimesh itself is not vendored with the reference (requirements.txt); the header text follows its published PLY template.

Asset formats (the reference's utils/utils.py:31-47, convert_mesh_format behind run.py --output_format): binary glTF (``.glb``) and vertex-coloured
Wavefront OBJ (``.obj``) in the asset frame -- (x, y, z) -> (x, z, y), z-up -> glTF's y-up, every face reversed; the reference's two rotations and
x flip compose to exactly that.  ``write_glb`` / ``write_obj`` / ``read_glb`` / ``read_obj`` / ``convert_mesh`` are the host layer (numpy, no GPU) and the
DEFINITION of the two files; ``export_asset`` is the device path (csrc/mesh_export.hip): buffers and OBJ text are produced on the device, one D2H copy
per buffer, one file write.  ``component_labels`` / ``filter_components`` are the host twin (and definition) of the device component filter
(csrc/mesh_components.hip); ``vertex_adjacency`` / ``smooth_vertices`` are the host twin (and definition) of the device adjacency table and Taubin
smoothing (csrc/mesh_smooth.hip).  ``texture_layout`` / ``texture_points`` / ``texture_corners`` / ``pack_texture`` are the host twins (and definition)
of the texture atlas (csrc/mesh_texture.hip); ``png_bytes`` / ``read_png`` its image file, ``write_textured`` / ``read_glb_texture`` / ``read_obj_texture``
the textured GLB and the OBJ + MTL + PNG triple; ``texture_frames`` / ``pack_normal_map`` are the host twins (and definition) of the tangent-space normal
map that goes with the atlas, ``decode_normal_map`` / ``read_glb_normal_map`` / ``read_obj_normal_map`` read it back.  No byte parity with trimesh's own OBJ / GLB writers is claimed (trimesh is not available to compare against)."""
import json
import os
import struct

import numpy as np

_VERTEX = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
_RGBA = [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]
_FACE = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])


def ply_header(n_vertices, n_faces, colors):
    lines = ["ply", "format binary_little_endian 1.0", "comment https://github.com/mikedh/trimesh", f"element vertex {n_vertices}",
             "property float x", "property float y", "property float z"]
    if colors:
        lines += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    lines += [f"element face {n_faces}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


_WARNED = False


def _host_packer(what, instead):
    """-> the binding (_lib) for a host-side packer of the library, or None after one warning.  FILE FORMATTING on the host, not device work: without a
    loadable library (a machine that only converts meshes) the numpy writers produce the same bytes (tests/test_mesh_io.py), 6 - 8 ms slower per million
    PLY records, seconds per million OBJ records.  Every compute op still refuses to run without the library."""
    from . import _lib
    try:
        _lib.lib()
        return _lib
    except (RuntimeError, OSError, AttributeError) as e:
        global _WARNED
        if not _WARNED:
            import warnings
            warnings.warn(f"o2345 mesh_io.{what}: libo2345_hip.so is not loadable ({e}); {instead} (same bytes)")
            _WARNED = True


def write_records(path, vertex_records, face_records, colors):
    """vertex_records / face_records: contiguous uint8 arrays (16 or 12 bytes per vertex, 13 per face)."""
    vertex_records = np.ascontiguousarray(vertex_records, np.uint8).reshape(-1)
    face_records = np.ascontiguousarray(face_records, np.uint8).reshape(-1)
    vs = 16 if colors else 12
    assert vertex_records.size % vs == 0 and face_records.size % 13 == 0
    with open(path, "wb") as f:
        f.write(ply_header(vertex_records.size // vs, face_records.size // 13, colors))
        f.write(vertex_records.data)            # straight from the arrays' buffers: no intermediate bytes objects
        f.write(face_records.data)


def write_ply(path, vertices, faces, vertex_colors=None):
    """Host arrays in (vertices [N,3] float, faces [M,3] int, vertex_colors [N,3|4] uint8 or None).  The two record arrays are packed by the library's
    host-side packer (o2345_ply_records_host: float64 -> float32, int64 -> int32, rgba; a few threads, no device work) -- numpy's 12 -> 13-byte row
    copies took 6 - 8 ms for the 1 M records of a 256^3 mesh, inside the reference's "export mesh time" bracket."""
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    c = None if vertex_colors is None else np.ascontiguousarray(vertex_colors, np.uint8)
    if c is not None and (c.ndim != 2 or c.shape[0] != v.shape[0] or c.shape[1] not in (3, 4)):
        raise ValueError(f"write_ply: vertex_colors must be [N,3] or [N,4] uint8 for N = {v.shape[0]} vertices, got {c.shape}")
    _lib = _host_packer("write_ply", "writing the PLY with the numpy packer")
    if _lib is None:
        return write_ply_numpy(path, v, f, c)
    vrec = np.empty((v.shape[0], 16 if c is not None else 12), np.uint8)
    frec = np.empty((f.shape[0], 13), np.uint8)
    _lib.call("o2345_ply_records_host", v, v.shape[0], c, 0 if c is None else c.shape[1], f, f.shape[0], vrec, frec)
    write_records(path, vrec, frec, c is not None)


def write_ply_numpy(path, vertices, faces, vertex_colors=None):
    """The same file from numpy structured arrays (the definition write_ply is tested against)."""
    vertices = np.asarray(vertices)
    faces = np.asarray(faces)
    dt = np.dtype(_VERTEX + (_RGBA if vertex_colors is not None else []))
    v = np.zeros(vertices.shape[0], dt)
    v["x"], v["y"], v["z"] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    if vertex_colors is not None:
        c = np.asarray(vertex_colors)
        v["red"], v["green"], v["blue"] = c[:, 0], c[:, 1], c[:, 2]
        v["alpha"] = c[:, 3] if c.shape[1] > 3 else 255
    fr = np.zeros(faces.shape[0], _FACE)
    fr["n"] = 3
    fr["idx"] = faces
    write_records(path, v.view(np.uint8), fr.view(np.uint8), vertex_colors is not None)


def read_ply(path):
    """Parser for the files written above -> (vertices float32 [N,3], faces int32 [M,3], colors uint8 [N,4] or None)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    colors = any(l == "property uchar red" for l in head)
    dt = np.dtype(_VERTEX + (_RGBA if colors else []))
    v = np.frombuffer(raw, dt, nv, end)
    f = np.frombuffer(raw, _FACE, nf, end + nv * dt.itemsize)
    assert end + nv * dt.itemsize + nf * 13 == len(raw) and (nf == 0 or (f["n"] == 3).all())
    verts = np.stack([v["x"], v["y"], v["z"]], 1)
    cols = np.stack([v["red"], v["green"], v["blue"], v["alpha"]], 1) if colors else None
    return verts, f["idx"].copy(), cols


def export_mesh(path, verts_idx, tris, grid_R, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None,
                vertex_colors=None):
    """Device path: verts_idx fp64 [N,3] index coordinates and tris [M,3] from ops.marching_cubes, optional fp32 colours in [0,1]
    (ops.color_points) -> PLY file.  scale_mat / trans_mat: 4x4 (numpy or tensor) as in the reference's sample dict."""
    from . import ops
    vrec, frec = ops.mesh_pack(verts_idx, tris, grid_R, bound_min, bound_max, scale_mat, trans_mat, vertex_colors)
    write_records(path, vrec.cpu().numpy(), frec.cpu().numpy(), vertex_colors is not None)
    return int(verts_idx.shape[0]), int(tris.shape[0])


# ------------------------------------------------------------------------------------------------------------------ asset formats (GLB / OBJ)
def to_asset_frame(vertices, faces):
    """PLY frame -> asset frame: y and z exchanged (a reflection), every face reversed (the two cancel: outward faces stay outward)."""
    return np.ascontiguousarray(np.asarray(vertices)[:, [0, 2, 1]]), np.ascontiguousarray(np.asarray(faces)[:, ::-1])


def _rgba(colors, n):
    if colors is None:
        return None
    c = np.ascontiguousarray(colors, np.uint8)
    if c.ndim != 2 or c.shape[0] != n or c.shape[1] not in (3, 4):
        raise ValueError(f"colors must be [N,3] or [N,4] uint8 for N = {n} vertices, got {c.shape}")
    if c.shape[1] == 3:
        c = np.concatenate([c, np.full((n, 1), 255, np.uint8)], 1)
    return c


def _host_mesh(positions, faces, colors, normals):
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= p.shape[0]):
        raise ValueError(f"faces index outside 0 .. {p.shape[0] - 1}")
    nr = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if nr is not None and nr.shape[0] != p.shape[0]:
        raise ValueError(f"normals must be [N,3] for N = {p.shape[0]} vertices, got {nr.shape}")
    return p, f.astype(np.uint32), _rgba(colors, p.shape[0]), nr


_GLB_MAGIC, _GLB_JSON, _GLB_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942


def glb_json(n, m, colors, normals, pos_min, pos_max, texcoords=False, image_bytes=0, tangents=False, normal_image_bytes=0, occlusion_image_bytes=0):
    """The JSON chunk (bytes, space-padded to a multiple of 4): one buffer, views in the order indices / POSITION / COLOR_0 / NORMAL, one accessor per
    view, one mesh with one triangle primitive, one node, one scene.  Fixed key order and separators: the bytes are reproducible.
    ``texcoords`` adds TEXCOORD_0 (VEC2 float32) after NORMAL; ``image_bytes`` > 0 adds a last view without a target that holds a PNG of that many bytes,
    and behind "buffers" the keys "materials" (baseColorTexture, metallic 0, roughness 1), "textures", "images", "samplers" (LINEAR / LINEAR,
    CLAMP_TO_EDGE: what texture_layout's gutters are made for); the primitive then names material 0.  Without the two the bytes are what they were.
    ``tangents`` adds TANGENT (VEC4 float32) after NORMAL; ``normal_image_bytes`` > 0 adds a second PNG view behind the first, "normalTexture": {"index":
    1} in the material and a second entry in "textures" and "images" (same sampler).  The two come together and need normals, texcoords and the first
    image; without them the bytes are, again, what they were.
    ``occlusion_image_bytes`` > 0 adds one more PNG view behind those, "occlusionTexture": {"index": k} as the LAST key of the material and entry k of
    "textures" and "images" (same sampler, the base colour's TEXCOORD_0), k = 2 behind a normal map and 1 without one.  It needs texcoords and the first
    image; without it the bytes are what they were."""
    if bool(tangents) != bool(normal_image_bytes) or (tangents and not (normals and texcoords and image_bytes)):
        raise ValueError("GLB export: a normal map is TANGENT and a second image, next to NORMAL, TEXCOORD_0 and the base colour image")
    if occlusion_image_bytes and not (texcoords and image_bytes):
        raise ValueError("GLB export: an occlusion map is one more image, next to TEXCOORD_0 and the base colour image")
    views, accessors, off = [], [], 0

    def add(nbytes, target, accessor):
        nonlocal off
        views.append({"buffer": 0, "byteOffset": off, "byteLength": nbytes, "target": target})
        accessors.append(dict({"bufferView": len(views) - 1, "byteOffset": 0}, **accessor))
        off += (nbytes + 3) // 4 * 4
        return len(accessors) - 1

    num = lambda a: [float(x) + 0.0 for x in a]                       # + 0.0: one spelling of zero
    indices = add(12 * m, 34963, {"componentType": 5125, "count": 3 * m, "type": "SCALAR"})
    attrs = {"POSITION": add(12 * n, 34962, {"componentType": 5126, "count": n, "type": "VEC3", "min": num(pos_min), "max": num(pos_max)})}
    if colors:
        attrs["COLOR_0"] = add(4 * n, 34962, {"componentType": 5121, "normalized": True, "count": n, "type": "VEC4"})
    if normals:
        attrs["NORMAL"] = add(12 * n, 34962, {"componentType": 5126, "count": n, "type": "VEC3"})
    if tangents:
        attrs["TANGENT"] = add(16 * n, 34962, {"componentType": 5126, "count": n, "type": "VEC4"})
    if texcoords:
        attrs["TEXCOORD_0"] = add(8 * n, 34962, {"componentType": 5126, "count": n, "type": "VEC2"})
    prim = {"attributes": attrs, "indices": indices, "mode": 4}
    if image_bytes:
        views.append({"buffer": 0, "byteOffset": off, "byteLength": int(image_bytes)})
        off += (int(image_bytes) + 3) // 4 * 4
        prim["material"] = 0
    if normal_image_bytes:
        views.append({"buffer": 0, "byteOffset": off, "byteLength": int(normal_image_bytes)})
        off += (int(normal_image_bytes) + 3) // 4 * 4
    if occlusion_image_bytes:
        views.append({"buffer": 0, "byteOffset": off, "byteLength": int(occlusion_image_bytes)})
        off += (int(occlusion_image_bytes) + 3) // 4 * 4
    doc = {"asset": {"version": "2.0", "generator": "o2345-hip"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [{"mesh": 0}],
           "meshes": [{"primitives": [prim]}], "accessors": accessors, "bufferViews": views,
           "buffers": [{"byteLength": off}]}
    if image_bytes:
        doc["materials"] = [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}]
        doc["textures"] = [{"sampler": 0, "source": 0}]
        doc["images"] = [{"bufferView": len(views) - 1 - bool(normal_image_bytes) - bool(occlusion_image_bytes), "mimeType": "image/png"}]
        doc["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
    if normal_image_bytes:
        doc["materials"][0]["normalTexture"] = {"index": 1}
        doc["textures"].append({"sampler": 0, "source": 1})
        doc["images"].append({"bufferView": len(views) - 1 - bool(occlusion_image_bytes), "mimeType": "image/png"})
    if occlusion_image_bytes:
        k = len(doc["textures"])
        doc["materials"][0]["occlusionTexture"] = {"index": k}
        doc["textures"].append({"sampler": 0, "source": k})
        doc["images"].append({"bufferView": len(views) - 1, "mimeType": "image/png"})
    js = json.dumps(doc, separators=(",", ":")).encode("ascii")
    return js + b" " * (-len(js) % 4)


def write_glb_buffers(path, indices, positions, rgba, normals, bounds, uv=None, png=None, tangents=None, normal_png=None, occlusion_png=None):
    """GLB from its buffers as they sit in the file (host arrays: indices uint32 [M,3], positions float32 [N,3], rgba uint8 [N,4] or None, normals
    float32 [N,3] or None; bounds [2,3] = per-axis min, max of positions): 12-byte header, JSON chunk, BIN chunk; every view is a multiple of 4 bytes.
    A textured file also has ``uv`` float32 [N,2] and ``png`` (the bytes of the image, zero-padded to a multiple of 4 in the file), and no ``rgba``.
    A normal map is ``tangents`` float32 [N,4] (behind the normals, which it needs) and ``normal_png``, a second image behind the first.
    ``occlusion_png``: the ambient occlusion map of a textured file, one more image behind those (the material's occlusionTexture)."""
    n, m = positions.shape[0], indices.shape[0]
    if n == 0 or m == 0:
        raise ValueError("GLB export: an empty mesh has no valid glTF form (accessors need count >= 1)")
    if (uv is None) != (png is None) or (uv is not None and rgba is not None):
        raise ValueError("GLB export: a textured file has uv and png and no vertex colours")
    bounds = np.asarray(bounds, np.float32).reshape(2, 3)
    if (tangents is None) != (normal_png is None) or (tangents is not None and (normals is None or uv is None)):
        raise ValueError("GLB export: a normal map is tangents and a second png, in a textured file with normals")
    if occlusion_png is not None and uv is None:
        raise ValueError("GLB export: an occlusion map is one more png in a textured file")
    js = glb_json(n, m, rgba is not None, normals is not None, bounds[0], bounds[1], uv is not None, 0 if png is None else len(png), tangents is not None,
                  0 if normal_png is None else len(normal_png), **({} if occlusion_png is None else {"occlusion_image_bytes": len(occlusion_png)}))
    image, normal_image, occlusion_image = (None if b is None else np.frombuffer(bytes(b) + b"\0" * (-len(b) % 4), np.uint8)
                                            for b in (png, normal_png, occlusion_png))
    if tangents is not None:
        tangents = np.ascontiguousarray(tangents, np.float32).reshape(n, 4)
    if uv is not None:
        uv = np.ascontiguousarray(uv, np.float32).reshape(n, 2)
    parts = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in (indices, positions, rgba, normals, tangents, uv, image, normal_image, occlusion_image)
             if a is not None]
    nbin = sum(a.size for a in parts)
    assert indices.dtype.itemsize == 4 and positions.dtype == np.float32 and nbin % 4 == 0
    with open(path, "wb") as f:
        f.write(struct.pack("<III", _GLB_MAGIC, 2, 12 + 8 + len(js) + 8 + nbin) + struct.pack("<II", len(js), _GLB_JSON) + js + struct.pack("<II", nbin, _GLB_BIN))
        for a in parts:
            f.write(a.data)


def write_glb(path, positions, faces, colors=None, normals=None):
    """Host arrays in (positions [N,3] float, faces [M,3] int, colors [N,3|4] uint8 or None, normals [N,3] float or None), ALREADY in the asset frame."""
    p, f, c, nr = _host_mesh(positions, faces, colors, normals)
    if p.shape[0] == 0 or f.shape[0] == 0:
        raise ValueError("GLB export: an empty mesh has no valid glTF form (accessors need count >= 1)")
    write_glb_buffers(path, f, p, c, nr, np.stack([p.min(0), p.max(0)]))


_GLB_TYPES = {5121: ("u1", 1), 5125: ("<u4", 4), 5126: ("<f4", 4)}
_GLB_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


def read_glb(path):
    """Parser for the files written above -> (positions float32 [N,3], faces int32 [M,3], colors uint8 [N,4] or None, normals float32 [N,3] or None).
    The texture of a textured file: read_glb_texture."""
    return _read_glb(path)[:4]


def read_glb_texture(path):
    """-> (uv float32 [N,2], image uint8 [H,W,4], sampler dict) of a textured file written above, or None for a file without a texture."""
    return _read_glb(path)[4]


def read_glb_normal_map(path):
    """-> (tangents float32 [N,4], image uint8 [H,W,4]) of a file written above with a normal map, or None for a file without one."""
    return _read_glb(path)[5]


def read_glb_occlusion(path):
    """-> the occlusion image uint8 [H,W,4] (the value in every colour channel) of a file written above with one, or None for a file without one."""
    return _read_glb(path)[6]


def _read_glb(path):
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<III", raw, 0)
    assert magic == _GLB_MAGIC and version == 2 and total == len(raw)
    jlen, jtype = struct.unpack_from("<II", raw, 12)
    assert jtype == _GLB_JSON
    doc = json.loads(raw[20:20 + jlen].decode("ascii"))
    blen, btype = struct.unpack_from("<II", raw, 20 + jlen)
    assert btype == _GLB_BIN and 28 + jlen + blen == len(raw)
    base = 28 + jlen

    def accessor(i):
        a = doc["accessors"][i]
        v = doc["bufferViews"][a["bufferView"]]
        dt, _ = _GLB_TYPES[a["componentType"]]
        w = _GLB_WIDTH[a["type"]]
        return np.frombuffer(raw, dt, a["count"] * w, base + v["byteOffset"] + a.get("byteOffset", 0)).reshape(-1, w)

    prim = doc["meshes"][0]["primitives"][0]
    at = prim["attributes"]
    faces = accessor(prim["indices"]).reshape(-1, 3).astype(np.int32)
    texture = normal_map = occlusion = None

    def image_of(tex):
        img = doc["images"][tex["source"]]
        v = doc["bufferViews"][img["bufferView"]]
        assert img["mimeType"] == "image/png" and "target" not in v
        return png_image(raw[base + v["byteOffset"]:base + v["byteOffset"] + v["byteLength"]])

    if "TEXCOORD_0" in at:
        mat = doc["materials"][prim["material"]]
        tex = doc["textures"][mat["pbrMetallicRoughness"]["baseColorTexture"]["index"]]
        texture = (accessor(at["TEXCOORD_0"]).copy(), image_of(tex), doc["samplers"][tex["sampler"]])
        if "normalTexture" in mat:
            assert "TANGENT" in at and "NORMAL" in at
            normal_map = (accessor(at["TANGENT"]).copy(), image_of(doc["textures"][mat["normalTexture"]["index"]]))
        if "occlusionTexture" in mat:
            occlusion = image_of(doc["textures"][mat["occlusionTexture"]["index"]])
    return (accessor(at["POSITION"]).copy(), faces, accessor(at["COLOR_0"]).copy() if "COLOR_0" in at else None,
            accessor(at["NORMAL"]).copy() if "NORMAL" in at else None, texture, normal_map, occlusion)


def obj_coordinate_digits(bounds):
    """K of the OBJ coordinate field: integer digits of the largest |coordinate| once rounded to 8 decimals (at least 1).  ``bounds``: any array holding
    the per-axis min and max (or the coordinates themselves).  Refuses non-finite values and K > 9 (the packers format through a 64-bit integer)."""
    b = np.asarray(bounds, np.float64)
    a = float(np.abs(b).max()) if b.size else 0.0
    if not np.isfinite(a) or a >= 1e9:
        raise ValueError(f"OBJ export: largest |coordinate| {a} is not finite or needs more than 9 integer digits")
    K = len(str(int(np.rint(a * 1e8)) // 10 ** 8))                      # a * 1e8 is exact in fp64 for a float32 a: 24-bit significand x 5^8 < 2^53
    if K > 9:
        raise ValueError(f"OBJ export: largest |coordinate| {a} needs more than 9 integer digits")
    return K


def obj_text_bytes(n, m, K, colors, normals):
    """Closed-form size of the OBJ text (== o2345_obj_text_bytes): every record of a kind has the same length."""
    dn = len(str(int(n)))
    return n * (1 + 3 * (K + 11) + (33 if colors else 0) + 1) + (n * 39 if normals else 0) + m * (1 + 3 * (1 + (2 * dn + 2 if normals else dn)) + 1)


_OBJ_TABLE = None


def obj_color_table():
    """256 x 11 bytes: entry c is " %.8f" % (c / 255) -- the colour field of an OBJ vertex record, formatted once."""
    global _OBJ_TABLE
    if _OBJ_TABLE is None:
        _OBJ_TABLE = np.frombuffer("".join(" %.8f" % (c / 255.0) for c in range(256)).encode("ascii"), np.uint8).reshape(256, 11).copy()
    return _OBJ_TABLE


def obj_text_numpy(positions, indices, rgba, normals, K):
    """The OBJ text from printf-style formatting on the host (the definition the library's packers are tested against): float32 positions / normals
    widened to float64 (exact), "%*.8f" rounds correctly."""
    n, dn, w = positions.shape[0], len(str(positions.shape[0])), K + 10
    vfmt = "v" + (" %%%d.8f" % w) * 3 + (" %.8f" * 3 if rgba is not None else "") + "\n"
    rows = positions.astype(np.float64).tolist()
    if rgba is not None:
        rows = [r + c for r, c in zip(rows, (rgba[:, :3].astype(np.float64) / 255.0).tolist())]
    out = [vfmt % tuple(r) for r in rows]
    if normals is not None:
        out += ["vn %11.8f %11.8f %11.8f\n" % tuple(r) for r in normals.astype(np.float64).tolist()]
    faces = (indices.astype(np.int64) + 1).tolist()
    if normals is not None:
        ffmt = "f" + (" %%%ds" % (2 * dn + 2)) * 3 + "\n"
        out += [ffmt % tuple("%d//%d" % (a, a) for a in r) for r in faces]
    else:
        ffmt = "f" + (" %%%dd" % dn) * 3 + "\n"
        out += [ffmt % tuple(r) for r in faces]
    return "".join(out).encode("ascii")


def write_obj_numpy(path, positions, faces, colors=None, normals=None):
    """The OBJ file from host formatting alone (the definition write_obj and the device path are tested against)."""
    p, f, c, nr = _host_mesh(positions, faces, colors, normals)
    with open(path, "wb") as fh:
        fh.write(obj_text_numpy(p, f, c, nr, obj_coordinate_digits(p)))


def write_obj(path, positions, faces, colors=None, normals=None):
    """Host arrays in (as write_glb), ALREADY in the asset frame -> vertex-coloured OBJ of fixed-width records ("v x y z [r g b]", "vn", "f a b c" or
    "f a//a b//b c//c", 1-based).  The text is packed by the library's host-side packer (o2345_obj_text_host; a few threads, no device work); without a
    loadable library the host formatter writes the same bytes, seconds slower per million records."""
    p, f, c, nr = _host_mesh(positions, faces, colors, normals)
    K = obj_coordinate_digits(p)
    _lib = _host_packer("write_obj", "formatting the OBJ on the host")
    if _lib is None:
        text = obj_text_numpy(p, f, c, nr, K)
    else:
        text = np.empty(obj_text_bytes(p.shape[0], f.shape[0], K, c is not None, nr is not None), np.uint8)
        assert text.size == _lib.call("o2345_obj_text_bytes", p.shape[0], f.shape[0], K, int(c is not None), int(nr is not None))
        _lib.call("o2345_obj_text_host", p, c, nr, p.shape[0], f, f.shape[0], K, text)
        text = text.data
    with open(path, "wb") as fh:
        fh.write(text)


def read_obj(path):
    """Parser for the files written above -> (positions float64 [N,3], faces int32 [M,3] 0-based, colors uint8 [N,3] or None, normals float64 [N,3] or
    None).  Positions stay float64: the decimal text is not the float32 it came from, only within 0.5e-8 of it."""
    v, vn, f = [], [], []
    with open(path, "r", encoding="ascii") as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([float(x) for x in t[1:]])
            elif t[0] == "vn":
                vn.append([float(x) for x in t[1:]])
            elif t[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in t[1:]])
    va = np.asarray(v, np.float64).reshape(len(v), -1) if v else np.zeros((0, 3))
    cols = np.rint(va[:, 3:6] * 255.0).astype(np.uint8) if va.shape[1] >= 6 else None
    return (np.ascontiguousarray(va[:, :3]), np.asarray(f, np.int32).reshape(-1, 3), cols, np.asarray(vn, np.float64).reshape(-1, 3) if vn else None)


def _asset_ext(path):
    ext = os.path.splitext(str(path))[1].lower()
    if ext not in (".glb", ".obj", ".ply"):
        raise ValueError(f"mesh export: format {ext!r} of {path!r} is not one of .ply, .glb, .obj")
    return ext


# ------------------------------------------------------------------------------------------------------------------ connected components
def component_labels(faces, n_vertices):
    """Label of every vertex of an indexed triangle mesh: the smallest vertex index of its connected component (vertices connected through triangles that
    share vertex indices; an unreferenced vertex is its own component).  int32 [n_vertices].  The host twin of ops.mesh_component_labels and the
    DEFINITION of its result.  Hook + pointer jumping: every round hooks each root under the smallest root it shares an edge with, then compresses all
    paths by repeated parent[parent]; the number of components at least halves per round, so the cost does not grow with the mesh diameter (label
    propagation needs one sweep per step of the longest shortest path)."""
    n = int(n_vertices)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64, copy=False)
    if f.size and (f.min() < 0 or f.max() >= n):
        raise ValueError(f"faces index outside 0 .. {n - 1}")
    parent = np.arange(n, dtype=np.int64)
    u = np.concatenate([f[:, 0], f[:, 1]])
    v = np.concatenate([f[:, 1], f[:, 2]])
    while u.size:
        pu, pv = parent[u], parent[v]                                  # roots: every path is fully compressed here
        live = pu != pv
        if not live.any():
            break
        u, v, pu, pv = u[live], v[live], pu[live], pv[live]
        np.minimum.at(parent, np.maximum(pu, pv), np.minimum(pu, pv))  # larger root under the smallest neighbouring root: parent[x] <= x, no cycles
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent.astype(np.int32)


def filter_components(verts, faces, colors=None, normals=None, min_faces=0, keep_largest=False):
    """Drop connected components by face count (host twin of ops.mesh_filter_components, and the definition of its result).  ``min_faces = n`` keeps the
    components with at least n faces, ``keep_largest`` only the one with the most faces (ties: the smaller label) among what ``min_faces`` left; whenever
    one of them is active, vertices that no face references are dropped too.  Kept vertices and faces stay in their original order; faces are
    renumbered; vertex rows (and colours, normals) are copied as they are.  Returns (verts, faces, colors, normals, kept, info): ``kept`` int32 new -> old
    vertex index, ``info`` = {"components", "components_kept"}.  With nothing selected the inputs are returned as they are (kept = all)."""
    v = np.asarray(verts)
    f = np.asarray(faces).reshape(-1, 3)
    n = v.shape[0]
    min_faces = int(min_faces)
    if min_faces < 0:
        raise ValueError(f"min_faces must be >= 0, got {min_faces}")
    lab = component_labels(f, n)
    n_comp = int(np.count_nonzero(lab == np.arange(n)))
    if min_faces == 0 and not keep_largest:
        return verts, faces, colors, normals, np.arange(n, dtype=np.int32), {"components": n_comp, "components_kept": n_comp}
    size = np.bincount(lab[f[:, 0]], minlength=n) if f.shape[0] else np.zeros(n, np.int64)      # faces per label
    good = size >= max(min_faces, 1)
    if keep_largest and good.any():
        best = int(np.argmax(np.where(good, size, -1)))                # argmax returns the FIRST maximum: the smaller label
        good = np.zeros(n, bool)
        good[best] = True
    keep_v = good[lab]
    kept = np.flatnonzero(keep_v).astype(np.int32)
    new_index = np.cumsum(keep_v) - keep_v                             # exclusive scan of the keep flags
    keep_f = keep_v[f[:, 0]] if f.shape[0] else np.zeros(0, bool)
    f_out = new_index[f[keep_f]].astype(f.dtype)
    take = lambda a: None if a is None else np.asarray(a)[kept]
    return v[kept], f_out, take(colors), take(normals), kept, {"components": n_comp, "components_kept": int(np.count_nonzero(good))}


# ------------------------------------------------------------------------------------------------------------------ adjacency and smoothing
def vertex_adjacency(faces, n_vertices):
    """Vertex -> neighbours table of an indexed triangle mesh in CSR form: (offsets int32 [n + 1], neighbours int32 [E], boundary uint8 [n]).  The host twin of
    ops.mesh_vertex_adjacency and the DEFINITION of its result.  Every triangle (a, b, c) contributes the ordered pairs (a,b), (b,a), (b,c), (c,b), (c,a),
    (a,c), minus those with equal ends; row v holds the distinct second elements of the pairs that start at v, ascending; the multiplicity of u in row v
    (the number of such pairs) is the number of triangles on edge {u, v}, and ``boundary[v] = 1`` iff some entry of row v has multiplicity exactly 1.  A
    vertex no triangle references has an empty row and boundary 0.  Independent of face order and of the rotation of a triangle's indices."""
    n = int(n_vertices)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64, copy=False)
    if n < 0 or n >= 2 ** 30 or 6 * f.shape[0] >= 2 ** 31:
        raise ValueError(f"vertex_adjacency: bad sizes ({n} vertices, {f.shape[0]} faces; the table is int32)")
    if f.size and (f.min() < 0 or f.max() >= n):
        raise ValueError(f"faces index outside 0 .. {n - 1}")
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    src, dst = np.concatenate([a, b, b, c, c, a]), np.concatenate([b, a, c, b, a, c])
    proper = src != dst
    pairs, mult = np.unique(src[proper] * max(n, 1) + dst[proper], return_counts=True)      # sorted by (first, second): the rows in order, ascending inside
    first, second = pairs // max(n, 1), pairs % max(n, 1)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(np.bincount(first, minlength=n))
    boundary = np.zeros(n, np.uint8)
    boundary[first[mult == 1]] = 1
    return offsets, second.astype(np.int32), boundary


def _check_smooth_args(iterations, lam, mu):
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"smooth: iterations must be a non-negative integer, got {iterations!r}")
    lam, mu = float(lam), float(mu)
    if not (np.isfinite(lam) and 0.0 < lam <= 1.0):
        raise ValueError(f"smooth: lam must be in (0, 1], got {lam!r}")
    if not (np.isfinite(mu) and mu <= 0.0):
        raise ValueError(f"smooth: mu must be finite and <= 0, got {mu!r}")
    return int(iterations), lam, mu


def smooth_vertices(verts, faces, iterations, lam=0.5, mu=-0.53, pin_boundary=True):
    """Taubin's lambda|mu smoothing of the vertex positions (host twin of ops.mesh_smooth, and the definition of its result, to the last bit) -> float64 [N,3].
    ``iterations`` times: one step with factor ``lam``, then one with ``mu`` unless ``mu == 0`` (plain Laplacian smoothing, which shrinks the shape).
    One step with factor f, every vertex from the OLD positions, in float64: acc = 0; acc = acc + p[u] over the neighbours u of v in ascending order (one
    sequential sum per coordinate); m = acc / deg; d = m - p[v]; p'[v] = p[v] + f * d, multiply and add apart.  A vertex without neighbours, or a boundary
    vertex (vertex_adjacency) while ``pin_boundary`` is on, keeps its value bit for bit: the rim of a mesh cut open by the volume's faces stays where it
    is.  The adjacency is built once; faces and vertex count never change.  ``iterations == 0`` returns ``verts`` itself."""
    iterations, lam, mu = _check_smooth_args(iterations, lam, mu)
    if iterations == 0:
        return verts
    p = np.array(verts, dtype=np.float64).reshape(-1, 3)               # a copy: the input is never written
    n = p.shape[0]
    offsets, nbr, boundary = vertex_adjacency(faces, n)
    off = offsets.astype(np.int64)
    deg = off[1:] - off[:-1]
    moving = np.flatnonzero((deg > 0) & ((boundary == 0) | (not pin_boundary)))
    if moving.size == 0:
        return p
    # the sum is sequential over the neighbour RANK k = 0 .. max degree - 1, vectorised over the rows that have a k-th entry: with the moving rows sorted
    # by falling degree those are a prefix (np.add.reduceat / sum(axis) would add in numpy's own pairwise order, which is not the definition)
    rows = moving[np.argsort(-deg[moving], kind="stable")]
    rdeg, start = deg[rows], off[rows]
    have = np.searchsorted(-rdeg, -np.arange(int(rdeg[0])), side="left")         # rows with degree > k = the first have[k] of them
    divisor = rdeg.astype(np.float64)[:, None]

    def step(p, f):
        acc = np.zeros((rows.size, 3), np.float64)
        for k, m in enumerate(have):
            acc[:m] = acc[:m] + p[nbr[start[:m] + k]]
        mean = acc / divisor
        d = mean - p[rows]
        fd = f * d
        out = p.copy()
        out[rows] = p[rows] + fd
        return out

    for _ in range(iterations):
        p = step(p, lam)
        if mu != 0.0:
            p = step(p, mu)
    return p


# ------------------------------------------------------------------------------------------------------------------ decimation
def _check_cell(cell):
    """-> 0.0 for off (None or 0), else the finite positive float"""
    if cell is None:
        return 0.0
    c = float(cell)
    if not (np.isfinite(c) and c >= 0.0):
        raise ValueError(f"decimate: cell must be a finite float >= 0, got {cell!r}")
    return c


def decimate_mesh(verts, faces, cell, colors=None):
    """Decimation by vertex clustering (host twin of ops.mesh_decimate, and the definition of its result, to the last bit) -> (verts float64 [Nc,3], faces
    [Mk,3] in the dtype of ``faces``, colors, cluster int32 [N], info).  ``cell`` None or 0: off, the inputs are returned as they are (cluster, info: None).
    Cell of a vertex: q = floor(p / cell) per axis in float64; equal q = one cluster; per axis max q - min q must be below 2^21 (the offsets q - min q pack
    into one 63-bit key; the shift does not change the partition, negative coordinates are legal).  Representative: the smallest member index.  Face
    (a, b, c) maps to its corners' clusters; degenerate (two mapped corners equal) faces are dropped; of the others, those over the same SET of three
    clusters are duplicates whatever their orientation or rotation, and the first in face order is kept.  Kept faces keep face order, corner order and
    orientation.  A cluster is kept iff a kept face references it; kept clusters are numbered by an exclusive scan of "is a kept representative" over the
    old vertex order; ``cluster[v]`` is that number, or -1 (clusters that only fed degenerate faces, specks inside one cell, unreferenced vertices).
    Position, per coordinate: acc = 0; acc = acc + p[u] over the members u in ascending index order (one sequential sum); acc / count.  ``colors`` uint8
    [N,3] or [N,4]: per channel (2 * sum + n) // (2 * n) over the members, the mean rounded half up, exact.  ``info`` = {"clusters" (distinct cells),
    "vertices", "triangles", "degenerate", "duplicate"}.  NOT promised: manifoldness -- where a thin part collapses, clustering leaves edges with more
    than two faces, or open ones.  Refused (ValueError): a negative or non-finite cell, a non-finite coordinate, a face index outside [0, N), an extent
    of 2^21 cells or more, N >= 2^30 or 3 M >= 2^31, colours that are not uint8."""
    cell = _check_cell(cell)
    if cell == 0.0:
        return verts, faces, colors, None, None
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    fin = np.asarray(faces).reshape(-1, 3)
    f = fin.astype(np.int64, copy=False)
    n, m = p.shape[0], f.shape[0]
    if n >= 2 ** 30 or 3 * m >= 2 ** 31:
        raise ValueError(f"decimate: bad sizes ({n} vertices, {m} faces; the tables are int32)")
    if not np.isfinite(p).all():
        raise ValueError("decimate: non-finite vertex coordinate")
    if f.size and (f.min() < 0 or f.max() >= n):
        raise ValueError(f"faces index outside 0 .. {n - 1}")
    col = None
    if colors is not None:
        col = np.asarray(colors)
        if col.dtype != np.uint8 or col.ndim != 2 or col.shape[0] != n or col.shape[1] not in (3, 4):
            raise ValueError(f"decimate: colours must be uint8 [N,3] or [N,4], got {col.dtype} {col.shape}")
    info = {"clusters": 0, "vertices": 0, "triangles": 0, "degenerate": m, "duplicate": 0}
    empty = (np.zeros((0, 3), np.float64), np.zeros((0, 3), fin.dtype), None if col is None else np.zeros((0, col.shape[1]), np.uint8))
    if n == 0:
        return (*empty, np.zeros(0, np.int32), info)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.floor(p / cell)
        q0 = q.min(axis=0)
        if not ((q.max(axis=0) - q0) < 2.0 ** 21).all():
            raise ValueError(f"decimate: the mesh extends over 2^21 cells or more of size {cell!r} along an axis")
    r = (q - q0).astype(np.int64)                                      # exact: both are integers less than 2^21 apart
    key = (r[:, 0] << 42) | (r[:, 1] << 21) | r[:, 2]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)      # first occurrence = smallest member index
    rep = first[inverse.reshape(-1)]
    info["clusters"] = int(first.size)
    mf = rep[f]                                                        # mapped faces
    alive = (mf[:, 0] != mf[:, 1]) & (mf[:, 1] != mf[:, 2]) & (mf[:, 0] != mf[:, 2]) if m else np.zeros(0, bool)
    keep_f = np.zeros(m, bool)
    live = np.flatnonzero(alive)
    if live.size:
        _, first_f = np.unique(np.sort(mf[live], axis=1), axis=0, return_index=True)          # first in face order of every vertex set
        keep_f[live[first_f]] = True
    info["degenerate"], info["triangles"] = int(m - live.size), int(np.count_nonzero(keep_f))
    info["duplicate"] = int(live.size) - info["triangles"]
    used = np.zeros(n, bool)
    used[mf[keep_f].reshape(-1)] = True                                # kept representatives
    new_index = np.cumsum(used) - used                                 # exclusive scan over the old vertex order
    cluster = np.where(used[rep], new_index[rep], -1).astype(np.int32)
    nc = int(np.count_nonzero(used))
    info["vertices"] = nc
    f_out = new_index[mf[keep_f]].astype(fin.dtype)
    if nc == 0:
        return (empty[0], f_out.reshape(-1, 3), empty[2], cluster, info)
    # members of every kept cluster in ascending index order: a stable sort by cluster.  The sum is sequential over the member RANK k, vectorised over the
    # clusters that have a k-th member: with the clusters sorted by falling count those are a prefix, as in smooth_vertices (np.add.reduceat / sum(axis)
    # would add in numpy's own pairwise order, which is not the definition)
    members = np.flatnonzero(cluster >= 0)
    members = members[np.argsort(cluster[members], kind="stable")]
    count = np.bincount(cluster[members], minlength=nc)
    start = np.cumsum(count) - count
    rows = np.argsort(-count, kind="stable")
    rcount, rstart = count[rows], start[rows]
    have = np.searchsorted(-rcount, -np.arange(int(rcount[0])), side="left")       # clusters with more than k members = the first have[k] rows
    acc = np.zeros((nc, 3), np.float64)
    for k, h in enumerate(have):
        acc[:h] = acc[:h] + p[members[rstart[:h] + k]]
    v_out = np.empty((nc, 3), np.float64)
    v_out[rows] = acc / rcount.astype(np.float64)[:, None]
    c_out = None
    if col is not None:
        cm = cluster[members]
        total = np.stack([np.bincount(cm, weights=col[members, k], minlength=nc) for k in range(col.shape[1])], 1).astype(np.int64)      # < 2^53: exact
        c_out = ((2 * total + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
    return v_out, f_out, c_out, cluster, info


# ------------------------------------------------------------------------------------------------------------------ simplification
SIMPLIFY_WIDE, SIMPLIFY_SHARE = 8, 2       # a round's participants: the cheapest max(1, min(WIDE need, ceil(C / SHARE))) candidates, by exponent bin
_QUADRIC_PAIRS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))      # the ten entries over (nx, ny, nz, d)


def _check_simplify_args(target_faces, max_error, max_rounds):
    for name, x in (("target_faces", target_faces), ("max_rounds", max_rounds)):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or x < 0 or x >= 2 ** 31:
            raise ValueError(f"simplify: {name} must be a non-negative integer below 2^31, got {x!r}")
    e = float(max_error)
    if not e >= 0.0:
        raise ValueError(f"simplify: max_error must be >= 0 (inf = no limit), got {max_error!r}")
    return int(target_faces), e, int(max_rounds)


def _cross(e1, e2):
    return (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])


def simplify_quadrics(P0, P1, P2):
    """The area-weighted plane quadric of every triangle (corners float64 [m,3] each) -> float64 [m,10], the entries xx xy xz xd yy yz yd zz zd dd:
    n = (P1 - P0) x (P2 - P0), nn = (nx nx + ny ny) + nz nz; nn > 0: s = 0.5 / sqrt(nn), d = -((nx P0x + ny P0y) + nz P0z), entry = (a b) s; else zeros."""
    with np.errstate(all="ignore"):
        nx, ny, nz = _cross(P1 - P0, P2 - P0)
        nn = (nx * nx + ny * ny) + nz * nz
        s = 0.5 / np.sqrt(nn)
        c = (nx, ny, nz, -((nx * P0[:, 0] + ny * P0[:, 1]) + nz * P0[:, 2]))
        K = np.stack([(c[a] * c[b]) * s for a, b in _QUADRIC_PAIRS], 1)
    K[~(nn > 0)] = 0.0
    return K


def simplify_error(Q, P):
    """p^T Q p of the quadrics Q float64 [k,10] at the points P float64 [k,3], the ONE expression of the definition (the cost is max(0, .) of it)."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    q = Q.T
    with np.errstate(all="ignore"):
        r0 = ((q[0] * x + q[1] * y) + q[2] * z) + q[3]
        r1 = ((q[1] * x + q[4] * y) + q[5] * z) + q[6]
        r2 = ((q[2] * x + q[5] * y) + q[7] * z) + q[8]
        r3 = ((q[3] * x + q[6] * y) + q[8] * z) + q[9]
        return ((x * r0 + y * r1) + z * r2) + r3


def simplify_keeps_side(T, corner, Pu):
    """The flip test: triangles T float64 [k,3,3], ``corner`` [k] the corner that moves to Pu [k,3] -> bool [k]: n . n' > 0 for the normals before and
    after ((P1 - P0) x (P2 - P0), the dot product (x x + y y) + z z); a zero normal on either side fails."""
    T2 = T.copy()
    T2[np.arange(T.shape[0]), corner] = Pu
    with np.errstate(all="ignore"):
        a = _cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
        b = _cross(T2[:, 1] - T2[:, 0], T2[:, 2] - T2[:, 0])
        return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) > 0.0


def _mix64(x):
    """the finaliser of splitmix64 on a uint64 array (the hash of the device's decimation tables)"""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _expand(rows_start, rows_count):
    """-> (owner, index): for every row r its entries rows_start[r] .. + rows_count[r], flattened"""
    owner = np.repeat(np.arange(rows_count.size), rows_count)
    first = np.cumsum(rows_count) - rows_count
    return owner, rows_start[owner] + (np.arange(owner.size) - first[owner])


def simplify_mesh(verts, faces, target_faces, max_error=np.inf, max_rounds=256, colors=None, trace=None):
    """Simplification by rounds of independent half-edge collapses ordered by Garland - Heckbert's quadric error (host twin of ops.mesh_simplify, and the
    definition of its result, to the last bit) -> (verts float64 [Nk,3], faces [Mk,3] in the dtype of ``faces``, colors, source int32 [Nk], merged int32 [N],
    info).  ``target_faces``: rounds run while more faces are alive; the last round may go below it ("at most n").  Everything is float64, one operation at
    a time, in the order written.  Placement is subset placement: collapsing v -> u removes v and u keeps its bits; positions never change.
    Quadrics, once, from the input: K_t = simplify_quadrics of face t; Q_v = the sequential entrywise sum of K_t over the faces of v in ascending face
    order.  After a collapse Q_u <- Q_u + Q_v.
    A round, on its live faces, with N(v) the distinct neighbours of v (vertex_adjacency's rows) and their multiplicities.  The half-edge v -> u (u in
    N(v)) is eligible iff (1) every edge at v has exactly two faces -- boundary vertices and vertices on non-manifold edges are never removed, though they
    may be targets; (2) |N(v) & N(u)| = 2, the link condition; (3) every face at v without u passes simplify_keeps_side with P_v replaced by P_u; (4) e =
    simplify_error(Q_v + Q_u, P_u) is finite and cost = (e if e > 0 else 0) <= max_error.  The candidate of v: its eligible u of least cost, ties to the
    smaller u.  With C candidates and need = ceil((live faces - target) / 2): bin(cost) = the biased exponent field of the double; B = the smallest bin
    whose cumulative count reaches max(1, min(8 need, ceil(C / 2))); the candidates with bin <= B take part, with priority (mix64(v + (round << 32)), v).
    v is selected iff its priority is the smallest among the participants within graph distance 2 (m1[y] = min over y and N(y), m2[v] = min of m1 over v
    and N(v), selected iff m2[v] is v's own): the closed 1-rings of the selected vertices are disjoint, so every test made on the round's mesh still holds
    when all selected collapses are applied at once.  Faces are remapped, those with two equal corners dropped; face order, corner order and orientation
    stay.  Stop: live faces <= target ("target"), no candidate ("blocked"), ``max_rounds`` rounds done ("rounds").
    Output: a vertex is kept iff a kept face references it, in the old order, bit for bit; faces renumbered by an exclusive scan; ``source`` new -> old;
    ``merged[v]`` the new index of the vertex v ended in, following the collapses, or -1; ``colors`` those of the kept vertices.  ``info`` = {"rounds",
    "vertices", "triangles", "collapses" (per round), "max_cost" (the largest applied), "stopped"}.  ``trace``: a list that receives, per round,
    {"faces" (the round's live faces, old indices), "selected", "targets"}.  NOT done: optimal (solved) placement, boundary and non-manifold collapses,
    a valence cap, an exact hit of the target.  Refused (ValueError): a non-finite coordinate, a face index outside [0, N), a face with a repeated
    index, N >= 2^30 or 6 M >= 2^31, bad arguments."""
    target, max_error, max_rounds = _check_simplify_args(target_faces, max_error, max_rounds)
    p = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    fin = np.asarray(faces).reshape(-1, 3)
    F = fin.astype(np.int64)                                           # a copy: the live faces, in face order
    n, m0 = p.shape[0], F.shape[0]
    if n >= 2 ** 30 or 6 * m0 >= 2 ** 31:
        raise ValueError(f"simplify: bad sizes ({n} vertices, {m0} faces; the tables are int32)")
    if not np.isfinite(p).all():
        raise ValueError("simplify: non-finite vertex coordinate")
    if F.size and (F.min() < 0 or F.max() >= n):
        raise ValueError(f"faces index outside 0 .. {n - 1}")
    repeated = int(np.count_nonzero((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])))
    if repeated:
        raise ValueError(f"simplify: {repeated} faces repeat a vertex index")
    # Q_v: sequential over the rank of a face in its vertex's row (rows by falling length: the rows with a k-th face are a prefix, as in smooth_vertices)
    K = simplify_quadrics(p[F[:, 0]], p[F[:, 1]], p[F[:, 2]])
    Q = np.zeros((n, 10), np.float64)
    if m0:
        cv = F.reshape(-1)
        order = np.argsort(cv, kind="stable")                          # by vertex, faces ascending inside
        cnt = np.bincount(cv, minlength=n)
        start = np.cumsum(cnt) - cnt
        rows = np.argsort(-cnt, kind="stable")
        rcnt, rstart = cnt[rows], start[rows]
        have = np.searchsorted(-rcnt, -np.arange(int(rcnt[0])), side="left")
        acc = np.zeros((n, 10), np.float64)
        for k, h in enumerate(have):
            acc[:h] = acc[:h] + K[order[rstart[:h] + k] // 3]
        Q[rows] = acc
    parent = np.arange(n, dtype=np.int64)
    collapses, max_cost, stopped = [], 0.0, None
    while stopped is None:
        m = F.shape[0]
        if m <= target:
            stopped = "target"
            break
        if len(collapses) == max_rounds:
            stopped = "rounds"
            break
        rnd = len(collapses)
        a, b, c = F[:, 0], F[:, 1], F[:, 2]
        key, mult = np.unique(np.concatenate([a, b, b, c, c, a]) * n + np.concatenate([b, a, c, b, a, c]), return_counts=True)
        first, second = key // n, key % n
        deg = np.bincount(first, minlength=n)
        off = np.cumsum(deg) - deg
        ok1 = (deg > 0) & (np.bincount(first, weights=(mult != 2), minlength=n) == 0)
        he = np.flatnonzero(ok1[first])
        hv, hu = first[he], second[he]
        # (2) the link condition: the w of N(v) that are in N(u)
        own, at = _expand(off[hv], deg[hv])
        q = hu[own] * n + second[at]
        i = np.minimum(np.searchsorted(key, q), key.size - 1)
        ok = np.bincount(own, weights=(key[i] == q), minlength=he.size) == 2
        he, hv, hu = he[ok], hv[ok], hu[ok]
        # (3) the faces at v without u keep their side
        cv = F.reshape(-1)
        order = np.argsort(cv, kind="stable")
        tcnt = np.bincount(cv, minlength=n)
        tstart = np.cumsum(tcnt) - tcnt
        own, at = _expand(tstart[hv], tcnt[hv])
        t, corner = order[at] // 3, order[at] % 3
        other = ~(F[t] == hu[own][:, None]).any(1)
        own, t, corner = own[other], t[other], corner[other]
        flips = ~simplify_keeps_side(p[F[t]], corner, p[hu[own]])
        ok = np.bincount(own, weights=flips, minlength=he.size) == 0
        he, hv, hu = he[ok], hv[ok], hu[ok]
        # (4) the cost
        e = simplify_error(Q[hv] + Q[hu], p[hu])
        cost = np.where(e > 0.0, e, 0.0)
        ok = np.isfinite(e) & (cost <= max_error)
        hv, hu, cost = hv[ok], hu[ok], cost[ok]
        if hv.size == 0:
            stopped = "blocked"
            break
        best = np.lexsort((hu, cost, hv))
        best = best[np.concatenate([[True], hv[best][1:] != hv[best][:-1]])]
        cv_, cu_, cc_ = hv[best], hu[best], cost[best]                 # the candidates, ascending v
        C = cv_.size
        need = (m - target + 1) // 2
        want = max(1, min(SIMPLIFY_WIDE * need, (C + SIMPLIFY_SHARE - 1) // SIMPLIFY_SHARE))
        bins = (cc_.view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7FF
        B = int(np.searchsorted(np.cumsum(np.bincount(bins, minlength=2048)), want, side="left"))
        part = bins <= B
        pv, pu, pc = cv_[part], cu_[part], cc_[part]
        h = _mix64(pv.astype(np.uint64) + (np.uint64(rnd) << np.uint64(32)))
        rank = np.empty(pv.size, np.int64)
        rank[np.lexsort((pv, h))] = np.arange(pv.size)                 # the order of the pairs (hash, v)
        R = np.full(n, n + 1, np.int64)
        R[pv] = rank
        m1 = R.copy()
        np.minimum.at(m1, first, R[second])
        m2 = m1.copy()
        np.minimum.at(m2, first, m1[second])
        sel = m2[pv] == rank
        sv, su = pv[sel], pu[sel]
        if trace is not None:
            trace.append({"faces": F.copy(), "selected": sv.copy(), "targets": su.copy()})
        parent[sv] = su
        Q[su] = Q[su] + Q[sv]
        remap = np.arange(n, dtype=np.int64)
        remap[sv] = su
        F = remap[F]
        F = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])]
        collapses.append(int(sv.size))
        max_cost = max(max_cost, float(pc[sel].max()))
    used = np.zeros(n, bool)
    used[F.reshape(-1)] = True
    new_index = np.cumsum(used) - used
    source = np.flatnonzero(used).astype(np.int32)
    root = parent
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    merged = np.where(used[root], new_index[root], -1).astype(np.int32)
    info = {"rounds": len(collapses), "vertices": int(source.size), "triangles": int(F.shape[0]), "collapses": collapses, "max_cost": max_cost,
            "stopped": stopped}
    return p[source], new_index[F].astype(fin.dtype), None if colors is None else np.asarray(colors)[source], source, merged, info


# ------------------------------------------------------------------------------------------------------------------ projection
def _check_project_args(resolution, iterations, level, tol, max_step, max_move, bound_min, bound_max):
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 1 <= iterations <= 64:
        raise ValueError(f"project: iterations must be an integer in [1, 64], got {iterations!r}")
    if isinstance(resolution, (bool, np.bool_)) or not isinstance(resolution, (int, np.integer)) or resolution < 2:
        raise ValueError(f"project: resolution must be an integer >= 2, got {resolution!r}")
    level, tol, max_step, max_move = float(level), float(tol), float(max_step), float(max_move)
    if not np.isfinite(level):
        raise ValueError(f"project: level must be finite, got {level!r}")
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"project: tol must be finite and >= 0, got {tol!r}")
    if not (np.isfinite(max_step) and max_step > 0.0):
        raise ValueError(f"project: max_step must be finite and > 0, got {max_step!r}")
    if not (np.isfinite(max_move) and max_move > 0.0):
        raise ValueError(f"project: max_move must be finite and > 0, got {max_move!r}")
    b0 = np.asarray(bound_min, np.float32).reshape(-1).astype(np.float64)          # float32 values, widened
    b1 = np.asarray(bound_max, np.float32).reshape(-1).astype(np.float64)
    if b0.shape != (3,) or b1.shape != (3,) or not (np.isfinite(b0).all() and np.isfinite(b1).all() and (b1 > b0).all()):
        raise ValueError(f"project: bound_max must be above bound_min on every axis, both finite, got {bound_min!r} and {bound_max!r}")
    return int(resolution), int(iterations), level, tol, max_step, max_move, b0, b1 - b0


def project_vertices(verts_idx, field, resolution, iterations, level=0.0, tol=5e-5, max_step=0.5, max_move=1.0, bound_min=(-1.0, -1.0, -1.0),
                     bound_max=(1.0, 1.0, 1.0)):
    """Newton projection of mesh vertices onto the level set ``sdf == level`` (host twin of ops.mesh_project, and the definition of its result, to the last
    bit when ``field`` is the device's own SDF kernel) -> (verts float64 [n,3] in index coordinates, info).  ``verts_idx`` float64 [n,3], index coordinates
    on a ``resolution``^3 grid (one grid spacing = 1); ``field(pts32 [m,3] float32) -> (s float32 [m], g float32 [m,3])`` is the SDF and its gradient at
    world points.  All arithmetic below is float64, every operation separate (never fused) and in the order written; there is no square root.
    With o the input position of a vertex and x its current one, bmin / bmax the float32 bounds widened to float64, ext = bmax - bmin:
    world point w_k = x_k / (R - 1) * ext_k + bmin_k, and the field sees float32(w) -- for (-1, 1) the pipeline's verts_idx / (R - 1) * 2 - 1 to the bit.
    A round evaluates (s, g) at every ACTIVE vertex (all in round 0), then per vertex: r = |float64(s) - level|;
      * s or g non-finite, or g2 = (gx gx + gy gy) + gz gz not > 0: STALLED -- the vertex leaves the active set and keeps x;
      * else r <= tol: CONVERGED -- leaves and keeps x;
      * else, in rounds 0 .. iterations - 1: t = (float64(s) - level) / g2; d_k = t g_k; e_k = d_k / ext_k * (R - 1), clamped to [-max_step, max_step] per
        axis; y_k = x_k - e_k, clamped to [o_k - max_move, o_k + max_move], then to [0, R - 1]; x <- y.  Each of the three clamps that changes a value
        counts one ``clamped`` event (up to nine per vertex and round);
      * else (round ``iterations``, the last, only classifies): UNCONVERGED.
    (s, g) -> (-s, -g) with level -> -level gives the same steps.  ``info`` = {"evaluated": the active count of each of the iterations + 1 rounds,
    "converged", "unconverged", "stalled", "clamped", "max_before": the largest r of round 0, "max_after": the largest r at which a vertex left or ended};
    the two maxima are Python floats, 0.0 for an empty mesh, and a non-finite r takes no part in them.  NOT promised: that a vertex stays on its sheet of
    the surface beyond the max_move box, or that triangles keep their orientation where the surface folds inside one cell.  Refused (ValueError): a
    non-finite coordinate, iterations outside [1, 64], a non-finite level, tol not finite or < 0, max_step or max_move not finite or <= 0, a bound with
    bmax <= bmin, resolution < 2."""
    R, iterations, level, tol, max_step, max_move, b0, ext = _check_project_args(resolution, iterations, level, tol, max_step, max_move, bound_min, bound_max)
    o = np.array(verts_idx, dtype=np.float64).reshape(-1, 3)            # a copy: the input is never written
    if not np.isfinite(o).all():
        raise ValueError("project: non-finite vertex coordinate")
    n = o.shape[0]
    rm1 = float(R - 1)
    x = o.copy()
    lo, hi = o - max_move, o + max_move
    info = {"evaluated": [], "converged": 0, "unconverged": 0, "stalled": 0, "clamped": 0, "max_before": 0.0, "max_after": 0.0}

    def finite_max(r):
        r = r[np.isfinite(r)]
        return float(r.max()) if r.size else 0.0

    def clamp(a, low, high):
        """-> (a limited to [low, high] by comparison, the number of values that changed)"""
        under, over = a < low, a > high
        return np.where(under, low, np.where(over, high, a)), int(np.count_nonzero(under)) + int(np.count_nonzero(over))

    active = np.arange(n)
    for rnd in range(iterations + 1):
        info["evaluated"].append(int(active.size))
        if active.size == 0:
            continue
        with np.errstate(over="ignore"):
            pts32 = np.ascontiguousarray((x[active] / rm1 * ext + b0).astype(np.float32))
        s, g = field(pts32)
        s, g = np.asarray(s).reshape(-1), np.asarray(g).reshape(-1, 3)
        if s.dtype != np.float32 or g.dtype != np.float32 or s.shape[0] != active.size or g.shape[0] != active.size:
            raise ValueError("project: the field must return float32 (s [m], g [m,3]) for the m points it is given")
        finite = np.isfinite(s) & np.isfinite(g).all(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            s64, g64 = s.astype(np.float64), g.astype(np.float64)
            ds = s64 - level
            r = np.abs(ds)
            g2 = g64[:, 0] * g64[:, 0] + g64[:, 1] * g64[:, 1] + g64[:, 2] * g64[:, 2]
            stalled = ~finite | ~(g2 > 0.0)
        converged = ~stalled & (r <= tol)
        moving = ~stalled & ~converged
        if rnd == 0:
            info["max_before"] = finite_max(r)
        info["stalled"] += int(np.count_nonzero(stalled))
        info["converged"] += int(np.count_nonzero(converged))
        if rnd == iterations:
            info["unconverged"] += int(np.count_nonzero(moving))
            info["max_after"] = max(info["max_after"], finite_max(r))
            break
        info["max_after"] = max(info["max_after"], finite_max(r[~moving]))
        idx = active[moving]
        t = ds[moving] / g2[moving]
        d = t[:, None] * g64[moving]
        e = d / ext * rm1
        e, c0 = clamp(e, -max_step, max_step)
        y = x[idx] - e
        y, c1 = clamp(y, lo[idx], hi[idx])
        y, c2 = clamp(y, 0.0, rm1)
        x[idx] = y
        info["clamped"] += c0 + c1 + c2
        active = idx
    return x, info


# ------------------------------------------------------------------------------------------------------------------ texture atlas
# One square cell of c x c texels per PAIR of triangles, cells in face order, row-major in a grid G cells wide.  DESIGN.md section 7 has the derivation;
# the functions below are the host twin of csrc/mesh_texture.hip and the DEFINITION of its results, to the last bit.
TEXTURE_MAX_SIDE = 16384


def _check_texel(texel):
    """-> 0 for off (None or 0), else the integer in [4, 64]"""
    if texel is None:
        return 0
    if isinstance(texel, (bool, np.bool_)) or not isinstance(texel, (int, np.integer)) or not (texel == 0 or 4 <= texel <= 64):
        raise ValueError(f"texture: texel must be 0 (off) or an integer in [4, 64], got {texel!r}")
    return int(texel)


def texture_layout(nt, texel):
    """The atlas of ``nt`` triangles at ``texel`` = c texels per cell edge -> {"texel": c, "cells": ceil(nt / 2), "grid": G = ceil(sqrt(cells)), "rows":
    ceil(cells / G), "width": G c, "height": rows c, "texels": cells c^2 (the texels of used cells: the length of the texel point list)}.  Triangles 2k
    and 2k + 1 share cell k, which sits at column k mod G, row k div G; the image need not be square.  Refused (ValueError): c outside [4, 64], nt < 1,
    a side over 16384, cells c^2 >= 2^31."""
    c = _check_texel(texel)
    if c == 0:
        raise ValueError("texture: texel must be an integer in [4, 64], got 0 (off)")
    if isinstance(nt, (bool, np.bool_)) or int(nt) != nt or nt < 1:
        raise ValueError(f"texture: the triangle count must be a positive integer, got {nt!r}")
    import math
    cells = (int(nt) + 1) // 2
    G = math.isqrt(cells - 1) + 1
    rows = (cells + G - 1) // G
    W, H = G * c, rows * c
    if W > TEXTURE_MAX_SIDE or H > TEXTURE_MAX_SIDE or cells * c * c >= 2 ** 31:
        raise ValueError(f"texture: {nt} triangles at texel {c} need an image of {W} x {H}; a side is limited to {TEXTURE_MAX_SIDE} and the texel list to 2^31")
    return {"texel": c, "cells": cells, "grid": G, "rows": rows, "width": W, "height": H, "texels": cells * c * c}


def texture_cell(texel):
    """The inside of one cell -> (owner uint8 [c, c] indexed [j, i]: 0 = triangle A (i + j <= c - 1), 1 = triangle B (i + j >= c); w float64 [c, c, 3]: the
    barycentric weights of the texel centre (i + 0.5, j + 0.5) with respect to its owner's UV corners; corners float64 [2, 3, 2]: those corners, A's
    (0.5, 0.5), (c - 1.5, 0.5), (0.5, c - 1.5) and B's (c - 0.5, c - 0.5), (2.5, c - 0.5), (c - 0.5, 2.5)).  A: w1 = i / (c - 2), w2 = j / (c - 2);
    B: w1 = (c - 1 - i) / (c - 3), w2 = (c - 1 - j) / (c - 3); both: w0 = (1 - w1) - w2.  Never clamped: texels in the gutter extrapolate, which is what
    makes bilinear sampling inside a triangle reproduce a linear function exactly."""
    c = int(texel)
    j, i = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    owner = (i + j >= c).astype(np.uint8)
    fi, fj = i.astype(np.float64), j.astype(np.float64)
    w1 = np.where(owner == 0, fi / float(c - 2), (float(c - 1) - fi) / float(c - 3))
    w2 = np.where(owner == 0, fj / float(c - 2), (float(c - 1) - fj) / float(c - 3))
    w0 = (1.0 - w1) - w2
    corners = np.array([[[0.5, 0.5], [c - 1.5, 0.5], [0.5, c - 1.5]], [[c - 0.5, c - 0.5], [2.5, c - 0.5], [c - 0.5, 2.5]]], np.float64)
    return owner, np.stack([w0, w1, w2], -1), corners


def _texture_mesh(verts_idx, faces, what):
    p = np.asarray(verts_idx, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64, copy=False)
    if f.size and (f.min() < 0 or f.max() >= p.shape[0]):
        raise ValueError(f"{what}: faces index outside 0 .. {p.shape[0] - 1}")
    return p, f


def _bounds64(bounds, what):
    b0 = np.asarray(bounds[0], np.float32).reshape(-1).astype(np.float64)           # float32 values, widened
    b1 = np.asarray(bounds[1], np.float32).reshape(-1).astype(np.float64)
    if b0.shape != (3,) or b1.shape != (3,) or not (np.isfinite(b0).all() and np.isfinite(b1).all() and (b1 > b0).all()):
        raise ValueError(f"{what}: bound_max must be above bound_min on every axis, both finite, got {bounds!r}")
    return b0, b1 - b0


def _texel_owners(L, nt):
    """-> int64 [cells, c^2]: the owner triangle of every cell-major texel, 2k or min(2k + 1, nt - 1) by texture_cell's A / B rule"""
    owner = texture_cell(L["texel"])[0]
    return np.minimum(2 * np.arange(L["cells"])[:, None] + owner.reshape(1, -1), int(nt) - 1)


def _cells_to_image(values, L, fill):
    """cell-major RGBA8 texels (uint8 [cells c^2, 4]) -> the image uint8 [height, width, 4] in raster order; the texels of unused cells are ``fill``"""
    c, G, cells = L["texel"], L["grid"], L["cells"]
    cell = np.tile(np.array(fill, np.uint8), (L["rows"] * G, c, c, 1))
    cell[:cells] = values.reshape(cells, c, c, 4)
    return np.ascontiguousarray(cell.reshape(L["rows"], G, c, c, 4).transpose(0, 2, 1, 3, 4).reshape(L["height"], L["width"], 4))


def texture_points(verts_idx, faces, texel, resolution, bounds=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))):
    """The surface point of every texel of every used cell (host twin of ops.mesh_texture_points, and the definition of its result, to the last bit) ->
    (points float64 [cells c^2, 3] in index coordinates, world float32 [cells c^2, 3]).  Cell-major: point k c^2 + j c + i is local texel (i, j) of cell k.
    Its owner (texture_cell) is triangle 2k or min(2k + 1, nt - 1) -- for an odd count the B half of the last cell repeats the last triangle -- with
    corners P0, P1, P2 in ``verts_idx``; p = (w0 P0 + w1 P1) + w2 P2 in float64, every operation separate, then each coordinate clamped to [0, R - 1].
    World point: float32(p / (R - 1) * ext + bmin) with the float32 ``bounds`` = (bound_min, bound_max) widened to float64, ext = bmax - bmin: what
    project_vertices shows the network.  Refused (ValueError): a non-finite coordinate of a referenced vertex, a face index outside [0, N), and what
    texture_layout refuses."""
    p, f = _texture_mesh(verts_idx, faces, "texture_points")
    L = texture_layout(f.shape[0], texel)
    if isinstance(resolution, (bool, np.bool_)) or int(resolution) != resolution or resolution < 2:
        raise ValueError(f"texture_points: resolution must be an integer >= 2, got {resolution!r}")
    b0, ext = _bounds64(bounds, "texture_points")
    if not np.isfinite(p[f.reshape(-1)]).all():
        raise ValueError("texture_points: non-finite vertex coordinate")
    c, rm1 = L["texel"], float(int(resolution) - 1)
    P = p[f[_texel_owners(L, f.shape[0])]]                                                  # [cells, c^2, 3 corners, 3]
    w = texture_cell(c)[1].reshape(1, c * c, 3, 1)
    x = (w[:, :, 0] * P[:, :, 0] + w[:, :, 1] * P[:, :, 1]) + w[:, :, 2] * P[:, :, 2]
    x = np.where(x < 0.0, 0.0, np.where(x > rm1, rm1, x)).reshape(-1, 3)
    return x, np.ascontiguousarray((x / rm1 * ext + b0).astype(np.float32))


def pack_texture(rgb, nt, texel):
    """Cell-major texel colours (float [cells c^2, 3], the order of texture_points) -> the image, uint8 [height, width, 4] in raster order (row 0 on top,
    where v = 0): colour = uint8(int(float32(x) * 255)), the truncation the vertex colours use, alpha 255; the texels of unused cells are 0, 0, 0, 0.
    Host twin of ops.mesh_texture_pack."""
    L = texture_layout(nt, texel)
    a = np.asarray(rgb, np.float32).reshape(-1, 3)
    if a.shape[0] != L["texels"]:
        raise ValueError(f"pack_texture: {L['texels']} texel colours expected, got {a.shape[0]}")
    with np.errstate(invalid="ignore"):
        q = (a * np.float32(255.0)).astype(np.int32).astype(np.uint8)
    return _cells_to_image(np.concatenate([q, np.full((q.shape[0], 1), 255, np.uint8)], 1), L, (0, 0, 0, 0))


def _mat44(m):
    return None if m is None else np.asarray(m.detach().cpu().numpy() if hasattr(m, "detach") else m, np.float32).reshape(-1, 4, 4)[0].astype(np.float64)


def frame_positions(verts_idx, resolution, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None):
    """Index coordinates -> the float32 positions of the PLY (csrc/mesh_math.h, mesh_vertex_f32, operation for operation): v / (R - 1) * ext + bmin with
    ext the FLOAT32 difference of the bounds; * s + t of scale_mat; the rows of trans_mat as ((T0 x + T1 y) + T2 z) + T3; rounded to float32 once."""
    p = np.asarray(verts_idx, dtype=np.float64).reshape(-1, 3)
    b0, b1 = np.asarray(bound_min, np.float32).reshape(3), np.asarray(bound_max, np.float32).reshape(3)
    v = p / float(int(resolution) - 1) * (b1 - b0).astype(np.float64) + b0.astype(np.float64)
    S, T = _mat44(scale_mat), _mat44(trans_mat)
    if S is not None:
        v = v * S[0, 0] + S[:3, 3]
    if T is not None:
        v = np.stack([((T[r, 0] * v[:, 0] + T[r, 1] * v[:, 1]) + T[r, 2] * v[:, 2]) + T[r, 3] for r in range(3)], 1)
    with np.errstate(over="ignore"):
        return v.astype(np.float32)


def frame_normals(grad, trans_mat=None):
    """SDF gradients float32 [N,3] -> the float32 unit normals of the asset frame (csrc/mesh_math.h, mesh_normal_f32, operation for operation, float64):
    g / |g|, through the 3x3 of trans_mat when given and renormalised, y and z exchanged; (0, 1, 0) for a zero or non-finite gradient."""
    g = np.asarray(grad, np.float32).reshape(-1, 3).astype(np.float64)
    T = _mat44(trans_mat)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = (l > 0.0) & (l < np.inf)
        g = g / l[:, None]
        if T is not None:
            w = np.stack([(T[r, 0] * g[:, 0] + T[r, 1] * g[:, 1]) + T[r, 2] * g[:, 2] for r in range(3)], 1)
            l = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
            ok2 = ok & (l > 0.0) & (l < np.inf)
            g = np.where(ok[:, None], w / l[:, None], g)
            ok = ok2
        out = np.where(ok[:, None], g[:, [0, 2, 1]], np.array([0.0, 1.0, 0.0])).astype(np.float32)
    return out


def texture_corner_pixels(nt, texel):
    """The corners of every triangle in the image, in texels, float64 [nt, 3, 2] in the triangle's own corner order: (cell_x c + u_local, cell_y c +
    v_local) with the local UV corners of texture_cell; exact (multiples of 0.5 below 2^15)."""
    L = texture_layout(nt, texel)
    c, G = L["texel"], L["grid"]
    t = np.arange(int(nt))
    k = t // 2
    local = texture_cell(c)[2][t % 2]
    return np.stack([((k % G) * c).astype(np.float64)[:, None] + local[:, :, 0], ((k // G) * c).astype(np.float64)[:, None] + local[:, :, 1]], -1)


def texture_corners(verts_idx, faces, texel, resolution, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None, grad=None):
    """The unwelded vertices of the textured mesh (host twin of ops.mesh_texture_corners, and the definition of its result, to the last bit) -> (positions
    float32 [3 nt, 3] in the asset frame, uv float32 [3 nt, 2], normals float32 [3 nt, 3] or None, bounds float32 [2, 3]).  Triangle t = (a, b, c) gives
    corners 3t, 3t + 1, 3t + 2 = c, b, a (the asset frame's reversed winding), so the index buffer is 0, 1, 2, ...  A corner's position is its vertex's
    position (frame_positions, y and z exchanged: the welded export's bits); its uv is ((cell_x c + u_local) / W, (cell_y c + v_local) / H) with the
    local UV corner of texture_cell, in float64, rounded to float32 once; its normal is its vertex's (frame_normals of ``grad`` float32 [N,3])."""
    p, f = _texture_mesh(verts_idx, faces, "texture_corners")
    L = texture_layout(f.shape[0], texel)
    c, nt = L["texel"], f.shape[0]
    vid = f[:, ::-1].reshape(-1)
    pos = np.ascontiguousarray(frame_positions(p, resolution, bound_min, bound_max, scale_mat, trans_mat)[:, [0, 2, 1]][vid])
    px = texture_corner_pixels(nt, c)[:, ::-1]                                               # corners reversed
    uv = np.stack([px[:, :, 0] / float(L["width"]), px[:, :, 1] / float(L["height"])], -1).reshape(-1, 2).astype(np.float32)
    nrm = None if grad is None else np.ascontiguousarray(frame_normals(grad, trans_mat)[vid])
    return pos, uv, nrm, np.stack([pos.min(0), pos.max(0)])


# ---- tangent-space normal map: the host twin of k_tex_frames / k_tex_normal_pack (csrc/mesh_normalmap_math.h) and the DEFINITION of their results, to the
# last bit.  All arithmetic is float64, one operation at a time, in the order written; a dot product is (x x + y y) + z z.
NORMAL_MAP_FLAT = (128, 128, 255, 255)
NORMAL_MAP_COUNTS = ("degenerate", "bad_gradient", "back_facing", "reserved")          # the counters block of the two device entries, int64 [4]
_DEFAULT_NORMAL, _DEFAULT_TANGENT = (0.0, 1.0, 0.0), (1.0, -0.0, 0.0, 1.0)                   # the negative zero marks the degenerate frame


def _length_ok(l):
    return (l > 0.0) & (l < np.inf)


def texture_frames(positions, uv):
    """One tangent frame per triangle from the file's own float32 buffers (texture_corners' positions [3 nt, 3] and uv [3 nt, 2], promoted to float64) ->
    (normals float32 [3 nt, 3], tangents float32 [3 nt, 4], degenerate: the number of degenerate triangles); host twin of ops.mesh_texture_frames.
    Triangle t has corners 3t, 3t + 1, 3t + 2 = p0, p1, p2 with uv0, uv1, uv2: e1 = p1 - p0, e2 = p2 - p0, N = unit(e1 x e2), the front face of the file's
    winding; (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0, det = du1 dv2 - du2 dv1, Pu = (e1 dv2 - e2 dv1) / det, Pv = (e2 du1 - e1 du2) / det; T =
    unit(Pu - N (N . Pu)); w = +1 if (N x T) . (-Pv) >= 0, else -1: green is up, and up is decreasing v, because row 0 of the image is on top.  NORMAL = N and
    TANGENT = (T, w) for all three corners (flat).  Degenerate -- |e1 x e2|, det or |Pu - N (N . Pu)| zero or not finite --: N = (0, 1, 0), TANGENT = (1, 0, 0,
    1), counted once.  Its TANGENT.y is the NEGATIVE zero: the value of the definition, and the mark that pack_normal_map knows a degenerate triangle by
    (frame_is_degenerate); a sound triangle never carries it, because every float32 component of its N and T has + 0 added, which turns a negative zero
    into a positive one and changes nothing else.  (A flat axis-aligned triangle has the frame (0, 1, 0), (1, 0, 0, 1) for good reasons.)"""
    p = np.asarray(positions, np.float32).reshape(-1, 3, 3).astype(np.float64)
    t = np.asarray(uv, np.float32).reshape(-1, 3, 2).astype(np.float64)
    if p.shape[0] != t.shape[0] or p.shape[0] < 1:
        raise ValueError(f"texture_frames: expected positions [3 M, 3] and uv [3 M, 2] of M >= 1 triangles, got {np.shape(positions)} and {np.shape(uv)}")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        c = _cross3(e1, e2)
        l = np.sqrt(_dot3(c, c))
        du1, dv1, du2, dv2 = (t[:, 1, 0] - t[:, 0, 0])[:, None], (t[:, 1, 1] - t[:, 0, 1])[:, None], (t[:, 2, 0] - t[:, 0, 0])[:, None], (t[:, 2, 1] - t[:, 0, 1])[:, None]
        det = du1 * dv2 - du2 * dv1
        n = c / l[:, None]
        Pu = (e1 * dv2 - e2 * dv1) / det
        Pv = (e2 * du1 - e1 * du2) / det
        tv = Pu - n * _dot3(n, Pu)[:, None]
        lt = np.sqrt(_dot3(tv, tv))
        T = tv / lt[:, None]
        w = np.where(_dot3(_cross3(n, T), -Pv) >= 0.0, 1.0, -1.0)
        ok = _length_ok(l) & _length_ok(np.abs(det[:, 0])) & _length_ok(lt)
        N = np.where(ok[:, None], n.astype(np.float32) + np.float32(0.0), np.array(_DEFAULT_NORMAL, np.float32))
        TW = np.where(ok[:, None], np.concatenate([T.astype(np.float32) + np.float32(0.0), w[:, None].astype(np.float32)], 1), np.array(_DEFAULT_TANGENT, np.float32))
    return np.ascontiguousarray(np.repeat(N, 3, 0)), np.ascontiguousarray(np.repeat(TW, 3, 0)), int((~ok).sum())


def frame_is_degenerate(tangents):
    """float32 [N,4] -> bool [N]: the mark texture_frames gives a degenerate triangle, a negative zero in TANGENT.y"""
    t = np.asarray(tangents, np.float32).reshape(-1, 4)
    return (t[:, 1] == 0.0) & np.signbit(t[:, 1])


def _unit_gradients(grad, trans_mat=None):
    """frame_normals' operations, kept in float64 -> (n [N,3] with y and z exchanged, ok [N]); n is undefined where ok is False"""
    g = np.asarray(grad, np.float32).reshape(-1, 3).astype(np.float64)
    T = _mat44(trans_mat)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        l = np.sqrt(_dot3(g, g))
        ok = _length_ok(l)
        g = g / l[:, None]
        if T is not None:
            w = np.stack([(T[r, 0] * g[:, 0] + T[r, 1] * g[:, 1]) + T[r, 2] * g[:, 2] for r in range(3)], 1)
            l = np.sqrt(_dot3(w, w))
            ok = ok & _length_ok(l)
            g = w / l[:, None]
    return g[:, [0, 2, 1]], ok


def _normal_channel(x):
    with np.errstate(invalid="ignore"):
        v = np.floor((x * 127.5 + 127.5) + 0.5)
        return np.where(v >= 0.0, np.where(v <= 255.0, v, 255.0), 0.0).astype(np.uint8)


def pack_normal_map(grad, normals, tangents, nt, texel, trans_mat=None):
    """Cell-major raw SDF gradients at the texel points (float32 [cells c^2, 3], the order of texture_points) and the frames of texture_frames -> (image
    uint8 [height, width, 4] in raster order like pack_texture, counts {"bad_gradient", "back_facing"}); host twin of ops.mesh_texture_normal_pack.
    A texel of a used cell has its owner triangle t by the A / B rule of texture_cell (for an odd count the B half of the last cell repeats the last
    triangle).  n = its gradient through the operations of frame_normals -- normalise, through the 3x3 of ``trans_mat`` (a 4x4, or a 3x3, float32) when given
    and renormalise, y and z exchanged -- kept in float64.  With the float32 N, T, w of corner 3t promoted to float64 and B = w (N x T): x = n . T, y = n . B,
    z = n . N; each channel is clamp(floor((x 127.5 + 127.5) + 0.5), 0, 255), alpha 255.  NORMAL_MAP_FLAT for a texel of an unused cell, of a triangle that
    holds the degenerate mark of texture_frames (frame_is_degenerate), and for a gradient whose length, before or behind
    the rotation, is zero or not finite.  Counts: bad gradients over every texel of a used cell; z < 0 (informative, no error) where z is computed."""
    L = texture_layout(nt, texel)
    nt = int(nt)
    g = np.asarray(grad, np.float32).reshape(-1, 3)
    N = np.asarray(normals, np.float32).reshape(-1, 3)
    TW = np.asarray(tangents, np.float32).reshape(-1, 4)
    if g.shape[0] != L["texels"] or N.shape[0] != 3 * nt or TW.shape[0] != 3 * nt:
        raise ValueError(f"pack_normal_map: expected {L['texels']} gradients and {3 * nt} normals and tangents, got {g.shape[0]}, {N.shape[0]} and {TW.shape[0]}")
    if trans_mat is not None and np.size(trans_mat) == 9:
        R = np.eye(4, dtype=np.float32)
        R[:3, :3] = np.asarray(trans_mat, np.float32).reshape(3, 3)
        trans_mat = R
    n, ok = _unit_gradients(g, trans_mat)
    tri = _texel_owners(L, nt).reshape(-1)                                                              # [cells c^2]
    Nf, Tf = N[3 * tri], TW[3 * tri]
    degenerate = frame_is_degenerate(Tf)
    Nd, Td, w = Nf.astype(np.float64), Tf[:, :3].astype(np.float64), Tf[:, 3:].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        B = w * _cross3(Nd, Td)
        z = _dot3(n, Nd)
        rgba = np.stack([_normal_channel(_dot3(n, Td)), _normal_channel(_dot3(n, B)), _normal_channel(z), np.full(z.shape, 255, np.uint8)], 1)
        back = ok & ~degenerate & (z < 0.0)
    rgba = np.where((ok & ~degenerate)[:, None], rgba, np.array(NORMAL_MAP_FLAT, np.uint8))
    return _cells_to_image(rgba, L, NORMAL_MAP_FLAT), {"bad_gradient": int((~ok).sum()), "back_facing": int(back.sum())}


def decode_normal_map(image):
    """RGBA8 texels -> the tangent-space vectors they stand for, float64 [..., 3] = c / 255 * 2 - 1 (not normalised).  For tests and inspection."""
    return np.asarray(image)[..., :3].astype(np.float64) / 255.0 * 2.0 - 1.0


def sample_texture(image, uv):
    """Bilinear sample the way a glTF viewer does with the file's sampler (LINEAR, CLAMP_TO_EDGE, texel centres at +0.5, no mipmaps) -> (value float64
    [n, C], touched: per sample the four (x, y, weight) it read).  ``image`` float [H, W, C], ``uv`` [n, 2] in [0, 1].  For tests and inspection."""
    img = np.asarray(image, np.float64)
    H, W = img.shape[:2]
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    x, y = uv[:, 0] * W - 0.5, uv[:, 1] * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    out, touched = np.zeros((uv.shape[0], img.shape[2])), []
    for dx, dy, wgt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        xi, yi = np.clip(x0 + dx, 0, W - 1).astype(np.int64), np.clip(y0 + dy, 0, H - 1).astype(np.int64)
        out += wgt[:, None] * img[yi, xi]
        touched.append((xi, yi, wgt))
    return out, touched


# ---- PNG: 8-bit RGBA, one IDAT, filter 0 on every row; stdlib zlib only
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind, data):
    import zlib
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(rgba, level=1):
    """uint8 [H, W, 4] -> the bytes of an 8-bit RGBA PNG: IHDR, one IDAT (zlib at ``level`` 0 .. 9, 0 = stored; every row has filter type 0), IEND."""
    import zlib
    a = np.ascontiguousarray(rgba, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"png_bytes: expected uint8 [H, W, 4], got {a.shape}")
    if isinstance(level, (bool, np.bool_)) or int(level) != level or not 0 <= level <= 9:
        raise ValueError(f"png_bytes: level must be an integer in [0, 9], got {level!r}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 4 * W), np.uint8)
    rows[:, 1:] = a.reshape(H, 4 * W)
    return (_PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)) + _png_chunk(b"IDAT", zlib.compress(rows.data, int(level)))
            + _png_chunk(b"IEND", b""))


def png_image(raw):
    """The bytes of a PNG written by png_bytes -> uint8 [H, W, 4]; checks every chunk's CRC.  Not a general PNG reader: 8-bit RGBA, filter 0 only."""
    import zlib
    if raw[:8] != _PNG_MAGIC:
        raise ValueError("png: bad signature")
    off, idat, head = 8, [], None
    while off < len(raw):
        n, = struct.unpack_from(">I", raw, off)
        kind, data = raw[off + 4:off + 8], raw[off + 8:off + 8 + n]
        if struct.unpack_from(">I", raw, off + 8 + n)[0] != zlib.crc32(kind + data) & 0xFFFFFFFF:
            raise ValueError(f"png: bad CRC in chunk {kind!r}")
        off += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif kind == b"IDAT":
            idat.append(data)
        elif kind == b"IEND":
            break
    if head is None or head[2:] != (8, 6, 0, 0, 0):
        raise ValueError(f"png: not an 8-bit RGBA image without interlace ({head})")
    W, H = head[:2]
    rows = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(H, 1 + 4 * W)
    if rows[:, 0].any():
        raise ValueError("png: a row filter other than 0")
    return np.ascontiguousarray(rows[:, 1:]).reshape(H, W, 4)


def read_png(path):
    """A file written with png_bytes -> uint8 [H, W, 4]."""
    return png_image(open(path, "rb").read())


# ---- textured OBJ: mesh.obj + mesh.mtl + mesh.png side by side
OBJ_MATERIAL = "material_0"


def obj_texture_text_bytes(n, K, normals):
    """Closed-form size of the textured OBJ's records (== o2345_obj_texture_text_bytes) for n = 3 nt unwelded vertices: n "v", n "vt", [n "vn",] n / 3 "f"."""
    dn = len(str(int(n)))
    return n * (1 + 3 * (K + 11) + 1) + n * 25 + (n * 39 if normals else 0) + (n // 3) * (1 + 3 * (1 + (3 * dn + 2 if normals else 2 * dn + 1)) + 1)


def obj_texture_text_numpy(positions, uv, normals, K):
    """The records of the textured OBJ from printf-style formatting on the host (the definition the device packer is tested against): "v" records as in
    obj_text_numpy without colours; "vt %10.8f %10.8f" with the second field float32(1 - v) (OBJ's origin is bottom-left); "vn" as before; "f a/a b/b c/c"
    or "f a/a/a b/b/b c/c/c" over the unwelded corners 1 .. n in order, each token right-aligned in 2 d + 1 or 3 d + 2 bytes, d = decimal digits of n."""
    n, dn, w = positions.shape[0], len(str(positions.shape[0])), K + 10
    vfmt = "v" + (" %%%d.8f" % w) * 3 + "\n"
    out = [vfmt % tuple(r) for r in positions.astype(np.float64).tolist()]
    uv = np.asarray(uv, np.float32)
    flipped = (1.0 - uv[:, 1].astype(np.float64)).astype(np.float32)
    out += ["vt %10.8f %10.8f\n" % (a, b) for a, b in zip(uv[:, 0].astype(np.float64).tolist(), flipped.astype(np.float64).tolist())]
    if normals is not None:
        out += ["vn %11.8f %11.8f %11.8f\n" % tuple(r) for r in normals.astype(np.float64).tolist()]
    tok = (lambda a: "%d/%d/%d" % (a, a, a)) if normals is not None else (lambda a: "%d/%d" % (a, a))
    ffmt = "f" + (" %%%ds" % (3 * dn + 2 if normals is not None else 2 * dn + 1)) * 3 + "\n"
    out += [ffmt % (tok(3 * t + 1), tok(3 * t + 2), tok(3 * t + 3)) for t in range(n // 3)]
    return "".join(out).encode("ascii")


def obj_texture_names(path):
    """-> (path of the .mtl, path of the .png) next to ``path``, same stem"""
    stem = os.path.splitext(str(path))[0]
    return stem + ".mtl", stem + ".png"


def obj_texture_header(path):
    return ("mtllib %s\nusemtl %s\n" % (os.path.basename(obj_texture_names(path)[0]), OBJ_MATERIAL)).encode("ascii")


def obj_normal_map_name(path):
    """-> path of the normal map's .png next to ``path``: stem_normal.png"""
    return os.path.splitext(str(path))[0] + "_normal.png"


def obj_occlusion_name(path):
    """-> path of the occlusion map's .png next to ``path``: stem_occlusion.png"""
    return os.path.splitext(str(path))[0] + "_occlusion.png"


def write_obj_texture_files(path, text, png, normal_png=None, occlusion_png=None):
    """``path`` (the header + ``text``: bytes or a uint8 array), its .mtl (one material, map_Kd) and its .png.  ``normal_png``: the tangent-space normal
    map as a second file, stem_normal.png, named by a ``map_Bump`` and a ``norm`` line of the .mtl (the two spellings readers know); the "vn" records of
    ``text`` then carry the flat normals.  An OBJ has no place for tangents: a reader derives them from the texture coordinates, the GLB is the defined form.
    ``occlusion_png``: the ambient occlusion map as stem_occlusion.png, named by a ``map_Ka`` line (the ambient colour's texture: an .mtl has no occlusion
    slot, and this is the line readers map to one; the GLB is the defined form)."""
    mtl, img = obj_texture_names(path)
    with open(path, "wb") as fh:
        fh.write(obj_texture_header(path))
        fh.write(text if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, np.uint8).data)
    with open(mtl, "wb") as fh:
        fh.write(("newmtl %s\nKa 1.00000000 1.00000000 1.00000000\nKd 1.00000000 1.00000000 1.00000000\nKs 0.00000000 0.00000000 0.00000000\nmap_Kd %s\n"
                  % (OBJ_MATERIAL, os.path.basename(img))).encode("ascii"))
        if normal_png is not None:
            name = os.path.basename(obj_normal_map_name(path))
            fh.write(("map_Bump %s\nnorm %s\n" % (name, name)).encode("ascii"))
        if occlusion_png is not None:
            fh.write(("map_Ka %s\n" % os.path.basename(obj_occlusion_name(path))).encode("ascii"))
    with open(img, "wb") as fh:
        fh.write(png)
    if normal_png is not None:
        with open(obj_normal_map_name(path), "wb") as fh:
            fh.write(normal_png)
    if occlusion_png is not None:
        with open(obj_occlusion_name(path), "wb") as fh:
            fh.write(occlusion_png)


def read_obj_normal_map(path):
    """The normal map of a textured OBJ written above -> uint8 [H,W,4], or None for a file without one; checks that ``map_Bump`` and ``norm`` agree."""
    here = os.path.dirname(str(path))
    mtl = open(obj_texture_names(path)[0], "r", encoding="ascii").read().split("\n")
    names = {k: [l.split()[1] for l in mtl if l.startswith(k + " ")] for k in ("map_Bump", "norm")}
    if not names["map_Bump"] and not names["norm"]:
        return None
    assert names["map_Bump"] == names["norm"] and len(names["norm"]) == 1
    return read_png(os.path.join(here, names["norm"][0]))


def read_obj_occlusion(path):
    """The occlusion map of a textured OBJ written above (its ``map_Ka`` line) -> uint8 [H,W,4], or None for a file without one."""
    names = [l.split()[1] for l in open(obj_texture_names(path)[0], "r", encoding="ascii").read().split("\n") if l.startswith("map_Ka ")]
    return read_png(os.path.join(os.path.dirname(str(path)), names[0])) if names else None


def read_obj_texture(path):
    """A textured OBJ written above -> (positions float64 [N,3], uv float64 [N,2] with v flipped back to the image's top-left origin, normals or None,
    faces int32 [M,3] 0-based position indices, image uint8 [H,W,4]); checks that every face token names the same index for every attribute and that
    mtllib / usemtl / map_Kd lead to the image."""
    v, vt, vn, f, mtllib, usemtl = [], [], [], [], None, None
    with open(path, "r", encoding="ascii") as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([float(x) for x in t[1:4]])
            elif t[0] == "vt":
                vt.append([float(t[1]), 1.0 - float(t[2])])
            elif t[0] == "vn":
                vn.append([float(x) for x in t[1:4]])
            elif t[0] == "f":
                parts = [x.split("/") for x in t[1:]]
                assert all(len(set(q)) == 1 and len(q) == (3 if vn else 2) for q in parts), line
                f.append([int(q[0]) - 1 for q in parts])
            elif t[0] == "mtllib":
                mtllib = t[1]
            elif t[0] == "usemtl":
                usemtl = t[1]
    here = os.path.dirname(str(path))
    mtl = open(os.path.join(here, mtllib), "r", encoding="ascii").read().split("\n")
    assert mtl[0] == "newmtl " + usemtl
    image = [l.split()[1] for l in mtl if l.startswith("map_Kd ")][0]
    return (np.asarray(v, np.float64).reshape(-1, 3), np.asarray(vt, np.float64).reshape(-1, 2), np.asarray(vn, np.float64).reshape(-1, 3) if vn else None,
            np.asarray(f, np.int32).reshape(-1, 3), read_png(os.path.join(here, image)))


def write_textured(path, positions, uv, normals, image, bounds=None, png_level=1, tangents=None, normal_image=None, occlusion_image=None):
    """Host arrays of a textured mesh (texture_corners + pack_texture) -> ``path`` by its extension: a ``.glb`` with the PNG inside, or the ``.obj`` /
    ``.mtl`` / ``.png`` triple.  The host layer and the DEFINITION of both files; export_asset with ``texture=`` is the device path.
    ``tangents`` + ``normal_image`` (texture_frames + pack_normal_map; ``normals`` are then texture_frames' flat normals, which glTF needs beside TANGENT):
    the normal map too -- TANGENT and a second image in the ``.glb``, ``stem_normal.png`` next to the ``.obj`` (which cannot carry the tangents).
    ``occlusion_image`` (occlusion_values through pack_texture): the occlusion map too -- one more image in the ``.glb``, ``stem_occlusion.png`` next to
    the ``.obj``."""
    ext = _asset_ext(path)
    if ext == ".ply":
        raise ValueError("texture: a .ply has no texture coordinates; the output is .glb or .obj")
    if (tangents is None) != (normal_image is None) or (tangents is not None and normals is None):
        raise ValueError("texture: a normal map is tangents and a normal image, next to the flat normals")
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    png = png_bytes(image, png_level)
    normal_png = None if normal_image is None else png_bytes(normal_image, png_level)
    occlusion_png = None if occlusion_image is None else png_bytes(occlusion_image, png_level)
    if ext == ".glb":
        idx = np.arange(p.shape[0], dtype=np.uint32).reshape(-1, 3)
        write_glb_buffers(path, idx, p, None, normals, np.stack([p.min(0), p.max(0)]) if bounds is None else bounds, uv=uv, png=png, tangents=tangents,
                          normal_png=normal_png, occlusion_png=occlusion_png)
    else:
        write_obj_texture_files(path, obj_texture_text_numpy(p, uv, normals, obj_coordinate_digits(p if bounds is None else bounds)), png, normal_png,
                                occlusion_png)


def convert_mesh(ply_path, out_path, min_component_faces=0, keep_largest=False, smooth_iterations=0, decimate_cell=0, simplify_faces=0, fill_holes=0):
    """convert_mesh_format (utils/utils.py:31-47) for a mesh already on disk: read the PLY, exchange y and z, reverse the faces, write ``out_path`` by its
    extension (.glb or .obj) with the PLY's vertex colours.  ``min_component_faces`` / ``keep_largest``: filter_components on the way (off by default).
    ``smooth_iterations`` (0 = off): smooth_vertices with its default factors and pinning, after the filter, on the file's float32 positions cast to
    float64, the result cast back to float32.  That is NOT byte-equal to the device export with the same count, which smooths the float64 index
    coordinates before the frame transform rounds them to float32.
    ``decimate_cell`` (0 = off): decimate_mesh after the filter and before the smoothing, with the cell in the FILE's own units, on the float32 positions
    cast to float64, the result cast back to float32, the colours merged as decimate_mesh defines.  For the same reason that is not byte-equal to the
    device export, which clusters the index coordinates (cell in units of the grid spacing) and colours the new vertices.
    ``simplify_faces`` (0 = off): simplify_mesh down to that many faces after the decimation and before the smoothing, on the float32 positions cast to
    float64 (the kept vertices keep their float32 bits), the colours those of the kept vertices.  Not byte-equal to the device export either, which
    collapses the index coordinates and colours the kept vertices afterwards.
    There is no ``project_iterations`` here: projecting vertices onto the SDF's zero set (project_vertices, ops.mesh_project) needs the network, and a
    mesh file has none; for the same reason there is no ``texture_texel``.
    ``fill_holes`` (0 = off): fill_holes with that ``max_edges`` (FILL_HOLES_ALL: every hole) after the simplification and before the smoothing, as in the
    device chain, on the float32 positions cast to float64, the result cast back to float32; a new vertex takes the mean colour of its rim.  Returns
    ``out_path``."""
    ext = _asset_ext(out_path)
    if ext == ".ply":
        raise ValueError("convert_mesh: the output is .glb or .obj")
    smooth_iterations = _check_smooth_args(smooth_iterations, 0.5, -0.53)[0]
    decimate_cell = _check_cell(decimate_cell)
    v, f, c = read_ply(ply_path)
    if min_component_faces or keep_largest:
        v, f, c, _, _, _ = filter_components(v, f, c, None, min_component_faces, keep_largest)
    if decimate_cell:
        v, f, c, _, _ = decimate_mesh(v.astype(np.float64), f, decimate_cell, c)
        v = v.astype(np.float32)
    if simplify_faces:
        v, f, c, _, _, _ = simplify_mesh(v.astype(np.float64), f, simplify_faces, colors=c)
        v = v.astype(np.float32)
    if fill_holes:
        v, f, c, _, _, _ = _fill_holes(v.astype(np.float64), f, fill_holes, c)
        v = v.astype(np.float32)
    if smooth_iterations:
        v = smooth_vertices(v.astype(np.float64), f, smooth_iterations).astype(np.float32)
    v, f = to_asset_frame(v, f)
    (write_glb if ext == ".glb" else write_obj)(out_path, v, f, c)
    return out_path


def textured_asset_buffers(verts_idx, tris, grid_R, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None, normals=None,
                           texture=None):
    """The device buffers of export_asset's textured branch, without a file (arguments as for export_asset; ``texture`` is required, the mesh not empty):
    the same ops calls in the same order -> dict(pos float32 [3M,3] in the asset frame, uv float32 [3M,2], image uint8 [H,W,4], idx, bounds[, nrm]; with
    ``texture["grad"]`` nrm float32 [3M,3] (the flat normals), tan float32 [3M,4], nimage uint8 [H,W,4] and counters; with ``texture["occlusion_hits"]``
    oimage uint8 [H,W,4], occlusion_values in the colour atlas's own packing), all on the device.  What
    ops.mesh_raster_textured / pipeline.render_textured_mesh render; nothing synchronises."""
    from . import ops
    if texture is None or not int(verts_idx.shape[0]) or not int(tris.shape[0]):
        raise ValueError("textured_asset_buffers: a texture dict and a mesh with triangles are needed")
    m = int(tris.shape[0])
    image = ops.mesh_texture_pack(texture["rgb"], m, texture["texel"])
    tgrad = texture.get("grad")
    pos, uv, nrm, idx, bounds = ops.mesh_texture_corners(verts_idx, tris, texture["texel"], grid_R, bound_min, bound_max, scale_mat, trans_mat,
                                                         None if tgrad is not None else normals)
    tan = nimage = counters = None
    if tgrad is not None:                                              # the frames of the file's own buffers; NORMAL is the flat normal beside TANGENT
        nrm, tan, counters = ops.mesh_texture_frames(pos, uv)
        nimage = ops.mesh_texture_normal_pack(tgrad, nrm, tan, m, texture["texel"], rotation=trans_mat, counters=counters)
    oimage = None
    if texture.get("occlusion_hits") is not None:
        oimage = ops.mesh_texture_pack(ops.mesh_occlusion_values(texture["occlusion_hits"], texture["occlusion_samples"]), m, texture["texel"])
    out = dict(pos=pos, uv=uv, image=image, nrm=nrm, tan=tan, nimage=nimage, oimage=oimage, idx=idx, bounds=bounds, counters=counters)
    return {k: t for k, t in out.items() if t is not None}


def read_textured_glb(path):
    """A textured ``.glb`` written by this package -> the host arrays of textured_asset_buffers: dict(pos, uv, image[, nrm, tan, nimage][, oimage]).  Refused
    (ValueError): a file without a texture, or one whose index buffer is not 0, 1, 2, ... (the textured export is unwelded)."""
    pos, faces, _, normals, texture, normal_map, occlusion = _read_glb(path)
    if texture is None:
        raise ValueError(f"{path}: the file has no texture (export it with texture_texel)")
    if pos.shape[0] != 3 * faces.shape[0] or not np.array_equal(faces.reshape(-1), np.arange(pos.shape[0])):
        raise ValueError(f"{path}: a textured asset of this package has 3 M unwelded vertices and the indices 0, 1, 2, ...")
    out = dict(pos=np.ascontiguousarray(pos, np.float32), uv=np.ascontiguousarray(texture[0], np.float32), image=np.ascontiguousarray(texture[1]))
    if normal_map is not None:
        out.update(nrm=np.ascontiguousarray(normals, np.float32), tan=np.ascontiguousarray(normal_map[0], np.float32), nimage=np.ascontiguousarray(normal_map[1]))
    if occlusion is not None:
        out.update(oimage=np.ascontiguousarray(occlusion))
    return out


def export_asset(path, verts_idx, tris, grid_R, bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), scale_mat=None, trans_mat=None,
                 vertex_colors=None, normals=None, texture=None, png_level=None):
    """Device path by extension: ``.ply`` -> export_mesh (reconstruction frame, unchanged); ``.glb`` / ``.obj`` -> asset frame.  Arguments as for export_mesh;
    ``normals``: the SDF gradient at the vertices, fp32 [N,3] on the device (exported as unit normals), or None.  Buffers and OBJ text are produced on
    the device (csrc/mesh_export.hip), copied to the host once each and written in one go.  Returns (n_vertices, n_triangles).
    ``texture`` = {"texel": c, "rgb": fp32 [cells c^2, 3] on the device, the colours at ops.mesh_texture_points' points[, "stats": that op's counters]}:
    the textured asset instead (csrc/mesh_texture.hip) -- 3 M unwelded vertices with TEXCOORD_0 and no vertex colours, the atlas as a PNG inside the
    ``.glb`` or as ``.mtl`` + ``.png`` next to the ``.obj`` (zlib level ``png_level``, None: the config default); a ``.ply`` path is refused.
    ``texture["grad"]`` (fp32 [cells c^2, 3] on the device: the raw SDF gradient at the same points): a tangent-space normal map too -- ops.mesh_texture_frames
    on the corner buffers, ops.mesh_texture_normal_pack with the 3x3 of ``trans_mat``; TANGENT and a second image in the ``.glb``, ``stem_normal.png`` next
    to the ``.obj``.  NORMAL is then the flat normal of the file's triangles whatever ``normals`` says (glTF needs NORMAL beside TANGENT, and the map is
    relative to it); ``texture["normal_counts"]`` is set to the three counts (ops.normal_map_counts).  Still one synchronisation.
    ``texture["occlusion_hits"]`` (int32 [cells c^2] on the device: ops.mesh_occlusion at the texel points) with ``texture["occlusion_samples"]``: the
    ambient occlusion map too, (S - hits) / S in the atlas's own packing -- the occlusionTexture of the ``.glb``, ``stem_occlusion.png`` and a ``map_Ka``
    line next to the ``.obj``; ``texture["occlusion_info"]`` is set to the dict of ``texture["occlusion_counts"]`` (device int64 [4]; occlusion_report).  Still one synchronisation."""
    ext = _asset_ext(path)
    if texture is not None and ext == ".ply":
        raise ValueError("texture: a .ply has no texture coordinates; the output is .glb or .obj")
    if ext == ".ply":
        return export_mesh(path, verts_idx, tris, grid_R, bound_min, bound_max, scale_mat, trans_mat, vertex_colors)
    from . import ops
    n, m = int(verts_idx.shape[0]), int(tris.shape[0])
    if texture is not None and n and m:
        from . import config
        level = config.mesh_texture_png_level(png_level)
        b = textured_asset_buffers(verts_idx, tris, grid_R, bound_min, bound_max, scale_mat, trans_mat, normals, texture)
        image, pos, uv, nrm, idx, bounds = b["image"], b["pos"], b["uv"], b.get("nrm"), b["idx"], b["bounds"]
        tan, nimage, counters, oimage = b.get("tan"), b.get("nimage"), b.get("counters"), b.get("oimage")
        text = ops.obj_texture_text(pos, uv, nrm, bounds=bounds) if ext == ".obj" else None
        dev = dict(image=image, text=text)
        if ext == ".glb":
            dev.update(idx=idx, pos=pos, nrm=nrm, tan=tan, uv=uv, bounds=bounds)
        dev.update(nimage=nimage, stats=texture.get("stats"), counters=counters, oimage=oimage, ocounts=texture.get("occlusion_counts") if oimage is not None else None)
        dev = {k: t for k, t in dev.items() if t is not None}
        host = dict(zip(dev, ops.to_host_numpy(*dev.values())))       # the one synchronisation of the whole chain
        if "stats" in host:
            ops.texture_check(host["stats"])
        if "counters" in host:
            texture["normal_counts"] = ops.normal_map_counts(host["counters"])
        if "ocounts" in host:
            texture["occlusion_info"] = occlusion_report(host["ocounts"])
        images = [host[k] for k in ("image", "nimage", "oimage") if k in host]
        if len(images) > 1:                                           # zlib releases the interpreter lock: the images compress side by side
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=len(images)) as pool:
                pngs = list(pool.map(lambda a: png_bytes(a, level), images))
        else:
            pngs = [png_bytes(images[0], level)]
        png = pngs[0]
        normal_png = pngs[1] if "nimage" in host else None
        occlusion_png = pngs[-1] if "oimage" in host else None
        if ext == ".obj":
            write_obj_texture_files(path, host["text"], png, normal_png, occlusion_png)
        else:
            write_glb_buffers(path, host["idx"].view(np.uint32), host["pos"], None, host.get("nrm"), host["bounds"], uv=host["uv"], png=png,
                              tangents=host.get("tan"), normal_png=normal_png, occlusion_png=occlusion_png)
        return 3 * m, m
    if n == 0 or m == 0:
        if ext == ".glb":
            raise ValueError("GLB export: an empty mesh has no valid glTF form (accessors need count >= 1)")
        open(path, "wb").close()                                      # a valid OBJ with no records
        return n, m
    pos, rgba, nrm, idx, bounds = ops.mesh_asset_pack(verts_idx, tris, grid_R, bound_min, bound_max, scale_mat, trans_mat, vertex_colors, normals)
    if ext == ".glb":
        host = ops.to_host_numpy(*[t for t in (idx, pos, rgba, nrm, bounds) if t is not None])
        h_idx, h_pos = host[0].view(np.uint32), host[1]
        h_rgba = host[2] if rgba is not None else None
        h_nrm = host[2 + (rgba is not None)] if nrm is not None else None
        write_glb_buffers(path, h_idx, h_pos, h_rgba, h_nrm, host[-1])
    else:
        text = ops.obj_text(pos, idx, rgba, nrm, bounds=bounds)
        with open(path, "wb") as fh:
            fh.write(ops.to_host_numpy(text)[0].data)
    return n, m


# ------------------------------------------------------------------------------------------------------------------ mesh-to-mesh distance
# the functions below are the host twin of csrc/mesh_distance.hip and the DEFINITION of its results: samples, d2 and nearest to the last bit.  All
# arithmetic is float64, one operation at a time, in the order written; a dot product is (x x + y y) + z z.
DISTANCE_MAX_LEVEL = 64
DISTANCE_MAX_SAMPLES = 2 ** 28
DISTANCE_MAX_THRESHOLDS = 8


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _check_spacing(spacing):
    """-> None (one sample per triangle) or the finite float > 0"""
    if spacing is None:
        return None
    if isinstance(spacing, (bool, np.bool_)) or not isinstance(spacing, (int, float, np.integer, np.floating)) or not (np.isfinite(spacing) and spacing > 0):
        raise ValueError(f"mesh_distance: spacing must be None or a finite float > 0, got {spacing!r}")
    return float(spacing)


def _check_thresholds(thresholds):
    th = [float(t) for t in thresholds]
    if len(th) > DISTANCE_MAX_THRESHOLDS:
        raise ValueError(f"mesh_distance: {len(th)} thresholds; at most {DISTANCE_MAX_THRESHOLDS}")
    if not all(np.isfinite(t) and t >= 0 for t in th):
        raise ValueError(f"mesh_distance: thresholds must be finite and >= 0, got {thresholds!r}")
    return th


def _distance_mesh(verts, faces, what):
    """-> (vertices float64 [N,3], faces int64 [M,3]); raises on an index out of range or a non-finite coordinate of a referenced vertex"""
    p = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64, copy=False)
    if f.size and (f.min() < 0 or f.max() >= p.shape[0]):
        raise ValueError(f"{what}: faces index outside 0 .. {p.shape[0] - 1}")
    if f.size and not np.isfinite(p[f.reshape(-1)]).all():
        raise ValueError(f"{what}: non-finite vertex coordinate")
    return p, f


def _normal2(P0, P1, P2):
    e1, e2 = P1 - P0, P2 - P0
    n = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                  e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
    return _dot3(n, n)


def sample_levels(verts, faces, spacing):
    """k_t of every triangle: 1 without a spacing, else the smallest integer k in [1, 64] with (k spacing)(k spacing) >= L2, L2 the largest of the squared
    lengths of P1 - P0, P2 - P1, P0 - P2, and 64 if there is none.  No square root and no division decide it."""
    p, f = _distance_mesh(verts, faces, "sample_levels")
    spacing = _check_spacing(spacing)
    k = np.ones(f.shape[0], np.int64)
    if spacing is None or not f.shape[0]:
        return k
    P = p[f]
    e = [P[:, 1] - P[:, 0], P[:, 2] - P[:, 1], P[:, 0] - P[:, 2]]
    L2 = np.maximum(np.maximum(_dot3(e[0], e[0]), _dot3(e[1], e[1])), _dot3(e[2], e[2]))
    k[:] = DISTANCE_MAX_LEVEL
    for kk in range(DISTANCE_MAX_LEVEL - 1, 0, -1):                   # descending: the smallest k that passes is written last
        ks = float(kk) * spacing
        k[ks * ks >= L2] = kk
    # the test is monotone in k (products of non-negative floats round monotonically), so "the smallest" and "the last written" agree
    return k


def sample_weights(k):
    """The barycentric weights of the k^2 samples of one triangle, float64 [k^2, 3]: upright sub-triangles first (j = 0 .. k - 1, i = 0 .. k - 1 - j: w1 =
    (3 i + 1) / (3 k), w2 = (3 j + 1) / (3 k)), then the inverted ones (j = 0 .. k - 2, i = 0 .. k - 2 - j: w1 = (3 i + 2) / (3 k), w2 = (3 j + 2) / (3 k));
    w0 = (1 - w1) - w2."""
    rows = [(i, j, 1) for j in range(k) for i in range(k - j)] + [(i, j, 2) for j in range(k - 1) for i in range(k - 1 - j)]
    ij = np.asarray(rows, np.int64)
    w1 = (3 * ij[:, 0] + ij[:, 2]) / float(3 * k)
    w2 = (3 * ij[:, 1] + ij[:, 2]) / float(3 * k)
    return np.stack([(1.0 - w1) - w2, w1, w2], 1)


def surface_samples(verts, faces, spacing=None):
    """Area-weighted samples of a mesh's surface (host twin of ops.mesh_surface_samples) -> (points float64 [n,3], weight float64 [n], triangle int32
    [n]).  Triangle t is split regularly into k_t^2 sub-triangles (sample_levels) and sampled at their centroids (sample_weights): p = (w0 P0 + w1 P1) +
    w2 P2; every sample of t weighs area_t / k_t^2, area_t = 0.5 sqrt(n . n), n = (P1 - P0) x (P2 - P0) -- a triangle without an area still yields its
    samples, of weight 0.  Samples are numbered triangle-major.  Refused (ValueError): 2^28 samples or more, a non-finite coordinate, an index outside
    [0, N), a spacing that is not None or a finite float > 0."""
    p, f = _distance_mesh(verts, faces, "surface_samples")
    k = sample_levels(p, f, spacing)
    k2 = k * k
    n = int(k2.sum())
    if n >= DISTANCE_MAX_SAMPLES:
        raise ValueError(f"surface_samples: {n} samples; the limit is 2^28 - 1 (raise the spacing)")
    off = np.cumsum(k2) - k2
    pts, wgt, tri = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    for K in np.unique(k):
        idx = np.nonzero(k == K)[0]
        w = sample_weights(int(K))
        for s in range(0, idx.size, 4096):
            sel = idx[s:s + 4096]
            P = p[f[sel]]                                             # [m, 3 corners, 3]
            x = (w[None, :, 0, None] * P[:, None, 0] + w[None, :, 1, None] * P[:, None, 1]) + w[None, :, 2, None] * P[:, None, 2]
            at = (off[sel][:, None] + np.arange(int(K) * int(K))[None]).reshape(-1)
            pts[at] = x.reshape(-1, 3)
            wgt[at] = np.repeat(0.5 * np.sqrt(_normal2(P[:, 0], P[:, 1], P[:, 2])) / float(int(K) * int(K)), int(K) * int(K))
            tri[at] = np.repeat(sel, int(K) * int(K)).astype(np.int32)
    return pts, wgt, tri


def closest_point_triangle(p, A, B, C, return_point=False):
    """Squared distance from points to triangles, broadcast over the leading axes (all [..., 3]) -> (d2 float64, region uint8): |p - q|^2 with q from the
    region walk of Ericson, Real-Time Collision Detection 5.1.5, the regions tested in the book's order -- 0 vertex A, 1 vertex B, 2 edge AB, 3 vertex C,
    4 edge AC, 5 edge BC, 6 face.  The first region whose test passes gives q; this code, one operation per line, is the definition.  ``return_point``
    adds q float64 [..., 3] as a third result (the alignment's point-to-plane terms need it)."""
    with np.errstate(all="ignore"):
        ab = B - A
        ac = C - A
        ap = p - A
        d1 = _dot3(ab, ap)
        d2 = _dot3(ac, ap)
        bp = p - B
        d3 = _dot3(ab, bp)
        d4 = _dot3(ac, bp)
        cp = p - C
        d5 = _dot3(ab, cp)
        d6 = _dot3(ac, cp)
        t1 = d1 * d4
        t2 = d3 * d2
        vc = t1 - t2
        t1 = d5 * d2
        t2 = d1 * d6
        vb = t1 - t2
        t1 = d3 * d6
        t2 = d5 * d4
        va = t1 - t2
        s43 = d4 - d3
        s56 = d5 - d6
        tests = [(d1 <= 0.0) & (d2 <= 0.0),
                 (d3 >= 0.0) & (d4 <= d3),
                 (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
                 (d6 >= 0.0) & (d5 <= d6),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0),
                 (va <= 0.0) & (s43 >= 0.0) & (s56 >= 0.0)]
        region = np.full(tests[0].shape, 6, np.uint8)
        for r in range(5, -1, -1):                                    # the first test that passes wins
            region = np.where(tests[r], np.uint8(r), region)
        shape = region.shape + (3,)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = s43 / (s43 + s56)
        den = 1.0 / ((va + vb) + vc)
        v = vb * den
        w = vc * den
        q = (A + ab * v[..., None]) + ac * w[..., None]
        q = np.where((region == 5)[..., None], B + w_bc[..., None] * (C - B), q)
        q = np.where((region == 4)[..., None], A + w_ac[..., None] * ac, q)
        q = np.where((region == 2)[..., None], A + v_ab[..., None] * ab, q)
        q = np.where((region == 3)[..., None], np.broadcast_to(C, shape), q)
        q = np.where((region == 1)[..., None], np.broadcast_to(B, shape), q)
        q = np.where((region == 0)[..., None], np.broadcast_to(A, shape), q)
        d = p - q
        return (_dot3(d, d), region, q) if return_point else (_dot3(d, d), region)


def closest_triangles(points, verts, faces, chunk=256):
    """For every point its closest triangle of a target mesh (host twin of ops.mesh_closest_triangle), by brute force -> (d2 float64 [n], nearest int32
    [n], region uint8 [n], ties int32 [n], degenerate).  A target triangle whose normal has n . n == 0 takes no part and is counted in ``degenerate``; d2
    is the minimum of closest_point_triangle over the others, ``nearest`` the smallest index among those that attain it, ``region`` that triangle's
    region, ``ties`` how many triangles attain the minimum bit for bit.  A target with no triangle left is an error."""
    p, f = _distance_mesh(verts, faces, "closest_triangles")
    x = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    P = p[f]
    usable = _normal2(P[:, 0], P[:, 1], P[:, 2]) != 0.0 if f.shape[0] else np.zeros(0, bool)
    index = np.nonzero(usable)[0]
    if not index.size:
        raise ValueError(f"closest_triangles: the target has no triangle with an area ({f.shape[0]} triangles, all degenerate)")
    A, B, C = P[index, 0][None], P[index, 1][None], P[index, 2][None]
    n = x.shape[0]
    d2, nearest, region, ties = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.int32)
    for s in range(0, n, chunk):
        m, reg = closest_point_triangle(x[s:s + chunk, None, :], A, B, C)
        m = np.where(np.isnan(m), np.inf, m)
        j = m.argmin(1)                                               # the first of equal minima: the smallest index
        rows = np.arange(j.size)
        best = m[rows, j]
        d2[s:s + chunk], nearest[s:s + chunk], region[s:s + chunk] = best, index[j], reg[rows, j]
        ties[s:s + chunk] = (m == best[:, None]).sum(1)
    return d2, nearest, region, ties, int(f.shape[0] - index.size)


def distance_summary(d2, weight, thresholds=()):
    """One direction's summary from the samples' squared distances and weights, d = sqrt(d2), W = sum w -> {"mean": sum w d / W, "rms": sqrt(sum w d^2 /
    W), "max": max d, "within": [sum w [d <= tau] / W per threshold], "samples", "area": W}.  The sums are math.fsum's (the device sums in another
    order; they agree to 1e-12)."""
    import math
    th = _check_thresholds(thresholds)
    d2, w = np.asarray(d2, np.float64), np.asarray(weight, np.float64)
    d = np.sqrt(d2)
    W = math.fsum(w)
    div = lambda s: s / W if W > 0 else float("nan")
    return {"mean": div(math.fsum(w * d)), "rms": math.sqrt(div(math.fsum(w * d2))) if W > 0 else float("nan"), "max": float(d.max()) if d.size else 0.0,
            "within": [div(math.fsum(w[d <= t])) for t in th], "samples": int(d.size), "area": W}


def distance_report(a_to_b, b_to_a, thresholds, degenerate_a, degenerate_b):
    """The two one-sided summaries -> the result of mesh_distance (shared with ops.mesh_distance)"""
    P, R = a_to_b["within"], b_to_a["within"]
    return {"a_to_b": a_to_b, "b_to_a": b_to_a, "chamfer": 0.5 * (a_to_b["mean"] + b_to_a["mean"]), "hausdorff": max(a_to_b["max"], b_to_a["max"]),
            "thresholds": list(thresholds), "precision": list(P), "recall": list(R),
            "fscore": [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(P, R)], "degenerate_targets": {"a": degenerate_a, "b": degenerate_b}}


def mesh_distance(va, fa, vb, fb, spacing=None, thresholds=(), return_samples=False, align=None):
    """Distance between mesh A (under test) and mesh B (the reference) as surfaces, on the host (the twin of ops.mesh_distance) -> {"a_to_b", "b_to_a": the
    one-sided summaries (distance_summary) of A's samples against B and of B's against A; "chamfer": the mean of the two means; "hausdorff": the larger
    of the two maxima; "thresholds"; "precision" = a_to_b.within, "recall" = b_to_a.within and "fscore" = 2 P R / (P + R) (0 when P + R == 0) per
    threshold; "degenerate_targets": {"a", "b"}, the triangles without an area that took no part as targets}.  Samples: surface_samples at ``spacing``
    (None: one per triangle).  ``return_samples`` adds "samples": {"a", "b"} -> {"points", "weight", "triangle", "d2", "nearest"}.  ``align`` (None: the
    meshes are taken to share a frame): True or a dict of align_meshes arguments (align_arguments) -- A is moved onto B by align_meshes first, the
    distances are those of the moved A, and "alignment" holds align_meshes' result."""
    th = _check_thresholds(thresholds)
    spacing = _check_spacing(spacing)
    va, fa = _distance_mesh(va, fa, "mesh_distance")
    vb, fb = _distance_mesh(vb, fb, "mesh_distance")
    alignment = None
    if align is not None and align is not False:
        alignment = align_meshes(va, fa, vb, fb, **align_arguments(align, spacing))
        va = transform_vertices(va, alignment["transform"])
    sides, degenerate, samples = {}, {}, {}
    for name, (v, f), (tv, tf), other in (("a_to_b", (va, fa), (vb, fb), "b"), ("b_to_a", (vb, fb), (va, fa), "a")):
        pts, w, tri = surface_samples(v, f, spacing)
        d2, nearest, _, _, degenerate[other] = closest_triangles(pts, tv, tf)
        sides[name] = distance_summary(d2, w, th)
        samples[name[0]] = {"points": pts, "weight": w, "triangle": tri, "d2": d2, "nearest": nearest}
    out = distance_report(sides["a_to_b"], sides["b_to_a"], th, degenerate["a"], degenerate["b"])
    if return_samples:
        out["samples"] = samples
    if alignment is not None:
        out["alignment"] = alignment
    return out


def read_mesh(path):
    """A mesh file by its extension (.ply, .glb, .obj) -> (vertices float64 [N,3], faces int32 [M,3], extension)"""
    ext = _asset_ext(path)
    v, f = {".ply": read_ply, ".glb": read_glb, ".obj": read_obj}[ext](path)[:2]
    return np.asarray(v, np.float64), f, ext


def load_mesh_pair(path_a, path_b):
    """Two mesh files in one frame -> ((va, fa), (vb, fb)): where one is a PLY and the other an asset, the PLY's mesh goes through to_asset_frame (an
    isometry, so nothing else needs converting)."""
    va, fa, ea = read_mesh(path_a)
    vb, fb, eb = read_mesh(path_b)
    if ea == ".ply" and eb != ".ply":
        va, fa = to_asset_frame(va, fa)
    if eb == ".ply" and ea != ".ply":
        vb, fb = to_asset_frame(vb, fb)
    return (va, fa), (vb, fb)


def compare_mesh_files(path_a, path_b, spacing=None, thresholds=(), return_samples=False, align=None):
    """mesh_distance of two mesh files (.ply, .glb, .obj; load_mesh_pair brings them into one frame)"""
    (va, fa), (vb, fb) = load_mesh_pair(path_a, path_b)
    return mesh_distance(va, fa, vb, fb, spacing, thresholds, return_samples, align)


# ------------------------------------------------------------------------------------------------------------------ mesh alignment
# the functions below are the host twin of csrc/mesh_align.hip and the DEFINITION of its results: the moved points, d2, nearest and the 48 terms of every
# (transform, sample) pair to the last bit (float64, one operation at a time, in the order written), the sums of a moments row as math.fsum of the terms.
# similarity_step and align_run -- the 7 x 7 solve and the loop -- are shared with the device path (ops.mesh_align), which only supplies the rows.
ALIGN_MAX_TRANSFORMS = 64
ALIGN_COLUMNS = 48
ALIGN_DEFAULT_AZIMUTHS = 8                       # what ``align=True`` searches: the azimuth of a single-image reconstruction is unknown


def _align_matrix(T, what):
    """3 x 4, 4 x 4 or 12 numbers -> float64 [3,4], finite"""
    T = np.asarray(T, np.float64)
    if T.shape == (4, 4):
        T = T[:3]
    elif T.shape == (12,):
        T = T.reshape(3, 4)
    if T.shape != (3, 4):
        raise ValueError(f"mesh_align: {what} must be a 3 x 4 or 4 x 4 matrix, got shape {T.shape}")
    if not np.isfinite(T).all():
        raise ValueError(f"mesh_align: {what} has a non-finite entry")
    return np.ascontiguousarray(T)


def _check_max_distance(max_distance):
    """-> the truncation distance tau as a float; 0.0 (None) means none"""
    if max_distance is None:
        return 0.0
    if isinstance(max_distance, (bool, np.bool_)) or not isinstance(max_distance, (int, float, np.integer, np.floating)) or not (
            np.isfinite(max_distance) and max_distance >= 0):
        raise ValueError(f"mesh_align: max_distance must be None or a finite float >= 0, got {max_distance!r}")
    return float(max_distance)


def _check_candidates(candidates):
    """None (the identity alone) or [K,3,3], 1 <= K <= 64, finite -> float64 [K,3,3]"""
    if candidates is None:
        return np.eye(3)[None].copy()
    R = np.asarray(candidates, np.float64)
    if R.ndim != 3 or R.shape[1:] != (3, 3):
        raise ValueError(f"mesh_align: candidates must be None or rotations [K,3,3], got shape {R.shape}")
    if not 1 <= R.shape[0] <= ALIGN_MAX_TRANSFORMS:
        raise ValueError(f"mesh_align: {R.shape[0]} candidates; between 1 and {ALIGN_MAX_TRANSFORMS}")
    if not np.isfinite(R).all():
        raise ValueError("mesh_align: candidates has a non-finite entry")
    return R


def rodrigues(omega):
    """The rotation by |omega| about omega: I + (sin t / t) K + ((1 - cos t) / t^2) K^2, K the cross-product matrix; the series below t = 1e-4"""
    w = np.asarray(omega, np.float64).reshape(3)
    t2 = float(w @ w)
    t = np.sqrt(t2)
    a, b = (1.0 - t2 / 6.0, 0.5 - t2 / 24.0) if t < 1e-4 else (np.sin(t) / t, (1.0 - np.cos(t)) / t2)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * K + b * (K @ K)


def rotation_candidates(n_azimuth, up=(0.0, 0.0, 1.0)):
    """-> float64 [n,3,3]: the rotations by 360 j / n degrees about ``up``, j = 0 .. n - 1 (j = 0 is the identity, to the bit)"""
    if isinstance(n_azimuth, (bool, np.bool_)) or not isinstance(n_azimuth, (int, np.integer)) or not 1 <= n_azimuth <= ALIGN_MAX_TRANSFORMS:
        raise ValueError(f"mesh_align: n_azimuth must be an integer in 1 .. {ALIGN_MAX_TRANSFORMS}, got {n_azimuth!r}")
    up = np.asarray(up, np.float64)
    if up.shape != (3,) or not np.isfinite(up).all() or not up.any():
        raise ValueError(f"mesh_align: up must be three finite numbers, not all zero, got {up!r}")
    axis = up / np.sqrt(up @ up)
    return np.stack([np.eye(3) if j == 0 else rodrigues(axis * (2.0 * np.pi * j / int(n_azimuth))) for j in range(int(n_azimuth))])


def align_apply(T, p):
    """ma_apply: T [..., 12] (the rows of [M | t]) and p [..., 3], broadcast -> x [..., 3], x_k = ((M_k0 p_0 + M_k1 p_1) + M_k2 p_2) + t_k"""
    T, p = np.asarray(T, np.float64), np.asarray(p, np.float64)
    return np.stack([((T[..., 4 * k] * p[..., 0] + T[..., 4 * k + 1] * p[..., 1]) + T[..., 4 * k + 2] * p[..., 2]) + T[..., 4 * k + 3] for k in range(3)], -1)


def transform_vertices(verts, T):
    """Vertices [N,3] under the transform T (3 x 4 or 4 x 4) -> float64 [N,3] (align_apply; ops.mesh_transform is its device form)"""
    return align_apply(_align_matrix(T, "transform").reshape(12), np.asarray(verts, np.float64).reshape(-1, 3))


def align_sample_terms(x, q, A, B, C, c, w):
    """ma_jacobian and ma_terms of csrc/mesh_align_math.h: moved points x, their closest points q on triangles (A, B, C) (all [..., 3]), the pivot c [3]
    and weights w [...] -> (terms [..., 35], J [..., 7], b [...]).  x' = x - c, n = ((B - A) x (C - A)) / sqrt(n . n), J = (x' x n, n, n . x'),
    b = n . (q - x); terms: (w J_i) J_j for i <= j, row-major, then (w J_i) b."""
    with np.errstate(all="ignore"):
        e1, e2 = B - A, C - A
        m = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
        l = np.sqrt(_dot3(m, m))
        n = m / l[..., None]
        xp = x - np.asarray(c, np.float64)
        J = np.stack([xp[..., 1] * n[..., 2] - xp[..., 2] * n[..., 1], xp[..., 2] * n[..., 0] - xp[..., 0] * n[..., 2],
                      xp[..., 0] * n[..., 1] - xp[..., 1] * n[..., 0], n[..., 0], n[..., 1], n[..., 2], _dot3(n, xp)], -1)
        b = _dot3(n, q - x)
        wj = w[..., None] * J
        terms = [wj[..., i] * J[..., j] for i in range(7) for j in range(i, 7)] + [wj[..., i] * b for i in range(7)]
        return np.stack(terms, -1), J, b


def align_terms(points, weights, transforms, verts=None, faces=None, max_distance=None, pivot=(0.0, 0.0, 0.0)):
    """What one step of the alignment adds up (host twin of o2345_mesh_align_step, per pair) -> {"terms" float64 [K,n,48], "moved" [K,n,3], "d2" [K,n],
    "nearest" int32 [K,n]}.  points [n,3], weights [n] or None (1), transforms [K,12] or [K,3,4]; the target (verts, faces), or none.  Pair (k, e): x =
    align_apply(T_k, p_e); d2 and nearest from closest_triangles of x (+inf and -1 when the target has no triangle with an area); MATCHED: nearest >= 0
    and d2 finite and >= 0; INLIER: matched and (tau == 0 or d2 <= tau tau), tau = max_distance.  Columns: 0 .. 34 align_sample_terms, 35 w, 36 w d2 (all
    for inliers); 37 w and 38 w min(d2, tau tau) for matched pairs; 39 .. 41 w x', 42 w |x'|^2 and 43 one for inliers (x' = x - pivot); 44 one for a
    matched pair that is no inlier; 45 one for an unmatched pair; 46, 47 zero.  Without a target every pair is an inlier with q = x and d2 = 0, columns
    0 .. 34 are zero, and nearest is -1."""
    tau = _check_max_distance(max_distance)
    p = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    n = p.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64).reshape(n)
    T = np.asarray(transforms, np.float64)
    T = T.reshape(-1, 12)
    K = T.shape[0]
    if not 1 <= K <= ALIGN_MAX_TRANSFORMS:
        raise ValueError(f"mesh_align: {K} transforms; between 1 and {ALIGN_MAX_TRANSFORMS}")
    if not np.isfinite(T).all():
        raise ValueError("mesh_align: a transform has a non-finite entry")
    c = np.asarray(pivot, np.float64).reshape(3)
    x = align_apply(T[:, None, :], p[None])
    terms = np.zeros((K, n, ALIGN_COLUMNS))
    d2, nearest = np.zeros((K, n)), np.full((K, n), -1, np.int32)
    wk = np.broadcast_to(w, (K, n))
    if faces is None:
        matched = np.ones((K, n), bool)
    else:
        tv, tf = _distance_mesh(verts, faces, "mesh_align")
        P = tv[tf]
        if tf.shape[0] and (_normal2(P[:, 0], P[:, 1], P[:, 2]) != 0.0).any():
            a, b = closest_triangles(x.reshape(-1, 3), tv, tf)[:2]
            d2, nearest = a.reshape(K, n), b.reshape(K, n)
        else:
            d2 = np.full((K, n), np.inf)
        matched = (nearest >= 0) & (d2 >= 0.0) & (d2 <= np.finfo(np.float64).max)
    tau2 = tau * tau
    inlier = matched & ((tau == 0.0) | (d2 <= tau2))
    with np.errstate(all="ignore"):
        xp = x - c
        terms[..., 37] = np.where(matched, wk, 0.0)
        terms[..., 38] = np.where(matched, wk * np.where(inlier, d2, tau2), 0.0)
        terms[..., 35] = np.where(inlier, wk, 0.0)
        terms[..., 36] = np.where(inlier, wk * d2, 0.0)
        terms[..., 39:42] = np.where(inlier[..., None], wk[..., None] * xp, 0.0)
        terms[..., 42] = np.where(inlier, wk * _dot3(xp, xp), 0.0)
        terms[..., 43] = inlier
        terms[..., 44] = matched & ~inlier
        terms[..., 45] = ~matched
        if faces is not None and inlier.any():
            tri = tf[np.maximum(nearest, 0)]
            A, B, C = tv[tri[..., 0]], tv[tri[..., 1]], tv[tri[..., 2]]
            q = closest_point_triangle(x, A, B, C, return_point=True)[2]
            terms[..., :35] = np.where(inlier[..., None], align_sample_terms(x, q, A, B, C, c, wk)[0], 0.0)
    return {"terms": terms, "moved": x, "d2": d2, "nearest": nearest}


def align_moments(terms):
    """The moments rows [K,48] of terms [K,n,48]: every column math.fsum's (the device sums in a fixed tree; they agree to 1e-12 of sum |term|)"""
    import math
    return np.array([[math.fsum(t[:, j]) for j in range(t.shape[1])] for t in np.asarray(terms)]).reshape(len(terms), ALIGN_COLUMNS)


def similarity_step(row, scale=True):
    """The Gauss-Newton update of one moments row (columns 0 .. 34: the upper triangle of sum w J J^T, row-major, and sum w J b) -> None when the system
    is singular or not finite ("degenerate"), else (M_inc float64 [3,3], shift float64 [3], u float64 [7]): u = (omega, tau, sigma) solves the 7 x 7
    system (the leading 6 x 6 with sigma = 0 when ``scale`` is off), M_inc = exp(sigma) rodrigues(omega), shift = tau.  compose_similarity applies it."""
    row = np.asarray(row, np.float64).reshape(-1)
    H = np.zeros((7, 7))
    H[np.triu_indices(7)] = row[:28]
    H = H + np.triu(H, 1).T
    g = row[28:35]
    m = 7 if scale else 6
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return None
    try:
        sol = np.linalg.solve(H[:m, :m], g[:m])
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(sol).all():
        return None
    u = np.zeros(7)
    u[:m] = sol
    return np.exp(u[6]) * rodrigues(u[:3]), u[3:6].copy(), u


def compose_similarity(T, M_inc, shift, pivot):
    """T [3,4] followed by x -> pivot + M_inc (x - pivot) + shift: M <- M_inc M, t <- M_inc (t - pivot) + pivot + shift"""
    c = np.asarray(pivot, np.float64)
    return np.concatenate([M_inc @ T[:, :3], (M_inc @ (T[:, 3] - c) + c + shift)[:, None]], 1)


def _align_score(row):
    return float(row[38] / row[37]) if row[37] > 0 and np.isfinite(row[38]) else float("inf")


def align_run(step, iterations=30, tol=1e-9, max_distance=None, scale=True, candidates=None, search_iterations=5, init=None):
    """The alignment loop over a supplier of moments rows (shared by align_meshes and ops.mesh_align).  ``step(side, transforms [K,12], pivot [3], tau,
    target)`` -> rows [K,48] of the samples of mesh ``side`` ("a" or "b") under the transforms, against B when ``target`` else without a target.
      pivot c and radius rho_B: the centroid and the rms radius of B's samples (two rows without a target: sum w x / W, then sum w |x - c|^2 / W).
      start of candidate rotation R_j: moment matching, s = rho_B / rho_A (1 without ``scale``), M = s R_j, t = c - s R_j c_A; with ``init`` (3 x 4 or
      4 x 4) instead x -> c + R_j (init(x) - c).  ``candidates`` None: the identity alone.
      search: all K > 1 candidates take ``search_iterations`` updates in lockstep (one row each per step; a degenerate one stops moving), then the one with
      the smallest score col38 / col37 is kept, ties to the smallest index, and goes on alone.  ``iterations`` bounds the kept candidate's updates in all.
      stop: an update with max(|omega|, |tau| / rho_B, |sigma|) < tol ("converged"), ``iterations`` updates, or a degenerate system.
    -> {"transform" [4,4], "scale", "rotation" [3,3], "translation" [3], "score", "rms", "inlier_fraction", "iterations", "converged", "candidate",
    "candidate_scores", "history": per evaluated transform of the kept candidate {"transform" [3,4], "score", "inliers", "rejected", "unmatched",
    "update": the size of the update taken from it, or None}, "pivot" [3]: the c of every row}."""
    for name, v in (("iterations", iterations), ("search_iterations", search_iterations)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"mesh_align: {name} must be an integer >= 0, got {v!r}")
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"mesh_align: tol must be a finite float >= 0, got {tol!r}")
    tau = _check_max_distance(max_distance)
    R = _check_candidates(candidates)
    T0 = None if init is None else _align_matrix(init, "init")
    K = R.shape[0]
    eye = np.eye(3, 4).reshape(1, 12)

    def centroid_radius(side):
        row = step(side, eye, np.zeros(3), 0.0, False)[0]
        if not (row[35] > 0 and np.isfinite(row[35:43]).all()):
            raise ValueError(f"mesh_align: mesh {side.upper()} has no surface to sample (total weight {float(row[35])!r})")
        c = row[39:42] / row[35]
        row = step(side, eye, c, 0.0, False)[0]
        return c, float(np.sqrt(row[42] / row[35]))

    c, rho_b = centroid_radius("b")
    c_a, rho_a = centroid_radius("a")
    if not (rho_a > 0 and rho_b > 0):
        raise ValueError(f"mesh_align: a mesh has no extent (rms radii {rho_a!r}, {rho_b!r})")
    T = np.zeros((K, 3, 4))
    for j in range(K):
        if T0 is None:
            s = rho_b / rho_a if scale else 1.0
            T[j, :, :3], T[j, :, 3] = s * R[j], c - s * (R[j] @ c_a)
        else:
            T[j] = compose_similarity(T0, R[j], np.zeros(3), c)

    def evaluate(Ts):
        rows = np.asarray(step("a", np.ascontiguousarray(Ts.reshape(-1, 12)), c, tau, True), np.float64).reshape(-1, ALIGN_COLUMNS)
        return rows

    def entry(Tk, row):
        return {"transform": Tk.copy(), "score": _align_score(row), "inliers": int(row[43]), "rejected": int(row[44]), "unmatched": int(row[45]), "update": None}

    def update(Tk, row):
        sol = similarity_step(row, scale)
        if sol is None:
            return None, None
        M_inc, shift, u = sol
        size = max(float(np.sqrt(u[:3] @ u[:3])), float(np.sqrt(shift @ shift)) / rho_b, abs(float(u[6])))
        return compose_similarity(Tk, M_inc, shift, c), size

    n_search = min(search_iterations, iterations) if K > 1 else 0
    alive, trails = [True] * K, [[] for _ in range(K)]
    for _ in range(n_search):
        rows = evaluate(T)
        for j in range(K):
            if alive[j]:
                trails[j].append(entry(T[j], rows[j]))
                new, size = update(T[j], rows[j])
                if new is None:
                    alive[j] = False
                else:
                    T[j], trails[j][-1]["update"] = new, size
    rows = evaluate(T)
    scores = [_align_score(r) for r in rows]
    kept = int(np.argmin(scores))                                     # the first of equal minima
    if not np.isfinite(scores[kept]):
        raise ValueError("mesh_align: no sample of A found a triangle of B (the target has no triangle with an area, or max_distance leaves no inlier)")
    Tk, row, history = T[kept].copy(), rows[kept], trails[kept]
    done, converged, stuck = len(history) if alive[kept] else iterations, False, not alive[kept]
    if history and alive[kept] and history[-1]["update"] < tol:
        converged = True
    while True:
        history.append(entry(Tk, row))
        if converged or stuck or done >= iterations:
            break
        new, size = update(Tk, row)
        if new is None:
            break
        Tk, done, history[-1]["update"] = new, done + 1, size
        row = evaluate(Tk[None])[0]
        converged = size < tol
    M = Tk[:, :3]
    s = float(np.cbrt(np.linalg.det(M)))
    full = np.eye(4)
    full[:3] = Tk
    n_updates = sum(1 for h in history if h["update"] is not None)
    return {"transform": full, "scale": s, "rotation": M / s, "translation": Tk[:, 3].copy(), "score": _align_score(row),
            "rms": float(np.sqrt(row[36] / row[35])) if row[35] > 0 else float("nan"), "inlier_fraction": float(row[35] / row[37]) if row[37] > 0 else 0.0,
            "iterations": n_updates, "converged": bool(converged), "candidate": kept, "candidate_scores": scores, "history": history, "pivot": c.copy()}


def align_meshes(va, fa, vb, fb, spacing=None, iterations=30, tol=1e-9, max_distance=None, scale=True, candidates=None, search_iterations=5, init=None):
    """The similarity transform (rotation, translation, uniform scale unless ``scale`` is off) that moves mesh A onto mesh B, on the host (the twin of
    ops.mesh_align and the definition): point-to-plane Gauss-Newton over A's surface samples (surface_samples at ``spacing``) against their closest
    triangles of B, from each of the ``candidates`` rotations ([K,3,3], e.g. rotation_candidates; None: the identity) -- see align_run for the loop, the
    stopping rule and the result.  ``max_distance``: samples farther than it from B take no part in the system, and count min(d2, max_distance^2) in the
    score.  One-sided: B's samples only give the pivot and the radius.  Refused (ValueError): what surface_samples refuses, iterations < 0, more than 64
    candidates, a negative or non-finite max_distance, an ``init`` that is not 3 x 4 or 4 x 4, non-finite entries."""
    spacing = _check_spacing(spacing)
    va, fa = _distance_mesh(va, fa, "mesh_align")
    vb, fb = _distance_mesh(vb, fb, "mesh_align")
    sets = {"a": surface_samples(va, fa, spacing)[:2], "b": surface_samples(vb, fb, spacing)[:2]}

    def step(side, transforms, pivot, tau, target):
        pts, w = sets[side]
        return align_moments(align_terms(pts, w, transforms, vb if target else None, fb if target else None, tau, pivot)["terms"])
    return align_run(step, iterations, tol, max_distance, scale, candidates, search_iterations, init)


def align_arguments(align, spacing=None):
    """The ``align`` argument of mesh_distance -> the keyword arguments of align_meshes: True searches ALIGN_DEFAULT_AZIMUTHS azimuths about z (the
    identity alone does not survive an unknown azimuth), a dict is taken as it is; the distance's ``spacing`` is the default of the alignment's."""
    if align is True:
        kw = {"candidates": rotation_candidates(ALIGN_DEFAULT_AZIMUTHS)}
    elif isinstance(align, dict):
        kw = dict(align)
    else:
        raise ValueError(f"mesh_distance: align must be None, True or a dict of mesh_align arguments, got {align!r}")
    kw.setdefault("spacing", spacing)
    return kw


def write_mesh(path, verts, faces):
    """A bare mesh to a file by its extension (.ply, .glb, .obj), positions as they are"""
    ext = _asset_ext(path)
    v, f = np.asarray(verts, np.float32), np.asarray(faces, np.int32)
    {".ply": write_ply_numpy, ".glb": write_glb, ".obj": write_obj_numpy}[ext](path, v, f)


# ------------------------------------------------------------------------------------------------------------------ mesh audit
# the functions below are the host twin of csrc/mesh_audit.hip and the DEFINITION of its results: counts, flags, per-triangle quality, minima and maxima
# to the last bit.  All arithmetic is float64, one operation at a time, in the order written; a dot product is (x x + y y) + z z.
AUDIT_QUALITY_SCALE = 6.928203230275509          # 4 sqrt(3): an equilateral triangle has quality 1
AUDIT_BINS = 10
AUDIT_VERTEX_BITS = {"boundary": 1, "nonmanifold": 2, "bowtie": 4, "unused": 8}
AUDIT_FACE_BITS = {"repeated": 1, "zero_area": 2, "boundary": 4, "nonmanifold": 8, "inconsistent": 16, "creased": 32}
# the integer counts of an audit: the names of the fields that hold them in the device's stats block (include/o2345.h, O2345AuditStats)
AUDIT_COUNTS = ("vertices", "edges", "faces", "repeated_faces", "zero_area_faces", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "creased_edges",
                "boundary_vertices", "nonmanifold_vertices", "bowtie_vertices", "unused_vertices")


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def audit_triangles(P0, P1, P2):
    """The per-triangle arithmetic of the audit (csrc/mesh_audit_math.h, au_triangle) on corner arrays [..., 3] -> dict(n, nn, area, vol, l, s, q): n = (P1 -
    P0) x (P2 - P0), nn = n . n, area = 0.5 sqrt(nn), vol = P0 . (P1 x P2), l = the squared lengths of P0P1, P1P2, P2P0, s = (l01 + l12) + l20, q = (4
    sqrt(3) area) / s, 0 where s == 0."""
    P0, P1, P2 = (np.asarray(P, np.float64) for P in (P0, P1, P2))
    with np.errstate(all="ignore"):                                     # products may overflow or underflow: the results are IEEE's either way
        n = _cross3(P1 - P0, P2 - P0)
        nn = _dot3(n, n)
        area = 0.5 * np.sqrt(nn)
        vol = _dot3(P0, _cross3(P1, P2))
        e = (P1 - P0, P2 - P1, P0 - P2)
        l = np.stack([_dot3(x, x) for x in e], -1)
        s = (l[..., 0] + l[..., 1]) + l[..., 2]
        q = np.where(s == 0.0, 0.0, (AUDIT_QUALITY_SCALE * area) / np.where(s == 0.0, 1.0, s))
    return {"n": n, "nn": nn, "area": area, "vol": vol, "l": l, "s": s, "q": q}


def audit_bins(q):
    """Histogram bin of every quality: min(9, floor(q 10)), -1 for a q that is not >= 0 (it enters no bin and no minimum)"""
    q = np.asarray(q, np.float64)
    ok = q >= 0.0
    with np.errstate(invalid="ignore"):
        b = np.minimum(float(AUDIT_BINS - 1), np.floor(np.where(ok, q, 0.0) * 10.0))
    return np.where(ok, b, -1.0).astype(np.int64)


def audit_report(counts, histogram, area, volume6, quality_sum, quality_min, edge2_min, edge2_max, components):
    """The raw results of an audit -> its report: what mesh_audit and ops.mesh_audit both return.  ``counts``: {name: int} over AUDIT_COUNTS; the doubles
    as the device's stats block holds them (sum of the volume terms, squared edge lengths).  Derived: euler = used vertices - edges + faces; watertight =
    no boundary, non-manifold or inconsistent edge, no bow-tie, no repeated triangle, at least one face; oriented = no inconsistent edge; genus =
    components - euler / 2 when watertight, else None; the quality and edge-length entries are None without a face."""
    import math
    out = {k: int(counts[k]) for k in AUDIT_COUNTS}
    faces = out["faces"]
    out["histogram"] = [int(x) for x in histogram]
    out["area"], out["volume"] = float(area), float(volume6) / 6.0
    out["quality_mean"] = float(quality_sum) / faces if faces else None
    out["quality_min"] = float(quality_min) if faces else None
    out["edge_min"] = math.sqrt(float(edge2_min)) if faces else None
    out["edge_max"] = math.sqrt(float(edge2_max)) if faces else None
    out["euler"] = out["vertices"] - out["edges"] + faces
    out["components"] = int(components)
    out["oriented"] = out["inconsistent_edges"] == 0
    out["watertight"] = bool(faces > 0 and out["boundary_edges"] == 0 and out["nonmanifold_edges"] == 0 and out["inconsistent_edges"] == 0
                             and out["bowtie_vertices"] == 0 and out["repeated_faces"] == 0)
    genus = out["components"] - out["euler"] / 2 if out["watertight"] else None
    out["genus"] = int(genus) if genus is not None and genus == int(genus) else genus
    return out


def mesh_audit(verts, faces, return_elements=False):
    """Audit of an indexed triangle mesh on the host (the twin of ops.mesh_audit, and the definition of its result): is it a closed, oriented 2-manifold,
    and how good are its triangles.  verts [N,3] (float64), faces int32 / int64 [M,3]; an index outside [0, N) and a non-finite coordinate are errors.
    Triangles: one with two equal indices is REPEATED -- counted, flagged, and no part of anything else; the others are the faces, with audit_triangles'
    normal, area, volume term and quality; zero-area iff n . n == 0.  Edges: half-edge 3 t + i runs from faces[t, i] to faces[t, (i + 1) % 3]; an undirected
    edge with m half-edges is boundary (m = 1), manifold (2) or non-manifold (>= 3); a manifold edge is inconsistent iff both half-edges run the same way,
    and a manifold, consistent edge whose triangles both have n . n > 0 is creased iff n . n' < 0 (a symptom, not an error: a tetrahedron's acute edges
    are creased).  Vertices: used (on a face), boundary (on a boundary edge), non-manifold (on an edge with m >= 3).  Fans: over the corners of the faces,
    every manifold edge joins, at each of its two ends, the corners of its two triangles; a vertex with two or more classes of corners that lies on no
    non-manifold edge is a bow-tie.  -> audit_report's dict: the counts of AUDIT_COUNTS, "histogram" (ten bins of quality), "area", "volume" (sum of the
    volume terms / 6: meaningful for a closed, consistent mesh), "quality_mean", "quality_min", "edge_min", "edge_max", "euler", "components" (the labels
    of component_labels that own a triangle), "oriented", "watertight", "genus".  The three sums are math.fsum's (the device sums in a fixed tree; they
    agree to 1e-12 of the sum of the terms' magnitudes).  ``return_elements`` adds "vertex_flags" uint8 [N] (AUDIT_VERTEX_BITS), "face_flags" uint8 [M]
    (AUDIT_FACE_BITS) and "quality" float64 [M] (0 for a repeated triangle).  Nothing depends on face order or on the rotation of a triangle's indices."""
    import math
    p = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64, copy=False)
    nv, nt = p.shape[0], f.shape[0]
    if nv >= 2 ** 30 or 6 * nt >= 2 ** 31:
        raise ValueError(f"mesh_audit: bad sizes ({nv} vertices, {nt} faces; the tables are int32)")
    if f.size and (f.min() < 0 or f.max() >= nv):
        raise ValueError(f"mesh_audit: faces index outside 0 .. {nv - 1}")
    if not np.isfinite(p).all():
        raise ValueError("mesh_audit: non-finite vertex coordinate")
    VB, FB = AUDIT_VERTEX_BITS, AUDIT_FACE_BITS
    repeated = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    live = np.flatnonzero(~repeated)                                    # the faces, ascending
    F = f[live]
    T = audit_triangles(p[F[:, 0]], p[F[:, 1]], p[F[:, 2]])
    face_flags = np.zeros(nt, np.uint8)
    face_flags[repeated] = FB["repeated"]
    zero = T["nn"] == 0.0
    face_flags[live[zero]] |= FB["zero_area"]
    quality = np.zeros(nt, np.float64)
    quality[live] = T["q"]
    bins = audit_bins(T["q"])
    # half-edges of the faces: id 3 t + i, from u to w
    hid = (3 * live[:, None] + np.arange(3)[None, :]).reshape(-1)
    u, w = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1)
    key, forward = np.minimum(u, w) * max(nv, 1) + np.maximum(u, w), u < w
    _, edge, m = np.unique(key, return_inverse=True, return_counts=True)
    edge = edge.reshape(-1)
    n_edges = m.size
    n_forward = np.bincount(edge, weights=forward, minlength=n_edges).astype(np.int64)
    order = np.argsort(edge, kind="stable")                              # half-edges grouped by edge, ascending id inside
    start = np.cumsum(m) - m
    is_boundary, is_manifold, is_nonmanifold = m == 1, m == 2, m >= 3
    inconsistent = is_manifold & (n_forward != 1)
    h1, h2 = order[start[is_manifold]], order[start[is_manifold] + 1]    # positions (in the half-edge arrays) of a manifold edge's two half-edges
    t1, t2 = h1 // 3, h2 // 3                                            # positions among the faces
    consistent = n_forward[is_manifold] == 1
    with np.errstate(all="ignore"):
        creased_m = consistent & (T["nn"][t1] > 0.0) & (T["nn"][t2] > 0.0) & (_dot3(T["n"][t1], T["n"][t2]) < 0.0)
    creased = np.zeros(n_edges, bool)
    creased[np.flatnonzero(is_manifold)[creased_m]] = True
    for name, on in (("boundary", is_boundary), ("nonmanifold", is_nonmanifold), ("inconsistent", inconsistent), ("creased", creased)):
        hit = on[edge].reshape(-1, 3).any(1)
        face_flags[live[hit]] |= FB[name]
    vbits = np.zeros(nv, np.uint8)
    for name, on in (("boundary", is_boundary), ("nonmanifold", is_nonmanifold)):
        sel = on[edge]
        vbits[u[sel]] |= VB[name]
        vbits[w[sel]] |= VB[name]
    # fans: union-find over the corners 3 t + i (component_labels on degenerate "faces" (x, y, y): the pairs to join)
    same = u[h1] == u[h2]                                                # both half-edges start at the same end
    c1u, c1w = hid[h1], 3 * live[t1] + (h1 % 3 + 1) % 3                  # the corners of triangle 1 at u (its half-edge's start) and at w
    c2s, c2e = hid[h2], 3 * live[t2] + (h2 % 3 + 1) % 3                  # the corners of triangle 2 at its half-edge's start and end
    x = np.concatenate([c1u, c1w])
    y = np.concatenate([np.where(same, c2s, c2e), np.where(same, c2e, c2s)])
    root = component_labels(np.stack([x, y, y], 1), 3 * nt)
    is_root = root[hid] == hid
    fans = np.bincount(u[is_root], minlength=nv)
    used = fans > 0
    bowtie = (fans >= 2) & ((vbits & VB["nonmanifold"]) == 0)
    vertex_flags = vbits | (bowtie * VB["bowtie"]).astype(np.uint8) | ((~used) * VB["unused"]).astype(np.uint8)
    counts = {"vertices": np.count_nonzero(used), "edges": n_edges, "faces": live.size, "repeated_faces": np.count_nonzero(repeated),
              "zero_area_faces": np.count_nonzero(zero), "boundary_edges": np.count_nonzero(is_boundary), "nonmanifold_edges": np.count_nonzero(is_nonmanifold),
              "inconsistent_edges": np.count_nonzero(inconsistent), "creased_edges": np.count_nonzero(creased),
              "boundary_vertices": np.count_nonzero(vbits & VB["boundary"]), "nonmanifold_vertices": np.count_nonzero(vbits & VB["nonmanifold"]),
              "bowtie_vertices": np.count_nonzero(bowtie), "unused_vertices": np.count_nonzero(~used)}
    binned = T["q"][bins >= 0]
    out = audit_report(counts, np.bincount(bins[bins >= 0], minlength=AUDIT_BINS), math.fsum(T["area"]), math.fsum(T["vol"]), math.fsum(T["q"]),
                       binned.min() if binned.size else np.inf, T["l"].min() if live.size else np.inf, T["l"].max() if live.size else 0.0,
                       np.unique(component_labels(f, nv)[f[:, 0]]).size)
    if return_elements:
        out.update(vertex_flags=vertex_flags, face_flags=face_flags, quality=quality)
    return out


# ------------------------------------------------------------------------------------------------------------------ hole filling
# the host twin of csrc/mesh_fill.hip and the DEFINITION of its result, to the last bit (include/o2345.h has the same text)
FILL_HOLES_ALL = 2 ** 31 - 1                     # max_edges that fills every hole
FILL_COUNTS = ("boundary", "holes", "filled", "too_long", "open", "longest", "vertices", "triangles")


def _check_max_edges(max_edges):
    """-> the longest hole that is filled, in edges: None = every hole, else an integer in [3, 2^31)"""
    if max_edges is None:
        return FILL_HOLES_ALL
    if isinstance(max_edges, bool) or int(max_edges) != max_edges or not 3 <= max_edges < 2 ** 31:
        raise ValueError(f"fill_holes: max_edges must be an integer in [3, 2^31) (a hole has at least three edges), got {max_edges!r}")
    return int(max_edges)


def boundary_loops(faces, n_vertices):
    """The boundary of a mesh as fill_holes reads it -> (origin, holes, n_open): ``origin`` int64 [B] the start vertex of every boundary half-edge in
    ascending half-edge order, ``holes`` the cycles as lists of positions in that order, each from its leader on in rank order, ordered by leader, and the
    number of boundary half-edges on chains.  Half-edge 3 t + i runs from faces[t, i] to faces[t, (i + 1) % 3]; a triangle with two equal indices takes no
    part; a half-edge is a boundary half-edge iff its undirected edge has no other half-edge.  A vertex is simple iff exactly one boundary half-edge
    leaves it and exactly one enters it; next(h) of a boundary half-edge that enters a simple vertex is the one that leaves it.  next is injective, so the
    boundary half-edges fall into cycles (the holes) and chains (which end at a vertex that is not simple)."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64, copy=False)
    nv = int(n_vertices)
    live = np.flatnonzero(~((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])))
    F = f[live]
    u, w = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1)                   # in ascending half-edge order: the faces ascend
    _, edge, m = np.unique(np.minimum(u, w) * max(nv, 1) + np.maximum(u, w), return_inverse=True, return_counts=True)
    on = m[edge.reshape(-1)] == 1
    bu, bw = u[on], w[on]
    nb = bu.size
    simple = (np.bincount(bu, minlength=nv) == 1) & (np.bincount(bw, minlength=nv) == 1)
    leaves = np.full(nv, -1, np.int64)
    leaves[bu] = np.arange(nb)                                          # read at simple vertices only: one writer there
    nxt = np.where(simple[bw], leaves[bw], -1)
    seen = np.zeros(nb, bool)
    starts = np.ones(nb, bool)
    starts[nxt[nxt >= 0]] = False                                       # without a predecessor: the head of a chain
    n_open = 0
    for j in np.flatnonzero(starts).tolist():
        while j >= 0:
            seen[j] = True
            n_open += 1
            j = int(nxt[j])
    holes = []
    for j in range(nb):                                                 # ascending: the first half-edge of a cycle that turns up is its leader
        if seen[j]:
            continue
        ring, k = [], j
        while not seen[k]:
            seen[k] = True
            ring.append(k)
            k = int(nxt[k])
        assert k == j and len(ring) >= 3, "a cycle of boundary half-edges has at least three"
        holes.append(ring)
    return bu, holes, n_open


def fill_holes(verts, faces, max_edges=None, colors=None, normals=None):
    """Closes the boundary loops of a mesh (host twin of ops.mesh_fill_holes, and the definition of its result, to the last bit) -> (verts float64
    [N + c,3], faces [M + k,3] in the dtype of ``faces``, colors, normals, hole int32 [k], info).  The holes are boundary_loops' cycles, ordered by their
    leader (the smallest half-edge); L = a hole's number of half-edges, o_k the origin of its half-edge of rank k (the distance from the leader along
    next).  A hole is filled iff L <= ``max_edges`` (None: every hole).  L == 3: one triangle (o_0, o_2, o_1), no new vertex.  L >= 4: one new vertex c,
    per coordinate acc = 0; acc = acc + P[o_k] for k = 0 .. L - 1 (one sequential float64 sum); c = acc / L; and the L triangles (o_{k+1 mod L}, o_k, c)
    in rank order.  Every new triangle carries the half-edge opposite to the one it closes: an oriented input stays oriented.  The input's vertices and
    faces come first, bit for bit and in order; the new vertices follow in hole order, the new triangles in hole order, then rank order; ``hole`` holds
    for every new triangle the number of its hole among the FILLED holes.  ``colors`` uint8 [N,3|4]: a new vertex takes, per channel, the mean of its
    rim rounded half up, (2 sum + L) // (2 L); ``normals`` float [N,3]: the mean of the rim's (a sequential float64 sum / L, cast back; not
    normalised).  ``info``: the counts of FILL_COUNTS -- boundary half-edges, holes, filled holes, holes left because L > max_edges, boundary half-edges
    on chains (left open: they end at a bow-tie of the rim, a non-manifold edge or inconsistently oriented neighbours), the longest hole, and the sizes of
    the output.  With no hole to fill the inputs themselves are returned.  A centroid fan is exact for a planar, star-shaped outline; for others it may
    fold over itself, and the mesh is combinatorially closed all the same.  Refused (ValueError): max_edges below 3, a face index outside [0, N), sizes
    beyond N + c < 2^30 or 3 (M + k) < 2^31."""
    max_edges = _check_max_edges(max_edges)
    p = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
    fin = np.asarray(faces).reshape(-1, 3)
    f = fin.astype(np.int64, copy=False)
    nv, nt = p.shape[0], f.shape[0]
    if nv >= 2 ** 30 or 3 * nt >= 2 ** 31:
        raise ValueError(f"fill_holes: bad sizes ({nv} vertices, {nt} faces; the tables are int32)")
    if f.size and (f.min() < 0 or f.max() >= nv):
        raise ValueError(f"fill_holes: faces index outside 0 .. {nv - 1}")
    origin, holes, n_open = boundary_loops(f, nv)
    filled = [ring for ring in holes if len(ring) <= max_edges]
    new_v, new_f, hole, new_c, new_n = [], [], [], [], []
    for number, ring in enumerate(filled):
        o, L = origin[ring], len(ring)
        if L == 3:
            new_f.append((o[0], o[2], o[1]))
            hole.append(number)
            continue
        acc = np.zeros(3, np.float64)
        for k in range(L):
            acc = acc + p[o[k]]
        c = nv + len(new_v)
        new_v.append(acc / np.float64(L))
        new_f += [(o[(k + 1) % L], o[k], c) for k in range(L)]
        hole += [number] * L
        if colors is not None:
            total = np.asarray(colors)[o].astype(np.int64).sum(axis=0)
            new_c.append(((2 * total + L) // (2 * L)).astype(np.uint8))
        if normals is not None:
            acc = np.zeros(3, np.float64)
            for k in range(L):
                acc = acc + np.asarray(normals)[o[k]].astype(np.float64)
            new_n.append(acc / np.float64(L))
    info = {"boundary": int(origin.size), "holes": len(holes), "filled": len(filled), "too_long": len(holes) - len(filled), "open": int(n_open),
            "longest": max((len(r) for r in holes), default=0), "vertices": nv + len(new_v), "triangles": nt + len(new_f)}
    if info["vertices"] >= 2 ** 30 or 3 * info["triangles"] >= 2 ** 31:
        raise ValueError(f"fill_holes: bad sizes ({info['vertices']} vertices, {info['triangles']} faces after the fill; the tables are int32)")
    hole = np.asarray(hole, np.int32).reshape(-1)
    if not filled:
        return verts, faces, colors, normals, hole, info
    v_out = np.concatenate([p, np.asarray(new_v, np.float64).reshape(-1, 3)])
    f_out = np.concatenate([fin, np.asarray(new_f, np.int64).reshape(-1, 3).astype(fin.dtype)])
    c_out, n_out = colors, normals
    if colors is not None and new_c:
        c_out = np.concatenate([np.asarray(colors), np.asarray(new_c, np.uint8).reshape(-1, np.asarray(colors).shape[1])])
    if normals is not None and new_n:
        n_out = np.concatenate([np.asarray(normals), np.asarray(new_n).astype(np.asarray(normals).dtype).reshape(-1, 3)])
    return v_out, f_out, c_out, n_out, hole, info


_fill_holes = fill_holes                         # for convert_mesh, whose keyword of that name hides the function


# ------------------------------------------------------------------------------------------------------------------ self-intersections
# the host twin of csrc/mesh_intersect.hip and the DEFINITION of its result, to the last bit (include/o2345.h has the same text; csrc/mesh_intersect_math.h
# the device form).  All arithmetic is float64, one operation at a time, in the order written; only comparisons decide.
INTERSECT_COUNTS = ("bad_index", "nonfinite", "faces", "skipped", "candidates", "pairs", "faces_hit", "max_hits")
INTERSECT_EXHAUSTIVE_MAX = 2 ** 16               # the device's exhaustive path (no grid) takes at most this many triangles


def intersect_orient(A, B, C, D):
    """orient(A, B, C, D) on arrays [..., 3]: a = A - D, b = B - D, c = C - D, X = b_y c_z - b_z c_y, Y = b_z c_x - b_x c_z, Z = b_x c_y - b_y c_x ->
    (a_x X + a_y Y) + a_z Z: six times the signed volume of the tetrahedron, unfiltered"""
    with np.errstate(all="ignore"):                                     # products may overflow or underflow: the results are IEEE's either way
        a, b, c = A - D, B - D, C - D
        X = b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]
        Y = b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]
        Z = b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]
        return (a[..., 0] * X + a[..., 1] * Y) + a[..., 2] * Z


def segment_crosses_triangle(P, Q, A, B, C):
    """Does the segment PQ cross the triangle (A, B, C), arrays [..., 3] -> bool [...]: P and Q strictly on opposite sides of the triangle's plane, and
    orient(P,Q,A,B), orient(P,Q,B,C), orient(P,Q,C,A) all > 0 or all < 0.  A zero or a NaN anywhere: no crossing (touching and coplanar contacts are
    not counted)."""
    sP, sQ = intersect_orient(A, B, C, P), intersect_orient(A, B, C, Q)
    o1, o2, o3 = intersect_orient(P, Q, A, B), intersect_orient(P, Q, B, C), intersect_orient(P, Q, C, A)
    with np.errstate(invalid="ignore"):
        return (((sP > 0.0) & (sQ < 0.0)) | ((sP < 0.0) & (sQ > 0.0))) & (((o1 > 0.0) & (o2 > 0.0) & (o3 > 0.0)) | ((o1 < 0.0) & (o2 < 0.0) & (o3 < 0.0)))


def triangles_intersect(p, ft, fu):
    """The narrow phase on candidates: vertices p [N,3], faces ft and fu int64 [n,3] that share at most one index -> bool [n]: some edge (X[i], X[(i + 1)
    % 3]) of one face, neither end an index of the other face Y, crosses Y with Y's corners in stored order; (X, Y) = (t, u), then (u, t)."""
    hit = np.zeros(ft.shape[0], bool)
    for X, Y in ((ft, fu), (fu, ft)):
        A, B, C = p[Y[:, 0]], p[Y[:, 1]], p[Y[:, 2]]
        for i in range(3):
            a, b = X[:, i], X[:, (i + 1) % 3]
            free = ~((a[:, None] == Y).any(1) | (b[:, None] == Y).any(1))
            hit |= free & segment_crosses_triangle(p[a], p[b], A, B, C)
    return hit


def intersect_report(counts):
    """The eight counts of INTERSECT_COUNTS, in order -> the report both mesh_intersections and ops.mesh_intersections return"""
    return {k: int(x) for k, x in zip(INTERSECT_COUNTS, counts)}


def mesh_intersections(verts, faces, return_pairs=False):
    """The self-intersections of an indexed triangle mesh on the host (the twin of ops.mesh_intersections, and the definition of its result): which
    pairs of triangles cross.  verts [N,3] (float64), faces int32 / int64 [M,3]; an index outside [0, N) and a non-finite coordinate of a referenced
    vertex are errors.  A face TAKES PART iff n . n != 0 for n = (P1 - P0) x (P2 - P0) (_normal2) and its three indices are distinct; the others are
    skipped and counted.  A pair t < u of faces that take part is a CANDIDATE iff their closed bounding boxes overlap on every axis and they share at
    most one vertex index (a fold along a shared edge is the audit's "creased"; coincident vertices with different indices share nothing).  A candidate
    INTERSECTS iff triangles_intersect says so: an edge of one, free of the other's indices, crosses the other strictly (segment_crosses_triangle).
    -> {"bad_index": 0, "nonfinite": 0, "faces", "skipped", "candidates", "pairs", "faces_hit": faces in at least one pair, "max_hits": the most pairs
    one face is in}; ``return_pairs`` adds "pairs_list" int32 [n,2] (t < u, sorted lexicographically) and "face_hits" int32 [M].  Candidates are found by
    brute force over t, vectorised over u.  Nothing depends on face order beyond the numbering of the pairs.  Not counted: coplanar overlap, contacts
    that only touch, a closed component nested inside another; the unfiltered determinant may take the wrong sign next to a degeneracy (the device
    takes the same one)."""
    p, f = _distance_mesh(verts, faces, "mesh_intersections")
    nv, nt = p.shape[0], f.shape[0]
    if nv >= 2 ** 30 or 3 * nt >= 2 ** 31:
        raise ValueError(f"mesh_intersections: bad sizes ({nv} vertices, {nt} faces; the tables are int32)")
    P0, P1, P2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    with np.errstate(all="ignore"):
        part = (_normal2(P0, P1, P2) != 0.0) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    corners = np.stack([P0, P1, P2], 1)                                  # [M,3,3]
    lo, hi = np.ascontiguousarray(corners.min(1).T), np.ascontiguousarray(corners.max(1).T)      # [3,M]: one contiguous row per axis
    cand = []
    for t in np.flatnonzero(part)[:-1] if part.any() else ():
        near = part[t + 1:].copy()
        for d in range(3):
            near &= lo[d, t] <= hi[d, t + 1:]
            near &= lo[d, t + 1:] <= hi[d, t]
        u = t + 1 + np.flatnonzero(near)
        u = u[(f[t][None, :, None] == f[u][:, None, :]).any(2).sum(1) <= 1]
        cand.append(np.stack([np.full(u.size, t, np.int64), u], 1))
    cand = np.concatenate(cand) if cand else np.zeros((0, 2), np.int64)
    candidates = cand.shape[0]
    hit = np.zeros(candidates, bool)
    for k in range(0, candidates, 1 << 16):
        hit[k:k + (1 << 16)] = triangles_intersect(p, f[cand[k:k + (1 << 16), 0]], f[cand[k:k + (1 << 16), 1]])
    pairs = cand[hit].astype(np.int32)                                   # brute force over t, ascending u: sorted as it comes
    face_hits = (np.bincount(pairs[:, 0], minlength=nt) + np.bincount(pairs[:, 1], minlength=nt)).astype(np.int32)
    out = intersect_report((0, 0, np.count_nonzero(part), nt - np.count_nonzero(part), candidates, pairs.shape[0], np.count_nonzero(face_hits),
                            face_hits.max() if nt else 0))
    if return_pairs:
        out.update(pairs_list=pairs, face_hits=face_hits)
    return out


# ------------------------------------------------------------------------------------------------------------------ ray cast and ambient occlusion
# the host twin of csrc/mesh_raycast.hip and the DEFINITION of its results, to the last bit (include/o2345.h has the same text; csrc/mesh_raycast_math.h
# the device form).  All arithmetic is float64, one operation at a time, in the order written; a dot product is (x x + y y) + z z; only comparisons decide.
OCCLUSION_COUNTS = ("bad_points", "bad_frames", "rays", "reserved")          # the counters block of o2345_mesh_occlusion, int64 [4]
OCCLUSION_MAX_SAMPLES = 1024
RAYCAST_EXHAUSTIVE_MAX = 2 ** 16                 # the device's exhaustive path (no grid) takes at most this many triangles
RAYCAST_SLACK = 2.0 ** -30                       # MD_SLACK: what the device's walk, and the twin's optional box filter, widen by
_GOLDEN = 0.6180339887498949


def occlusion_directions(samples):
    """The direction table of the occlusion, float64 [S,3], 1 <= S <= 1024: a cosine-weighted Fibonacci set about +z.  Entry i: r2 = (i + 0.5) / S,
    phi = 2 pi frac(i 0.6180339887498949), (sqrt(r2) cos phi, sqrt(r2) sin phi, sqrt(1 - r2)).  Computed on the host only: the device receives the table
    and never evaluates a sine."""
    if isinstance(samples, (bool, np.bool_)) or not isinstance(samples, (int, np.integer)) or not 1 <= samples <= OCCLUSION_MAX_SAMPLES:
        raise ValueError(f"mesh_occlusion: samples must be an integer in 1 .. {OCCLUSION_MAX_SAMPLES}, got {samples!r}")
    i = np.arange(int(samples), dtype=np.float64)
    r2 = (i + 0.5) / float(samples)
    x = i * _GOLDEN
    phi = (2.0 * np.pi) * (x - np.floor(x))
    r = np.sqrt(r2)
    return np.ascontiguousarray(np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r2)], 1))


def ray_frame(n):
    """rc_frame on directions [..., 3] -> (T, B, N, ok): len = sqrt(n . n); ok iff len is finite and > 0; N = n / len per component; s = copysign(1, N_z);
    a = -1 / (s + N_z); b = (N_x N_y) a; T = (1 + (s N_x)(N_x a), s b, -(s N_x)); B = (b, s + (N_y N_y) a, -N_y) (Duff et al., JCGT 2017).  Rows that are
    not ok hold NaNs or garbage and are not to be used."""
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot3(n, n))
        ok = (length > 0.0) & np.isfinite(length)
        N = n / length[..., None]
        s = np.copysign(1.0, N[..., 2])
        a = -1.0 / (s + N[..., 2])
        b = (N[..., 0] * N[..., 1]) * a
        T = np.stack([1.0 + (s * N[..., 0]) * (N[..., 0] * a), s * b, -(s * N[..., 0])], -1)
        B = np.stack([b, s + (N[..., 1] * N[..., 1]) * a, -N[..., 1]], -1)
    return T, B, N, ok


def _raycast_mesh(verts, faces):
    """-> (vertices float64 [N,3], faces int64 [M,3] with indices out of range replaced by 0, usable bool [M]): a triangle is usable iff its indices lie in
    [0, N), its nine coordinates are finite and n . n != 0 (the grid's rule).  Nothing raises: the device skips the others too."""
    p = np.ascontiguousarray(np.asarray(verts, dtype=np.float64).reshape(-1, 3))
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    inside = ((f >= 0) & (f < p.shape[0])).all(1)
    f = np.where(inside[:, None], f, 0)
    if p.shape[0] == 0:
        return p, f, np.zeros(f.shape[0], bool)
    P0, P1, P2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    with np.errstate(all="ignore"):
        usable = inside & np.isfinite(P0).all(1) & np.isfinite(P1).all(1) & np.isfinite(P2).all(1) & (_normal2(P0, P1, P2) != 0.0)
    return p, f, usable


def segment_hits(P, Q, verts, faces, any_hit=False, prefilter=False, chunk=4096):
    """What the segments P -> Q ([n,3] each) hit on the mesh -> (t float64 [n], tri int32 [n]): the nearest hit, (inf, -1) without one; ``any_hit``: bool
    [n] instead.  A segment hits a usable triangle (A, B, C), corners in stored order, iff segment_crosses_triangle's decisions hold: sP = orient(A,B,C,P)
    and sQ = orient(A,B,C,Q) strictly of opposite sign, orient(P,Q,A,B), orient(P,Q,B,C), orient(P,Q,C,A) all > 0 or all < 0; a zero or a NaN anywhere is
    no hit, so a segment through a shared edge or vertex hits neither neighbour.  A segment with a non-finite coordinate hits nothing.  t = sP / (sP - sQ);
    the nearest hit has the smallest t, among equal t the smallest triangle index; a NaN t never wins.  Exhaustive over the triangles, vectorised over
    chunks of segments.  ``prefilter``: only triangles whose bounding box meets the segment's, widened by 2^-30 of the largest coordinate, are tested --
    the argument of the device's grid walk (a hit point lies in both boxes up to rounding), for inputs too large for the plain form; not the definition."""
    p, f, usable = _raycast_mesh(verts, faces)
    P, Q = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3)) for x in (P, Q))
    n = P.shape[0]
    ids = np.flatnonzero(usable)
    A, B, C = p[f[ids, 0]], p[f[ids, 1]], p[f[ids, 2]]
    best_t, best_tri, flags = np.full(n, np.inf), np.full(n, -1, np.int32), np.zeros(n, bool)
    if prefilter and ids.size:
        lo, hi = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)
        scale = max(float(np.abs(lo).max()), float(np.abs(hi).max()))
    chunk = max(1, min(int(chunk), (1 << (21 if prefilter else 18)) // max(1, ids.size)))          # the pairs of a chunk in flight
    for k in range(0, n if ids.size else 0, chunk):
        Pk, Qk = P[k:k + chunk], Q[k:k + chunk]
        near = (np.isfinite(Pk).all(1) & np.isfinite(Qk).all(1))[:, None] & np.ones(ids.size, bool)[None, :]
        if prefilter:
            with np.errstate(all="ignore"):
                slack = RAYCAST_SLACK * (scale + np.maximum(np.abs(Pk), np.abs(Qk)).max(1))[:, None, None]
                near &= ((np.minimum(Pk, Qk)[:, None, :] - slack <= hi[None]) & (lo[None] <= np.maximum(Pk, Qk)[:, None, :] + slack)).all(2)
        si, ti = np.nonzero(near)
        sP, sQ = intersect_orient(A[ti], B[ti], C[ti], Pk[si]), intersect_orient(A[ti], B[ti], C[ti], Qk[si])
        with np.errstate(all="ignore"):
            sides = ((sP > 0.0) & (sQ < 0.0)) | ((sP < 0.0) & (sQ > 0.0))     # the pairs that fail here are no hits whatever the other three say
            si, ti, sP, sQ = si[sides], ti[sides], sP[sides], sQ[sides]
            Ps, Qs, At, Bt, Ct = Pk[si], Qk[si], A[ti], B[ti], C[ti]
            o1, o2, o3 = intersect_orient(Ps, Qs, At, Bt), intersect_orient(Ps, Qs, Bt, Ct), intersect_orient(Ps, Qs, Ct, At)
            hit = ((o1 > 0.0) & (o2 > 0.0) & (o3 > 0.0)) | ((o1 < 0.0) & (o2 < 0.0) & (o3 < 0.0))
            t = sP / (sP - sQ)
        if any_hit:
            flags[k + si[hit]] = True
            continue
        good = hit & ~np.isnan(t)
        s, tt, tr = si[good], t[good], ids[ti[good]]
        order = np.lexsort((tr, tt, s))                                  # by segment, then t, then triangle index
        s = s[order]
        first = np.ones(s.size, bool)
        first[1:] = s[1:] != s[:-1]
        best_t[k + s[first]] = tt[order][first]
        best_tri[k + s[first]] = tr[order][first]
    return flags if any_hit else (best_t, best_tri)


def _check_ray_length(what, max_distance):
    if isinstance(max_distance, (bool, np.bool_)) or not isinstance(max_distance, (int, float, np.integer, np.floating)) or not (
            np.isfinite(max_distance) and max_distance > 0):
        raise ValueError(f"{what}: max_distance must be a finite float > 0, got {max_distance!r}")
    return float(max_distance)


def ray_cast(origins, directions, verts, faces, max_distance, any_hit=False, prefilter=False):
    """Rays from ``origins`` along ``directions`` ([n,3] each, any length) up to ``max_distance`` direction lengths -> (distance float64 [n] in direction
    lengths = t max_distance, inf without a hit; tri int32 [n], -1 without a hit); ``any_hit``: bool [n].  The segment is P = origin, Q = origin +
    max_distance direction per component (segment_hits has the rules).  The twin of ops.mesh_ray_cast, and its definition."""
    L = _check_ray_length("mesh_ray_cast", max_distance)
    P = np.asarray(origins, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        Q = P + L * np.asarray(directions, np.float64).reshape(-1, 3)
        out = segment_hits(P, Q, verts, faces, any_hit, prefilter)
        return out if any_hit else (out[0] * L, out[1])


def occlusion_defaults(lo, hi, max_distance=None, bias=None):
    """(max_distance, bias) of an occlusion call over a mesh whose vertices span [lo, hi]: None -> the box's diagonal sqrt((dx dx + dy dy) + dz dz) (no ray
    ends inside the mesh's extent) and 1e-6 of it; both checked (max_distance finite and > 0, bias finite and >= 0)."""
    d = [float(b) - float(a) for a, b in zip(lo, hi)]
    diagonal = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    L = _check_ray_length("mesh_occlusion", diagonal if max_distance is None and diagonal > 0 else (1.0 if max_distance is None else max_distance))
    if bias is None:
        bias = 1e-6 * L
    if isinstance(bias, (bool, np.bool_)) or not isinstance(bias, (int, float, np.integer, np.floating)) or not (np.isfinite(bias) and bias >= 0):
        raise ValueError(f"mesh_occlusion: bias must be a finite float >= 0, got {bias!r}")
    return L, float(bias)


def occlusion_rays(points, T, B, N, table, max_distance, bias):
    """rc_occlusion_ray: points and their frames [n,3], the table [S,3] -> (P [n,3], Q [n,S,3]): P = p + bias N, d_i = (x_i T + y_i B) + z_i N,
    Q_i = P + max_distance d_i, per component"""
    with np.errstate(all="ignore"):
        P = points + bias * N
        d = (table[None, :, 0, None] * T[:, None, :] + table[None, :, 1, None] * B[:, None, :]) + table[None, :, 2, None] * N[:, None, :]
        return P, P[:, None, :] + max_distance * d


def occlusion_report(counts):
    """The four counters of OCCLUSION_COUNTS, in order -> the dict both mesh_occlusion and ops.mesh_occlusion return (without the reserved entry)"""
    return {k: int(x) for k, x in zip(OCCLUSION_COUNTS[:3], counts)}


def mesh_occlusion(points, verts, faces, normals=None, owners=None, samples=64, max_distance=None, bias=None, prefilter=False):
    """Ambient occlusion of ``points`` [n,3] against the mesh on the host (the twin of ops.mesh_occlusion, and the definition of its result) -> (hits
    int32 [n], counts dict).  The direction n of a point: ``normals`` [n,3] alone; or with ``owners`` int [n] the face normal (P1 - P0) x (P2 - P0) of
    that triangle in stored order, multiplied by -1 when ``normals`` is given too and its dot product with the given direction is < 0 (a zero or NaN
    direction turns nothing).  An owner outside [0, M) or an unusable owner triangle, or a direction without a frame (ray_frame), casts nothing: hits 0,
    counted as bad_frames; a point with a non-finite coordinate likewise, counted as bad_points.  Otherwise P = p + bias N and Q_i = P + max_distance d_i
    with d_i = (x_i T + y_i B) + z_i N per component over occlusion_directions(samples); hits = the number of i whose segment hits anything
    (segment_hits); counts["rays"] = samples times the points that cast.  The exposure of a point is (S - hits) / S (occlusion_values).  Defaults:
    occlusion_defaults over all vertices.  Binary visibility, no distance falloff; face normals give faceted values on a coarse mesh."""
    if normals is None and owners is None:
        raise ValueError("mesh_occlusion: a point needs a direction (normals) or an owner triangle (owners)")
    table = occlusion_directions(samples)
    p, f, usable = _raycast_mesh(verts, faces)
    pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    n, S = pts.shape[0], table.shape[0]
    finite_v = p[np.isfinite(p).all(1)]
    L, bias = occlusion_defaults(*((finite_v.min(0), finite_v.max(0)) if finite_v.size else ((0, 0, 0), (0, 0, 0))), max_distance, bias)
    bad_point = ~np.isfinite(pts).all(1)
    with np.errstate(all="ignore"):
        if owners is not None:
            o = np.asarray(owners).reshape(-1).astype(np.int64)
            ok = (o >= 0) & (o < f.shape[0])
            o = np.where(ok, o, 0)
            ok &= usable[o] if f.shape[0] else False
            fo = f[o] if f.shape[0] else np.zeros((n, 3), np.int64)
            P0, P1, P2 = (p[fo[:, k]] if p.shape[0] else np.zeros((n, 3)) for k in range(3))
            e1, e2 = P1 - P0, P2 - P0
            nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            if normals is not None:
                nrm = np.where((_dot3(nrm, np.asarray(normals, np.float64).reshape(-1, 3)) < 0.0)[:, None], -nrm, nrm)
        else:
            nrm, ok = np.asarray(normals, np.float64).reshape(-1, 3), np.ones(n, bool)
        T, B, N, framed = ray_frame(nrm)
        cast = ~bad_point & ok & framed
        hits = np.zeros(n, np.int32)
        who = np.flatnonzero(cast)
        step = max(1, 65536 // S)
        for k in range(0, who.size, step):
            w = who[k:k + step]
            P, Q = occlusion_rays(pts[w], T[w], B[w], N[w], table, L, bias)
            flags = segment_hits(np.broadcast_to(P[:, None, :], Q.shape).reshape(-1, 3), Q.reshape(-1, 3), p, np.where(usable[:, None], f, -1), True, prefilter)
            hits[w] = flags.reshape(-1, S).sum(1)
    counts = occlusion_report((np.count_nonzero(bad_point), np.count_nonzero(~bad_point & ~(ok & framed)), S * who.size))
    return hits, counts


def occlusion_values(hits, samples):
    """hits int [n] of ``samples`` rays -> the exposure float32 [n,3]: float32((S - hits) / S) in every channel, what pack_texture turns into the occlusion
    image (1 = open, 0 = closed; glTF reads the red channel)."""
    v = ((float(samples) - np.asarray(hits, np.float64)) / float(samples)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(v.reshape(-1, 1), 3, 1))
