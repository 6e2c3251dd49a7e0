"""Asset formats on the CPU: the host layer of mesh_io (write_glb / write_obj / read_glb / read_obj / convert_mesh), which is the definition the device
path (tests/test_gpu_mesh_formats.py) is compared against.

Orientation rule, restated: the asset frame is the PLY frame with y and z exchanged, (x, y, z) -> (x, z, y) -- a reflection, z-up -> glTF's y-up -- and
every face reversed, (a, b, c) -> (c, b, a); the reflection and the reversal cancel, so a closed mesh keeps the sign of its volume."""
import importlib
import json
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

mio = importlib.import_module("one-2-3-45_amd.mesh_io")


def _mesh(seed, n=300, m=411, scale=1.0):
    rng = np.random.default_rng(seed)
    v = (rng.normal(0, 1, (n, 3)) * scale).astype(np.float32)
    f = rng.integers(0, n, (m, 3))
    c = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    g = rng.normal(0, 1, (n, 3))
    nr = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    return v, f, c, nr


def _lib_or_none():
    try:
        return importlib.import_module("one-2-3-45_amd._lib").lib()
    except (RuntimeError, OSError, AttributeError):
        return None


def _parse_glb(raw):
    """Independent GLB parser (struct + json): -> (doc, bin chunk bytes), asserting the container rules on the way."""
    magic, version, total = struct.unpack_from("<III", raw, 0)
    assert magic == 0x46546C67 and raw[:4] == b"glTF" and version == 2 and total == len(raw)
    jlen, jtype = struct.unpack_from("<II", raw, 12)
    assert jtype == 0x4E4F534A and jlen % 4 == 0
    doc = json.loads(raw[20:20 + jlen])
    blen, btype = struct.unpack_from("<II", raw, 20 + jlen)
    assert btype == 0x004E4942 and blen % 4 == 0 and 20 + jlen + 8 + blen == len(raw)
    return doc, raw[28 + jlen:]


@pytest.mark.parametrize("colors,normals", [(False, False), (True, False), (True, True), (False, True)])
def test_glb_roundtrip_and_structure(tmp_path, colors, normals):
    v, f, c, nr = _mesh(0)
    p = str(tmp_path / "a.glb")
    mio.write_glb(p, v, f, c if colors else None, nr if normals else None)
    v2, f2, c2, n2 = mio.read_glb(p)
    assert v2.dtype == np.float32 and np.array_equal(v2.view(np.uint32), v.view(np.uint32))                # bit-exact
    assert np.array_equal(f2, f)
    assert (c2 is None) == (not colors) and (n2 is None) == (not normals)
    if colors:
        assert c2.dtype == np.uint8 and np.array_equal(c2[:, :3], c) and (c2[:, 3] == 255).all()
    if normals:
        assert np.array_equal(n2.view(np.uint32), nr.view(np.uint32))
    # structure, with a parser of the test's own
    raw = open(p, "rb").read()
    doc, bin_ = _parse_glb(raw)
    assert doc["asset"] == {"version": "2.0", "generator": "o2345-hip"}
    assert len(doc["buffers"]) == 1 and doc["buffers"][0]["byteLength"] <= len(bin_) and len(doc["meshes"]) == 1 and len(doc["nodes"]) == 1
    assert doc["scenes"] == [{"nodes": [0]}] and doc["scene"] == 0 and doc["nodes"][0] == {"mesh": 0}
    prim, = doc["meshes"][0]["primitives"]
    assert prim["mode"] == 4
    size = {5121: 1, 5125: 4, 5126: 4}
    width = {"SCALAR": 1, "VEC3": 3, "VEC4": 4}
    for a in doc["accessors"]:
        view = doc["bufferViews"][a["bufferView"]]
        assert a["byteOffset"] + a["count"] * size[a["componentType"]] * width[a["type"]] <= view["byteLength"]
        assert view["byteOffset"] % 4 == 0 and view["byteOffset"] + view["byteLength"] <= doc["buffers"][0]["byteLength"]
    order = [prim["indices"], prim["attributes"]["POSITION"]] + [prim["attributes"][k] for k in ("COLOR_0", "NORMAL") if k in prim["attributes"]]
    views = [doc["accessors"][i]["bufferView"] for i in order]
    assert views == list(range(len(views)))                                       # indices / POSITION / COLOR_0 / NORMAL
    offs = [doc["bufferViews"][i]["byteOffset"] for i in views]
    assert offs == sorted(offs) and offs[0] == 0
    assert [doc["bufferViews"][i]["target"] for i in views] == [34963] + [34962] * (len(views) - 1)
    ia, pa = doc["accessors"][prim["indices"]], doc["accessors"][prim["attributes"]["POSITION"]]
    assert (ia["componentType"], ia["type"], ia["count"]) == (5125, "SCALAR", 3 * len(f))
    assert (pa["componentType"], pa["type"], pa["count"]) == (5126, "VEC3", len(v))
    assert np.array_equal(np.asarray(pa["min"], np.float64), v.min(0).astype(np.float64)) and np.array_equal(np.asarray(pa["max"], np.float64), v.max(0).astype(np.float64))
    idx = np.frombuffer(bin_, "<u4", ia["count"], doc["bufferViews"][ia["bufferView"]]["byteOffset"])
    assert idx.max() < pa["count"]
    if colors:
        ca = doc["accessors"][prim["attributes"]["COLOR_0"]]
        assert (ca["componentType"], ca["type"], ca["normalized"], ca["count"]) == (5121, "VEC4", True, len(v))
    if normals:
        na = doc["accessors"][prim["attributes"]["NORMAL"]]
        assert (na["componentType"], na["type"], na["count"]) == (5126, "VEC3", len(v))
    # reproducible bytes
    mio.write_glb(str(tmp_path / "b.glb"), v, f, c if colors else None, nr if normals else None)
    assert open(str(tmp_path / "b.glb"), "rb").read() == raw


def test_empty_mesh(tmp_path):
    with pytest.raises(ValueError):
        mio.write_glb(str(tmp_path / "e.glb"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    p = str(tmp_path / "e.obj")
    mio.write_obj(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    assert os.path.getsize(p) == 0
    v, f, c, n = mio.read_obj(p)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c is None and n is None


def _obj_size(n, m, K, colors, normals):
    """Closed form, restated: coordinate field = space + sign + K digits + '.' + 8 digits; colour field = space + 10; 'vn' fields = space + 11."""
    dn = len(str(n))
    v_len = 1 + 3 * (1 + 1 + K + 1 + 8) + (3 * 11 if colors else 0) + 1
    vn_len = 2 + 3 * 12 + 1
    f_len = 1 + 3 * (1 + (2 * dn + 2 if normals else dn)) + 1
    return n * v_len + (n * vn_len if normals else 0) + m * f_len


@pytest.mark.parametrize("writer", ["write_obj", "write_obj_numpy"])
@pytest.mark.parametrize("maxabs,K", [(0.5, 1), (9.999999, 1), (10.0, 2), (12345.678, 5)])
@pytest.mark.parametrize("colors,normals", [(False, False), (True, False), (True, True)])
def test_obj_roundtrip_size_and_alignment(tmp_path, writer, maxabs, K, colors, normals):
    v, f, c, nr = _mesh(1, n=1203, m=2000)
    v = (v / np.abs(v).max() * np.float32(maxabs) * np.float32(0.999)).astype(np.float32)
    v[7, 1] = np.float32(maxabs) * (-1 if K == 2 else 1)                  # the widest value, once negative
    v[8] = [-1e-12, 1e-12, -0.0]                                          # "-0.00000000", " 0.00000000", "-0.00000000"
    v[9] = [0.000000005, -0.000000015, 0.123456785]                       # next to ties of the 8th decimal
    assert np.abs(v).max() == np.float32(maxabs)
    p = str(tmp_path / "a.obj")
    getattr(mio, writer)(p, v, f, c if colors else None, nr if normals else None)
    raw = open(p, "rb").read()
    n, m = len(v), len(f)
    assert mio.obj_coordinate_digits(v) == K
    assert len(raw) == _obj_size(n, m, K, colors, normals) == mio.obj_text_bytes(n, m, K, colors, normals)
    L = _lib_or_none()
    if L is not None:
        assert L.o2345_obj_text_bytes(n, m, K, int(colors), int(normals)) == len(raw)
    lines = raw.decode("ascii").split("\n")
    assert lines[-1] == ""
    kinds = {}
    for l in lines[:-1]:
        kinds.setdefault(l.split(" ")[0], set()).add(len(l))
    assert set(kinds) == ({"v", "f", "vn"} if normals else {"v", "f"}) and all(len(s) == 1 for s in kinds.values()), kinds
    assert [l[:2] for l in lines[:n]] == ["v "] * n and [l[:2] for l in lines[-1 - m:-1]] == ["f "] * m      # v records, [vn records,] f records
    # the three special rows, as printf writes them
    w = K + 10
    assert lines[8][:1 + 3 * (w + 1)] == "v" + " %*s" % (w, "-0.00000000") + " %*s" % (w, "0.00000000") + " %*s" % (w, "-0.00000000")
    assert lines[7].split()[2] == "%.8f" % float(v[7, 1])
    # round trip
    v2, f2, c2, n2 = mio.read_obj(p)
    assert np.array_equal(f2, f) and v2.shape == (n, 3)
    # correct rounding at 8 decimals, in exact arithmetic on the text: |decimal - float32| <= 0.5e-8
    half = Fraction(5, 10 ** 9)
    for i in range(n):
        toks = lines[i].split()[1:4]
        for d in range(3):
            assert abs(Fraction(toks[d]) - Fraction(float(v[i, d]))) <= half, (i, d, toks[d], float(v[i, d]))
    assert np.array_equal(v2, np.array([[float(t) for t in l.split()[1:4]] for l in lines[:n]]))
    if colors:
        assert c2.dtype == np.uint8 and np.array_equal(c2, c)
    else:
        assert c2 is None
    if normals:
        for i in range(n):
            for d, t in enumerate(lines[n + i].split()[1:4]):
                assert abs(Fraction(t) - Fraction(float(nr[i, d]))) <= half, (i, d, t)
        assert n2.shape == (n, 3)
        assert all(t.split("//")[0] == t.split("//")[1] for l in lines[-1 - m:-1] for t in l.split()[1:])
    else:
        assert n2 is None and "/" not in lines[-2]


def test_obj_refuses_more_than_nine_integer_digits(tmp_path):
    v, f, _, _ = _mesh(2)
    v[0, 0] = 1e9
    with pytest.raises(ValueError):
        mio.write_obj(str(tmp_path / "a.obj"), v, f)
    v[0, 0] = np.inf
    with pytest.raises(ValueError):
        mio.write_obj(str(tmp_path / "a.obj"), v, f)
    v[0, 0] = 999999999.0 - 64                                          # nine digits are fine
    mio.write_obj(str(tmp_path / "a.obj"), v, f)
    assert mio.obj_coordinate_digits(v) == 9


def _signed_volume(v, f):
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


@pytest.mark.parametrize("ext", [".glb", ".obj"])
def test_convert_mesh(tmp_path, ext):
    # an octahedron with outward faces, off-centre and anisotropic so that no symmetry hides a wrong permutation
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 3], [0, 0, -3]], np.float64) + [0.25, -0.5, 0.125]
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    c = np.arange(18, dtype=np.uint8).reshape(6, 3) * 13
    assert _signed_volume(v, f) > 0
    ply = str(tmp_path / "mesh.ply")
    mio.write_ply(ply, v, f, c)
    pv, pf, pc = mio.read_ply(ply)
    out = mio.convert_mesh(ply, str(tmp_path / ("mesh" + ext)))
    assert out == str(tmp_path / ("mesh" + ext)) and os.path.exists(out)
    v2, f2, c2, n2 = (mio.read_glb if ext == ".glb" else mio.read_obj)(out)
    if ext == ".glb":
        assert np.array_equal(v2.view(np.uint32), np.ascontiguousarray(pv[:, [0, 2, 1]]).view(np.uint32))
    else:
        assert np.abs(v2 - pv[:, [0, 2, 1]].astype(np.float64)).max() <= 0.5e-8
    assert np.array_equal(f2, pf[:, ::-1]) and np.array_equal(c2[:, :3], pc[:, :3]) and n2 is None
    vol0, vol1 = _signed_volume(pv, pf), _signed_volume(v2, f2)
    assert vol0 > 0 and vol1 > 0 and abs(vol1 - vol0) <= 1e-6 * vol0          # reflection x reversal = orientation kept
    assert _signed_volume(pv[:, [0, 2, 1]], pf) < 0                           # the reflection alone would turn the mesh inside out
    with pytest.raises(ValueError):
        mio.convert_mesh(ply, str(tmp_path / "mesh.stl"))


def test_host_packer_equals_numpy_writer(tmp_path):
    """o2345_obj_text_host (threaded above 65,536 records) == the printf-style host formatter, byte for byte."""
    if _lib_or_none() is None:
        pytest.skip("libo2345_hip.so is not built: write_obj already IS the numpy writer")
    rng = np.random.default_rng(3)
    n, m = 70001, 90003
    v = (rng.normal(0, 30, (n, 3))).astype(np.float32)
    v[:4] = [[-1e-12, 0.0, -0.0], [123.456789, -99.99999999, 0.000000005], [1e-8, -1e-8, 1.5e-8], [2.5e-8, -0.5, 100.0]]
    f = rng.integers(0, n, (m, 3))
    g = rng.normal(0, 1, (n, 3)).astype(np.float32)
    nr = g / np.linalg.norm(g, axis=1, keepdims=True)
    nr[:3] = [[1, 0, 0], [0, -1, 0], [0, 0, 1]]
    for cols, nrm in ((None, None), (rng.integers(0, 256, (n, 3)).astype(np.uint8), None), (rng.integers(0, 256, (n, 4)).astype(np.uint8), nr)):
        a, b = str(tmp_path / "a.obj"), str(tmp_path / "ref.obj")
        mio.write_obj(a, v, f, cols, nrm)
        mio.write_obj_numpy(b, v, f, cols, nrm)
        assert open(a, "rb").read() == open(b, "rb").read()
