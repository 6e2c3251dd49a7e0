"""Connected components of a mesh on the CPU: the host twin (mesh_io.component_labels / filter_components / convert_mesh's filter), which DEFINES what the
device kernels (csrc/mesh_components.hip, tests/test_gpu_mesh_components.py) must return, plus the C ABI's declarations and the two config knobs.

Component = vertices connected through triangles that share vertex indices; label = the smallest vertex index of the component; size = faces."""
import importlib
import importlib.util
import os

import numpy as np
import pytest

import mesh_components_util as mcu

mio = importlib.import_module("one-2-3-45_amd.mesh_io")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mc_skimage.npz")


def _golden_meshes():
    d = np.load(GOLDEN)
    return {k[:-len(":faces")]: (d[k], int(d[k[:-len(":faces")] + ":verts"].shape[0])) for k in d.files if k.endswith(":faces")}


def _labels_are_minima(lab):
    n = lab.shape[0]
    first = np.full(n, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return bool((first[lab] == lab).all())


def test_labels_match_scipy_on_the_stored_meshes():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    meshes = _golden_meshes()
    assert {"two_spheres", "torus", "noise_cube"} <= set(meshes)
    n_comp = {}
    for name, (f, n) in meshes.items():
        lab = mio.component_labels(f, n)
        assert lab.dtype == np.int32 and lab.shape == (n,)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        g = sparse.coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
        nc, want = csgraph.connected_components(g, directed=False)
        assert mcu.partition_equal(lab, want) and len(np.unique(lab)) == nc, name
        assert _labels_are_minima(lab), name
        n_comp[name] = nc
    assert n_comp["torus"] == 1 and n_comp["noise_cube"] > 2          # not vacuous: a mesh with several components is among them


@pytest.mark.parametrize("permuted", [True, False])
def test_strip_is_one_component_whatever_its_diameter(permuted):
    """200,000 triangles in a row: label propagation needs one sweep per step of the diameter (35,606 sweeps, minutes); hook + pointer jumping does not."""
    f, n = mcu.strip(100_000, permuted)
    assert f.shape == (200_000, 3) and n == 200_002
    lab = mio.component_labels(f, n)
    assert lab.shape == (n,) and not lab.any()


def _two_blobs():
    """vertices 0..11: [0] unreferenced, A = {1, 2, 3, 4} (2 faces), [5] unreferenced, B = {6..10} (3 faces), [11] unreferenced"""
    f = np.array([[2, 1, 3], [6, 7, 8], [3, 2, 4], [8, 7, 9], [10, 9, 8]], np.int64)
    v = np.random.default_rng(0).normal(size=(12, 3))
    v[3, 0] = -0.0
    v[7, 1] = np.nan                       # bit-for-bit copies: a NaN payload and a negative zero survive
    return v, f


def test_filter_keeps_order_renumbers_and_copies_bitwise():
    v, f = _two_blobs()
    c = np.arange(36, dtype=np.uint8).reshape(12, 3)
    nr = np.arange(36, dtype=np.float32).reshape(12, 3)
    assert mio.component_labels(f, 12).tolist() == [0, 1, 1, 1, 1, 5, 6, 6, 6, 6, 6, 11]
    # nothing selected: the inputs themselves, unreferenced vertices included
    v0, f0, c0, n0, kept0, info0 = mio.filter_components(v, f, c, nr)
    assert v0 is v and f0 is f and c0 is c and n0 is nr and kept0.tolist() == list(range(12)) and info0 == {"components": 5, "components_kept": 5}
    # min_faces = 1: every referenced vertex, unreferenced ones dropped
    v1, f1, c1, n1, kept1, info1 = mio.filter_components(v, f, c, nr, min_faces=1)
    assert kept1.tolist() == [1, 2, 3, 4, 6, 7, 8, 9, 10] and kept1.dtype == np.int32 and (np.diff(kept1) > 0).all()
    assert v1.tobytes() == v[kept1].tobytes() and (c1 == c[kept1]).all() and (n1 == nr[kept1]).all()
    assert f1.tolist() == [[1, 0, 2], [4, 5, 6], [2, 1, 3], [6, 5, 7], [8, 7, 6]] and f1.dtype == f.dtype
    assert info1 == {"components": 5, "components_kept": 2}
    # min_faces = 3: B only, in its original face order
    v3, f3, _, _, kept3, info3 = mio.filter_components(v, f, min_faces=3)
    assert kept3.tolist() == [6, 7, 8, 9, 10] and f3.tolist() == [[0, 1, 2], [2, 1, 3], [4, 3, 2]] and info3["components_kept"] == 1
    assert v3.tobytes() == v[kept3].tobytes()
    # keep_largest alone = B; with a threshold that B misses: nothing
    assert mio.filter_components(v, f, keep_largest=True)[4].tolist() == [6, 7, 8, 9, 10]
    ve, fe, ce, _, kepte, infoe = mio.filter_components(v, f, c, min_faces=4, keep_largest=True)
    assert ve.shape == (0, 3) and fe.shape == (0, 3) and ce.shape == (0, 3) and kepte.shape == (0,) and infoe == {"components": 5, "components_kept": 0}
    # a threshold above everything: empty
    assert mio.filter_components(v, f, min_faces=10 ** 9)[1].shape == (0, 3)


def test_tie_for_largest_goes_to_the_smaller_label():
    v, f = _two_blobs()
    a = f[[0, 2]]                                           # component A (label 1, 2 faces)
    f2 = np.concatenate([a + 20, f[:1] * 0 + [[40, 41, 42]], a])          # a copy of A at label 21 FIRST in face order, a 1-face component, then A itself
    v2 = np.random.default_rng(1).normal(size=(43, 3))
    _, fo, _, _, kept, info = mio.filter_components(v2, f2, keep_largest=True)
    assert kept.tolist() == [1, 2, 3, 4] and fo.tolist() == [[1, 0, 2], [2, 1, 3]] and info["components_kept"] == 1
    # both controls: the tie is among what the threshold left
    assert mio.filter_components(v2, f2, min_faces=2, keep_largest=True)[4].tolist() == [1, 2, 3, 4]
    assert mio.filter_components(v2, f2, min_faces=2)[4].tolist() == [1, 2, 3, 4, 21, 22, 23, 24]
    assert mio.filter_components(v2, f2, min_faces=3, keep_largest=True)[4].size == 0


def test_filter_of_an_empty_mesh_and_idempotence():
    e = mio.filter_components(np.zeros((0, 3)), np.zeros((0, 3), np.int64), keep_largest=True)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[4].shape == (0,) and e[5] == {"components": 0, "components_kept": 0}
    assert mio.component_labels(np.zeros((0, 3), np.int64), 0).shape == (0,)
    assert mio.component_labels(np.zeros((0, 3), np.int64), 4).tolist() == [0, 1, 2, 3]
    only_verts = mio.filter_components(np.ones((4, 3)), np.zeros((0, 3), np.int64), min_faces=1)
    assert only_verts[0].shape == (0, 3) and only_verts[5] == {"components": 4, "components_kept": 0}
    with pytest.raises(ValueError):
        mio.component_labels(np.array([[0, 1, 4]]), 4)
    d = np.load(GOLDEN)
    v, f = d["noise_cube:verts"], d["noise_cube:faces"]
    for kw in (dict(min_faces=20), dict(keep_largest=True), dict(min_faces=20, keep_largest=True)):
        v1, f1, _, _, k1, i1 = mio.filter_components(v, f, **kw)
        v2, f2, _, _, k2, i2 = mio.filter_components(v1, f1, **kw)
        assert 0 < f1.shape[0] < f.shape[0]
        assert v2.tobytes() == v1.tobytes() and f2.tobytes() == f1.tobytes() and k2.tolist() == list(range(len(k1)))
        assert i2["components"] == i2["components_kept"] == i1["components_kept"]


@pytest.mark.parametrize("ext", [".glb", ".obj"])
def test_convert_mesh_with_the_filter_is_filter_then_writer(tmp_path, ext):
    d = np.load(GOLDEN)
    v, f = d["noise_cube:verts"].astype(np.float32), d["noise_cube:faces"]
    c = np.random.default_rng(2).integers(0, 256, (v.shape[0], 4)).astype(np.uint8)
    c[:, 3] = 255
    ply = str(tmp_path / "m.ply")
    mio.write_ply(ply, v, f, c)
    out = mio.convert_mesh(ply, str(tmp_path / ("m" + ext)), keep_largest=True)
    rv, rf, rc = mio.read_ply(ply)
    fv, ff, fc, _, kept, info = mio.filter_components(rv, rf, rc, keep_largest=True)
    assert info["components"] > 2 and info["components_kept"] == 1 and 0 < len(kept) < len(rv) and (fc == c[kept]).all()
    av, af = mio.to_asset_frame(fv, ff)
    want = str(tmp_path / ("want" + ext))
    (mio.write_glb if ext == ".glb" else mio.write_obj)(want, av, af, fc)
    assert open(out, "rb").read() == open(want, "rb").read()
    # the colours follow their vertices through the file
    back = (mio.read_glb if ext == ".glb" else mio.read_obj)(out)
    assert (back[2][:, :3] == c[kept][:, :3]).all()
    # filter off: the file convert_mesh always wrote
    plain, off = str(tmp_path / ("p" + ext)), str(tmp_path / ("o" + ext))
    mio.convert_mesh(ply, plain)
    mio.convert_mesh(ply, off, min_component_faces=0, keep_largest=False)
    assert open(plain, "rb").read() == open(off, "rb").read() != open(out, "rb").read()


def test_cabi_declares_and_exports_the_component_entries():
    L = importlib.import_module("one-2-3-45_amd._lib")
    protos = L.parse_header()
    names = ("o2345_mesh_components_workspace_bytes", "o2345_mesh_components_count", "o2345_mesh_components_emit")
    assert all(n in protos for n in names)
    lib = L.lib()
    assert all(hasattr(lib, n) for n in names) and lib.o2345_version() == 231
    small, big = lib.o2345_mesh_components_workspace_bytes(0, 0), lib.o2345_mesh_components_workspace_bytes(1000, 2000)
    assert 0 < small < big and big >= 4 * (3 * 1000 + 2000)
    # argument checks come before any device work
    import ctypes
    out = [ctypes.c_longlong() for _ in range(4)]
    rc = lib.o2345_mesh_components_count(None, 2, 3, 1, 0, 0, None, 0, None, *[ctypes.byref(o) for o in out], None)
    assert rc != 0 and b"index_bytes" in lib.o2345_last_error()
    rc = lib.o2345_mesh_components_count(None, 4, 3, 1, 0, 0, None, 0, None, *[ctypes.byref(o) for o in out], None)
    assert rc != 0 and b"null pointer" in lib.o2345_last_error()
    rc = lib.o2345_mesh_components_count(None, 4, 2 ** 30, 1, 0, 0, None, 0, None, *[ctypes.byref(o) for o in out], None)
    assert rc != 0 and b"bad sizes" in lib.o2345_last_error()


def _fresh_config(monkeypatch, **env):
    for k in ("O2345_MESH_MIN_COMPONENT_FACES", "O2345_MESH_KEEP_LARGEST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = importlib.import_module("one-2-3-45_amd.config").__file__
    spec = importlib.util.spec_from_file_location("o2345_config_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                      # a private copy: the package's own config module is not touched
    return mod


def test_config_knobs(monkeypatch):
    c = _fresh_config(monkeypatch)
    assert c.MESH_MIN_COMPONENT_FACES == 0 and c.MESH_KEEP_LARGEST is False
    assert c.mesh_min_component_faces() == 0 and c.mesh_keep_largest() is False and c.mesh_min_component_faces(7) == 7 and c.mesh_keep_largest(1) is True
    c = _fresh_config(monkeypatch, O2345_MESH_MIN_COMPONENT_FACES="", O2345_MESH_KEEP_LARGEST="0")
    assert c.MESH_MIN_COMPONENT_FACES == 0 and c.MESH_KEEP_LARGEST is False
    c = _fresh_config(monkeypatch, O2345_MESH_MIN_COMPONENT_FACES=" 250 ", O2345_MESH_KEEP_LARGEST="1")
    assert c.MESH_MIN_COMPONENT_FACES == 250 and c.MESH_KEEP_LARGEST is True and c.mesh_min_component_faces() == 250 and c.mesh_keep_largest() is True
    assert c.mesh_min_component_faces(0) == 0 and c.mesh_keep_largest(False) is False          # an explicit argument wins over the environment
    for bad in ("-1", "many", "2.5"):
        with pytest.raises(ValueError):
            _fresh_config(monkeypatch, O2345_MESH_MIN_COMPONENT_FACES=bad)
        with pytest.raises(ValueError):
            _fresh_config(monkeypatch, O2345_MESH_KEEP_LARGEST=bad)
    with pytest.raises(ValueError):
        c.mesh_min_component_faces(-3)
