"""CPU: the binding's table of the C ABI (one-2-3-45_amd/_lib.py) -- element types and host / device pointers as include/o2345.h declares them -- and
the one converter and call path built on it.  No device is touched: every refused call fails on the host, and the calls made are host functions or
fail in the library's own argument checks."""
import ctypes
import importlib
import re

import numpy as np
import pytest
import torch

L = importlib.import_module("one-2-3-45_amd._lib")

ELEMENTS = {"float32", "float64", "int32", "uint8", "int64", "size_t", "void"}
RENAMED = {"bound_min", "bound_max", "scale_mat", "trans_mat", "thresholds"}


PROTOTYPES = L.prototypes()


def pointers():
    return [(fn, p) for fn, (_, params) in PROTOTYPES.items() for p in params if p.ctype is ctypes.c_void_p]


def test_every_pointer_has_an_element_type_and_the_host_rule_holds():
    ptrs = pointers()
    assert len(ptrs) > 300
    for fn, p in ptrs:
        struct = p.elem.startswith("struct ")
        assert struct or p.elem in ELEMENTS, (fn, p)
        assert p.host == (p.name.endswith("_host") or fn.endswith("_host")), (fn, p)
        assert p.elem != "size_t" or p.host, (fn, p)
    host = {(fn, p.name) for fn, p in ptrs if p.host}
    assert len(host) == 65                                # 59 + the camera of the three raster entries, passed as o2345_camera_rays takes it
    for fn in ("o2345_mesh_raster_count", "o2345_mesh_raster_emit", "o2345_mesh_raster_shade_textured", "o2345_camera_rays"):
        cam = {p.name: p for f, p in ptrs if f == fn and p.name in ("K_host", "c2w_host")}
        assert set(cam) == {"K_host", "c2w_host"} and all(p.host and p.elem == "float32" for p in cam.values()), fn
        assert not [p for p in PROTOTYPES[fn][1] if p.ctype is ctypes.c_float and p.name != "ambient"], fn          # no camera scalar is left
    assert {("o2345_surface_trace", "bound_min_host"), ("o2345_mesh_distance_reduce", "thresholds_host"), ("o2345_render_rays", "io_host"),
            ("o2345_ply_records_host", "faces"), ("o2345_struct_layout", "offsets_host")} <= host
    assert not {("o2345_sdf_grid_sparse_x3", "background"), ("o2345_mesh_decimate_count", "tris"), ("o2345_costvol_index", "n_rows_dev")} & host
    table = {(fn, p.name): p.elem for fn, p in ptrs}
    structs = {(fn, p.name): p.elem[7:] for fn, p in ptrs if p.elem.startswith("struct ")}
    assert structs == {("o2345_render_rays", "io_host"): "O2345RenderIO", ("o2345_mesh_project", "stats"): "O2345ProjectStats",
                       ("o2345_mesh_texture_points", "stats"): "O2345TextureStats", ("o2345_surface_trace", "stats"): "O2345SurfaceStats",
                       ("o2345_mesh_distance_reduce", "stats"): "O2345DistanceStats", ("o2345_mesh_simplify_count", "stats"): "O2345SimplifyStats",
                       ("o2345_mesh_audit", "stats"): "O2345AuditStats"}
    assert not [k for k in structs if k[1] == "stats" and k in host] and "void* stats" not in open(L.HEADER).read()
    assert table["o2345_costvol_index", "origin_host"] == "float32" and table["o2345_mesh_smooth", "boundary_or_null"] == "uint8"
    assert table["o2345_list_sort_by_visibility", "keys_out"] == "int32" and table["o2345_color_points_x3", "stats_dev"] == "int64"
    assert table["o2345_mesh_decimate_count", "tris"] == "void" and table["o2345_mc_verts_to_world", "extent_host"] == "float64"
    assert not [(fn, p.name) for fn, (_, params) in PROTOTYPES.items() for p in params if p.name in RENAMED]
    fields = {p.name: p for p in L.struct_fields("O2345RenderIO")}
    assert fields["nviews"].elem == "uint8" and fields["color_stats"].elem == "int64" and fields["rays_o"].elem == "float32" and fields["R"].elem is None
    assert not any(p.host for p in fields.values())


def test_an_unknown_pointee_type_is_an_error_at_parse_time(tmp_path):
    for decl in ("int o2345_x(const short* a, void* stream);", "int o2345_x(size_t* sizes, void* stream);", "int o2345_x(short n);"):
        path = tmp_path / "h.h"
        path.write_text(decl)
        with pytest.raises(ValueError, match="o2345_x"):
            L.prototypes(str(path))
    path.write_text("int o2345_x(size_t* sizes_host);")
    assert L.prototypes(str(path))["o2345_x"][1][0] == L.Param("sizes_host", ctypes.c_void_p, "size_t", True)


_CT = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "void": None, "double": ctypes.c_double}


def parse_header_before(path):
    """_lib.parse_header as it was before the table kept element types: every `*` a c_void_p."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"typedef struct.*?\}\s*\w+;", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(o2345_\w+)\s*\(([^;{]*?)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        def ctype(decl):
            decl = decl.strip()
            if "*" in decl:
                return ctypes.c_char_p if decl.startswith("const char") else ctypes.c_void_p
            base = re.sub(r"\b(const|unsigned)\b", "", decl).strip()
            base = " ".join(base.split()[:-1]) if len(base.split()) > 1 and base.split()[-1] not in ("long", "int") else base
            for k in ("long long", "size_t", "float", "double", "int"):
                if base.startswith(k):
                    return _CT[k]
            raise ValueError(f"cannot map C type {decl!r} in {name}")
        argt = [] if args in ("", "void") else [ctype(a) for a in args.split(",")]
        rest = ctypes.c_char_p if (ret.startswith("const char") or name in ("o2345_last_error", "o2345_knobs")) else (_CT["size_t"] if ret == "size_t" else ctypes.c_int)
        protos[name] = (rest, argt)
    return protos


def test_parse_header_and_parse_struct_return_what_they_returned():
    assert L.parse_header() == parse_header_before(L.HEADER) and len(L.parse_header()) >= 110
    lib = L.lib()
    for name, (rest, argt) in L.parse_header().items():
        assert getattr(lib, name).argtypes == argt and getattr(lib, name).restype is rest
        assert all(t in (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_size_t) for t in argt), name
    fields = L.parse_struct("O2345RenderIO")
    assert fields[0] == ("sdf_blob", ctypes.c_void_p) and ("R", ctypes.c_int) in fields and ("weight_cull", ctypes.c_float) in fields
    assert fields == L.RenderIO._fields_


def args_of(name, **given):
    """Arguments that bind accepts for every parameter of ``name`` (null pointers, zeros), with ``given`` put in by parameter name."""
    params = PROTOTYPES[name][1]
    assert set(given) <= {p.name for p in params}
    return tuple(given.get(p.name, None if p.elem else 0) for p in params)


@pytest.mark.parametrize("name, param, value, got", [
    ("o2345_costvol_index", "proj", torch.zeros(4, 4, 4), "cpu"),                                       # a CPU tensor for a device pointer
    ("o2345_costvol_index", "proj", np.zeros((4, 4, 4), np.float32), "numpy"),                          # a numpy array for a device pointer
    ("o2345_costvol_index", "origin_host", torch.zeros(3), "tensor"),                                   # a tensor for a host pointer
    ("o2345_costvol_index", "origin_host", np.zeros(3, np.float64), "float64"),                         # float64 for const float*
    ("o2345_costvol_index", "origin_host", np.zeros((3, 2), np.float32)[:, 0], "C-contiguous=False"),   # a non-contiguous numpy array
    ("o2345_marching_cubes_count", "nv_host", ctypes.c_int(), "c_int"),                                 # c_int where long long* is declared
    ("o2345_mesh_distance_grid_count", "dims_host", (ctypes.c_longlong * 3)(), "_Array_3"),                # 8-byte integers where int* is declared
    ("o2345_mesh_distance_grid_count", "cell_host", ctypes.c_longlong(), "c_long"),                     # an integer where double* is declared
    ("o2345_render_rays", "io_host", ctypes.c_int(), "c_int"),
    ("o2345_costvol_index", "V", 2 ** 31, "2147483648"),                                                # does not fit int
    ("o2345_costvol_index", "V", -2 ** 31 - 1, "-2147483649"),
    ("o2345_costvol_index", "V", 1.0, "float"),
    ("o2345_costvol_index", "workspace_bytes", -1, "-1"),                                               # does not fit size_t
    ("o2345_scatter_dense", "nvox", 2 ** 63, str(2 ** 63)),                                             # does not fit long long
])
def test_bind_refuses(name, param, value, got):
    with pytest.raises(ValueError) as e:
        L.bind(name, args_of(name, **{param: value}))
    msg = str(e.value)
    assert msg.startswith(f"{name}: {param}: expected ") and ", got " in msg and got in msg.split(", got ")[1], msg


def test_bind_accepts():
    for name, (_, params) in PROTOTYPES.items():
        bound = L.bind(name, args_of(name))                                        # None for every pointer of every entry
        assert all(b is None for b, p in zip(bound, params) if p.elem)
    name = "o2345_mesh_distance_grid_count"
    dims, edge, ne = (ctypes.c_int * 3)(), ctypes.c_double(), ctypes.c_longlong()
    bound = dict(zip((p.name for p in PROTOTYPES[name][1]), L.bind(name, args_of(name, dims_host=dims, cell_host=edge, n_entries_host=ne, nv=2 ** 40))))
    assert bound["dims_host"] == ctypes.addressof(dims) and bound["cell_host"] == ctypes.addressof(edge) and bound["n_entries_host"] == ctypes.addressof(ne)
    assert bound["nv"] == 2 ** 40 and bound["stream"] is None
    idx = np.arange(6, dtype=np.uint32)                                            # uint32_t is int32 storage: signedness is not told apart
    assert L.bind("o2345_obj_text_host", args_of("o2345_obj_text_host", indices=idx))[4] == idx.ctypes.data
    assert L.bind("o2345_costvol_index", args_of("o2345_costvol_index", V=np.int64(7), H=True))[1:3] == [7, 1]
    with pytest.raises(ValueError, match="o2345_version: expected 0 arguments"):
        L.bind("o2345_version", (1,))


def test_call_returns_values_and_raises_on_a_failing_status():
    w, h = ctypes.c_int(), ctypes.c_int()
    assert L.call("o2345_mesh_texture_texels", 33, 8, w, h) == 17 * 64 and (w.value, h.value) == (5 * 8, 4 * 8)       # 17 cells, G = 5: 5 x 4 cells
    assert L.call("o2345_version") == L.ABI_VERSION == 231
    assert L.call("o2345_obj_text_bytes", 0, 0, 12, 0, 0) == 0 and b"=" in L.call("o2345_knobs")
    with pytest.raises(RuntimeError, match=r"o2345 sdf_mlp failed \(-?\d+\): .*null pointer") as e:
        L.call("o2345_sdf_mlp", 0, None, None, 8, None, None, None, 10, 0, 1.0, None, None, None, None, None)
    assert L.lib().o2345_last_error().decode() in str(e.value)
    with pytest.raises(ValueError, match="o2345_sdf_mlp: expected 15 arguments"):
        L.call("o2345_sdf_mlp", 0, None)


def test_render_io_fields_take_tensors_through_the_same_check():
    io = L.RenderIO()
    with pytest.raises(ValueError, match="O2345RenderIO: rays_o: expected .* got a tensor of torch.float32 on cpu"):
        io.point(rays_o=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="O2345RenderIO: nviews: expected .*uint8"):
        io.point(nviews=np.zeros(4, np.uint8))
    with pytest.raises(KeyError):
        io.point(R=4)                                                              # not a pointer field
    io.point(rays_o=None, color_stats=None)
    assert io.rays_o is None and io.color_stats is None


class FakeTensor:
    """What the converter asks of a device tensor (_lib does not import torch): enough to check dtype and contiguity rules without a GPU."""
    is_cuda, device = True, "cuda:0"

    def __init__(self, dtype, contiguous=True, numel=0):
        self.dtype, self._c, self._n = dtype, contiguous, numel

    def is_contiguous(self):
        return self._c

    def numel(self):
        return self._n

    def data_ptr(self):
        return 4096


def test_device_pointers_check_dtype_and_contiguity():
    name = "o2345_sdf_mlp_x3"
    assert L.bind(name, args_of(name, index=FakeTensor(torch.int32), pts=FakeTensor(torch.float32)))[3:6] == [4096, 4096, None]
    for param, t, got in (("index", FakeTensor(torch.int64), "torch.int64"), ("pts", FakeTensor(torch.float32, False), "contiguous=False"),
                          ("out_sdf", FakeTensor(torch.float64), "torch.float64")):
        with pytest.raises(ValueError, match=f"{name}: {param}: expected .* got .*{got}"):
            L.bind(name, args_of(name, **{param: t}))
    io = L.RenderIO()
    with pytest.raises(ValueError, match="O2345RenderIO: color_mask: expected .*uint8.* got .*torch.float32"):
        io.point(color_mask=FakeTensor(torch.float32))
    io.point(color_mask=FakeTensor(torch.uint8), color_stats=FakeTensor(torch.int64))
    assert io.color_mask == 4096 and io.color_stats == 4096
    assert L.bind("o2345_mesh_pack_faces", args_of("o2345_mesh_pack_faces", tris=FakeTensor(torch.int16)))[0] == 4096        # void*: any dtype


# ---------------------------------------------------------------------------------------------------------- the declared structs
# The stats blocks of the C ABI as they were when each was a private struct of its .hip file (ProjStats, TexStats, SurfStats, MdStats) and a list of
# byte offsets in ops.py: the independent statement of their layout.  name -> (sizeof, [(field, offset)]).  The last two were int64 arrays whose entries
# an enum of the header named (commit 7cbf4a6): their offsets are 8 x those enumerators' values, their sizes 8 x the two that counted the entries (8, 32).
FROZEN = {
    "O2345ProjectStats": (328, [("n_nonfinite", 0), ("converged", 8), ("unconverged", 16), ("stalled", 24), ("clamped", 32), ("max_before", 40),
                                ("max_after", 48), ("reserved", 56), ("count", 64)]),
    "O2345TextureStats": (16, [("n_nonfinite", 0), ("n_bad", 8)]),
    "O2345SurfaceStats": (72, [("hits", 0), ("entry_hits", 8), ("box_misses", 16), ("misses", 24), ("stalled", 32), ("bad_rays", 40), ("samples", 48),
                               ("lookups", 56), ("n_list", 64), ("reserved", 68)]),
    "O2345DistanceStats": (128, [("sum_w", 0), ("sum_wd", 8), ("sum_wd2", 16), ("within", 24), ("max_d2_bits", 88), ("n", 96), ("n_unmatched", 104),
                                 ("n_degenerate", 112), ("n_bad", 120)]),
    "O2345SimplifyStats": (64, [("rounds", 0), ("vertices", 8), ("triangles", 16), ("stopped", 24), ("max_cost_bits", 32), ("reserved", 40)]),
    "O2345AuditStats": (256, [("bad_index", 0), ("nonfinite", 8), ("vertices", 16), ("edges", 24), ("faces", 32), ("repeated_faces", 40), ("zero_area_faces", 48),
                              ("boundary_edges", 56), ("nonmanifold_edges", 64), ("inconsistent_edges", 72), ("creased_edges", 80), ("boundary_vertices", 88),
                              ("nonmanifold_vertices", 96), ("bowtie_vertices", 104), ("unused_vertices", 112), ("reserved", 120), ("histogram", 128),
                              ("area", 208), ("volume6", 216), ("quality_sum", 224), ("quality_min", 232), ("edge2_min", 240), ("edge2_max", 248)]),
}
STATS_ENTRY = {"O2345ProjectStats": "o2345_mesh_project", "O2345TextureStats": "o2345_mesh_texture_points", "O2345SurfaceStats": "o2345_surface_trace",
               "O2345DistanceStats": "o2345_mesh_distance_reduce", "O2345SimplifyStats": "o2345_mesh_simplify_count", "O2345AuditStats": "o2345_mesh_audit"}


def test_stats_struct_layouts_are_frozen():
    assert list(L.STRUCTS) == L.struct_names() == ["O2345RenderIO", "O2345ProjectStats", "O2345TextureStats", "O2345SurfaceStats", "O2345DistanceStats",
                                                      "O2345SimplifyStats", "O2345AuditStats"]
    assert L.STRUCTS["O2345RenderIO"] is L.RenderIO
    for name, (size, offsets) in FROZEN.items():
        cls = L.STRUCTS[name]
        assert cls.__name__ == name[5:] and cls._fields_ == L.parse_struct(name)
        assert ctypes.sizeof(cls) == size and [(f, getattr(cls, f).offset) for f, _ in cls._fields_] == offsets, name
    P, D = L.STRUCTS["O2345ProjectStats"], L.STRUCTS["O2345DistanceStats"]
    assert P.count.size == 66 * 4 and D.within.size == 8 * 8 and dict(D._fields_)["sum_w"] is ctypes.c_double and dict(P._fields_)["clamped"] is ctypes.c_ulonglong
    lib = L.lib()                                                                  # the compiled side says the same
    for which, name in enumerate(L.STRUCTS):
        assert lib.o2345_struct_size(which) == ctypes.sizeof(L.STRUCTS[name]) and lib.o2345_struct_layout(which, None, 0) == len(L.STRUCTS[name]._fields_)
    assert lib.o2345_struct_size(len(L.STRUCTS)) == 0 and lib.o2345_struct_layout(-1, None, 0) == 0


def test_the_names_python_keeps_are_the_headers():
    ops, mio = importlib.import_module("one-2-3-45_amd.ops"), importlib.import_module("one-2-3-45_amd.mesh_io")
    A = L.STRUCTS["O2345AuditStats"]
    fields = dict(A._fields_)
    assert all(fields[k] is ctypes.c_ulonglong for k in mio.AUDIT_COUNTS) and len(set(mio.AUDIT_COUNTS)) == len(mio.AUDIT_COUNTS) == 13
    assert A.histogram.size == 8 * mio.AUDIT_BINS and fields["histogram"] is ctypes.c_ulonglong * mio.AUDIT_BINS
    assert all(fields[k] is ctypes.c_double for k in ("area", "volume6", "quality_sum", "quality_min", "edge2_min", "edge2_max"))
    codes = {k.lower(): int(v) for k, v in re.findall(r"O2345_SIMPLIFY_STOPPED_(\w+) = (\d+)", open(L.HEADER).read())}
    assert len(codes) == 3 == len(ops._SIMPLIFY_STOPPED) and all(ops._SIMPLIFY_STOPPED[v] == k for k, v in codes.items())


def test_struct_parser_reads_arrays_and_several_names_per_declaration(tmp_path):
    path = tmp_path / "h.h"
    path.write_text("/* typedef struct O2345Ghost { int x; } O2345Ghost; */\n"
                    "typedef struct O2345Demo { unsigned long long a, b;  /* two */ double w[8]; int n[3], m;\n const float* p; uint8_t* q; } O2345Demo;\n"
                    "typedef struct O2345Next { float f; } O2345Next;\nint o2345_x(O2345Demo* demo, const O2345Next* next_host, void* stream);")
    assert L.struct_names(str(path)) == ["O2345Demo", "O2345Next"]
    assert L.parse_struct("O2345Demo", str(path)) == [("a", ctypes.c_ulonglong), ("b", ctypes.c_ulonglong), ("w", ctypes.c_double * 8), ("n", ctypes.c_int * 3),
                                                       ("m", ctypes.c_int), ("p", ctypes.c_void_p), ("q", ctypes.c_void_p)]
    fields = {p.name: p for p in L.struct_fields("O2345Demo", str(path))}
    assert fields["p"].elem == "float32" and fields["q"].elem == "uint8" and fields["w"].elem is None and not any(p.host for p in fields.values())
    params = L.prototypes(str(path))["o2345_x"][1]
    assert [(p.name, p.elem, p.host) for p in params[:2]] == [("demo", "struct O2345Demo", False), ("next_host", "struct O2345Next", True)]
    path.write_text("typedef struct O2345Demo { const float* a, *b; } O2345Demo;")
    with pytest.raises(ValueError, match="O2345Demo: one pointer per declaration"):
        L.struct_fields("O2345Demo", str(path))
    for text in ("typedef struct O2345Demo { short s[4]; } O2345Demo;", "typedef struct O2345Demo { float* p[4]; } O2345Demo;"):
        path.write_text(text)
        with pytest.raises(ValueError, match="O2345Demo"):
            L.struct_fields("O2345Demo", str(path))
    path.write_text("int o2345_x(int n[3]);")                                       # an array is a field, never a parameter
    with pytest.raises(ValueError, match="o2345_x"):
        L.prototypes(str(path))
    with pytest.raises(ValueError, match="O2345Missing is not declared"):
        L.struct_fields("O2345Missing", str(path))


@pytest.mark.parametrize("struct", sorted(FROZEN))
def test_a_stats_tensor_smaller_than_its_struct_is_refused(struct):
    name, size = STATS_ENTRY[struct], FROZEN[struct][0]
    stats = [p.name for p in PROTOTYPES[name][1]].index("stats")
    assert L.bind(name, args_of(name, stats=FakeTensor(torch.uint8, numel=size)))[stats] == 4096
    assert L.bind(name, args_of(name, stats=FakeTensor(torch.uint8, numel=2 * size)))[stats] == 4096           # a row of a larger buffer, a guard band behind it
    for t, got in ((FakeTensor(torch.uint8, numel=size - 1), rf"torch.uint8 .*\[{size - 1}\]"), (FakeTensor(torch.float32, numel=size), "torch.float32"),
                   (FakeTensor(torch.uint8, False, numel=size), "contiguous=False"), (np.zeros(size, np.uint8), "numpy"), (bytes(size), "bytes")):
        with pytest.raises(ValueError, match=rf"^{name}: stats: expected None or a contiguous GPU tensor of uint8 \[>= {size}\] \({struct}\), got .*{got}"):
            L.bind(name, args_of(name, stats=t))


def test_read_struct_takes_a_host_copy_and_checks_its_length():
    raw = np.arange(72, dtype=np.uint8)
    st = L.read_struct("O2345SurfaceStats", raw)
    assert st.hits == int(raw[:8].view(np.uint64)[0]) and st.n_list == int(raw[64:68].view(np.int32)[0]) and st.reserved == int(raw[68:].view(np.int32)[0])
    assert bytes(st) == raw.tobytes() == bytes(L.read_struct("O2345SurfaceStats", raw.tobytes())) == bytes(L.read_struct("O2345SurfaceStats", np.r_[raw, raw]))
    raw[0] = 255
    assert st.hits & 255 == 0                                                      # a copy
    with pytest.raises(ValueError, match="O2345SurfaceStats: expected at least 72 bytes, got 71"):
        L.read_struct("O2345SurfaceStats", raw[:71])


# The four decoders of ops.py on synthetic blocks laid out with explicit byte offsets.  The expected values were recorded from the decoders at commit
# 08e2544, which sliced the blocks at literal offsets (stats[:64].view(np.uint64), raw[88:].view(np.uint64), ...), for these same bytes.
def _put(raw, offset, dtype, values):
    v = np.atleast_1d(np.asarray(values, dtype))
    raw[offset:offset + v.nbytes] = v.view(np.uint8)


def _project_block(n_nonfinite=0):
    raw = np.zeros(328, np.uint8)
    _put(raw, 0, np.uint64, [n_nonfinite, 11, 12, 13, 14])
    _put(raw, 40, np.float64, [0.1, 1.5e-7])                  # max_before, max_after: bit patterns of doubles
    _put(raw, 56, np.uint64, 99)                              # reserved: not reported
    _put(raw, 64, np.int32, 1000 - 7 * np.arange(66))
    return raw


def _surface_block():
    raw = np.zeros(72, np.uint8)
    _put(raw, 0, np.uint64, 2 ** 40 + 101 + np.arange(8))
    _put(raw, 64, np.int32, [55, 7])
    return raw


def _texture_block(n_nonfinite=0, n_bad=0):
    raw = np.zeros(16, np.uint8)
    _put(raw, 0, np.uint64, [n_nonfinite, n_bad])
    return raw


def _distance_block(n_unmatched=0, n_bad=0, sum_w=7.3):
    raw = np.zeros(128, np.uint8)
    _put(raw, 0, np.float64, [sum_w, 2.1, 0.9])
    _put(raw, 24, np.float64, 0.3 + 0.7 * np.arange(8))
    _put(raw, 88, np.float64, 0.3)                            # max_d2_bits
    _put(raw, 96, np.uint64, [4096, n_unmatched, 5, n_bad])
    return raw


# The two decoders of the mesh units that came later, likewise: the expected values were recorded from ops.simplify_info and ops.audit_info at commit
# 7cbf4a6, which indexed an int64 array through the header's enumerators, for these same bytes.
def _simplify_block(rounds, stopped, max_rounds=5):
    raw = np.zeros(64 + 8 * max_rounds, np.uint8)
    _put(raw, 0, np.int64, [rounds, 2 ** 33 + 7, 2 ** 34 + 9, stopped])
    _put(raw, 32, np.float64, 0.0625 + 1e-9)                  # max_cost_bits
    _put(raw, 40, np.int64, [97, 98, 99])                     # reserved: not reported
    _put(raw, 64, np.int64, 500 - 3 * np.arange(max_rounds))  # behind the struct: the collapses of every round
    return raw


def _audit_block(bad_index=0, nonfinite=0):
    raw = np.zeros(256, np.uint8)
    _put(raw, 0, np.uint64, [bad_index, nonfinite])
    _put(raw, 16, np.uint64, 2 ** 35 + 1000 + 11 * np.arange(13))
    _put(raw, 120, np.uint64, 99)                             # reserved: not reported
    _put(raw, 128, np.uint64, 3 + 7 * np.arange(10))          # histogram
    _put(raw, 208, np.float64, [12.5, -7.75, 33.3, np.inf, 1e-4, 9.0])        # area, volume6, quality_sum, quality_min, edge2_min, edge2_max: doubles
    return raw


def test_stats_decoders_return_what_they_returned():
    ops = importlib.import_module("one-2-3-45_amd.ops")
    want = {"evaluated": [1000, 993, 986, 979, 972, 965], "converged": 11, "unconverged": 12, "stalled": 13, "clamped": 14, "max_before": 0.1, "max_after": 1.5e-07}
    got = ops.project_info(_project_block(), 5)
    assert got == want and [type(v) for v in got.values()] == [list, int, int, int, int, float, float] and type(got["evaluated"][0]) is int
    assert ops.project_info(_project_block(), 64)["evaluated"][-2:] == [559, 552] and len(ops.project_info(_project_block(), 65)["evaluated"]) == 66
    got = ops.surface_info(_surface_block(), 640)
    assert got == {"rays": 640, "hits": 1099511627877, "entry_hits": 1099511627878, "box_misses": 1099511627879, "misses": 1099511627880,
                   "stalled": 1099511627881, "bad_rays": 1099511627882, "samples": 1099511627883, "lookups": 1099511627884}
    assert list(got) == ["rays", "hits", "entry_hits", "box_misses", "misses", "stalled", "bad_rays", "samples", "lookups"] and all(type(v) is int for v in got.values())
    assert ops.surface_info(torch.from_numpy(_surface_block()).numpy().reshape(1, 72), 640) == got            # as pipeline.py hands it over: stats.cpu().numpy()
    assert ops.texture_check(_texture_block()) is None and ops.texture_check(np.stack([_texture_block(), _texture_block(1, 1)])[0]) is None
    within = [0.0410958904109589, 0.136986301369863, 0.2328767123287671, 0.32876712328767116, 0.4246575342465753, 0.5205479452054794, 0.6164383561643835,
              0.7123287671232876]
    for k in (0, 3, 8):
        got, degenerate = ops.distance_summary(_distance_block(), k, 12)
        assert got == {"mean": 0.28767123287671237, "rms": 0.3511234415883917, "max": 0.5477225575051661, "within": within[:k], "samples": 4096, "area": 7.3}
        assert degenerate == 5 and [type(v) for v in got.values()] == [float, float, float, list, int, float] and all(type(w) is float for w in got["within"])
    got, degenerate = ops.distance_summary(_distance_block(sum_w=0.0), 2)
    assert np.isnan([got["mean"], got["rms"]] + got["within"]).all() and len(got["within"]) == 2 and (got["max"], got["samples"], got["area"], degenerate) == (0.5477225575051661, 4096, 0.0, 5)
    assert ops.distance_summary(np.stack([_distance_block(), _distance_block(3)])[0], 3) == ops.distance_summary(_distance_block(), 3)      # a row of the [2, 128] read-back
    for (rounds, stopped), collapses, word in (((0, 0), [], "target"), ((3, 1), [500, 497, 494], "blocked"), ((5, 2), [500, 497, 494, 491, 488], "rounds")):
        raw = _simplify_block(rounds, stopped)                                     # five rounds of room: the last case fills the buffer
        got = ops.simplify_info(raw)
        assert got == {"rounds": rounds, "vertices": 8589934599, "triangles": 17179869193, "collapses": collapses, "max_cost": 0.062500001, "stopped": word}
        assert list(got) == ["rounds", "vertices", "triangles", "collapses", "max_cost", "stopped"]
        assert [type(v) for v in got.values()] == [int, int, int, list, float, str] and all(type(c) is int for c in got["collapses"])
        assert ops.simplify_info(raw.view(np.int64)) == got == ops.simplify_info(raw.tobytes())          # an int64 array, as it was handed over before; bytes
    want = {"vertices": 34359739368, "edges": 34359739379, "faces": 34359739390, "repeated_faces": 34359739401, "zero_area_faces": 34359739412,
            "boundary_edges": 34359739423, "nonmanifold_edges": 34359739434, "inconsistent_edges": 34359739445, "creased_edges": 34359739456,
            "boundary_vertices": 34359739467, "nonmanifold_vertices": 34359739478, "bowtie_vertices": 34359739489, "unused_vertices": 34359739500,
            "histogram": [3, 10, 17, 24, 31, 38, 45, 52, 59, 66], "area": 12.5, "volume": -1.2916666666666667, "quality_mean": 9.691575253824997e-10,
            "quality_min": float("inf"), "edge_min": 0.01, "edge_max": 3.0, "euler": 34359739379, "components": 4, "oriented": False, "watertight": False,
            "genus": None}
    got = ops.audit_info(_audit_block(), 77, 4)
    assert got == want and list(got) == list(want) and all(type(c) is int for c in got["histogram"])
    assert [type(v) for v in got.values()] == [int] * 13 + [list] + [float] * 6 + [int, int, bool, bool, type(None)]
    assert ops.audit_info(_audit_block().view(np.int64), 77, lambda: 4) == got == ops.audit_info(_audit_block().tobytes(), 77, 4)


@pytest.mark.parametrize("decode, message", [
    (lambda ops: ops.project_info(_project_block(3), 5), "o2345 mesh_project: 3 vertices have a non-finite coordinate"),
    (lambda ops: ops.texture_check(_texture_block(2, 0)), "o2345 mesh_texture_points: 2 triangles have a non-finite vertex coordinate"),
    (lambda ops: ops.texture_check(_texture_block(2, 4)), "o2345 mesh_texture_points: 4 triangles index outside the vertex array"),
    (lambda ops: ops.distance_summary(_distance_block(n_bad=6, n_unmatched=9), 1), "o2345 mesh_distance: 6 target triangles have an index out of range or a non-finite coordinate"),
    (lambda ops: ops.distance_summary(_distance_block(n_unmatched=9), 1), "o2345 mesh_distance: 9 of 4096 samples found no triangle: the target has no triangle with an area"),
    (lambda ops: ops.distance_summary(_distance_block(n_unmatched=9), 1, 12),
     "o2345 mesh_distance: 9 of 4096 samples found no triangle: the target has no triangle with an area (12 triangles, 5 degenerate)"),
    (lambda ops: ops.audit_info(_audit_block(3, 5), 77, 4), "o2345 mesh_audit: 3 triangles index outside 0 .. 76"),         # before the non-finite count
    (lambda ops: ops.audit_info(_audit_block(3, 0), 77, 4), "o2345 mesh_audit: 3 triangles index outside 0 .. 76"),
    (lambda ops: ops.audit_info(_audit_block(0, 5), 77, 4), "o2345 mesh_audit: 5 vertices have a non-finite coordinate"),
])
def test_stats_decoders_raise_what_they_raised(decode, message):
    with pytest.raises(RuntimeError) as e:
        decode(importlib.import_module("one-2-3-45_amd.ops"))
    assert str(e.value) == message
