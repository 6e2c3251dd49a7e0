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
        assert p.host == (p.name.endswith("_host") or fn.endswith("_host") or struct), (fn, p)
        assert p.elem != "size_t" or p.host, (fn, p)
    host = {(fn, p.name) for fn, p in ptrs if p.host}
    assert len(host) == 59
    assert {("o2345_surface_trace", "bound_min_host"), ("o2345_mesh_distance_reduce", "thresholds_host"), ("o2345_render_rays", "io"),
            ("o2345_ply_records_host", "faces"), ("o2345_render_io_layout", "offsets_host")} <= host
    assert not {("o2345_sdf_grid_sparse_x3", "background"), ("o2345_mesh_decimate_count", "tris"), ("o2345_costvol_index", "n_rows_dev")} & host
    table = {(fn, p.name): p.elem for fn, p in ptrs}
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
    ("o2345_render_rays", "io", ctypes.c_int(), "c_int"),
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
    assert L.call("o2345_version") == L.ABI_VERSION == 210
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

    def __init__(self, dtype, contiguous=True):
        self.dtype, self._c = dtype, contiguous

    def is_contiguous(self):
        return self._c

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
