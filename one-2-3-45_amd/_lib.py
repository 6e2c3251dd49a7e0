"""ctypes loader and call path for libo2345_hip.so.  Everything the binding knows about an entry point is read from include/o2345.h: the prototypes,
the element type of every pointer, whether a pointer is a host or a device pointer (the header's rule: a pointer is a HOST pointer if and only if its
name ends in _host, or the function's name ends in _host), and every struct that crosses the boundary.  ``call`` converts and checks the arguments of
one entry against that table and raises on a non-zero status.  There is NO fallback: if the library is missing or a call fails, this raises.  torch
is not imported here: a device tensor is recognised by what it offers (is_cuda, is_contiguous(), dtype, data_ptr(), numel())."""
import ctypes
import os
import re
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "o2345.h")
LIB_PATH = os.environ.get("O2345_LIB") or os.path.join(HERE, "libo2345_hip.so")       # O2345_LIB: an A/B build variant (build.build_variant)

ABI_VERSION = 231         # include/o2345.h: o2345_version()

_CT = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "void": None, "double": ctypes.c_double,
       "unsigned long long": ctypes.c_ulonglong}
# pointee C type -> element type: the dtype a device tensor must have ("void": any; "size_t": host arrays only)
_ELEM = {"float": "float32", "double": "float64", "int": "int32", "int32_t": "int32", "uint32_t": "int32", "uint8_t": "uint8", "unsigned char": "uint8",
         "long long": "int64", "unsigned long long": "int64", "size_t": "size_t", "void": "void"}

# one parameter of a declared function or one field of a declared struct.  elem: None for a scalar, "struct <name>", or an element type of _ELEM;
# host: a pointer the host dereferences
Param = namedtuple("Param", "name ctype elem host")


def _param(decl, fn, what):
    m = re.fullmatch(r"(?:const\s+)?([\w ]+?)\s*(\*?)\s*(\w+)(?:\s*\[(\d+)\])?", " ".join(decl.split()))
    if not m or (m.group(4) and (m.group(2) or what != "field")):             # name[N]: a fixed-size array of scalars, in a struct only
        raise ValueError(f"cannot parse {what} {decl!r} of {fn}")
    base, star, name, count = m.groups()
    if not star:
        if base not in _CT or _CT[base] is None:
            raise ValueError(f"cannot map C type {decl!r} in {fn}")
        return Param(name, _CT[base] * int(count) if count else _CT[base], None, False)
    struct = base.startswith("O2345")
    host = name.endswith("_host") or fn.endswith("_host")
    if not struct and (base not in _ELEM or (base == "size_t" and not host)):
        raise ValueError(f"cannot map pointee type of {decl!r} in {fn}")
    return Param(name, ctypes.c_void_p, "struct " + base if struct else _ELEM[base], host)


def prototypes(path=HEADER):
    """-> {name: (restype, [Param])} for every function declared in the header."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"typedef struct.*?\}\s*\w+;", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(o2345_\w+)\s*\(([^;{]*?)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        rest = ctypes.c_char_p if (ret.startswith("const char") or name in ("o2345_last_error", "o2345_knobs")) else (_CT["size_t"] if ret == "size_t" else ctypes.c_int)
        protos[name] = (rest, [] if args in ("", "void") else [_param(a, name, "parameter") for a in args.split(",")])
    return protos


def parse_header(path=HEADER):
    """-> {name: (restype, [argtypes])} for every function declared in the header: what load_library attaches (every pointer a c_void_p)."""
    return {name: (rest, [p.ctype for p in params]) for name, (rest, params) in prototypes(path).items()}


def struct_names(path=HEADER):
    """-> the names of the header's ``typedef struct O2345...`` declarations, in order: a struct's position is its number in o2345_struct_layout."""
    return re.findall(r"typedef struct (O2345\w+)\s*\{", re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S))


def struct_fields(name, path=HEADER):
    """-> [Param] of ``typedef struct <name> {...} <name>;`` in the header, in declaration order: the binding's struct is GENERATED from the one
    declaration the C side compiles (csrc/ includes the same header), never kept by hand.  Its pointers are device pointers; ``name[N]`` is an array."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    m = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S)
    if not m:
        raise ValueError(f"{name} is not declared in {path}")
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        if "*" in decl and "," in decl:
            raise ValueError(f"{name}: one pointer per declaration, got {decl!r}")
        typ, names = ("", decl) if "*" in decl else re.fullmatch(r"(.*?)(\w+(?:\s*\[\d+\])?(?:\s*,.*)?)", decl).groups()      # "unsigned long long " + "a, b[8]"
        fields += [_param(f"{typ} {n}", name, "field") for n in names.split(",")]
    return fields


def parse_struct(name, path=HEADER):
    """-> [(field, ctypes type)] of the struct, in declaration order (every pointer a c_void_p)."""
    return [(p.name, p.ctype) for p in struct_fields(name, path)]


# ---------------------------------------------------------------------------------------------------------- the converter
def _got(v):
    if isinstance(v, np.ndarray):
        return f"a numpy array of {v.dtype}, C-contiguous={v.flags.c_contiguous}"
    return f"a tensor of {v.dtype} on {v.device}, contiguous={v.is_contiguous()}" if hasattr(v, "data_ptr") else f"{type(v).__name__} {v!r}"


def _device_pointer(where, elem):
    """A struct on the device is a uint8 tensor (torch has no struct dtype) of at least the struct's size."""
    nbytes = ctypes.sizeof(STRUCTS[elem[7:]]) if elem.startswith("struct ") else 0
    elem, what = ("uint8", f"uint8 [>= {nbytes}] ({elem[7:]})") if nbytes else (elem, elem)
    want = getattr(sys.modules.get("torch"), elem, None)           # None: any dtype, or torch is not imported yet (whoever holds a tensor has done that)

    def conv(v):
        if v is None:
            return None
        try:
            if v.is_cuda and v.is_contiguous() and (v.dtype is want or elem == "void" or v.dtype is getattr(sys.modules["torch"], elem)) and (
                    not nbytes or v.numel() >= nbytes):
                return v.data_ptr()
        except AttributeError:
            pass
        raise ValueError(f"{where}: expected None or a contiguous GPU tensor of {what}, got {_got(v)}" + (f" [{v.numel()}]" if nbytes and hasattr(v, "numel") else ""))
    return conv


def _host_pointer(where, elem):
    """Signedness is not told apart, as little as the element table tells uint32_t from int32_t: the matching type has the element's size and is of
    its kind, integer or floating.  A struct is passed as the ctypes Structure of its name."""
    dt = None if elem == "void" or elem.startswith("struct ") else np.dtype(np.uintp if elem == "size_t" else elem)
    size, kinds, codes = (dt.itemsize,) + (("f", "fd") if dt.kind == "f" else ("iu", "bBhHiIlLqQ")) if dt else (0, "", "")

    def conv(v):
        if v is None:
            return None
        if isinstance(v, np.ndarray):
            if v.flags.c_contiguous and (elem == "void" or (v.dtype.itemsize == size and v.dtype.kind in kinds)):
                return v.ctypes.data
        elif isinstance(v, ctypes.Structure):
            if elem == "struct O2345" + type(v).__name__:
                return ctypes.addressof(v)
        elif isinstance(v, (ctypes._SimpleCData, ctypes.Array)):
            et = v._type_ if isinstance(v, ctypes.Array) else type(v)
            if elem == "void" or (ctypes.sizeof(et) == size and getattr(et, "_type_", None) in tuple(codes)):      # the format code of a simple type
                return ctypes.addressof(v)
        raise ValueError(f"{where}: expected None, a C-contiguous numpy array or a ctypes object of {elem} on the host, got {_got(v)}")
    return conv


def _integer(where, ct):
    bits = 8 * ctypes.sizeof(ct)
    lo, hi = (0, 2 ** bits - 1) if ct is ctypes.c_size_t else (-2 ** (bits - 1), 2 ** (bits - 1) - 1)

    def conv(v):
        i = v if type(v) is int else getattr(v, "__index__", lambda: None)()
        if i is None or not lo <= i <= hi:
            raise ValueError(f"{where}: expected an integer in [{lo}, {hi}], got {_got(v)}")
        return i
    return conv


def _converter(p, where):
    if p.elem is None:
        return None if p.ctype in (ctypes.c_float, ctypes.c_double) else _integer(where, p.ctype)
    if p.name == "stream" and p.elem == "void":
        return None                 # like float and double: ctypes' own conversion
    return (_host_pointer if p.host else _device_pointer)(where, p.elem)


# name -> (params, binder, n, stream, status) of a declared function.  binder: its arguments -> the list ctypes passes, ONE expression per parameter
# compiled once (a float and the stream pass as they are; a Python int in [0, 2^31) fits every C integer type; the rest goes through its converter);
# stream: the last parameter is `void* stream`; status: the int it returns is a status, not a value
_SIGNATURES = {}


def signature(name):
    for n, (rest, params) in () if _SIGNATURES else prototypes().items():          # all built once, at the first call
        conv = {f"c{k}": _converter(p, f"{n}: {p.name}") for k, p in enumerate(params)}
        expr = [f"a{k}" if conv[f"c{k}"] is None else f"c{k}(a{k})" if p.elem else f"a{k} if type(a{k}) is int and 0 <= a{k} < 2147483648 else c{k}(a{k})"
                for k, p in enumerate(params)]
        binder = eval(f"lambda {', '.join(f'a{k}' for k in range(len(params)))}: [{', '.join(expr)}]", conv)
        _SIGNATURES[n] = (params, binder, len(params), bool(params) and params[-1][::2] == ("stream", "void"),
                          rest is ctypes.c_int and not n.endswith(("_floats", "_version", "_layout")))
    return _SIGNATURES[name]


def bind(name, args):
    """The arguments of entry ``name`` as the header declares them -> what ctypes passes: a device pointer takes None or a contiguous GPU tensor of the
    declared element type, a host pointer None, a C-contiguous numpy array or a ctypes object of it (passed by reference), an integer must fit its C
    type.  Every refusal is a ValueError ``o2345_<fn>: <param>: expected ..., got ...``."""
    params, binder, n, _, _ = _SIGNATURES.get(name) or signature(name)
    if len(args) != n:
        raise ValueError(f"{name}: expected {n} arguments ({', '.join(p.name for p in params)}), got {len(args)}")
    return binder(*args)


def call(name, *args):
    """Entry ``name`` on bind's arguments; its last parameter `void* stream`, when left out, is the current torch stream of the current device.  A
    function that returns a status returns nothing here and raises RuntimeError with o2345_last_error() when it fails; any other function (*_bytes,
    *_floats, o2345_mesh_texture_texels, ...) returns its value."""
    params, binder, n, stream, status = _SIGNATURES.get(name) or signature(name)
    if stream and len(args) == n - 1:
        args += (sys.modules["torch"].cuda.current_stream().cuda_stream,)
    rc = getattr(_LIB or lib(), name)(*(binder(*args) if len(args) == n else bind(name, args)))         # the library current at call time: tests make another one current
    if status and rc:
        check(rc, name[6:])
    return None if status else rc


class RenderIO(ctypes.Structure):
    _fields_ = parse_struct("O2345RenderIO")
    _pointers = {p.name: _device_pointer(f"O2345RenderIO: {p.name}", p.elem) for p in struct_fields("O2345RenderIO") if p.elem}

    def point(self, **tensors):
        """Pointer fields <- tensors (or None), each checked like a device pointer parameter of its declared element type."""
        for k, t in tensors.items():
            setattr(self, k, self._pointers[k](t))


# every struct the header declares, in its order -> the Structure generated from its text (RenderIO and the six stats blocks)
STRUCTS = {name: RenderIO if name == "O2345RenderIO" else type(name[5:], (ctypes.Structure,), {"_fields_": parse_struct(name)}) for name in struct_names()}


def read_struct(name, block):
    """A host copy of a block (bytes, or an array of at least the struct's size: its first bytes) -> the generated Structure, fields by name."""
    raw = block if isinstance(block, (bytes, bytearray)) else np.ascontiguousarray(block).reshape(-1).view(np.uint8)
    if len(raw) < ctypes.sizeof(STRUCTS[name]):
        raise ValueError(f"{name}: expected at least {ctypes.sizeof(STRUCTS[name])} bytes, got {len(raw)}")
    return STRUCTS[name].from_buffer_copy(raw)


def check_struct_layout(L, name, path=LIB_PATH, cls=None):
    """The loaded library's own sizeof / offsetof table against the generated Structure (``cls``: another one, for a test): a field added to, removed
    from or reordered in only one of the header the library was compiled with and the header this binding parsed fails HERE, at load time, instead of
    corrupting calls."""
    cls, which = cls or STRUCTS[name], list(STRUCTS).index(name)
    want = (ctypes.c_size_t * 256)()
    n, size = L.o2345_struct_layout(which, want, 256), L.o2345_struct_size(which)
    mine = [(f, getattr(cls, f).offset) for f, _ in cls._fields_]
    if n != len(mine) or size != ctypes.sizeof(cls) or any(int(want[i]) != off for i, (_, off) in enumerate(mine)):
        theirs = [int(want[i]) for i in range(min(n, 256))]
        raise RuntimeError(f"{name} layout mismatch between {path} ({n} fields, {size} bytes, offsets {theirs}) and "
                           f"{HEADER} ({len(mine)} fields, {ctypes.sizeof(cls)} bytes, offsets {[o for _, o in mine]}): rebuild the library")


_LIB = None


def load_library(path):
    """dlopen ``path``, attach the header's prototypes, check ABI version and struct layouts.  ``lib()`` does this once for the product library; tests load
    build variants (libo2345_hip_<tag>.so) next to it with this."""
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python __graft_entry__.py build` (hipcc, gfx950). "
                           "There is no CPU fallback for the reconstruction path.")
    L = ctypes.CDLL(path)
    if L.o2345_version() != ABI_VERSION:          # first: a library of another ABI need not export what this header declares
        raise RuntimeError(f"{path} implements ABI {L.o2345_version()}, this binding expects {ABI_VERSION}: rebuild the library")
    for name, (rest, argt) in parse_header().items():
        fn = getattr(L, name)          # AttributeError if the library does not export a declared symbol
        fn.restype, fn.argtypes = rest, argt
    for name in STRUCTS:
        check_struct_layout(L, name, path)
    L.o2345_knobs()                    # the environment knobs are read now, once (csrc/common.h)
    return L


def lib():
    global _LIB
    if _LIB is None:
        _LIB = load_library(LIB_PATH)
    return _LIB


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError(f"o2345 {what} failed ({rc}): {lib().o2345_last_error().decode()}")
