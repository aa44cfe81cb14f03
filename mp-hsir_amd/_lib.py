"""ctypes binding of libmphsir.so, read from include/mphsir.h at import: the header is the one description of the C ABI, and its structs,
prototypes and constants are parsed here, not restated.  No CPU fallback: if the HIP library is missing or does not load, every op
raises -- build it with ``python mp-hsir_amd/build.py``.
"""
import ctypes
import os
import re

import torch  # noqa: F401  -- must come first: libmphsir.so binds to the HIP runtime PyTorch-ROCm already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, os.environ.get("MPHSIR_LIB_AB", "libmphsir.so"))      # MPHSIR_LIB_AB: another in-tree build of the same sources, for A/B timing on one box
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mphsir.h")
_lib = None
_is_emu = False

_SCALARS = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
_POINTEES = set(_SCALARS) | {"void", "char", "double", "uint8_t"}      # what a pointer bound as c_void_p may point to


class _Args(ctypes.Structure):
    """base of every mphsir_*_args struct: the first member, struct_size, is filled in on construction (the library refuses a struct
    of another size: include/mphsir.h)"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = ctypes.sizeof(self)


def _refuse(where, decl):
    raise RuntimeError("mp-hsir_amd: include/mphsir.h: %s: cannot bind `%s` (the binding does not model it)" % (where, " ".join(decl.split())))


def _ctype(where, decl, structs):
    """(ctypes type, [names]) of a member (`int32_t B, H, W`, `const float* w9`) or an argument (`int dtype`, `const mphsir_x_args*`)"""
    m = re.fullmatch(r"\s*(const\s+)?(\w+)\s*(\*?)\s*((?:\w+\s*,\s*)*\w+)?\s*", decl)      # no `[`, `(`, `:`, `**`, `struct`, two-word types
    if not m:
        _refuse(where, decl)
    const, ty, star, names = m.groups()
    names = re.split(r"\s*,\s*", names) if names else []
    if star and ty in structs:
        return ctypes.POINTER(structs[ty]), names
    if star and ty in _POINTEES and len(names) <= 1:
        return ctypes.c_void_p, names
    if not star and not const and ty in _SCALARS:
        return _SCALARS[ty], names
    _refuse(where, decl)


def parse_header(text):
    """-> (structs {C name: ctypes.Structure subclass}, prototypes {name: (restype, argtypes)}, constants {NAME: int | float}) of a header
    written like include/mphsir.h.  Anything else (an array or bit-field member, a nested struct or union, a function pointer, an unknown
    type name, a pointer to a pointer) raises RuntimeError with the name of the struct or function and the declaration."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    structs, protos, consts = {}, {}, {}
    for name, value in re.findall(r"^[ \t]*#define[ \t]+(MPHSIR_\w+)[ \t]+\(?([-+.\w]+)\)?[ \t]*$", text, flags=re.M):
        consts[name] = float(value) if re.search(r"[.eE]", value) and not value.lower().startswith("0x") else int(value, 0)
    text = re.sub(r'^[ \t]*#.*$|^extern "C" \{[ \t]*$|^\}[ \t]*$', " ", text, flags=re.M)      # preprocessor lines, the extern "C" bracket

    def enum(m):
        for item in m.group(1).split(","):
            k, _, v = item.partition("=")
            consts[k.strip()] = int(v, 0) if re.fullmatch(r"\s*\w+\s*", k) and v.strip() else _refuse("enum", item)
        return " "

    def struct(m):
        name, body = m.groups()
        fields = []
        for decl in filter(str.strip, body.split(";")):
            t, names = _ctype(name, decl, {})
            fields += [(n, t) for n in names] if names else _refuse(name, decl)
        base = _Args if fields[:1] == [("struct_size", ctypes.c_uint32)] else ctypes.Structure
        cls = "".join(w.capitalize() for w in name[len("mphsir_"):].split("_"))
        structs[name] = type(cls, (base,), {"_fields_": fields, "__doc__": "struct %s of include/mphsir.h" % name})
        return " "

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+(mphsir_\w+)\s*\{((?:[^{}]|\{[^{}]*\})*)\}\s*\1\s*;", struct, text)
    for decl in filter(str.strip, text.split(";")):      # what is left is prototypes: `restype name(arguments)`
        m = re.fullmatch(r"\s*(const\s+char\s*\*|\w+)\s*\b(mphsir_\w+)\s*\(([^()]*)\)\s*", decl)
        if not m:
            _refuse((re.search(r"mphsir_\w+", decl) or re.search(r"\S+", decl)).group(), decl)
        ret, name, args = m.groups()
        res = ctypes.c_char_p if "*" in ret else _SCALARS.get(ret) or _refuse(name, decl)
        args = [] if args.strip() in ("", "void") else args.split(",")
        protos[name] = (res, [_ctype(name, a, structs)[0] for a in args])
    return structs, protos, consts


def _read_header():
    if not os.path.exists(_HEADER):
        raise RuntimeError("mp-hsir_amd: header %s not found -- the binding is read from it" % _HEADER)
    with open(_HEADER) as f:
        return parse_header(f.read())


STRUCTS, _SYMBOLS, CONSTANTS = _read_header()      # once per process: load() binds from these, it does not read the file again
globals().update({cls.__name__: cls for cls in STRUCTS.values()})      # GemmArgs, MlpArgs, ..., GemmTnProblem, ReduceSeg
TN_GROUP_MAX = CONSTANTS["MPHSIR_TN_GROUP_MAX"]
REDUCE_MAX_SEGS = CONSTANTS["MPHSIR_REDUCE_MAX_SEGS"]

# Additions to the ABI: headers beside mphsir.h that include it and declare entry points added after its surface was frozen by count
# (tests/test_cabi.py pins the entry points, structs and kernel ids of mphsir.h itself).  The same parser, tables of their own.
_ADDITIONS = ("mphsir_accum.h",)


def _read_additions(names=_ADDITIONS):
    structs, protos = {}, {}
    for name in names:
        path = os.path.join(os.path.dirname(_HEADER), name)
        if not os.path.exists(path):
            raise RuntimeError("mp-hsir_amd: header %s not found -- the binding is read from it" % path)
        with open(path) as f:
            s, p, _ = parse_header(f.read())
        structs.update(s)
        protos.update(p)
    return structs, protos


ADDED_STRUCTS, _ADDED_SYMBOLS = _read_additions()      # mphsir_multi_accum_args / mphsir_multi_accum
globals().update({cls.__name__: cls for cls in ADDED_STRUCTS.values()})      # MultiAccumArgs

# include/mphsir_bands.h (spectral windows of whole-scene inference): tables of its own, because tests/test_accum_host.py pins the contents
# of the two above as tests/test_cabi.py pins those of mphsir.h; checked by tests/test_scene_bands_host.py
BANDS_STRUCTS, _BANDS_SYMBOLS = _read_additions(("mphsir_bands.h",))
globals().update({cls.__name__: cls for cls in BANDS_STRUCTS.values()})      # SceneGatherBandsArgs, SceneBlendBandsArgs


def symbols():
    """Every entry point include/mphsir.h declares (checked by tests/test_cabi.py)."""
    return sorted(_SYMBOLS)


def added_symbols():
    """Every entry point the addition headers declare (include/mphsir_accum.h; checked by tests/test_accum_host.py)."""
    return sorted(_ADDED_SYMBOLS)


def bands_symbols():
    """Every entry point include/mphsir_bands.h declares (checked by tests/test_scene_bands_host.py)."""
    return sorted(_BANDS_SYMBOLS)


def _bind(lib):
    for name, (res, args) in list(_SYMBOLS.items()) + list(_ADDED_SYMBOLS.items()) + list(_BANDS_SYMBOLS.items()):
        fn = getattr(lib, name)     # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


def load(path=None):
    """Load (once) and return the library.  Raises RuntimeError if it cannot be loaded."""
    global _lib, _is_emu
    if _lib is not None and path is None:
        return _lib
    p = path or _PATH
    if not os.path.exists(p):
        raise RuntimeError("mp-hsir_amd: HIP library %s not found -- run `python mp-hsir_amd/build.py` "
                           "(there is no CPU fallback)" % p)
    try:
        lib = _bind(ctypes.CDLL(p))
    except (OSError, AttributeError) as e:
        raise RuntimeError("mp-hsir_amd: cannot load %s: %s" % (p, e))
    _lib = lib
    _is_emu = path is not None and "hipemu" in os.path.abspath(path)
    return _lib


def use_library_for_tests(path):
    """TESTS ONLY: bind the ops to another build of the same sources (tests/hipemu)."""
    return load(path)


def is_emulated():
    return _is_emu


def check(rc, what):
    if rc != 0:
        raise RuntimeError("mp-hsir_amd: %s failed (%d): %s" % (what, rc, load().mphsir_last_error().decode()))
