"""TEST INFRASTRUCTURE shared by the test_*_meta.py files: the kernels of one built object as tools/kernel_meta.py describes them, and the
args structs of include/mphsir.h that are declared as `struct ...; typedef ...;` (they may have float members) as ctypes fields."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

_CTYPE_OF = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}


def object_kernels(stem):
    """kernel_meta.object_kernels of mp-hsir_amd/build/<stem>.o; the library is built first when the object is missing"""
    build = os.path.join(ROOT, "mp-hsir_amd", "build")
    if not os.path.exists(os.path.join(build, stem + ".o")):
        sys.path.insert(0, os.path.join(ROOT, "mp-hsir_amd"))
        import build as B
        B.build(verbose=False)
    import kernel_meta
    return kernel_meta.object_kernels(os.path.join(build, stem + ".o"))


def kernels_by_name(stem):
    """{demangled name without return type, arguments and template arguments: [its instances in <stem>.o]}"""
    ks = {}
    for k in object_kernels(stem):
        ks.setdefault(re.sub(r"^void ", "", k["demangled"].split("(")[0]).split("<")[0], []).append(k)
    return ks


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mphsir.h")).read(), flags=re.S)


def header_struct(name):
    m = re.search(r"struct %s \{(.*?)\};\s*typedef struct %s %s;" % (name, name, name), header_text(), flags=re.S)
    assert m, "include/mphsir.h does not declare struct %s" % name
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        if "*" in decl:
            pm = re.match(r"^(?:const )?\w+\s*\*\s*(\w+)$", decl)
            assert pm, decl
            fields.append((pm.group(1), ctypes.c_void_p))
        else:
            ty, names = decl.split(" ", 1)
            fields += [(n.strip(), _CTYPE_OF[ty]) for n in names.split(",")]
    return fields
