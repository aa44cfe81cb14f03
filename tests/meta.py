"""TEST INFRASTRUCTURE shared by the test_*_meta.py files: the kernels of one built object as tools/kernel_meta.py describes them."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


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

