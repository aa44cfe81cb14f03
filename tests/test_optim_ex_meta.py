"""The clip / EMA kernels (mp-hsir_amd/csrc/optim.hip) in the built code object (CPU test): the names tools and profiles match on, no
register spills, no scratch, the earlier optimizer kernels still there -- and the two args structs of include/mphsir.h against their
ctypes images.  (tests/test_cabi.py compares every `typedef struct mphsir_* {` of the header with its mirror, but its parser knows
integer and pointer members only; these two structs are the first with float members, are declared as `struct ...; typedef ...;`,
and are compared here with a parser that knows float.)"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_new_kernels_exist_and_do_not_spill():
    build = os.path.join(ROOT, "mp-hsir_amd", "build")
    if not os.path.exists(os.path.join(build, "optim.o")):
        sys.path.insert(0, os.path.join(ROOT, "mp-hsir_amd"))
        import build as B
        B.build(verbose=False)
    import kernel_meta
    ks = {}
    for k in kernel_meta.object_kernels(os.path.join(build, "optim.o")):
        ks.setdefault(re.sub(r"^void ", "", k["demangled"].split("(")[0]).split("<")[0], []).append(k)
    assert sorted(ks) == ["mphsir::flat_adamw_ex_kernel", "mphsir::flat_adamw_kernel", "mphsir::grad_check_kernel", "mphsir::grad_norm_finish_kernel",
                          "mphsir::grad_sqnorm_kernel", "mphsir::scaler_update_kernel"], sorted(ks)
    assert len(ks["mphsir::flat_adamw_ex_kernel"]) == 2          # with and without the EMA arena
    for name in ("flat_adamw_ex_kernel", "grad_sqnorm_kernel", "grad_norm_finish_kernel"):
        for k in ks["mphsir::" + name]:
            assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
            assert k["max_flat_workgroup_size"] == 256
    # streaming kernels: full occupancy needs at most 64 registers per lane at 8 waves per SIMD
    assert all(k.get("vgpr_count", 0) <= 64 for k in ks["mphsir::flat_adamw_ex_kernel"] + ks["mphsir::grad_sqnorm_kernel"])


_CTYPE_OF = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}


def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "mphsir.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"struct %s \{(.*?)\};\s*typedef struct %s %s;" % (name, name, name), text, flags=re.S)
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


def test_the_two_args_structs_match_their_ctypes_images():
    import mp_hsir_amd._lib as L
    for name, cls in (("mphsir_grad_norm_args", L.GradNormArgs), ("mphsir_flat_adamw_ex_args", L.FlatAdamwExArgs)):
        want = _header_struct(name)
        got = list(cls._fields_)
        assert [n for n, _ in got] == [n for n, _ in want], (name, got, want)
        for (n, tg), (_, tw) in zip(got, want):
            assert ctypes.sizeof(tg) == ctypes.sizeof(tw) and (tg is ctypes.c_float) == (tw is ctypes.c_float), (name, n, tg, tw)
        assert want[0] == ("struct_size", ctypes.c_uint32) and cls().struct_size == ctypes.sizeof(cls)
    assert {"mphsir_grad_norm", "mphsir_grad_norm_workspace_bytes", "mphsir_flat_adamw_ex"} <= set(L.symbols())
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mphsir_grad_norm_args" in md and "mphsir_flat_adamw_ex_args" in md
