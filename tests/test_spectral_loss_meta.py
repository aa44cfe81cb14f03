"""The spectral-loss kernels (mp-hsir_amd/csrc/spectral_loss.hip) in the built code object (CPU test): the names tools and profiles match on,
no register spills, no scratch, workgroups of 256 -- and the args struct of include/mphsir.h against its ctypes image, with the float-aware
parser of tests/test_optim_ex_meta.py (the struct has float members and is declared as `struct ...; typedef ...;`)."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_kernels_exist_and_do_not_spill():
    build = os.path.join(ROOT, "mp-hsir_amd", "build")
    if not os.path.exists(os.path.join(build, "spectral_loss.o")):
        sys.path.insert(0, os.path.join(ROOT, "mp-hsir_amd"))
        import build as B
        B.build(verbose=False)
    import kernel_meta
    ks = {}
    for k in kernel_meta.object_kernels(os.path.join(build, "spectral_loss.o")):
        ks.setdefault(re.sub(r"^void ", "", k["demangled"].split("(")[0]).split("<")[0], []).append(k)
    assert sorted(ks) == ["mphsir::spectral_loss_finish_kernel", "mphsir::spectral_loss_kernel"], sorted(ks)
    assert len(ks["mphsir::spectral_loss_kernel"]) == 2           # the 16-byte path and the scalar path
    for group in ks.values():
        for k in group:
            assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
            assert k["max_flat_workgroup_size"] == 256
    # two workgroups per CU at the training shape: 24.6 KB of LDS and at most 128 registers per lane leave room for four
    assert all(k.get("vgpr_count", 0) <= 128 and k.get("group_segment_fixed_size", 0) <= 40 * 1024 for k in ks["mphsir::spectral_loss_kernel"])


_CTYPE_OF = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mphsir.h")).read(), flags=re.S)


def _header_struct(name):
    m = re.search(r"struct %s \{(.*?)\};\s*typedef struct %s %s;" % (name, name, name), _header_text(), flags=re.S)
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


def test_the_args_struct_matches_its_ctypes_image():
    import mp_hsir_amd._lib as L
    want = _header_struct("mphsir_spectral_loss_args")
    got = list(L.SpectralLossArgs._fields_)
    assert [n for n, _ in got] == [n for n, _ in want], (got, want)
    for (n, tg), (_, tw) in zip(got, want):
        assert ctypes.sizeof(tg) == ctypes.sizeof(tw) and (tg is ctypes.c_float) == (tw is ctypes.c_float), (n, tg, tw)
    assert want[0] == ("struct_size", ctypes.c_uint32) and L.SpectralLossArgs().struct_size == ctypes.sizeof(L.SpectralLossArgs)
    assert [n for n, _ in want][1:] == ["y", "clean", "grad", "out", "workspace", "workspace_bytes", "B", "C", "H", "W", "w_sam", "w_sdiff"]
    assert {"mphsir_spectral_loss", "mphsir_spectral_loss_workspace_bytes"} <= set(L.symbols())
    assert "mphsir_spectral_loss_args" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_header_constants():
    import spectral_loss_ref as R
    text = _header_text()
    m = re.search(r"#define MPHSIR_SAM_MIN_SIN (\S+)", text)
    assert m and float(m.group(1)) == R.MIN_SIN
    ids = dict(re.findall(r"#define (MPHSIR_K_\w+) (\d+)", text))
    assert ids["MPHSIR_K_SPECTRAL_LOSS"] == "39" and ids["MPHSIR_K_SPECTRAL_LOSS_FINISH"] == "40" and ids["MPHSIR_K_COUNT"] == "41"
    assert ids["MPHSIR_K_L1_LOSS"] == "28", "the default loss keeps its id"
