"""Spectral windows, what needs neither a GPU nor the emulator: the band plan, the C ABI of include/mphsir_bands.h, the code objects of
the two kernels, test.py's flag."""
import ctypes
import os
import re

import pytest
import torch

import scene_bands_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_plan_equals_the_restatement_and_has_its_properties():
    """C in {4, 5, 8, 12, 31, 100}, every legal ovb, Cs up to 4C + 2: first window at 0, last ending at Cs, strictly ascending origins,
    neighbours sharing at least ovb bands, at most 3 windows over any band -- reached at (Cs, C, ovb) = (12, 5, 2)"""
    from mp_hsir_amd.scene import plan_bands
    worst = 0
    for C in B.PLAN_C:
        for ovb in range(C // 2 + 1):
            for Cs in range(1, 4 * C + 3):
                ob = plan_bands(Cs, C, ovb)
                assert ob == B.plan_bands(Cs, C, ovb), (Cs, C, ovb)
                assert ob[0] == 0 and all(b > a for a, b in zip(ob, ob[1:]))
                if Cs <= C:
                    assert ob == [0]
                    continue
                assert ob[-1] + C == Cs
                assert all(a + C - b >= ovb for a, b in zip(ob, ob[1:])), (Cs, C, ovb, ob)
                cover = max(sum(o <= c < o + C for o in ob) for c in range(Cs))
                assert cover <= 3, (Cs, C, ovb, ob)
                worst = max(worst, cover)
    assert worst == 3 and plan_bands(12, 5, 2) == [0, 2, 4, 7]
    assert plan_bands(210, 100, 25) == [0, 55, 110] and plan_bands(45, 31, 8) == [0, 14] and len(plan_bands(191, 31, 8)) == 8
    for C, bad in ((5, 3), (5, -1), (31, 16), (4, 3)):
        with pytest.raises(ValueError):
            plan_bands(2 * C, C, bad)
        with pytest.raises(ValueError):
            B.plan_bands(2 * C, C, bad)


def _real_library():
    import mp_hsir_amd._lib as L
    saved = (L._lib, L._is_emu)
    L._lib, L._is_emu = None, False
    return L, L.load(), saved


def test_header_binding_exports_and_integration_md_agree():
    """include/mphsir_bands.h <-> the ctypes tables <-> the library's exports <-> the C text INTEGRATION.md shows; the surfaces of
    include/mphsir.h and include/mphsir_accum.h are what they were"""
    L, lib, saved = _real_library()
    try:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mphsir_bands.h")).read(), flags=re.S)
        assert sorted(set(re.findall(r"\b(mphsir_\w+)\s*\(", text))) == L.bands_symbols() == ["mphsir_scene_blend_bands", "mphsir_scene_gather_bands"]
        assert list(L.BANDS_STRUCTS) == ["mphsir_scene_gather_bands_args", "mphsir_scene_blend_bands_args"]
        assert L.BANDS_STRUCTS["mphsir_scene_gather_bands_args"] is L.SceneGatherBandsArgs and L.BANDS_STRUCTS["mphsir_scene_blend_bands_args"] is L.SceneBlendBandsArgs
        assert len(L.symbols()) == 92 and L.added_symbols() == ["mphsir_multi_accum"] and list(L.ADDED_STRUCTS) == ["mphsir_multi_accum_args"]
        assert not set(L.bands_symbols()) & set(L.symbols()) and not set(L.BANDS_STRUCTS) & (set(L.STRUCTS) | set(L.ADDED_STRUCTS))
        i32, ptr = ctypes.c_int32, ctypes.c_void_p
        want = {
            L.SceneGatherBandsArgs: [("struct_size", ctypes.c_uint32), ("scene", ptr), ("origins", ptr), ("tiles", ptr)] + [
                (n, i32) for n in ("j0", "count", "n_tiles", "G", "modes_packed", "C", "Cs", "H", "W", "th", "tw")],
            L.SceneBlendBandsArgs: [("struct_size", ctypes.c_uint32), ("tiles", ptr), ("ob", ptr), ("oy", ptr), ("ox", ptr), ("scene", ptr)] + [
                (n, i32) for n in ("nb", "ny", "nx", "C", "Cs", "H", "W", "th", "tw", "ov", "ovb", "clamp01")]}
        md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert "include/mphsir_bands.h" in md
        for cls, fields in want.items():
            assert cls._fields_ == fields and issubclass(cls, L._Args) and cls().struct_size == ctypes.sizeof(cls)
            cname = [k for k, v in L.BANDS_STRUCTS.items() if v is cls][0]
            fn = getattr(lib, cname[:-len("_args")])          # AttributeError: the library does not export it
            assert fn.argtypes == [ctypes.POINTER(cls), ctypes.c_void_p] and fn.restype is ctypes.c_int
            m = re.search(r"struct %s \{(.*?)\};" % cname, md, flags=re.S)
            assert m, "INTEGRATION.md shows struct %s" % cname
            body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
            shown = []
            for d in filter(str.strip, body.split(";")):
                names = re.split(r"\s*,\s*", d.strip())
                shown += [re.split(r"[\s*]+", names[0])[-1]] + names[1:]
            assert shown == [n for n, _ in fields], shown
            assert "int %s(const %s* a, void* stream);" % (cname[:-len("_args")], cname) in md
        assert ctypes.sizeof(L.SceneGatherBandsArgs) == 80 and ctypes.sizeof(L.SceneBlendBandsArgs) == 96
        assert "MPHSIR_K_SCENE_BANDS" not in L.CONSTANTS and L.CONSTANTS["MPHSIR_K_COUNT"] == 41, "both launch under MPHSIR_K_SCENE"
    finally:
        L._lib, L._is_emu = saved


def test_a_struct_of_another_size_and_cpu_tensors_are_refused():
    from mp_hsir_amd import ops
    L, lib, saved = _real_library()
    try:
        for cls, fn in ((L.SceneGatherBandsArgs, lib.mphsir_scene_gather_bands), (L.SceneBlendBandsArgs, lib.mphsir_scene_blend_bands)):
            a = cls()
            a.struct_size += 4
            assert fn(ctypes.byref(a), None) == L.CONSTANTS["MPHSIR_EINVAL"]
            assert b"struct_size" in lib.mphsir_last_error()
            assert fn(ctypes.byref(cls()), None) == L.CONSTANTS["MPHSIR_EINVAL"] and b"null pointer" in lib.mphsir_last_error()
        z = torch.zeros(1, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="GPU only"):
            ops.scene_gather_bands(torch.zeros(7, 32, 32), torch.zeros(1, 3, dtype=torch.int32), 5, 32, 32, 0, (0,), torch.empty(1, 5, 32, 32))
        with pytest.raises(RuntimeError, match="GPU only"):
            ops.scene_blend_bands(torch.zeros(1, 5, 32, 32), z, z, z, 0, 0, 7, 32, 32)
    finally:
        L._lib, L._is_emu = saved


def test_code_objects_of_the_two_kernels():
    """no spills, no scratch, the siblings' budget of 64 registers (8 waves per SIMD: what their measured bandwidth rests on), the gather's
    LDS within the 20 KiB that leave 8 workgroups per CU; the new source file has no LDS (tests/test_emu_schedules.py keeps a table of
    the files that have)"""
    import meta
    gather = [k for k in meta.object_kernels("scene_d4") if "bands_gather_kernel" in k["name"]]
    blend = [k for k in meta.object_kernels("scene_bands") if "bands_blend_kernel" in k["name"]]
    assert len(gather) == 1 and len(blend) == 1, (gather, blend)
    assert len(meta.object_kernels("scene_bands")) == 1 and len(meta.object_kernels("scene_d4")) == 3
    for k in gather + blend:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_count", 0) <= 64, "%s: %d registers leave fewer than 8 waves per SIMD" % (k["name"], k.get("vgpr_count", 0))
        assert k["max_flat_workgroup_size"] == 256
    assert 0 < gather[0].get("group_segment_fixed_size", 0) <= 20 * 1024
    assert blend[0].get("group_segment_fixed_size", 0) == 0


def test_test_py_flag_and_refusals():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mphsir_test_py", os.path.join(ROOT, "mp-hsir_amd", "test.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    p = T.build_parser()
    assert p.parse_args([]).band_overlap == -1 and p.parse_args(["--band_overlap", "8"]).band_overlap == 8
    assert "not a tuned value" in " ".join(p.format_help().split())
    o = p.parse_args(["--mode", "13"])
    with pytest.raises(SystemExit, match="mode 13"):
        T.check_other_band_count(o, "urban", 210, 100)
    with pytest.raises(SystemExit, match="mode 9"):
        T.check_other_band_count(p.parse_args(["--mode", "9"]), "urban", 210, 100)
    T.check_other_band_count(p.parse_args(["--mode", "9"]), "pavia", 45, 31)
    T.check_other_band_count(p.parse_args(["--mode", "0"]), "urban", 210, 100)
