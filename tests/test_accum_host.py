"""Gradient accumulation, what needs neither a GPU nor the emulator: the flag, its help text, the refusals by name, the kernel id."""
import pytest
import torch


def test_flag_default_and_help():
    from mp_hsir_amd import options
    p = options.build_parser()
    assert p.parse_args([]).accum_steps == 1 and options.options.accum_steps == 1
    assert p.parse_args(["--accum_steps", "4"]).accum_steps == 4
    text = " ".join(p.format_help().split()).replace("- ", "-")      # argparse wraps at hyphens: "micro- batches"
    assert "--accum_steps" in text
    for phrase in ("K micro-batches equal K data-parallel ranks, not one batch of K * batch_size", "TVSP couples the samples of a batch",
                   "the learning rate is the user's to scale, as with more GPUs"):
        assert phrase in text, phrase


@pytest.mark.parametrize("bad", [0, -1, -8, 2.0, True, None])
def test_engine_refuses_bad_values_by_name(bad):
    from mp_hsir_amd.engine import DataParallelEngine
    with pytest.raises(ValueError, match="accum_steps"):
        DataParallelEngine(torch.nn.Linear(2, 2), lr=1e-3, accum_steps=bad)


def test_engine_default_is_off():
    from mp_hsir_amd.engine import DataParallelEngine
    eng = DataParallelEngine(torch.nn.Linear(2, 2), lr=1e-3)
    assert eng.accum_steps == 1 and eng.group_loss is None and not eng._eager_hyper
    assert DataParallelEngine(torch.nn.Linear(2, 2), lr=1e-3, accum_steps=3)._eager_hyper


def test_kernel_exists_and_does_not_spill():
    import meta
    ks = meta.kernels_by_name("arena")
    assert "mphsir::multi_accum_kernel" in ks and len(ks["mphsir::multi_accum_kernel"]) == 1, sorted(ks)
    for k in ks["mphsir::multi_accum_kernel"]:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k["max_flat_workgroup_size"] == 256 and k.get("group_segment_fixed_size", 0) == 0


def test_header_binding_and_integration_md_agree():
    """include/mphsir_accum.h <-> the ctypes binding <-> the struct INTEGRATION.md shows <-> the library's export; the surface of
    include/mphsir.h itself is what it was (tests/test_cabi.py pins its counts)"""
    import ctypes
    import os
    import re
    import mp_hsir_amd._lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mphsir_accum.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mphsir_\w+)\s*\(", text))) == L.added_symbols() == ["mphsir_multi_accum"]
    assert list(L.ADDED_STRUCTS) == ["mphsir_multi_accum_args"] and L.ADDED_STRUCTS["mphsir_multi_accum_args"] is L.MultiAccumArgs
    assert "mphsir_multi_accum" not in L.symbols() and "mphsir_multi_accum_args" not in L.STRUCTS
    fields = L.MultiAccumArgs._fields_
    assert fields == [("struct_size", ctypes.c_uint32), ("table_dev", ctypes.c_void_p), ("nseg", ctypes.c_int32), ("total_blocks", ctypes.c_int64),
                      ("micro", ctypes.c_int32), ("micro_dev", ctypes.c_void_p)]
    assert issubclass(L.MultiAccumArgs, L._Args) and L.MultiAccumArgs().struct_size == ctypes.sizeof(L.MultiAccumArgs) == 48
    lib = L.load()
    assert lib.mphsir_multi_accum.argtypes == [ctypes.POINTER(L.MultiAccumArgs), ctypes.c_void_p] and lib.mphsir_multi_accum.restype is ctypes.c_int
    assert "MPHSIR_K_MULTI_ACCUM" not in L.CONSTANTS and L.CONSTANTS["MPHSIR_K_MULTI_COPY"] == 27, "the launch runs under the hand-over's id"
    md = open(os.path.join(root, "INTEGRATION.md")).read()
    m = re.search(r"struct mphsir_multi_accum_args \{(.*?)\};", md, flags=re.S)
    assert m, "INTEGRATION.md shows the struct"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    shown = [re.split(r"[\s*]+", d.strip())[-1] for d in body.split(";") if d.strip()]
    assert shown == [n for n, _ in fields], shown
    assert "int mphsir_multi_accum(const mphsir_multi_accum_args* a, void* stream);" in md and "include/mphsir_accum.h" in md
