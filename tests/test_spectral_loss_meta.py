"""The spectral-loss kernels (mp-hsir_amd/csrc/spectral_loss.hip) in the built code object (CPU test): the names tools and profiles match on,
no register spills, no scratch, workgroups of 256 -- and the args struct of include/mphsir.h against its ctypes image, with the float-aware
parser of tests/meta.py (the struct has float members and is declared as `struct ...; typedef ...;`)."""
import ctypes
import os
import re

import meta


def test_kernels_exist_and_do_not_spill():
    ks = meta.kernels_by_name("spectral_loss")
    assert sorted(ks) == ["mphsir::spectral_loss_finish_kernel", "mphsir::spectral_loss_kernel"], sorted(ks)
    assert len(ks["mphsir::spectral_loss_kernel"]) == 2           # the 16-byte path and the scalar path
    for group in ks.values():
        for k in group:
            assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
            assert k["max_flat_workgroup_size"] == 256
    # two workgroups per CU at the training shape: 24.6 KB of LDS and at most 128 registers per lane leave room for four
    assert all(k.get("vgpr_count", 0) <= 128 and k.get("group_segment_fixed_size", 0) <= 40 * 1024 for k in ks["mphsir::spectral_loss_kernel"])


def test_the_args_struct_matches_its_ctypes_image():
    import mp_hsir_amd._lib as L
    want = meta.header_struct("mphsir_spectral_loss_args")
    got = list(L.SpectralLossArgs._fields_)
    assert [n for n, _ in got] == [n for n, _ in want], (got, want)
    for (n, tg), (_, tw) in zip(got, want):
        assert ctypes.sizeof(tg) == ctypes.sizeof(tw) and (tg is ctypes.c_float) == (tw is ctypes.c_float), (n, tg, tw)
    assert want[0] == ("struct_size", ctypes.c_uint32) and L.SpectralLossArgs().struct_size == ctypes.sizeof(L.SpectralLossArgs)
    assert [n for n, _ in want][1:] == ["y", "clean", "grad", "out", "workspace", "workspace_bytes", "B", "C", "H", "W", "w_sam", "w_sdiff"]
    assert {"mphsir_spectral_loss", "mphsir_spectral_loss_workspace_bytes"} <= set(L.symbols())
    assert "mphsir_spectral_loss_args" in open(os.path.join(meta.ROOT, "INTEGRATION.md")).read()


def test_header_constants():
    import spectral_loss_ref as R
    text = meta.header_text()
    m = re.search(r"#define MPHSIR_SAM_MIN_SIN (\S+)", text)
    assert m and float(m.group(1)) == R.MIN_SIN
    ids = dict(re.findall(r"#define (MPHSIR_K_\w+) (\d+)", text))
    assert ids["MPHSIR_K_SPECTRAL_LOSS"] == "39" and ids["MPHSIR_K_SPECTRAL_LOSS_FINISH"] == "40" and ids["MPHSIR_K_COUNT"] == "41"
    assert ids["MPHSIR_K_L1_LOSS"] == "28", "the default loss keeps its id"
