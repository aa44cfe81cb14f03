"""The spectral-loss kernels (mp-hsir_amd/csrc/spectral_loss.hip) in the built code object (CPU test): the names tools and profiles match on,
no register spills, no scratch, workgroups of 256 -- and the constants of include/mphsir.h that belong to them, as mp_hsir_amd._lib
reads them.  (The args struct is pinned by tests/test_cabi.py.)"""
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


def test_header_constants():
    import mp_hsir_amd._lib as L
    import spectral_loss_ref as R
    ids = L.CONSTANTS
    assert ids["MPHSIR_SAM_MIN_SIN"] == R.MIN_SIN
    assert ids["MPHSIR_K_SPECTRAL_LOSS"] == 39 and ids["MPHSIR_K_SPECTRAL_LOSS_FINISH"] == 40 and ids["MPHSIR_K_COUNT"] == 41
    assert ids["MPHSIR_K_L1_LOSS"] == 28, "the default loss keeps its id"
