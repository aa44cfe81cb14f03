"""The clip / EMA kernels (mp-hsir_amd/csrc/optim.hip) in the built code object (CPU test): the names tools and profiles match on, no
register spills, no scratch, the earlier optimizer kernels still there.  (The two args structs are pinned by tests/test_cabi.py.)"""
import meta


def test_new_kernels_exist_and_do_not_spill():
    ks = meta.kernels_by_name("optim")
    assert sorted(ks) == ["mphsir::flat_adamw_ex_kernel", "mphsir::flat_adamw_kernel", "mphsir::grad_check_kernel", "mphsir::grad_norm_finish_kernel",
                          "mphsir::grad_sqnorm_kernel", "mphsir::scaler_update_kernel"], sorted(ks)
    assert len(ks["mphsir::flat_adamw_ex_kernel"]) == 2          # with and without the EMA arena
    for name in ("flat_adamw_ex_kernel", "grad_sqnorm_kernel", "grad_norm_finish_kernel"):
        for k in ks["mphsir::" + name]:
            assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
            assert k["max_flat_workgroup_size"] == 256
    # streaming kernels: full occupancy needs at most 64 registers per lane at 8 waves per SIMD
    assert all(k.get("vgpr_count", 0) <= 64 for k in ks["mphsir::flat_adamw_ex_kernel"] + ks["mphsir::grad_sqnorm_kernel"])

