"""The two patch-sampling kernels (mp-hsir_amd/csrc/patch_sample.hip) in the built code object (CPU test): stable names, no register spills,
no scratch, and the register / LDS figures DESIGN.md's occupancy reasoning relies on: at most 32 VGPRs and 48 bytes of LDS per workgroup
of 256 threads, so neither limits residency -- a CU holds its maximum of 8 such workgroups (32 waves, 8 per SIMD)."""
import meta


def test_patch_sample_kernels_do_not_spill_and_fit_full_occupancy():
    ks = {k["demangled"].split("(")[0]: k for k in meta.object_kernels("patch_sample")}
    assert sorted(ks) == ["mphsir::patch_minmax_kernel", "mphsir::patch_normalise_kernel"], sorted(ks)
    for k in ks.values():
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k["max_flat_workgroup_size"] == 256
        assert k.get("group_segment_fixed_size", 0) == 48, "4 waves x {min, max, NaN flag}: %s" % k.get("group_segment_fixed_size")
        assert k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 32, "%d registers: 8 waves per SIMD need <= 512 / 8 = 64, DESIGN.md states <= 32" % k.get("vgpr_count", 0)
