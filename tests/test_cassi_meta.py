"""The two CASSI kernels (mp-hsir_amd/csrc/cassi.hip) in the built code object (CPU test): stable names, no register spills, no scratch,
and the register / LDS figures DESIGN.md section 5 states: at most 32 (measure) and 48 (emit) VGPRs and 48 bytes of LDS per workgroup of
256 threads, so neither limits residency -- a CU holds its maximum of 8 such workgroups (32 waves, 8 per SIMD, which needs <= 64 VGPRs)."""
import meta


def test_cassi_kernels_do_not_spill_and_fit_full_occupancy():
    ks = {k["demangled"].split("(")[0]: k for k in meta.object_kernels("cassi")}
    assert sorted(ks) == ["mphsir::cassi_emit_kernel", "mphsir::cassi_measure_kernel"], sorted(ks)
    for name, k in ks.items():
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k["max_flat_workgroup_size"] == 256
        assert k.get("group_segment_fixed_size", 0) == 48, "4 waves x {min, max, NaN flag}: %s" % k.get("group_segment_fixed_size")
        regs = k.get("vgpr_count", 0) + k.get("agpr_count", 0)
        limit = 32 if name.endswith("measure_kernel") else 48
        assert regs <= limit, "%s: %d registers, DESIGN.md states <= %d (8 waves per SIMD need <= 512 / 8 = 64)" % (name, regs, limit)
