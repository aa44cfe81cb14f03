"""The two scene-quality kernels (mp-hsir_amd/csrc/quality.hip) in the built code objects (CPU test): stable names, no register spills, no
scratch, and registers / LDS within the occupancy the kernel was laid out for.

Planned occupancy of quality_partials_kernel: TWO workgroups of 256 threads per CU, i.e. 2 waves per SIMD.  The 160 KiB of LDS of a
gfx950 CU then allow 80 KiB per workgroup (the kernel holds a double-buffered fp32 stage of both cubes and five planes of fp64 row
sums: about 70 KiB), and 2 waves per SIMD allow 256 VGPRs per lane.  The second workgroup is what runs while the first waits at one of
its two barriers per band.  quality_finish_kernel is one wave per workgroup without LDS."""
import meta

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 2


def test_quality_kernels_fit_the_planned_occupancy_and_do_not_spill():
    ks = {k["demangled"].split("(")[0]: k for k in meta.object_kernels("quality")}
    assert sorted(ks) == ["mphsir::quality_finish_kernel", "mphsir::quality_partials_kernel"], sorted(ks)
    for k in ks.values():
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
    part, fin = ks["mphsir::quality_partials_kernel"], ks["mphsir::quality_finish_kernel"]
    assert part["max_flat_workgroup_size"] == 256 and fin["max_flat_workgroup_size"] == 64
    assert 0 < part["group_segment_fixed_size"] <= LDS_PER_CU // WORKGROUPS_PER_CU, part
    assert part.get("vgpr_count", 0) + part.get("agpr_count", 0) <= 512 // WORKGROUPS_PER_CU, part     # 512 registers per lane and SIMD, one wave of each workgroup per SIMD
    assert fin.get("group_segment_fixed_size", 0) == 0 and fin.get("vgpr_count", 0) <= 64
