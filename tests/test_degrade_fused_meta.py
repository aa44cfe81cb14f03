"""The fused degradation kernel (mp-hsir_amd/csrc/degrade.hip) in the built code object: present, no register spills, no scratch, and the
register count the occupancy it is laid out for needs (CPU test, as tests/test_ensemble_meta.py)."""
import meta


def test_degrade_kernel_does_not_spill_and_keeps_five_workgroups_per_cu():
    ks = [k for k in meta.object_kernels("degrade") if "degrade_batch_kernel" in k["name"]]
    assert len(ks) == 2, "two instances, generated and explicit draws: %s" % [k["name"] for k in ks]
    for k in ks:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
    # the training shape: N = 64 with the 21 x 21 halo and the 32 x 32 image of sr f = 2, as the host sizes the dynamic LDS
    lds = ((64 + 20) * ((64 + 20) | 1) + 4 + 32 * 32) * 4
    assert 5 * lds <= 160 * 1024 < 6 * lds, "%d bytes of LDS per workgroup: five workgroups = 20 waves per CU is the layout's occupancy" % lds
    for k in ks:
        assert k.get("group_segment_fixed_size", 0) == 0, "the plane is dynamic LDS, sized per launch by the host: no static LDS beside it, got %d" % \
            k.get("group_segment_fixed_size", 0)
        assert k.get("vgpr_count", 0) <= 96, "%d registers: five waves per SIMD (one per resident workgroup) need <= 512 / 5 -> 96" % k.get("vgpr_count", 0)
