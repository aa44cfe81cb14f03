"""The tiled degradation kernel (mp-hsir_amd/csrc/degrade.hip, degrade_planes_kernel) in the built code object: its four instances are
present, spill nothing, use no scratch and no static LDS, and keep the register count of the occupancy the file's header claims (CPU
test, as tests/test_degrade_fused_meta.py)."""
import meta


def planes_lds_bytes(hmax, factors, blur):
    """the host's formula (degrade_planes_lds_floats): the 64 x 64 tile with the largest halo and an odd pitch, 4 floats of slack, then the
    low-resolution pixels under the tile (64 / f a side when f divides 64, else 63 / f + 2) or the 21 x 21 weights"""
    P = 64 + 2 * hmax
    low = max([64 // f if 64 % f == 0 else 63 // f + 2 for f in factors] + [0]) ** 2
    if blur:
        low = max(low, 21 * 21)
    return (P * (P | 1) + 4 + low) * 4


def test_planes_kernel_instances_do_not_spill_and_keep_five_workgroups_per_cu():
    ks = [k for k in meta.object_kernels("degrade") if "degrade_planes_kernel" in k["name"]]
    assert len(ks) == 4, "generated / explicit draws x dwordx4 / scalar access: %s" % [k["name"] for k in ks]
    for k in ks:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("group_segment_fixed_size", 0) == 0, "the tile is dynamic LDS, sized per launch by the host: no static LDS beside it"
        assert k.get("vgpr_count", 0) <= 96, "%d registers: five waves per SIMD (one per resident workgroup) need <= 512 / 5 -> 96" % k.get("vgpr_count", 0)
    # both default training menus: the 21 x 21 halo and sr f = 2 -- the plane form's budget at N = 64, five workgroups = 20 waves per CU
    lds = planes_lds_bytes(10, [2, 4, 8], True)
    assert 5 * lds <= 160 * 1024 < 6 * lds, "%d bytes of LDS per workgroup" % lds
    # a scene under a mode without a stencil: LDS would let nine workgroups in, the eight waves per SIMD let eight
    assert 9 * planes_lds_bytes(0, [], False) <= 160 * 1024 and 8 * planes_lds_bytes(0, [8], False) <= 160 * 1024
    for k in ks:
        assert k.get("vgpr_count", 0) <= 64, "%d registers: eight waves per SIMD need <= 64" % k.get("vgpr_count", 0)
