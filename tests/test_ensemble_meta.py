"""The two self-ensemble kernels (mp-hsir_amd/csrc/scene_d4.hip) in the built code objects: no register spills, no scratch, and the
register budget the two scene kernels are held to (CPU test, as tests/test_scene_meta.py)."""
import meta


def test_d4_kernels_do_not_spill():
    ks = [k for k in meta.object_kernels("scene_d4") if "d4_gather_kernel" in k["name"] or "d4_fold_kernel" in k["name"]]
    assert sorted("gather" in k["name"] for k in ks) == [False, True], [k["name"] for k in ks]
    for k in ks:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_count", 0) <= 64, "%s: %d registers leave fewer than 8 waves per SIMD" % (k["name"], k.get("vgpr_count", 0))
        assert k.get("group_segment_fixed_size", 0) <= 20 * 1024, "%s: %d bytes of LDS leave fewer than 8 workgroups per CU" % (
            k["name"], k.get("group_segment_fixed_size", 0))
