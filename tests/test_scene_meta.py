"""The two whole-scene kernels (mp-hsir_amd/csrc/scene.hip) in the built code objects: no register spills, no scratch (CPU test).
tests/test_kernel_meta.py guards the kernels of the training step by name; these two are fp32, not templated, and outside its patterns."""
import meta


def test_scene_kernels_do_not_spill():
    ks = [k for k in meta.object_kernels("scene") if "scene_gather_kernel" in k["name"] or "scene_blend_kernel" in k["name"]]
    assert sorted("gather" in k["name"] for k in ks) == [False, True], [k["name"] for k in ks]
    for k in ks:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("vgpr_count", 0) <= 64, "%s: %d registers leave fewer than 8 waves per SIMD" % (k["name"], k.get("vgpr_count", 0))
