"""The clip / EMA kernels (mp-hsir_amd/csrc/optim.hip) in the built code object (CPU test): the names tools and profiles match on, no
register spills, no scratch, the earlier optimizer kernels still there -- and the two args structs of include/mphsir.h against their
ctypes images.  (tests/test_cabi.py compares every `typedef struct mphsir_* {` of the header with its mirror, but its parser knows
integer and pointer members only; these two structs are the first with float members, are declared as `struct ...; typedef ...;`,
and are compared here with the parser of tests/meta.py, which knows float.)"""
import ctypes
import os

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


def test_the_two_args_structs_match_their_ctypes_images():
    import mp_hsir_amd._lib as L
    for name, cls in (("mphsir_grad_norm_args", L.GradNormArgs), ("mphsir_flat_adamw_ex_args", L.FlatAdamwExArgs)):
        want = meta.header_struct(name)
        got = list(cls._fields_)
        assert [n for n, _ in got] == [n for n, _ in want], (name, got, want)
        for (n, tg), (_, tw) in zip(got, want):
            assert ctypes.sizeof(tg) == ctypes.sizeof(tw) and (tg is ctypes.c_float) == (tw is ctypes.c_float), (name, n, tg, tw)
        assert want[0] == ("struct_size", ctypes.c_uint32) and cls().struct_size == ctypes.sizeof(cls)
    assert {"mphsir_grad_norm", "mphsir_grad_norm_workspace_bytes", "mphsir_flat_adamw_ex"} <= set(L.symbols())
    md = open(os.path.join(meta.ROOT, "INTEGRATION.md")).read()
    assert "mphsir_grad_norm_args" in md and "mphsir_flat_adamw_ex_args" in md
