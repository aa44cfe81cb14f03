"""The fused degradation launch (mp-hsir_amd/csrc/degrade.hip) on the CPU emulator: the Philox restatement against known answers, the
kernel's generated draws against it, every kind against the reference fixtures with explicit draws, one mixed batch against the tensor
functions of mp-hsir_amd/degrade.py, the smallest planes, the properties of generated mode, the refusals, and
DegradationSynthesizer(fused=True).  The checks live in tests/degrade_fused_ref.py; tests/test_degrade_fused_gpu.py runs them on the GPU."""
import numpy as np
import pytest

import degrade_fused_ref as R
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


def test_philox_known_answers():
    """Random123's known answers for Philox4x32-10 (counter words, then key words)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in R.philox4x32_10(*ctr, *key)) == want
    # vectorised over the counter as `draws` uses it
    got = R.philox4x32_10(np.array([0, 0x243f6a88], np.uint64), np.array([0, 0x85a308d3], np.uint64), np.array([0, 0x13198a2e], np.uint64),
                          np.array([0, 0x03707344], np.uint64), np.array([0, 0xa4093822], np.uint64), np.array([0, 0x299f31d0], np.uint64))
    assert [int(v[1]) for v in got] == list(kat[2][2]) and [int(v[0]) for v in got] == list(kat[0][2])
    R.check_kernel_philox_known_answer("cpu")


def test_generated_uniforms_are_bitwise_the_helpers():
    R.check_generated_uniforms("cpu")
    R.check_generated_uniforms("cpu", seed=3, ordinal=(1 << 32) + 7)          # the low word of the ordinal is the counter word


def test_generated_normal_against_the_float64_helper_and_its_moments():
    R.check_generated_normal("cpu")


@pytest.mark.parametrize("name", ["gauss", "noniid", "stripe", "deadline", "impulse", "mask", "bandloss", "gblur7", "gblur9", "gblur15", "cblur9",
                                  "sblur5", "sr2", "sr4", "sr8"])
def test_reference_fixtures_with_explicit_draws_all_modes(name):
    assert name in R.fixture_cases()[1]
    R.check_fixtures("cpu", names=[name])


def test_fused_equals_the_tensor_path_on_one_mixed_batch():
    R.check_mixed_batch("cpu")


def test_smallest_planes():
    R.check_small_planes("cpu")


def test_blur_21_at_64_against_the_float64_oracle():
    R.check_blur21_at_64("cpu")


def test_largest_plane():
    R.check_largest_plane("cpu")


def test_generated_mode_is_a_function_of_seed_ordinal_and_element():
    R.check_generated_properties("cpu")


def test_a_nan_poisons_exactly_its_dependents():
    R.check_nan_poisons_its_dependents("cpu")


def test_refusals():
    R.check_refusals("cpu")


def test_synthesizer_fused():
    R.check_synthesizer_fused("cpu")


def test_sources_and_flag_pass_fused_degrade_through(tmp_path):
    from mp_hsir_amd.data import PatchDB, PatchDBSource, SyntheticPatchSource, write_patch_db
    from mp_hsir_amd.options import build_parser
    assert build_parser().parse_args([]).fused_degrade == 0 and build_parser().parse_args(["--fused_degrade", "1"]).fused_degrade == 1
    types = ["gaussianN", "inpaint", "bandmiss"]
    s = SyntheticPatchSource(5, 16, 4, 6, "cpu", 2024, 0, de_types=types, fused_degrade=True)
    assert s.syn.fused
    _, deg, cl, prompt = s.next()
    assert deg.shape == cl.shape == (4, 5, 16, 16) and prompt.shape == (4, 1) and int(prompt.max()) < 3
    assert not SyntheticPatchSource(5, 16, 4, 6, "cpu", 2024, 0, de_types=types).syn.fused
    rs = np.random.RandomState(0)
    write_patch_db(str(tmp_path / "db"), [rs.rand(31, 16, 16).astype(np.float32) for _ in range(8)], ["ICVL_%d.mat" % i for i in range(8)])
    db = PatchDB(str(tmp_path / "db"), dataset_names=None)
    src = PatchDBSource(db, 4, types, "natural_scene", "cpu", seed=5, fused_degrade=True)
    assert src.syn.fused and not PatchDBSource(db, 4, types, "natural_scene", "cpu", seed=5).syn.fused
    _, deg, cl, prompt = src.next()
    assert deg.shape == cl.shape == (4, 31, 16, 16) and prompt.shape == (4, 1) and bool(np.isfinite(deg.numpy()).all())
