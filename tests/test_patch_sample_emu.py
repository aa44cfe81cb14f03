"""mphsir_patch_sample, scene_store.SceneStore and data.SceneStoreSource on the CPU: the two kernels of mp-hsir_amd/csrc/patch_sample.hip
through the emulated build against the numpy restatement of tests/patch_sample_ref.py.  Small shapes only: the fibers are slow.  The 64-bit
offsets are covered here by type (the level table is int64 on both sides, patch_sample_ref.Tables asserts it, ops.patch_sample refuses
anything else); the value range past 2^31 is the GPU test's."""
import pytest
import torch

import patch_sample_ref as R
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("C", [1, 3, 5])
def test_matches_numpy_over_two_pyramids(C):
    R.check_shapes("cpu", C)


def test_aligned_and_elementwise_rows():
    R.check_alignment("cpu")


def test_extremes_in_different_bands_first_and_last_element():
    R.check_extremes("cpu")


def test_nan_constant_and_infinite_windows():
    R.check_nan_and_inf("cpu")


def test_two_calls_are_bitwise_equal():
    R.check_reproducible("cpu")


def test_refusals_launch_nothing():
    R.check_refusals("cpu")


def test_device_side_values_are_clamped_into_the_tables():
    R.check_device_values_are_clamped("cpu")


def test_level_table_must_be_int64():
    from mp_hsir_amd import ops
    t = R.Tables([torch.rand(1, 8, 8).numpy()], "cpu")
    rec = torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(AssertionError, match="int64"):
        ops.patch_sample(t.arena, t.levels.to(torch.int32), t.levels_host, rec, None, 1, 8)
    with pytest.raises(AssertionError, match="int64"):
        ops.patch_sample(t.arena, t.levels, t.levels_host, rec, torch.zeros(1, dtype=torch.int32), 1, 8)


def test_store_records_against_numpy():
    R.check_store_against_numpy("cpu")


def test_source_equals_patch_db_source(tmp_path):
    R.check_source_equals_patch_db_source("cpu", tmp_path)


def test_jittered_windows_stay_inside_and_off_the_mask():
    R.check_jitter("cpu")
