"""Gradient accumulation on the CPU: multi_accum_kernel through the emulated build, the engine's accumulate path, eager, on the
two-convolution network of tests/optim_ex_ref.py (a step of the tiny MP-HSIR net takes 75 s through the emulator: that network runs these
checks on the GPU, tests/test_accum_gpu.py), and accumulation against two gloo ranks on the toy net of tests/test_host_logic.py."""
import pytest

import accum_ref as A
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


def test_kernel_stores_then_adds_host_and_device_index():
    A.check_kernel_forms("cpu")


def test_copy_form_is_the_old_launch():
    A.check_copy_form_is_the_old_launch("cpu")


def test_refusals_launch_nothing():
    A.check_refusals("cpu")


def test_engine_off_is_off():
    A.check_off_is_off("cpu", "conv")


def test_engine_arena_holds_the_sum():
    A.check_arena_holds_the_sum("cpu", "conv")


def test_engine_the_step():
    A.check_the_step("cpu", "conv")


@pytest.mark.parametrize("scaler", [True, False])
def test_engine_a_non_finite_micro_batch_skips_the_group(scaler):
    A.check_nonfinite_micro_batch("cpu", "conv", scaler)


@pytest.mark.timeout(600)
def test_accumulation_is_data_parallelism_gloo(tmp_path):
    A.check_emu_accumulation_is_data_parallelism(tmp_path)
