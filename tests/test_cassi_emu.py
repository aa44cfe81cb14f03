"""mphsir_cassi, the cassi branches of the synthesiser, of the synthetic source and of test.py on the CPU: the two kernels of
mp-hsir_amd/csrc/cassi.hip through the emulated build against the numpy restatement, the tensor form and the reference's own outputs
(tests/cassi_ref.py).  The same checks run on the GPU in tests/test_cassi_gpu.py."""
import pytest

import cassi_ref as R
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("step", [1, 2, 3])
def test_square_batch_under_every_mode(step):
    R.check_square_all_modes("cpu", step)


def test_non_square_planes_without_augmentation():
    R.check_non_square("cpu")


def test_element_wise_path_for_odd_widths():
    R.check_scalar_path("cpu")


def test_equals_the_reference_function():
    R.check_golden("cpu")


def test_task_filter_touches_only_its_samples():
    R.check_task_filter("cpu")


def test_origins_are_clamped_and_default_to_zero():
    R.check_origins("cpu")


def test_nan_zero_and_infinite_samples():
    R.check_nan_and_zero("cpu")


def test_two_calls_are_bitwise_equal():
    R.check_reproducible("cpu")


def test_refusals_launch_nothing():
    R.check_refusals("cpu")


@pytest.mark.parametrize("menu,N", [(["cassi"], 64), (["gaussianN", "cassi", "blur"], 64), (["gaussianN", "cassi", "blur"], 192)])
def test_fused_synthesizer_with_cassi_in_the_menu(menu, N):
    R.check_synthesizer("cpu", menu, N)


def test_synthetic_source_with_the_fine_tune_menu():
    R.check_source("cpu")


def test_menus_without_cassi_issue_the_launches_they_issued_before():
    R.check_launch_list("cpu")


def test_test_py_mode_13_fused_equals_tensor_form():
    R.check_test_py_mode_13("cpu")
