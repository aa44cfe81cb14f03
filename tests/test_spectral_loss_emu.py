"""The training loss with spectral terms on the CPU: the two kernels of mp-hsir_amd/csrc/spectral_loss.hip through the emulated build against
the float64 restatement of tests/spectral_loss_ref.py, the restatement itself against float64 autograd, and the engine's loss path, eager, on
the two-convolution network of tests/optim_ex_ref.py (the tiny MP-HSIR net runs these checks on the GPU, tests/test_spectral_loss_gpu.py)."""
import pytest

import spectral_loss_ref as R
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[1] >= 3], ids=str)
def test_restatement_matches_float64_autograd(shape):
    R.check_restatement_vs_autograd(shape)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_loss_components_and_gradient(shape):
    R.check_values("cpu", shape)


def test_scalar_path_one_element_past_a_16_byte_boundary():
    R.check_values("cpu", (2, 31, 16, 16), offset=True)
    R.check_paths_agree("cpu")


def test_edge_semantics():
    R.check_edges("cpu")


def test_a_zero_weight_leaves_its_term_out():
    R.check_zero_weight("cpu")


@pytest.mark.parametrize("shape", [R.SHAPES[2], R.SHAPES[3]], ids=str)
def test_two_runs_are_bitwise_equal(shape):
    R.check_reproducible("cpu", shape)


def test_refusals_launch_nothing():
    R.check_refusals("cpu")


def test_engine_off_by_default_and_the_launch_list_with_the_loss_on():
    R.check_engine_off_by_default("cpu", kind="conv")


def test_engine_returns_the_kernels_loss_and_reports_components():
    R.check_engine_loss_and_components("cpu", kind="conv")


def test_engine_loss_scaler_path():
    R.check_engine_fp16_scaler("cpu", kind="conv")
