"""Global-norm clipping and EMA weights on the CPU: the kernels of mp-hsir_amd/csrc/optim.hip through the emulated build against the
float64 restatement of tests/optim_ex_ref.py, and the engine's clip / EMA path, eager, on the two-convolution network of optim_ex_ref (a
step of the tiny MP-HSIR net takes 75 s through the emulator: that network runs these checks on the GPU, tests/test_optim_ex_gpu.py)."""
import pytest

import optim_ex_ref as R
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("n", R.SIZES)
def test_norm_matches_numpy_float64(n):
    R.check_norm("cpu", n)


@pytest.mark.parametrize("n", R.SIZES)
def test_clip_factor_and_the_unclipped_step(n):
    R.check_coef("cpu", n)


@pytest.mark.parametrize("n", R.SIZES)
def test_without_stats_and_ema_it_is_flat_adamw_bitwise(n):
    R.check_bitwise_link("cpu", n)


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("n", R.SIZES)
def test_five_clipped_steps_with_ema(n, warmup):
    R.check_clipped_ema_steps("cpu", n, warmup)


@pytest.mark.parametrize("with_scaler", [False, True])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", R.SIZES[1:])
def test_a_non_finite_gradient_skips_the_step(n, bad, with_scaler):
    R.check_nonfinite("cpu", n, bad, with_scaler)


@pytest.mark.parametrize("n", R.SIZES)
def test_two_runs_are_bitwise_equal(n):
    R.check_reproducible("cpu", n)


def test_refusals_launch_nothing():
    R.check_refusals("cpu")


def test_engine_off_by_default():
    R.check_engine_off("cpu", kind="conv")


def test_engine_measure_only_clip_plus_ema_then_active_clip():
    norm1 = R.check_engine_measure_and_ema("cpu", kind="conv")
    R.check_engine_active_clip("cpu", norm1, kind="conv")


def test_engine_ema_weights_context():
    R.check_engine_ema_weights("cpu", kind="conv")
