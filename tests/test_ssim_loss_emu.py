"""The SSIM term of the training loss on the CPU: the two ssim_loss kernels of mp-hsir_amd/csrc/arena.hip through the emulated build against
the float64 restatement of tests/ssim_loss_ref.py, the restatement itself against float64 autograd and metrics.ssim_bands, the kernels' bits
under the adversarial wave schedules of tests/test_emu_schedules.py, and the engine's loss path, eager, on the two-convolution network (the
tiny MP-HSIR net runs these checks on the GPU, tests/test_ssim_loss_gpu.py).

test_restatement_matches_float64_autograd_and_ssim_bands validates the REFERENCE, not the kernels: it runs no new product code (and so
passes on a tree without the feature); it is there to show that the restatement every other test of this file, of
tests/test_ssim_loss_gpu.py and of tests/test_ssim_loss_host.py measures the kernels against is independent of them and right."""
import pytest

import guard
import ssim_loss_ref as R
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


RESTATEMENT_SHAPES = [(2, 3, 7, 7), (1, 1, 7, 20), (2, 3, 13, 13), (1, 2, 23, 38), (1, 3, 45, 70), (2, 31, 16, 16), (1, 2, 64, 64)]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", RESTATEMENT_SHAPES, ids=str)
def test_restatement_matches_float64_autograd_and_ssim_bands(shape, family):
    R.check_restatement(shape, family)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_ssim_loss_and_gradient(shape, family):
    R.check_values("cpu", shape, family)


def test_one_element_past_a_16_byte_boundary_and_two_runs():
    R.check_values("cpu", (2, 31, 16, 16), offset=True)
    R.check_reproducible_and_alignment("cpu")


def test_ssim_is_the_one_quality_bands_reports():
    R.check_quality_agrees("cpu", (1, 3, 45, 70))


def test_edge_semantics():
    R.check_edges("cpu")


def test_refusals_launch_nothing():
    R.check_refusals("cpu")


def test_bits_do_not_depend_on_the_wave_schedule():
    """the value check under the default schedule, then under every adversarial schedule: every recorded tensor (what ops handed back and
    every buffer the guard gave a kernel to write) holds the same bits"""
    import build_emu
    import test_emu_schedules as S
    from mp_hsir_amd import ops
    lib = S._handle(build_emu.OUT)

    def run(mode, seed):
        lib.hipemu_set_schedule(mode, seed)
        ops.ACCOUNT = {}
        try:
            with guard.recording() as rec:
                R.check_values("cpu", (1, 2, 23, 38), "smooth")
            return list(rec), set(ops.ACCOUNT), lib.hipemu_max_waves()
        finally:
            ops.ACCOUNT = None
            lib.hipemu_set_schedule(0, 0)

    run(0, 0)                                   # the workspace of this shape exists from here on
    base, seen, waves = run(0, 0)
    assert base and "ssim_loss" in seen and waves > 1
    for mode, seed in S.schedules(waves):
        got, seen_s, waves_s = run(mode, seed)
        assert (seen_s, waves_s, len(got)) == (seen, waves, len(base)), S.describe(mode, seed)
        for i, ((what, a), (_, b)) in enumerate(zip(base, got)):
            diff = guard.first_difference(a, b)
            assert diff is None, "under %s: recorded tensor %d of %d (%s): %s" % (S.describe(mode, seed), i, len(base), what, diff)


@pytest.mark.parametrize("kw", R.LOSSES, ids=["ssim", "sam+sdiff+ssim"])
def test_engine_returns_the_kernels_loss_and_reports_components(kw):
    R.check_engine_loss_and_components("cpu", kw, kind="conv")


def test_engine_without_the_term_launches_what_it_always_did():
    R.check_engine_without_the_term("cpu", kind="conv")


def test_engine_loss_scaler_path():
    R.check_engine_fp16_scaler("cpu", kind="conv")


def test_engine_three_eager_steps_twice_give_the_same_bits():
    """graph mode needs a GPU (tests/test_ssim_loss_gpu.py); here: two eager engines train bitwise the same three steps"""
    from mp_hsir_amd.engine import SpectralLoss
    _, l0, p0, _ = R.run_engine("cpu", "conv", 3, loss_fn=SpectralLoss(0.1, 0.1, 0.2))
    _, l1, p1, _ = R.run_engine("cpu", "conv", 3, loss_fn=SpectralLoss(0.1, 0.1, 0.2))
    assert [R.bits(a) for a in l0] == [R.bits(b) for b in l1] and p0 == p1
