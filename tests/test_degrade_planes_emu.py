"""The tiled degradation launch (mphsir_degrade_planes, mp-hsir_amd/csrc/degrade.hip) on the CPU emulator: bitwise equal to the plane form
where both exist, against the tensor functions of mp-hsir_amd/degrade.py beyond it, generated draws on a non-square plane, the optional
pointers, the refusals, degrade.SceneDegrader and DegradationSynthesizer(fused=True) beyond 128 x 128.  The checks live in
tests/degrade_planes_ref.py; tests/test_degrade_planes_gpu.py runs them on the GPU."""
import types

import pytest
import torch

import degrade_planes_ref as P
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("N", [128, 96])
@pytest.mark.parametrize("explicit", [False, True], ids=["generated", "explicit"])
def test_bitwise_equal_to_the_plane_form(N, explicit):
    """N = 128: 2 x 2 tiles, seams on both axes; N = 96: partial tiles.  Every kind, subtype, stencil and factor under every mode"""
    assert len(P.check_bitwise_against_the_plane_form("cpu", N, explicit)) == len(P.VARIANTS) * 8


@pytest.mark.parametrize("shape,with_sr", [((1, 5, 72, 136), True), ((1, 3, 67, 131), False)], ids=["72x136", "67x131"])
def test_against_the_tensor_functions_beyond_the_plane_form(shape, with_sr):
    P.check_against_the_tensor_functions("cpu", shape, with_sr)


def test_generated_draws_on_a_non_square_plane():
    P.check_generated_draws("cpu")


def test_clean_aug_and_aug_may_be_null():
    P.check_optional_pointers("cpu")


def test_refusals():
    P.check_refusals("cpu")


def test_scene_degrader_modes_0_to_10():
    P.check_scene_degrader("cpu")


def test_synthesizer_fused_at_192():
    P.check_synthesizer("cpu")


def test_a_training_source_at_patch_256():
    """what train.py --patch_size 256 --fused_degrade 1 builds: the plane form refused these patches ("does not fit in LDS")"""
    from mp_hsir_amd.data import SyntheticPatchSource
    s = SyntheticPatchSource(5, 256, 2, 6, "cpu", 2024, 0, de_types=["gaussianN", "blur", "sr", "inpaint", "bandmiss"], fused_degrade=True)
    _, deg, cl, prompt = s.next()
    assert deg.shape == cl.shape == (2, 5, 256, 256) and prompt.shape == (2, 1) and bool(torch.isfinite(deg).all())


def test_test_py_has_the_flag_and_refuses_poisson():
    import importlib
    T = importlib.import_module("mp_hsir_amd.test")
    assert T.build_parser().parse_args([]).fused_degrade == 0
    o = T.build_parser().parse_args(["--fused_degrade", "1", "--mode", "11"])
    # evaluate_quality reads the band count off the net before it looks at the mode: a stand-in with that one attribute
    net = types.SimpleNamespace(patch_embed=types.SimpleNamespace(proj=types.SimpleNamespace(weight=torch.zeros(1, 31, 1, 1))))
    with pytest.raises(SystemExit, match="Poisson"):
        T.evaluate_quality(o, net, "cpu")
