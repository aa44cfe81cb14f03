"""The quality meter on the CPU: mp-hsir_amd/csrc/quality_meter.hip through the emulated build against the float64 restatement of
tests/quality_meter_ref.py, bitwise (adds and one divide per image: no tolerance)."""
import pytest

import quality_meter_ref as R
from emu import bind_emulator


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("use", R.USES)
@pytest.mark.parametrize("B,C", R.SHAPES)
def test_table_equals_the_restatement_bitwise(B, C, use):
    R.check_values("cpu", B, C, use)


def test_the_row_does_not_depend_on_how_the_set_was_cut():
    R.check_split_invariance("cpu")


def test_two_runs_are_bitwise_equal():
    R.check_reproducible("cpu")


def test_edge_semantics():
    R.check_edges("cpu")


def test_refusals_launch_nothing():
    R.check_refusals("cpu")


def test_more_images_than_one_chunk():
    """300 images: the kernel takes them in chunks of its 256 threads, the row is one chain across the chunks"""
    R.check_values("cpu", 300, 3, "random")
