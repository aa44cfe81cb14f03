"""The window-attention backward that forms the total d_sa itself (MPHSIR_BRANCH_BWD_FUSED), on the CPU emulator: the same
checks as tests/test_branch_bwd_gpu.py (tests/branch_bwd_checks.py), device = cpu."""
import pytest
import torch

import branch_bwd_checks as BB
from emu import bind_emulator

HALF = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


def test_dsa_fits():
    BB.check_dsa_fits("cpu")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("C,heads", BB.PROLOGUE_CASES)
def test_win_attn_bwd_dsa_prologue(dtype, C, heads, shift):
    BB.check_dsa_prologue("cpu", dtype, C, heads, shift)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("name", BB.BLOCK_NAMES)
def test_block_backward_switch_on_and_off(name, shift):
    BB.check_block("cpu", torch.bfloat16, name, shift)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("name", BB.BLOCK_NAMES)
def test_block_backward_deterministic(name, shift):
    BB.check_block_deterministic("cpu", torch.bfloat16, name, shift)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shift", [0, 4])
def test_win_attn_bwd_dsa_prologue_single_window(dtype, shift):
    """the smallest accepted shape, one 8x8 window: an overrun of one window lands in a guard band (tests/guard.py), not in the tensor"""
    BB.check_dsa_prologue("cpu", dtype, 64, 2, shift, shape=(1, 8, 8))
