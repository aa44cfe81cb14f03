"""The window-attention backward that forms the total d_sa itself (MPHSIR_BRANCH_BWD_FUSED), on a real MI355X: the same
checks as tests/test_branch_bwd_emu.py (tests/branch_bwd_checks.py), device = cuda."""
import pytest
import torch

import branch_bwd_checks as BB

pytestmark = pytest.mark.gpu
HALF = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


def test_dsa_fits():
    BB.check_dsa_fits("cuda")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("C,heads", BB.PROLOGUE_CASES)
def test_win_attn_bwd_dsa_prologue(dtype, C, heads, shift):
    BB.check_dsa_prologue("cuda", dtype, C, heads, shift)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("name", BB.BLOCK_NAMES)
def test_block_backward_switch_on_and_off(name, shift):
    BB.check_block("cuda", torch.bfloat16, name, shift)


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("name", BB.BLOCK_NAMES)
def test_block_backward_deterministic(name, shift):
    BB.check_block_deterministic("cuda", torch.bfloat16, name, shift)


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("shift", [0, 4])
def test_win_attn_bwd_dsa_prologue_single_window(dtype, shift):
    """the smallest accepted shape, one 8x8 window: an overrun of one window lands in a guard band (tests/guard.py), not in the tensor"""
    BB.check_dsa_prologue("cuda", dtype, 64, 2, shift, shape=(1, 8, 8))
