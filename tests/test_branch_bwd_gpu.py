"""The window-attention backward that forms the total d_sa itself (ops.BRANCH_BWD_FUSED), on a real MI355X: the same
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


# ---- the block backward off the unit Gaussian (branch_bwd_checks.PROFILES): win_attn_bwd's own LayerNorm epsilon and recomputed softmax
# under flat rows and peaked / saturated logits, at one window and at (2, 16, 16), both shifts; bars from kernel_checks.yard_bar ----
@pytest.mark.parametrize("B,hw,inputs", BB.PROFILE_CASES)
@pytest.mark.parametrize("shift", [0, 4])
def test_block_backward_input_profiles(shift, B, hw, inputs):
    BB.check_block("cuda", torch.bfloat16, "nat_enc1", shift, B=B, hw=hw, inputs=inputs)


def test_guard_and_slice_bounds_were_active():
    """the profile cases above ran under tests/guard.py and compared through kernel_checks.close: one more case moves both counters"""
    import guard
    import kernel_checks as K
    g0 = list(guard.STATS.get("branch_bwd_checks", [0, 0, {}]))
    s0 = list(K.SLICE_STATS.get("check_block", [0, 0.0, ""]))
    BB.check_block("cuda", torch.bfloat16, "nat_enc1", 4, B=1, hw=(8, 8), inputs="flat")
    g1, s1 = guard.STATS["branch_bwd_checks"], K.SLICE_STATS["check_block"]
    assert g1[0] >= g0[0] + 1 and s1[0] > s0[0] and 0 < s1[1] < K.SLICE_F, (g0, g1, s0, s1)
    assert ("check_block", "flat", "bfloat16", "dx") in K.PROFILE_STATS
    print("\n".join(line for line in K.profile_report() if "check_block" in line))
