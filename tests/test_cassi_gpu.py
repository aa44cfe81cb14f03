"""mphsir_cassi, the cassi branches of the synthesiser, of the synthetic source and of test.py on a real MI355X: the checks of
tests/cassi_ref.py on the GPU, plus what only the GPU can show -- a captured launch pair that follows its device tables, a sample past
element 2^31 of the batch, and a training step of the one-task net fed by the fused cassi source."""
import numpy as np
import pytest
import torch

import cassi_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


@pytest.mark.parametrize("step", [1, 2, 3])
def test_square_batch_under_every_mode(step):
    R.check_square_all_modes("cuda", step)


def test_non_square_planes_without_augmentation():
    R.check_non_square("cuda")


def test_element_wise_path_for_odd_widths():
    R.check_scalar_path("cuda")


def test_equals_the_reference_function():
    R.check_golden("cuda")


def test_task_filter_touches_only_its_samples():
    R.check_task_filter("cuda")


def test_origins_are_clamped_and_default_to_zero():
    R.check_origins("cuda")


def test_nan_zero_and_infinite_samples():
    R.check_nan_and_zero("cuda")


def test_two_calls_are_bitwise_equal():
    R.check_reproducible("cuda")


def test_refusals_launch_nothing():
    R.check_refusals("cuda")


@pytest.mark.parametrize("menu,N", [(["cassi"], 64), (["gaussianN", "cassi", "blur"], 64), (["gaussianN", "cassi", "blur"], 192)])
def test_fused_synthesizer_with_cassi_in_the_menu(menu, N):
    R.check_synthesizer("cuda", menu, N)


def test_synthetic_source_with_the_fine_tune_menu():
    R.check_source("cuda")


def test_menus_without_cassi_issue_the_launches_they_issued_before():
    R.check_launch_list("cuda")


def test_test_py_mode_13_fused_equals_tensor_form():
    R.check_test_py_mode_13("cuda")


def test_training_shape_matches_numpy():
    """the shape the source runs at: B = 32, C = 31, 64 x 64, the default 256 x 256 binary mask, random origins and modes"""
    from mp_hsir_amd import degrade as D
    rs = np.random.RandomState(3)
    x = rs.rand(32, 31, 64, 64).astype(np.float32)
    mask = D.CassiMask("cpu", seed=1).mask.numpy()
    origins = np.stack([rs.randint(0, 193, 32), rs.randint(0, 193, 32)], axis=1)
    R.check_one("cuda", x, mask, origins, 2, rs.randint(0, 8, 32), True, "training shape")


def test_a_captured_pair_follows_its_device_tables():
    """the launch pair captured in a graph reads clean, origin and aug from device memory: replayed after they were overwritten it gives
    what an eager call gives then; two eager repeats are bitwise equal"""
    from mp_hsir_amd import ops
    g0 = torch.Generator().manual_seed(5)
    B, C, N = 4, 9, 32
    clean = torch.rand((B, C, N, N), generator=g0).cuda()
    mask = torch.rand((48, 40), generator=g0).cuda()
    origin = torch.tensor([(0, 0), (3, 5), (16, 8), (9, 1)], dtype=torch.int32, device="cuda")
    aug = torch.tensor([0, 3, 5, 6], dtype=torch.int32, device="cuda")
    out = (torch.empty_like(clean), torch.empty_like(clean))
    ws = torch.empty((ops._lib.load().mphsir_cassi_workspace_bytes(B, C, N, N, 2) // 4,), device="cuda")
    ops.cassi(clean, mask, origin, 2, aug=aug, out=out, workspace=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.cassi(clean, mask, origin, 2, aug=aug, out=out, workspace=ws)
    for turn in range(3):
        if turn:
            clean.copy_(torch.rand((B, C, N, N), generator=g0))
            origin.copy_(torch.randint(0, 9, (B, 2), generator=g0).int())
            aug.copy_(torch.randint(0, 8, (B,), generator=g0).int())
        out[0].fill_(-3.0)
        out[1].fill_(-3.0)
        g.replay()
        torch.cuda.synchronize()
        one = ops.cassi(clean, mask, origin, 2, aug=aug, want_clean_aug=True)
        two = ops.cassi(clean, mask, origin, 2, aug=aug, want_clean_aug=True)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
        assert torch.equal(out[0], one[0]) and torch.equal(out[1], one[1]), turn
        assert R.same_floats(out[0].cpu().numpy(), R.tensor_form("cuda", clean.cpu().numpy(), mask.cpu().numpy(), origin.cpu().numpy(), 2, aug.cpu().numpy()))


def test_a_sample_past_two_to_the_31_elements():
    """B = 18 samples of 31 x 2048 x 2048 (allocated, never filled): sample 17 starts at element 2.2e9 of both cubes; the task filter
    processes that sample alone, so the element arithmetic must be 64-bit and nothing else is touched"""
    from mp_hsir_amd import degrade as D, ops
    free, _ = torch.cuda.mem_get_info()
    if free < 32 * 1024 ** 3:
        pytest.skip("needs 32 GB of free device memory, %.1f GB are free" % (free / 1024 ** 3))
    B, C, N = 18, 31, 2048
    assert (B - 1) * C * N * N > 2 ** 31
    clean = torch.empty((B, C, N, N), device="cuda")
    degraded = torch.empty((B, C, N, N), device="cuda")
    clean[B - 1] = torch.rand((C, N, N), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    degraded[B - 2:].fill_(-7.0)
    mask = D.CassiMask("cuda", seed=2, shape=(N, N + 8))
    task = torch.zeros(B, dtype=torch.int32, device="cuda")
    task[B - 1] = 1
    origin = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    origin[B - 1, 1] = 5
    ops.cassi(clean, mask.mask, origin, 2, task=task, task_id=1, out=(degraded, None))
    want = D.cassi_measure(clean[B - 1:], mask.mask, origin[B - 1:], 2)
    assert torch.equal(degraded[B - 1:], want) and bool(torch.isfinite(want).all())
    assert float(degraded[B - 2].min()) == -7.0 == float(degraded[B - 2].max())


def test_one_training_step_of_the_one_task_net_on_fused_cassi_batches():
    """DataParallelEngine, the tiny one-task net, batch 2, 64 x 64, graph off, fed by SyntheticPatchSource(["cassi"], fused): the loss is
    finite and the parameters move"""
    import model_checks as M
    from golden.cases import TINY_CFG
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    net = M.build_net(dict(TINY_CFG, task_classes=1), "cuda", torch.float32).train()
    eng = DataParallelEngine(net, lr=1e-3, use_graph=False)
    src = SyntheticPatchSource(8, 64, 2, 1, "cuda", de_types=["cassi"], fused_degrade=True)
    before = [p.detach().clone() for p in net.parameters()]
    _, degraded, clean, prompt = src.next()
    assert int(prompt.abs().max()) == 0
    loss = eng.train_step(degraded, clean, prompt, lr=1e-3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and float(loss) > 0
    assert sum(not torch.equal(a, b) for a, b in zip(before, net.parameters())) > len(before) // 2
