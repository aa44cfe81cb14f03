"""Gradient accumulation on a real MI355X: the checks of tests/accum_ref.py on the GPU -- the kernel with the index from the host and from
a device int32, captured once and replayed; the engine on the tiny net, eager and in graph mode; checkpoint / resume; two gloo ranks sharing
the GPU against one accumulating process; train.py end to end."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import accum_ref as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


def test_kernel_stores_then_adds_host_and_device_index_and_replayed():
    eager = A.check_kernel("cuda", "host")
    A.check_kernel_forms("cuda")
    assert A.check_kernel_graph() == eager, "the replayed launch and the eager launch give different arenas"


def test_copy_form_is_the_old_launch():
    A.check_copy_form_is_the_old_launch("cuda")


def test_refusals_launch_nothing():
    A.check_refusals("cuda")


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_off_is_off(use_graph):
    A.check_off_is_off("cuda", "tiny", use_graph)


def test_engine_arena_holds_the_sum():
    A.check_arena_holds_the_sum("cuda", "tiny")


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_the_step(use_graph):
    A.check_the_step("cuda", "tiny", use_graph)


@pytest.mark.parametrize("loss", ["l1", "sam"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_eager_equals_graph(dtype, loss):
    A.check_eager_equals_graph(dtype, loss)


@pytest.mark.parametrize("scaler", [True, False])
def test_engine_a_non_finite_micro_batch_skips_the_group(scaler):
    A.check_nonfinite_micro_batch("cuda", "tiny", scaler)


def test_checkpoint_resume_continues_bitwise(tmp_path):
    A.check_checkpoint(tmp_path)


@pytest.mark.timeout(600)
def test_two_ranks_equal_one_process_with_accum_steps_2_bitwise(tmp_path):
    A.check_gpu_two_ranks_equal_accum2(tmp_path)


@pytest.mark.timeout(600)
def test_two_ranks_with_accum_steps_2_against_torch_adamw(tmp_path):
    A.check_gpu_two_ranks_accum2_against_torch(tmp_path)


@pytest.mark.parametrize("extra", [[], ["--grad_clip", "1.0", "--ema_decay", "0.999", "--loss_ssim", "0.2"]], ids=["plain", "clip_ema_ssim"])
def test_train_py_end_to_end(extra):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "train.py"), "--accum_steps", "2", "--steps_per_epoch", "7",
           "--epochs", "1", "--log_every", "1", "--batch_size", "4", "--patch_size", "32", "--allow_surrogate_clip", "1"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    notes = [ln for ln in r.stdout.splitlines() if ln.startswith("note: --accum_steps")]
    assert notes == ["note: --accum_steps 2: 7 batches per epoch -> 3 optimizer steps, 1 not drawn"], r.stdout[-2000:]
    if extra:
        pat = r"^epoch 0 it (\d+) lr \S+ grad_norm (\S+) clip (\S+) train_loss (\S+) l1 \S+ sam_deg \S+ sdiff \S+ ssim \S+$"
    else:
        pat = r"^epoch 0 it (\d+) lr \S+ train_loss (\S+)$"
    rows = [m.groups() for m in (re.match(pat, ln) for ln in r.stdout.splitlines()) if m]
    print(rows)
    assert len(rows) == 3 and [int(row[0]) for row in rows] == [1, 2, 3], r.stdout[-2000:]
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("epoch ")]) == 3
    for row in rows:
        assert all(math.isfinite(float(v)) for v in row[1:]), row
