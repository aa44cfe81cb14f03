"""The training loss with spectral terms on a real MI355X: the checks of tests/spectral_loss_ref.py on the GPU (the shapes of the emulator
tests plus the training patch one element past a 16-byte boundary), the launch pair captured in a hipGraph and replayed on new contents,
the engine on the tiny net (fp32, bf16, fp16; eager and graph mode; off by default), a checkpoint round trip and train.py end to end."""
import importlib
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import model_checks as M
import spectral_loss_ref as R
from golden.cases import TINY_CFG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_loss_components_and_gradient(shape):
    R.check_values("cuda", shape)


def test_scalar_path_at_the_training_patch_one_element_past_a_16_byte_boundary():
    R.check_values("cuda", R.SHAPE_GPU, offset=True)
    R.check_paths_agree("cuda", R.SHAPE_GPU)


def test_edge_semantics():
    R.check_edges("cuda")


def test_a_zero_weight_leaves_its_term_out():
    R.check_zero_weight("cuda")


@pytest.mark.parametrize("shape", [R.SHAPES[2], R.SHAPES[6]], ids=str)
def test_two_runs_are_bitwise_equal(shape):
    R.check_reproducible("cuda", shape)


def test_refusals_launch_nothing():
    R.check_refusals("cuda")


def test_captured_launch_pair_follows_new_contents():
    """both launches captured in one graph and replayed three times on new contents of the same buffers: every replay within the bars"""
    from mp_hsir_amd import ops
    shape = (2, 31, 64, 64)
    y, c = torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
    ops.spectral_loss_grad(y, c + 0.5, 0.1, 0.3)          # the workspace of this shape exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss, g, out = ops.spectral_loss_grad(y, c, 0.1, 0.3)
    results = []
    for t in range(3):
        ym, cm = R.make_inputs(shape, seed=20 + t)
        y.copy_(ym)
        c.copy_(cm)
        graph.replay()
        results.append((ym, cm, out.clone(), g.clone(), loss.clone()))
    torch.cuda.synchronize()
    del graph                     # destroyed before anything can fail: a graph kept alive by a failure's frames dies at the collector's whim
    for t, (ym, cm, o, gg, ls) in enumerate(results):
        R.assert_within_bars(o, gg, R.reference(ym, cm, 0.1, 0.3), "replay %d" % t)
        assert R.bits(ls) == R.bits(o[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_three_steps_eager_and_graph_are_bitwise_equal(dtype):
    """losses, gradient arenas and parameters of three steps, eager against graph mode.  Under the default loss the two modes differ from
    the first replayed optimizer step on (the library forms Adam's bias corrections with fp32 powf in an eager step, a replayed step
    reads the ones the engine staged from float64); under a SpectralLoss the eager step stages them too (engine._eager_hyper)."""
    R.check_engine_eager_vs_graph("cuda", dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_returns_the_kernels_loss_and_reports_components(dtype):
    R.check_engine_loss_and_components("cuda", dtype=dtype)


def test_engine_fp16_runs_through_the_scaler():
    R.check_engine_fp16_scaler("cuda")


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_off_by_default(use_graph):
    R.check_engine_off_by_default("cuda", use_graph=use_graph)


def test_checkpoint_round_trip_keeps_the_loss_weights(tmp_path, capsys):
    from mp_hsir_amd.engine import DataParallelEngine, SpectralLoss
    T = importlib.import_module("mp_hsir_amd.train")
    net = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    eng = DataParallelEngine(net, lr=2e-3, loss_fn=SpectralLoss(0.1, 0.1))
    eng.train_step(*R.batch(0, "cuda", "tiny"))
    path = str(tmp_path / "epoch=0.ckpt")
    T.save_checkpoint(path, net, eng, epoch=0)
    assert torch.load(path, map_location="cpu")["mphsir_loss"] == {"sam": 0.1, "sdiff": 0.1}
    net2 = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    T.load_warm_start(net2, path, torch.device("cuda"), DataParallelEngine(net2, lr=2e-3, loss_fn=SpectralLoss(0.1, 0.1)), resume=True)
    assert "loss weights" not in capsys.readouterr().out
    T.load_warm_start(net2, path, torch.device("cuda"), DataParallelEngine(net2, lr=2e-3, loss_fn=SpectralLoss(0.2, 0.1)), resume=True)
    assert "trained with loss weights sam 0.1 sdiff 0.1, this run continues with sam 0.2 sdiff 0.1" in capsys.readouterr().out


def _train(*extra):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "train.py"), "--epochs", "1", "--steps_per_epoch", "6",
           "--log_every", "2", "--batch_size", "4", "--patch_size", "32", "--allow_surrogate_clip", "1"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_train_py_logs_the_three_terms():
    out = _train("--loss_sam", "0.1", "--loss_sdiff", "0.1")
    rows = [m.groups() for m in (re.match(r"^epoch \d+ it \d+ lr \S+ train_loss (\S+) l1 (\S+) sam_deg (\S+) sdiff (\S+)$", ln) for ln in out.splitlines()) if m]
    print(rows)
    assert len(rows) == 3, out[-2000:]
    for loss, l1, sam, sd in rows:
        assert all(math.isfinite(float(v)) and float(v) > 0 for v in (loss, l1, sam, sd)) and float(loss) > float(l1)


def test_train_py_without_the_flags_prints_the_rows_of_always():
    out = _train()
    rows = [ln for ln in out.splitlines() if re.match(r"^epoch \d+ it \d+ lr \S+ train_loss (\S+)$", ln)]
    assert len(rows) == 3 and not any(" l1 " in ln or "sam_deg" in ln for ln in out.splitlines() if ln.startswith("epoch ")), out[-2000:]
