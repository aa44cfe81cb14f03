"""The SSIM term of the training loss on a real MI355X: the checks of tests/ssim_loss_ref.py on the GPU (the shapes of the emulator tests
plus the training patch), the base pair and the SSIM pair captured in one hipGraph and replayed on new contents, the engine on the tiny net
(fp32, bf16, fp16; eager and graph mode; the term off), a checkpoint round trip and train.py end to end."""
import importlib
import os
import re
import subprocess
import sys

import pytest
import torch

import model_checks as M
import ssim_loss_ref as R
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


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("shape", R.SHAPES + [R.SHAPE_GPU], ids=str)
def test_ssim_loss_and_gradient(shape, family):
    R.check_values("cuda", shape, family)


def test_one_element_past_a_16_byte_boundary_and_two_runs():
    R.check_values("cuda", (2, 31, 16, 16), offset=True)
    R.check_reproducible_and_alignment("cuda")
    R.check_reproducible_and_alignment("cuda", R.SHAPE_GPU)


@pytest.mark.parametrize("shape", [(1, 3, 45, 70), R.SHAPE_GPU], ids=str)
def test_ssim_is_the_one_quality_bands_reports(shape):
    R.check_quality_agrees("cuda", shape)


def test_edge_semantics():
    R.check_edges("cuda")


def test_refusals_launch_nothing():
    R.check_refusals("cuda")


def test_captured_base_and_ssim_pairs_follow_new_contents():
    """the spectral pair and the SSIM pair captured in one graph and replayed three times on new contents of the same buffers: every replay
    within the bars"""
    from mp_hsir_amd import ops
    import spectral_loss_ref as SL
    shape = (2, 31, 64, 64)
    y, c = torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
    ops.spectral_loss_grad(y, c + 0.5, 0.1, 0.3)          # the workspaces of this shape exist before the capture
    ops.ssim_loss_grad(y, c + 0.5, R.W_SSIM)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        lb, gb, parts = ops.spectral_loss_grad(y, c, 0.1, 0.3)
        gb0 = gb.clone()
        loss, g, out = ops.ssim_loss_grad(y, c, R.W_SSIM, base_loss=lb.reshape(1), grad=gb)
    results = []
    for t in range(3):
        ym, cm = R.make_inputs(shape, FAMILY_OF_REPLAY[t], seed=20 + t)
        y.copy_(ym)
        c.copy_(cm)
        graph.replay()
        results.append((ym, cm, out.clone(), g.clone(), loss.clone(), gb0.clone(), parts.clone()))
    torch.cuda.synchronize()
    del graph                     # destroyed before anything can fail: a graph kept alive by a failure's frames dies at the collector's whim
    for t, (ym, cm, o, gg, ls, g0, p) in enumerate(results):
        SL.assert_within_bars(p, g0, SL.reference(ym, cm, 0.1, 0.3), "replay %d base" % t)
        R.assert_within_bars(o, gg, R.reference(ym, cm, R.W_SSIM, g_base=g0, base=float(p[0])), "replay %d" % t)
        assert R.bits(ls) == R.bits(o[0])


FAMILY_OF_REPLAY = ("noise", "smooth", "flat")


@pytest.mark.parametrize("kw", R.LOSSES, ids=["ssim", "sam+sdiff+ssim"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_three_steps_eager_and_graph_are_bitwise_equal(dtype, kw):
    R.check_engine_eager_vs_graph("cuda", kw, dtype=dtype)


@pytest.mark.parametrize("kw", R.LOSSES, ids=["ssim", "sam+sdiff+ssim"])
def test_engine_returns_the_kernels_loss_and_reports_components(kw):
    R.check_engine_loss_and_components("cuda", kw)


def test_engine_fp16_runs_through_the_scaler():
    R.check_engine_fp16_scaler("cuda")


def test_engine_without_the_term_launches_what_it_always_did():
    R.check_engine_without_the_term("cuda")


def test_checkpoint_round_trip_keeps_the_ssim_weight(tmp_path, capsys):
    from mp_hsir_amd.engine import DataParallelEngine, SpectralLoss
    T = importlib.import_module("mp_hsir_amd.train")
    net = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    eng = DataParallelEngine(net, lr=2e-3, loss_fn=SpectralLoss(0.1, 0.1, 0.2))
    eng.train_step(*R.batch(0, "cuda", "tiny"))
    path = str(tmp_path / "epoch=0.ckpt")
    T.save_checkpoint(path, net, eng, epoch=0)
    assert torch.load(path, map_location="cpu")["mphsir_loss"] == {"sam": 0.1, "sdiff": 0.1, "ssim": 0.2}
    net2 = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    T.load_warm_start(net2, path, torch.device("cuda"), DataParallelEngine(net2, lr=2e-3, loss_fn=SpectralLoss(0.1, 0.1, 0.2)), resume=True)
    assert "loss weights" not in capsys.readouterr().out
    T.load_warm_start(net2, path, torch.device("cuda"), DataParallelEngine(net2, lr=2e-3, loss_fn=SpectralLoss(0.1, 0.1)), resume=True)
    assert "trained with loss weights sam 0.1 sdiff 0.1 ssim 0.2, this run continues with sam 0.1 sdiff 0.1 ssim 0" in capsys.readouterr().out


def _train(*extra):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "train.py"), "--epochs", "1", "--steps_per_epoch", "6",
           "--log_every", "2", "--batch_size", "4", "--patch_size", "32", "--allow_surrogate_clip", "1"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_train_py_logs_the_ssim():
    out = _train("--loss_ssim", "0.2")
    rows = [m.groups() for m in (re.match(r"^epoch \d+ it \d+ lr \S+ train_loss (\S+) .*ssim (\S+)$", ln) for ln in out.splitlines()) if m]
    print(rows)
    assert len(rows) == 3, out[-2000:]
    for loss, s in rows:
        assert float(loss) > 0 and 0.0 < float(s) < 1.0


def test_train_py_without_the_flag_prints_the_rows_of_always():
    out = _train()
    rows = [ln for ln in out.splitlines() if re.match(r"^epoch \d+ it \d+ lr \S+ train_loss (\S+)$", ln)]
    assert len(rows) == 3 and not any("ssim" in ln for ln in out.splitlines() if ln.startswith("epoch ")), out[-2000:]
