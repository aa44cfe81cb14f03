"""Global-norm clipping and EMA weights on a real MI355X: the checks of tests/optim_ex_ref.py on the GPU (the arena sizes of the emulator
tests plus one past the 2048-block cap), the launches captured in a hipGraph and replayed on new gradients and new staged scalars, the
engine on the tiny net eager and in graph mode, checkpoint / resume with both features on, and train.py end to end."""
import importlib
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import model_checks as M
import optim_ex_ref as R
from golden.cases import TINY_CFG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = R.SIZES + [R.SIZE_GPU]


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


@pytest.mark.parametrize("n", SIZES)
def test_norm_matches_numpy_float64(n):
    R.check_norm("cuda", n)


@pytest.mark.parametrize("n", SIZES)
def test_clip_factor_and_the_unclipped_step(n):
    R.check_coef("cuda", n)


@pytest.mark.parametrize("n", SIZES)
def test_without_stats_and_ema_it_is_flat_adamw_bitwise(n):
    R.check_bitwise_link("cuda", n)


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_five_clipped_steps_with_ema(n, warmup):
    R.check_clipped_ema_steps("cuda", n, warmup)


@pytest.mark.parametrize("with_scaler", [False, True])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", SIZES[1:])
def test_a_non_finite_gradient_skips_the_step(n, bad, with_scaler):
    R.check_nonfinite("cuda", n, bad, with_scaler)


@pytest.mark.parametrize("n", SIZES)
def test_two_runs_are_bitwise_equal(n):
    R.check_reproducible("cuda", n)


def test_refusals_launch_nothing():
    R.check_refusals("cuda")


def test_captured_launches_follow_new_gradients_and_new_scalars():
    """grad_norm + flat_adamw_ex captured in one graph and replayed three times; between replays the gradient arena is overwritten and the
    staged hyper (lr, bias corrections, EMA decay) changes: every replay within the bar of the restatement"""
    from mp_hsir_amd import ops
    n, dev = 3 * 1024 + 4, "cuda"
    p, m, v = R._fresh(n, dev, 700)
    ema, stats, g = p.clone(), ops.new_optim_stats(dev), torch.zeros(n, device=dev)
    ws, hyper = ops.grad_norm_workspace(g), torch.zeros(4, device=dev)
    ref = R.RefState(p, ema=p)
    max_norm = 0.5 * math.sqrt(n)
    start = R.bits(p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.grad_norm(g, stats, max_norm, 0.5, workspace=ws)
        ops.flat_adamw_ex(p, g, m, v, 0.0, 0, grad_scale=0.5, hyper=hyper, stats=stats, ema=ema)
    assert R.bits(p) == start, "capturing must not run the launches"
    for t in (1, 2, 3):
        g.copy_(R.normals(n, 700 + t, dev, scale=2.0 + t))
        lr, d = 1e-2 / t, R.ema_decay_at(0.9, t, t != 2)
        bc = (1.0 - 0.9 ** t, math.sqrt(1.0 - 0.999 ** t))
        hyper.copy_(torch.tensor([lr, bc[0], bc[1], d]))
        graph.replay()
        norm, coef = ref.step(g, lr, t, max_norm=max_norm, grad_scale=0.5, decay=d, bc=bc)
        assert coef < 1.0 and abs(float(stats[1]) - coef) <= 2 * R.ulp32(coef) and abs(float(stats[0]) - norm) <= 2 * R.ulp32(norm)
        ref.compare(p, m, v, ema, "replay %d (lr %.3g, decay %.3f, coef %.3f)" % (t, lr, d, coef))


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_off_by_default(use_graph):
    R.check_engine_off("cuda", use_graph)


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_measure_only_clip_plus_ema_then_active_clip(use_graph):
    norm1 = R.check_engine_measure_and_ema("cuda", use_graph)
    R.check_engine_active_clip("cuda", norm1, use_graph)


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_ema_weights_context(use_graph):
    R.check_engine_ema_weights("cuda", use_graph)


def test_checkpoint_resume_with_clip_and_ema_continues_bitwise(tmp_path):
    """save_checkpoint after 2 steps -> a NEW model + engine, load_warm_start(resume=True) -> 2 more steps == 4 steps straight through,
    bitwise: parameters, moments, EMA and the skip count (set by hand after the first step); test.py's loader yields the EMA weights of the file"""
    from golden.detfill import seeded_input
    from mp_hsir_amd.engine import DataParallelEngine
    T = importlib.import_module("mp_hsir_amd.train")
    E = importlib.import_module("mp_hsir_amd.test")
    kw = dict(lr=2e-3, grad_clip=0.2, ema_decay=0.9)

    def batch(step):
        return (seeded_input("ck_x%d" % step, (2, 8, 32, 32)).cuda(), seeded_input("ck_c%d" % step, (2, 8, 32, 32)).cuda(),
                torch.tensor([[1], [3]]).cuda())

    def run(eng, steps):
        for s in steps:
            torch.manual_seed(100 + s)
            eng.train_step(*batch(s), lr=2e-3)
            if s == 0:
                eng.optim_stats[2] = 3.0          # as if three earlier steps had been skipped: the count must travel through the file
        torch.cuda.synchronize()

    net_a = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    eng_a = DataParallelEngine(net_a, **kw)
    run(eng_a, range(4))
    net_b = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    eng_b = DataParallelEngine(net_b, **kw)
    run(eng_b, range(2))
    assert eng_b.grad_stats()["skipped"] == 3 and eng_b.grad_stats()["coef"] < 1.0
    path = str(tmp_path / "epoch=7.ckpt")
    T.save_checkpoint(path, net_b, eng_b, epoch=7)
    net_c = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    with torch.no_grad():
        for p in net_c.parameters():
            p.mul_(0.5)                           # everything must come from the file
    eng_c = DataParallelEngine(net_c, **kw)
    n, start = T.load_warm_start(net_c, path, torch.device("cuda"), eng_c, resume=True)
    assert start == 8 and n == len(net_c.state_dict())
    run(eng_c, range(2, 4))
    for (k, va), vc in zip(net_a.state_dict().items(), net_c.state_dict().values()):
        assert torch.equal(va, vc), k
    sa, sc = eng_a.optimizer_state(), eng_c.optimizer_state()
    assert sa["step"] == sc["step"] == 4 and torch.isfinite(eng_a.flat_p).all()
    for k in sa["exp_avg"]:
        assert torch.equal(sa["exp_avg"][k], sc["exp_avg"][k]) and torch.equal(sa["exp_avg_sq"][k], sc["exp_avg_sq"][k]) and torch.equal(sa["ema"][k], sc["ema"][k]), k
    assert sa["optim_stats"][2] == sc["optim_stats"][2] == 3.0 and torch.equal(sa["optim_stats"], sc["optim_stats"])
    # test.py's loader
    ckpt = torch.load(path, map_location="cpu")
    ema_sd, live_sd = E.checkpoint_weights(ckpt, use_ema=True, path=path), E.checkpoint_weights(ckpt, path=path)
    want = eng_b.ema_state_dict()
    assert set(ema_sd) == set(want) and all(torch.equal(ema_sd[k], want[k].cpu()) for k in want)
    assert any(not torch.equal(ema_sd[k], live_sd[k]) for k in ema_sd)
    del ckpt["state_dict_ema"]
    with pytest.raises(SystemExit, match="holds no state_dict_ema"):
        E.checkpoint_weights(ckpt, use_ema=True, path=path)
    # a state without "ema": the EMA starts from the loaded parameters
    state = eng_b.optimizer_state()
    del state["ema"]
    eng_b.load_optimizer_state(state)
    assert torch.equal(eng_b.flat_ema, eng_b.flat_p)


def test_train_py_logs_the_norm_and_the_clip_factor():
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "train.py"), "--epochs", "1", "--steps_per_epoch", "6",
           "--log_every", "2", "--batch_size", "4", "--patch_size", "32", "--allow_surrogate_clip", "1", "--grad_clip", "1.0", "--ema_decay", "0.999"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    rows = [m.groups() for m in (re.match(r"^epoch \d+ it \d+ lr \S+ grad_norm (\S+) clip (\S+) train_loss (\S+)$", ln) for ln in r.stdout.splitlines()) if m]
    print(rows)
    assert len(rows) == 3, r.stdout[-2000:]
    for norm, clip, loss in rows:
        assert math.isfinite(float(norm)) and 0.0 < float(clip) <= 1.0 and math.isfinite(float(loss))
