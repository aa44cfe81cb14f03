"""In-training validation on a real MI355X: the quality meter against the float64 restatement of tests/quality_meter_ref.py (bitwise), its
launch captured in a hipGraph, the Validator on the tiny net against metrics.compute_quality and test.evaluate_quality, training left
undisturbed (eager and graph mode, fp32 and bf16, EMA weights), and train.py end to end."""
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import model_checks as M
import quality_meter_ref as R
import validate_checks as C
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


# ---- the meter ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use", R.USES)
@pytest.mark.parametrize("B,C", R.SHAPES)
def test_meter_table_equals_the_restatement_bitwise(B, C, use):
    R.check_values("cuda", B, C, use)


def test_meter_row_does_not_depend_on_how_the_set_was_cut():
    R.check_split_invariance("cuda")


def test_meter_two_runs_are_bitwise_equal():
    R.check_reproducible("cuda")


def test_meter_edge_semantics():
    R.check_edges("cuda")


def test_meter_refusals_launch_nothing():
    R.check_refusals("cuda")


def test_meter_more_images_than_one_chunk():
    R.check_values("cuda", 300, 3, "random")


def test_meter_captured_launch_follows_new_contents():
    """the launch captured once (reset, then onto the row) and replayed on new contents of the same buffers: every replay is the
    restatement of its contents, bitwise"""
    from mp_hsir_amd import ops
    B, C = 5, 31
    dev = "cuda"
    p, s = torch.zeros((B, C), dtype=torch.float64, device=dev), torch.ones((B, C), dtype=torch.float64, device=dev)
    a, px = torch.zeros((B,), dtype=torch.float64, device=dev), torch.zeros((B,), dtype=torch.int64, device=dev)
    use = torch.ones((B, C), dtype=torch.uint8, device=dev)
    table = torch.full((2, 8), -7.0, dtype=torch.float64, device=dev)
    ops.quality_meter(table, 1, p, s, a, px, use=use, n=4, reset=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        ops.quality_meter(table, 1, p, s, a, px, use=use, n=4, reset=True)
        ops.quality_meter(table, 1, p, s, a, px, use=use, n=B, reset=False)
    got, want = [], []
    for t in range(3):
        hp, hs, ha, hpx = R.make_values(B, C, seed=30 + t)
        hu = R.make_use("random", B, C, seed=30 + t)
        for dst, src in ((p, hp), (s, hs), (a, ha), (px, hpx), (use, hu)):
            dst.copy_(torch.from_numpy(src))
        graph.replay()
        got.append(table.clone())
        want.append(R.meter_ref(R.meter_ref(None, hp, hs, ha, use=hu, n=4, reset=True), hp, hs, ha, use=hu))
    torch.cuda.synchronize()
    del graph
    for g, w in zip(got, want):
        assert R.bits(g[1]) == R.bits(w) and R.bits(g[0]) == R.bits(np.full(8, -7.0)), (g, w)


# ---- the Validator on the tiny net ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """(net, set, validator at batch 2, result, restored crops, table bytes, prompts seen, training flag and RNG states around the pass):
    computed once, shared by the tests below and left unchanged"""
    from mp_hsir_amd import validate
    net = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    vset = C.make_vset("cuda", "tiny", net)
    val = validate.Validator(net, vset, batch=2)
    seen = []
    hook = net.register_forward_pre_hook(lambda mod, args: seen.append(args[1].clone()))
    rng = C._rng_states("cuda")
    result, restored = val.run(return_restored=True)
    hook.remove()
    return dict(net=net, vset=vset, val=val, result=result, restored=restored, table=R.bits(val.last_table), seen=seen,
                training=net.training, rng_same=all(torch.equal(a, b) for a, b in zip(rng, C._rng_states("cuda"))))


def test_validator_equals_compute_quality_image_by_image(tiny):
    """per mode psnr, ssim, sam: both sides are float64 sums of at most 5 * 8 values of one magnitude in another order, so they agree to a
    few n 2^-53 -- the bar is 1e-12 relative; counts exactly.  Mode 10 scores the completed bands only (compute_quality's `degraded`)."""
    from mp_hsir_amd import metrics
    vset, result, restored = tiny["vset"], tiny["result"], tiny["restored"]
    for m in vset.modes:
        per = [metrics.compute_quality(restored[m][i:i + 1], vset.clean[i:i + 1], vset.degraded[m][i:i + 1] if m == 10 else None) for i in range(len(vset))]
        counted = [q for q in per if q["count"] > 0]
        assert result[m]["n"] == len(counted) and result[m]["skipped"] == len(per) - len(counted) and result[m]["nonfinite"] == 0
        assert result[m]["n"] > 0
        for key in ("psnr", "ssim", "sam"):
            want = float(np.mean(np.array([q[key] for q in counted], dtype=np.float64)))
            print("mode %d %s validator %.17g image by image %.17g rel %.3g" % (m, key, result[m][key], want, abs(result[m][key] - want) / abs(want)))
            assert abs(result[m][key] - want) <= 1e-12 * abs(want)
    assert result[10]["n"] == 5 and int(vset.use[10].sum()) == 5 * int(0.3 * 8), "mode 10 masks int(0.3 * 8) = 2 bands of every crop"
    means = [result[m]["psnr"] for m in vset.modes]
    assert result["mean"]["psnr"] == sum(means) / 3 and result["mean"]["modes"] == list(vset.modes) and result["mean"]["left_out"] == []


def test_validator_two_passes_are_bitwise_equal(tiny):
    tiny["val"].run()
    assert R.bits(tiny["val"].last_table) == tiny["table"]


def test_validator_batches_hold_one_mode_and_nothing_else_changes(tiny):
    seen = tiny["seen"]
    assert len(seen) == 9 and all(p.dim() == 1 and p.numel() == 2 and len(set(p.tolist())) == 1 for p in seen), "a batch mixed prompt ids"
    assert [int(p[0]) for p in seen] == [0] * 3 + [2] * 3 + [5] * 3            # modes 0, 5, 10: prompt ids 0, 2, 5
    assert tiny["training"] is True and tiny["rng_same"]


def test_validator_at_batch_1_equals_test_py(tmp_path):
    """mode 0 over three cubes written as .npy files of exactly the crop size: test.evaluate_quality with --fused_degrade 1 --quality fused
    makes the same launches on the same inputs (its SceneDegrader is seeded with --seed + 1, hence val seed = seed + 1)"""
    from mp_hsir_amd import validate
    T = importlib.import_module("mp_hsir_amd.test")
    cubes = np.random.default_rng(99).random((3, 8, 64, 64), dtype=np.float32)
    for i, c in enumerate(cubes):
        np.save(str(tmp_path / ("cube%d.npy" % i)), c)
    files = sorted(str(tmp_path / f) for f in os.listdir(tmp_path))
    net = M.build_net(TINY_CFG, "cuda", torch.float32)
    o = T.build_parser().parse_args(["--test_dir", str(tmp_path), "--mode", "0", "--fused_degrade", "1", "--quality", "fused", "--seed", "31"])
    p, s, sam, n = T.evaluate_quality(o, net, torch.device("cuda"))
    vset = validate.ValidationSet(files, "natural_scene", "cuda", modes=[0], patch=64, seed=32, net=net)
    assert vset.files == ["cube0.npy", "cube1.npy", "cube2.npy"] and torch.equal(vset.clean.cpu(), torch.from_numpy(cubes))
    r = validate.Validator(net, vset, batch=1).run()[0]
    print("validator %.17g %.17g %.17g; test.py %.17g %.17g %.17g" % (r["psnr"], r["ssim"], r["sam"], p, s, sam))
    assert r["n"] == n == 3
    for got, want in ((r["psnr"], p), (r["ssim"], s), (r["sam"], sam)):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)


# ---- training is not disturbed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_training_is_not_disturbed_by_a_pass(use_graph, dtype):
    C.check_training_undisturbed("cuda", "tiny", use_graph=use_graph, dtype=dtype)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_training_with_ema_weights_is_not_disturbed_by_a_pass(use_graph):
    C.check_training_undisturbed("cuda", "tiny", use_graph=use_graph, ema=True)


def test_ema_weights_without_an_ema_arena_stop_with_a_message():
    from mp_hsir_amd import validate
    from mp_hsir_amd.engine import DataParallelEngine
    net = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    val = validate.Validator(net, C.make_vset("cuda", "tiny", net), batch=2, engine=DataParallelEngine(net, lr=1e-3), weights="ema")
    with pytest.raises(RuntimeError, match="keeps no EMA weights"):
        val.run()
    assert net.training


def test_a_training_step_issues_the_launches_of_always():
    C.check_off_by_default("cuda", "tiny")


# ---- train.py end to end --------------------------------------------------------------------------------------------------------------------
def _train(*extra, ok=True):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "train.py"), "--epochs", "1", "--steps_per_epoch", "6",
           "--log_every", "2", "--batch_size", "4", "--patch_size", "32", "--allow_surrogate_clip", "1", "--data_type", "natural_scene"] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout, r.stderr


VAL_MODE = r"^val epoch (\d+) mode (\d+) psnr (\S+) ssim (\S+) sam (\S+) n (\d+)( nonfinite \d+)?$"
VAL_MEAN = r"^val epoch (\d+) mean psnr (\S+) ssim (\S+) sam (\S+)$"


def test_train_py_validates_keeps_the_best_and_resumes(tmp_path):
    cubes = tmp_path / "held_out"
    cubes.mkdir()
    for i in range(3):
        np.save(str(cubes / ("scene%d.npy" % i)), np.random.default_rng(70 + i).random((31, 64, 64), dtype=np.float32))
    ckpts = str(tmp_path / "ckpt")
    flags = ["--val_dir", str(cubes), "--val_every", "1", "--val_patch", "64", "--val_batch", "2", "--val_modes", "0,8", "--save_best", "1", "--ckpt_dir", ckpts]
    out, _ = _train(*flags)
    lines = out.splitlines()
    modes = [m.groups() for m in (re.match(VAL_MODE, ln) for ln in lines) if m]
    mean = [m.groups() for m in (re.match(VAL_MEAN, ln) for ln in lines) if m]
    print(modes, mean)
    assert [(e, m, n) for e, m, _, _, _, n, _ in modes] == [("0", "0", "3"), ("0", "8", "3")] and len(mean) == 1 and mean[0][0] == "0", out[-2000:]
    assert all(math.isfinite(float(v)) for row in modes for v in row[2:5]) and all(math.isfinite(float(v)) for v in mean[0][1:])
    assert lines.index("val epoch 0 mean psnr %s ssim %s sam %s" % mean[0][1:]) > max(i for i, ln in enumerate(lines) if ln.startswith("epoch 0 it "))
    best = os.path.join(ckpts, "best.ckpt")
    assert os.path.exists(best)
    ck = torch.load(best, map_location="cpu")
    val = ck["mphsir_val"]
    assert val["protocol"] == {"modes": [0, 8], "patch": 64, "crops": 1, "seed": 2025, "weights": "auto", "files": ["scene0.npy", "scene1.npy", "scene2.npy"]}
    assert len(val["history"]) == 1 and val["history"][0]["epoch"] == 0 and val["best"]["epoch"] == 0 and ck["epoch"] == 0
    assert abs(val["best"]["psnr"] - float(mean[0][1])) < 1e-4
    out2, _ = _train(*flags, "--ckpt_path", best, "--resume", "1", "--epochs", "2")
    assert "validation: 1 earlier passes restored, best mean psnr %.4f at epoch 0" % val["best"]["psnr"] in out2, out2[-2000:]
    mean2 = [m.groups() for m in (re.match(VAL_MEAN, ln) for ln in out2.splitlines()) if m]
    assert "another protocol" not in out2 and len(mean2) == 1 and mean2[0][0] == "1", out2[-2000:]
    again = torch.load(best, map_location="cpu")["mphsir_val"]
    if float(mean2[0][1]) > val["best"]["psnr"] + 1e-3:                        # epoch 1 improved on the restored best: best.ckpt is epoch 1's
        assert [row["epoch"] for row in again["history"]] == [0, 1] and again["best"]["epoch"] == 1
    elif float(mean2[0][1]) < val["best"]["psnr"] - 1e-3:                      # it did not: the restored best stands and the file is untouched
        assert [row["epoch"] for row in again["history"]] == [0] and again["best"] == val["best"]


def test_train_py_without_the_flags_prints_what_it_always_printed():
    out, _ = _train()
    lines = out.splitlines()
    assert not any(ln.startswith("val ") for ln in lines)
    assert len([ln for ln in lines if re.match(r"^epoch \d+ it \d+ lr \S+ train_loss (\S+)$", ln)]) == 3 and \
        all(re.match(r"^epoch \d+ it \d+ lr \S+ train_loss (\S+)$", ln) for ln in lines if ln.startswith("epoch ")), out[-2000:]


def test_train_py_val_every_without_val_dir_ends_with_a_message():
    out, err = _train("--val_every", "1", ok=False)
    assert "--val_every 1 needs --val_dir" in err and not any(ln.startswith("epoch ") for ln in out.splitlines())
