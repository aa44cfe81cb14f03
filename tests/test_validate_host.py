"""In-training validation without a GPU: the host logic of mp-hsir_amd/validate.py (crop placement, refusals by name, the best-checkpoint
rule, the protocol note of --resume, the sharding rule, the flags), and the pass itself on the two-convolution network of
tests/optim_ex_ref.py through the emulated kernels: one process against metrics.compute_quality image by image, and two gloo ranks
against one."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def V():
    from mp_hsir_amd import validate
    return validate


# ---- crop placement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (100, 70), (130, 64)])
@pytest.mark.parametrize("k", [1, 2])
def test_crop_placement(H, W, k):
    P = 64
    got = V().crop_origins(H, W, P, k * k)
    ys = [(H - P) // 2] if k == 1 else [(H - P) * j // (k - 1) for j in range(k)]
    xs = [(W - P) // 2] if k == 1 else [(W - P) * i // (k - 1) for i in range(k)]
    assert got == [(y, x) for y in ys for x in xs]
    assert all(0 <= y <= H - P and 0 <= x <= W - P for y, x in got)
    if k == 2:
        assert got[0] == (0, 0) and got[-1] == (H - P, W - P)          # the grid reaches both edges


def test_crop_placement_refusals():
    with pytest.raises(ValueError, match="square"):
        V().crop_origins(128, 128, 64, 3)
    with pytest.raises(ValueError, match="smaller than the 64 x 64 crop"):
        V().crop_origins(63, 128, 64, 1)


# ---- refusals by name -----------------------------------------------------------------------------------------------------------------------
def _cube(tmp_path, name, shape):
    path = str(tmp_path / name)
    np.save(path, np.random.default_rng(1).random(shape, dtype=np.float32))
    return path


def test_set_refuses_by_name(tmp_path):
    v = V()
    with pytest.raises(ValueError, match="multiple of 64"):
        v.ValidationSet([], "natural_scene", "cpu", modes=[0], patch=96)
    with pytest.raises(ValueError, match=r"cube bands30\.npy has shape \(30, 64, 64\), the model takes 31 bands"):
        v.ValidationSet([_cube(tmp_path, "bands30.npy", (30, 64, 64))], "natural_scene", "cpu", modes=[0], patch=64)
    with pytest.raises(ValueError, match=r"cube small\.npy: a cube of 64 x 100 is smaller than the 128 x 128 crop"):
        v.ValidationSet([_cube(tmp_path, "small.npy", (31, 64, 100))], "natural_scene", "cpu", modes=[0], patch=128)
    for mode, word in ((11, "Poisson"), (12, "real degraded"), (13, "CASSI")):
        with pytest.raises(ValueError, match="mode %d .*%s" % (mode, word)):
            v.check_modes([0, mode])
    with pytest.raises(ValueError, match="unknown mode 14"):
        v.check_modes([14])
    with pytest.raises(ValueError, match="no cube"):
        v.ValidationSet([], "natural_scene", "cpu", modes=[0], patch=64)


def test_default_modes_are_those_whose_prompt_id_the_net_has():
    v = V()
    assert v.default_modes("natural_scene", 6) == tuple(range(11))
    assert v.default_modes("remote_sensing", 7) == tuple(range(11))
    assert v.default_modes("remote_sensing", 6) == tuple(range(10))        # mode 10 is prompt id 6 there
    assert v.default_modes("natural_scene", 1) == (0, 6)


# ---- best tracking, protocol, sharding --------------------------------------------------------------------------------------------------------
def _result(psnr, nonfinite=0, n=3):
    rows = [[n, psnr * n, 0.9 * n, 2.0 * n, nonfinite, psnr - 1, psnr + 1, 0], [n, (psnr + 2) * n, 0.8 * n, 3.0 * n, 0, psnr, psnr + 3, 0]]
    return V().summarise(rows, (0, 5))


def test_summarise_and_the_best_rule():
    v = V()
    r = _result(30.0)
    assert r[0]["psnr"] == 30.0 and r[5]["psnr"] == 32.0 and r["mean"]["psnr"] == 31.0 and r["mean"]["modes"] == [0, 5] and r["mean"]["left_out"] == []
    assert r[0]["n"] == 3 and r[0]["psnr_min"] == 29.0 and r[5]["psnr_max"] == 33.0
    h = v.History({"seed": 1})
    assert h.add(0, r) and h.best["epoch"] == 0
    assert not h.add(1, _result(29.0)) and h.best["epoch"] == 0
    assert not h.add(2, _result(40.0, nonfinite=1)) and h.best["epoch"] == 0, "an epoch with a non-finite image became best"
    assert h.add(3, _result(30.5)) and h.best == dict(epoch=3, psnr=31.5, ssim=pytest.approx(0.85), sam=2.5)
    assert [row["epoch"] for row in h.rows] == [0, 1, 2, 3] and h.rows[2]["nonfinite"] == 1
    # a mode in which nothing was scored is left out of the mean, and the result says so; with nothing scored at all nothing becomes best
    r = v.summarise([[2, 60.0, 1.8, 4.0, 0, 29.0, 31.0, 0], [0, 0, 0, 0, 0, math.inf, -math.inf, 2]], (0, 10))
    assert r["mean"]["psnr"] == 30.0 and r["mean"]["modes"] == [0] and r["mean"]["left_out"] == [10] and r[10]["n"] == 0 and r[10]["skipped"] == 2
    assert math.isnan(r[10]["psnr"])
    none = v.summarise([[0, 0, 0, 0, 0, math.inf, -math.inf, 2]], (10,))
    assert not v.improves(none, None) and math.isnan(none["mean"]["psnr"])
    lines = v.result_lines(4, _result(30.0, nonfinite=2))
    assert lines[0] == "val epoch 4 mode 0 psnr 30.0000 ssim 0.90000 sam 2.0000 n 3 nonfinite 2"
    assert lines[1] == "val epoch 4 mode 5 psnr 32.0000 ssim 0.80000 sam 3.0000 n 3" and lines[2] == "val epoch 4 mean psnr 31.0000 ssim 0.85000 sam 2.5000"


def test_protocol_change_on_resume():
    v = V()
    proto = {"modes": [0, 8], "patch": 64, "crops": 1, "seed": 5, "weights": "auto", "files": ["a.npy"]}
    h = v.History(proto)
    h.add(0, _result(30.0))
    state = h.state()
    same = v.History(dict(proto))
    assert same.restore(state) is None and same.best == h.best and len(same.rows) == 1
    other = v.History(dict(proto, seed=6, patch=128))
    note = other.restore(state)
    assert note == "note: the checkpoint was validated under another protocol (patch, seed differ): its history is kept, the best starts anew"
    assert other.best is None and len(other.rows) == 1
    assert other.add(1, _result(20.0)), "after a protocol change the first pass is the best"


def test_sharding_rule():
    v = V()
    for n, world in ((5, 2), (8, 3), (2, 4), (0, 2)):
        parts = [v.shard(n, world, r) for r in range(world)]
        assert all(i % world == r for r, p in enumerate(parts) for i in p)
        assert sorted(i for p in parts for i in p) == list(range(n))


def test_flags():
    from mp_hsir_amd.options import build_parser
    o = build_parser().parse_args([])
    assert (o.val_dir, o.val_every, o.val_patch, o.val_crops, o.val_batch, o.val_modes, o.val_weights, o.save_best) == ("", 0, 256, 1, 4, "", "auto", 0)
    o = build_parser().parse_args(["--val_dir", "d", "--val_every", "2", "--val_modes", "0,5,7", "--val_weights", "ema", "--save_best", "1", "--val_seed", "9"])
    assert (o.val_dir, o.val_every, o.val_modes, o.val_weights, o.save_best, o.val_seed) == ("d", 2, "0,5,7", "ema", 1, 9)


# ---- the pass through the emulated kernels --------------------------------------------------------------------------------------------------
def _spawn(out, world, port=29547):
    worker = os.path.join(ROOT, "tests", "validate_dist_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, worker, out], env=dict(env, RANK=str(r))) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    return [torch.load(out + str(r)) for r in range(world)]


def test_one_process_equals_compute_quality_image_by_image():
    import validate_dist_worker as W
    from mp_hsir_amd import metrics
    net, vset, val = W.build(False)
    was = net.training
    seen = []
    hook = net.register_forward_pre_hook(lambda mod, args: seen.append(args[1].clone()))
    rng = torch.get_rng_state()
    result, restored = val.run(return_restored=True)
    hook.remove()
    assert net.training == was and torch.equal(torch.get_rng_state(), rng)
    assert all(p.dim() == 1 and len(set(p.tolist())) == 1 for p in seen), "a batch mixed prompt ids"
    assert [int(p[0]) for p in seen] == [0] * 3 + [4] * 3 + [5] * 3          # 5 crops in batches of 2: three forwards per mode
    for m in (0, 8):
        per = [metrics.compute_quality(restored[m][i:i + 1], vset.clean[i:i + 1]) for i in range(5)]
        for key in ("psnr", "ssim", "sam"):
            want = float(np.mean(np.array([q[key] for q in per], dtype=np.float64)))
            assert abs(result[m][key] - want) <= 1e-12 * abs(want), (m, key, result[m][key], want)
        assert result[m]["n"] == 5 and result[m]["nonfinite"] == 0 and result[m]["skipped"] == 0
        assert result[m]["psnr_min"] <= result[m]["psnr"] <= result[m]["psnr_max"]
    assert result[10]["n"] == 0 and result[10]["skipped"] == 5 and result["mean"]["left_out"] == [10] and result["mean"]["modes"] == [0, 8]
    assert result["mean"]["psnr"] == (result[0]["psnr"] + result[8]["psnr"]) / 2
    first = val.last_table.numpy().tobytes()
    val.run()
    assert val.last_table.numpy().tobytes() == first, "two passes over unchanged weights differ"


def test_two_ranks_return_what_one_returns(tmp_path):
    one = _spawn(str(tmp_path / "one"), 1, port=29547)[0]
    two = _spawn(str(tmp_path / "two"), 2, port=29548)
    assert repr(two[0]["result"]) == repr(two[1]["result"]) and torch.equal(two[0]["table"], two[1]["table"])      # repr: a mode left out holds NaN means
    a, b = one["table"], two[0]["table"]
    for slot in (0, 4, 7, 5, 6):                                     # counts, min and max: exactly
        assert torch.equal(a[:, slot], b[:, slot]), (slot, a[:, slot], b[:, slot])
    for slot in (1, 2, 3):                                           # the sums: the ranks' partial sums are added in another order
        assert bool(((a[:, slot] - b[:, slot]).abs() <= 1e-12 * a[:, slot].abs()).all()), (slot, a[:, slot], b[:, slot])
    assert one["result"]["mean"]["left_out"] == [10] and int(a[0, 0]) == 5


@pytest.mark.parametrize("ema", [False, True], ids=["raw", "ema"])
def test_training_is_not_disturbed_by_a_pass(ema):
    """eager steps of the two-convolution network through the emulated optimizer kernels (the tiny net, graph mode and bf16: the GPU tests)"""
    from emu import bind_emulator
    bind_emulator()
    import validate_checks as C
    C.check_training_undisturbed("cpu", kind="conv", ema=ema)


def test_a_training_step_issues_the_launches_of_always():
    from emu import bind_emulator
    bind_emulator()
    import validate_checks as C
    C.check_off_by_default("cpu", kind="conv")
