"""Spectral windows on a real MI355X: the band gather / blend kernels (the checks of tests/test_scene_bands_emu.py, device = cuda, plus
the two sensor-sized shapes), SceneRestorer(bands=...) over callables and over the full-width network, and test.py end to end on cubes
whose band count is not the model's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import model_checks as M
import scene_bands_checks as K
import scene_bands_ref as B
from golden.cases import NATURAL_CFG
from util import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = B.SHAPES + B.GPU_SHAPES
IDS = ["-".join(map(str, s)) for s in ALL]


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_gather_is_a_bitwise_copy(shape):
    K.check_gather("cuda", shape, all_modes=shape != B.GPU_SHAPES[1])      # 48 items of 31 x 256 x 256: the plain cut (eight times that is seconds of numpy)


def test_gather_any_origin_repeats_and_tail():
    K.check_gather_any_origin("cuda")


@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_blend_matches_the_definition(shape):
    K.check_blend("cuda", shape)


@pytest.mark.parametrize("shape", ALL, ids=IDS)
def test_round_trip_and_padding_never_leaks(shape):
    K.check_round_trip("cuda", shape)


def test_one_window_is_the_old_path_bitwise():
    K.check_one_window_is_the_old_path("cuda", B.SHAPES[6])
    K.check_same_launches_with_bands_set("cuda", B.SHAPES[6])


@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("shape", [B.SHAPES[0], B.SHAPES[2], B.SHAPES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_restorer_with_identity_callable_returns_the_scene(shape, G):
    K.check_restorer_identity("cuda", shape, G, 5)


@pytest.mark.parametrize("shape,G", [(B.SHAPES[0], 1), (B.SHAPES[1], 4), (B.SHAPES[2], 8), (B.SHAPES[3], 4), (B.SHAPES[4], 1)])
def test_restorer_with_a_band_dependent_callable(shape, G):
    K.check_restorer_band_dependent("cuda", shape, G, 4)


@pytest.mark.parametrize("G", [1, 4])
def test_restorer_does_not_depend_on_tile_batch(G):
    K.check_restorer_batch_sizes("cuda", B.SHAPES[1], G)


def _noisy_scene(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((C, H, W), generator=g) + torch.randn((C, H, W), generator=g) * (70.0 / 255.0)).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batched_items_against_batch_1_forwards(dtype):
    """45 x 70 x 100 under the 31-band network, tile 64 / overlap 16 / tile_batch 4: band origins [0, 14] x 2 x 2 tiles = 8 items, 2
    forwards.  Each restored item against the batch-1 forward of the same gathered item, under the bars of tests/test_scene_gpu.py's T6:
    fp32 the project's parity bound, 1e-3 relative L2; bf16 at most 1.5 x the yardstick net(x.repeat(4,1,1,1))[0] against net(x)[0] on the
    first item, what the network itself does across batch sizes without any of the scene code."""
    from mp_hsir_amd import ops
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(NATURAL_CFG, "cuda", dtype)
    scene = _noisy_scene(45, 70, 100, 4)
    r = SceneRestorer(net, tile=64, overlap=16, tile_batch=4, graphed=False)
    assert (r.bands, r.band_overlap) == (31, 7)
    th, tw, ob, oy, ox, origins3 = B.plan(45, 70, 100, 31, 64, 16, 7)
    assert r.plan_bands(45) == ob == [0, 14] and len(origins3) == 8
    restored, store = r(scene, 0, return_tiles=True)
    assert restored.shape == scene.shape and restored.dtype == torch.float32 and torch.isfinite(restored).all() and store.shape == (8, 31, 64, 64)
    xs = ops.scene_gather_bands(scene, torch.tensor(origins3, dtype=torch.int32, device="cuda"), 31, 64, 64, 0, (0,),
                                torch.empty((8, 31, 64, 64), device="cuda"))
    ids1 = torch.zeros(1, dtype=torch.long, device="cuda")
    with torch.no_grad():
        singles = [net(xs[s:s + 1], ids1)[0] for s in range(8)]
        yard = rel_l2(net(xs[:1].repeat(4, 1, 1, 1), ids1.repeat(4))[0].cpu(), singles[0].cpu())
    devs = [rel_l2(store[s].cpu(), singles[s].cpu()) for s in range(8)]
    print("band items %s: per-item rel-L2 vs batch-1 forwards %s; batch-4-of-one-item vs batch-1 yardstick %.3g"
          % (str(dtype).split(".")[1], ["%.3g" % d for d in devs], yard))
    if dtype == torch.float32:
        assert max(devs) <= 1e-3
    else:
        assert max(devs) <= 1.5 * yard
    want, _ = B.blend(store.cpu().numpy(), ob, oy, ox, 16, 7, 45, 70, 100)
    assert np.abs(restored.cpu().numpy().astype(np.float64) - want).max() <= B.BLEND_TOL * max(1.0, float(store.abs().max()))


def _run_test_py(args, cwd):
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "test.py")] + args
    return subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)


def test_test_py_restores_cubes_of_another_band_count(tmp_path):
    """two 45 x 100 x 130 cubes under the 31-band model: --tile keeps them whole; without --tile the 64 x 128 crop is one spatial tile;
    mode 13 ends with a message"""
    cubes = tmp_path / "cubes"
    cubes.mkdir()
    rng = np.random.default_rng(5)
    for name in ("a", "b"):
        np.save(cubes / (name + ".npy"), rng.random((45, 100, 130), dtype=np.float32))
    common = ["--test_dir", str(cubes), "--allow_surrogate_clip", "1", "--mode", "0", "--save_restored", "1"]
    for extra, out, shape in ((["--tile", "64", "--tile_overlap", "16"], "out", (45, 100, 130)), ([], "out_crop", (45, 64, 128))):
        r = _run_test_py(common + extra + ["--output_path", str(tmp_path / out)], str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if " psnr " in ln and " ssim " in ln]
        assert len(lines) == 2 and lines[0].startswith("a ") and lines[1].startswith("b "), r.stdout
        saved = sorted((tmp_path / out).rglob("restored_*.npy"))
        assert [s.name for s in saved] == ["restored_a.npy", "restored_b.npy"]
        for s in saved:
            a = np.load(s)
            assert a.shape == shape and a.dtype == np.float32 and np.isfinite(a).all()
    r = _run_test_py(["--test_dir", str(cubes), "--allow_surrogate_clip", "1", "--mode", "13", "--task_classes", "1", "--tile", "64",
                      "--output_path", str(tmp_path / "out_13")], str(tmp_path))
    assert r.returncode != 0 and "Traceback" not in r.stderr and "mode 13" in r.stderr, r.stderr[-2000:]
