"""Whole-scene inference on a real MI355X: the gather / blend kernels at scene sizes, SceneRestorer over the full-width network, and
test.py --tile end to end.  The kernel checks are those of tests/test_scene_emu.py, device = cuda."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import model_checks as M
import scene_ref as R
from golden.cases import NATURAL_CFG
from util import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [(31, 1000, 700), (100, 307, 1280)]
# scenes WITH mirror padding under tile 256: a padded axis beside a multi-tile axis each way round (W % 4 != 0), and both axes padded
PADDED_SCENES = [(31, 200, 1001), (100, 307, 150), (5, 70, 90)]
TILE, OV = 256, 32


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _plan(H, W):
    th, tw, oy, ox = R.plan_tiles(H, W, TILE, OV)
    return th, tw, oy, ox, [(y, x) for y in oy for x in ox]


@pytest.mark.parametrize("C,H,W", SCENES)
def test_gather_is_a_bitwise_copy(C, H, W):
    from mp_hsir_amd import ops
    th, tw, oy, ox, origins = _plan(H, W)
    scene = torch.from_numpy(np.random.default_rng(0).random((C, H, W), dtype=np.float32))
    got = ops.scene_gather_tiles(scene.cuda(), _i32(origins), th, tw).cpu().numpy()
    assert np.array_equal(got, R.gather(scene.numpy(), origins, th, tw))
    odd = [(-5, -3), (H - 10, W - 20), (-th + 1, W - 1), (H - 10, W - 20), (7, 9)]          # negative, overhanging, repeated
    got = ops.scene_gather_tiles(scene.cuda(), _i32(odd), th, tw).cpu().numpy()
    assert np.array_equal(got, R.gather(scene.numpy(), odd, th, tw))


@pytest.mark.parametrize("C,H,W", SCENES + PADDED_SCENES)
def test_blend_matches_the_definition(C, H, W):
    from mp_hsir_amd import ops
    th, tw, oy, ox, origins = _plan(H, W)
    tiles = torch.from_numpy(np.random.default_rng(1).random((len(origins), C, th, tw), dtype=np.float32))
    td = tiles.cuda()
    got = ops.scene_blend_tiles(td, _i32(oy), _i32(ox), OV, H, W)
    again = ops.scene_blend_tiles(td, _i32(oy), _i32(ox), OV, H, W)
    want, cover = R.blend(tiles.numpy(), oy, ox, OV, H, W)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print("blend %s: max abs error %.3g (bound %.3g), cover up to %d" % ((C, H, W), err, R.BLEND_TOL, cover.max()))
    assert err <= R.BLEND_TOL
    assert torch.equal(got, again), "the blend is not reproducible"


@pytest.mark.parametrize("C,H,W", SCENES + PADDED_SCENES)
def test_round_trip_and_padding_never_leaks(C, H, W):
    from mp_hsir_amd import ops
    th, tw, oy, ox, origins = _plan(H, W)
    scene = torch.from_numpy(np.random.default_rng(2).random((C, H, W), dtype=np.float32)).cuda()
    tiles = ops.scene_gather_tiles(scene, _i32(origins), th, tw)
    for t, (y, x) in enumerate(origins):
        tiles[t, :, max(H - y, 0):, :] = float("nan")
        tiles[t, :, :, max(W - x, 0):] = float("nan")
    poisoned = int(torch.isnan(tiles[:, 0]).sum())
    assert poisoned == R.padded_positions(oy, ox, th, tw, H, W)
    assert (poisoned > 0) == ((C, H, W) in PADDED_SCENES), "a padded scene must have padding to poison (and only those have)"
    back = ops.scene_blend_tiles(tiles, _i32(oy), _i32(ox), OV, H, W)
    assert torch.isfinite(back).all()
    err = float((back.double() - scene.double()).abs().max())
    print("round trip %s: %d poisoned positions per band, max abs error %.3g (bound %.3g)" % ((C, H, W), poisoned, err, R.BLEND_TOL))
    assert err <= R.BLEND_TOL
    _, cover = R.blend(np.zeros((len(origins), 1, th, tw)), oy, ox, OV, H, W)
    one = torch.from_numpy(cover == 1).cuda()
    assert one.any() and torch.equal(back[:, one], scene[:, one])


def _noisy_scene(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((C, H, W), generator=g) + torch.randn((C, H, W), generator=g) * (70.0 / 255.0)).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_tile_scene_equals_the_plain_forward_bitwise(dtype):
    """T5: a 256 x 256 scene is one unpadded tile: the restorer (eager and through the captured graph) == net(scene[None], id)"""
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(NATURAL_CFG, "cuda", dtype)
    scene = _noisy_scene(31, 256, 256, 3)
    with torch.no_grad():
        want = net(scene[None], torch.tensor([1], device="cuda"))[0]
    eager = SceneRestorer(net, graphed=False)(scene, 1)
    assert torch.equal(eager, want)
    graphed = SceneRestorer(net, graphed=True)
    outs = [graphed(scene, 1) for _ in range(4)]                # two eager warm-up calls, the capture, one more replay
    assert all(torch.equal(o, want) for o in outs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batched_tiles_against_batch_1_forwards(dtype):
    """T6: 31 x 300 x 520 under tile 256 / overlap 32 / tile_batch 4 = 2 x 3 tiles, the second batch filled by repeating the last tile.
    Each restored tile against the batch-1 forward of the same gathered tile.  fp32: the project's parity bound, 1e-3 relative L2.
    bf16: the yardstick is what the network itself does across batch sizes WITHOUT any of the scene code -- net(x.repeat(4,1,1,1))[0]
    against net(x)[0] on a 256 x 256 cube (x = the scene's first tile, so both numbers are taken on the same kind of data): the batch
    size changes which kernel forms the host picks, the only legitimate source of a difference; a tile may deviate by at most 1.5 x
    that."""
    from mp_hsir_amd import ops
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(NATURAL_CFG, "cuda", dtype)
    scene = _noisy_scene(31, 300, 520, 4)
    r = SceneRestorer(net, tile=256, overlap=32, tile_batch=4, graphed=False)
    p = r.plan(300, 520)
    assert (p.ny, p.nx, p.th, p.tw) == (2, 3, 256, 256)
    restored, tiles = r(scene, 0, return_tiles=True)
    assert restored.shape == scene.shape and restored.dtype == torch.float32 and torch.isfinite(restored).all()
    xs = ops.scene_gather_tiles(scene, _i32(p.origins), 256, 256)
    ids1 = torch.zeros(1, dtype=torch.long, device="cuda")
    with torch.no_grad():
        singles = [net(xs[t:t + 1], ids1)[0] for t in range(len(p))]
        yard = rel_l2(net(xs[:1].repeat(4, 1, 1, 1), ids1.repeat(4))[0].cpu(), singles[0].cpu())
    devs = [rel_l2(tiles[t].cpu(), singles[t].cpu()) for t in range(len(p))]
    print("T6 %s: per-tile rel-L2 vs batch-1 forwards %s; batch-4-of-one-cube vs batch-1 yardstick %.3g"
          % (str(dtype).split(".")[1], ["%.3g" % d for d in devs], yard))
    if dtype == torch.float32:
        assert max(devs) <= 1e-3
    else:
        assert max(devs) <= 1.5 * yard


def _run_test_py(args, cwd):
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "test.py")] + args
    return subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)


def test_test_py_tiles_whole_scenes_and_saves_them(tmp_path):
    """T7: two 31 x 200 x 330 cubes; --tile keeps them whole and writes them; without --tile the 192 x 320 crop is evaluated as before
    (and written too: --save_restored works either way)"""
    cubes = tmp_path / "cubes"
    cubes.mkdir()
    rng = np.random.default_rng(5)
    for name in ("a", "b"):
        np.save(cubes / (name + ".npy"), rng.random((31, 200, 330), dtype=np.float32))
    common = ["--test_dir", str(cubes), "--allow_surrogate_clip", "1", "--mode", "0", "--save_restored", "1"]
    r = _run_test_py(common + ["--tile", "128", "--tile_overlap", "16", "--output_path", str(tmp_path / "out")], str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if " psnr " in ln and " ssim " in ln]
    assert len(lines) == 2 and lines[0].startswith("a ") and lines[1].startswith("b "), r.stdout
    saved = sorted((tmp_path / "out").rglob("restored_*.npy"))
    assert [s.name for s in saved] == ["restored_a.npy", "restored_b.npy"]
    for s in saved:
        a = np.load(s)
        assert a.shape == (31, 200, 330) and a.dtype == np.float32 and np.isfinite(a).all()
    r = _run_test_py(common + ["--output_path", str(tmp_path / "out_crop")], str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert len([ln for ln in r.stdout.splitlines() if " psnr " in ln and " ssim " in ln]) == 2
    saved = sorted((tmp_path / "out_crop").rglob("restored_*.npy"))
    assert [s.name for s in saved] == ["restored_a.npy", "restored_b.npy"]
    for s in saved:
        a = np.load(s)
        assert a.shape == (31, 192, 320) and a.dtype == np.float32 and np.isfinite(a).all()
    r = _run_test_py(common + ["--tile", "100", "--output_path", str(tmp_path / "out_bad")], str(tmp_path))      # a user error ends in a message
    assert r.returncode != 0 and "Traceback" not in r.stderr and "multiple of 64" in r.stderr
