"""Self-ensemble on a real MI355X: the d4 gather / fold kernels at scene sizes against tests/ensemble_ref.py, SceneRestorer(ensemble=8)
over the full-width network against batch-1 forwards of the transformed scene, and test.py --ensemble end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ensemble_ref as E
import model_checks as M
import scene_ref as R
from golden.cases import NATURAL_CFG
from util import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, OV = 256, 32
# (C, H, W, modes): two unpadded scenes under all eight transforms; a padded, non-square scene (200 -> 256 rows) under the four flips
CASES = [(31, 1000, 700, E.MODES8), (100, 307, 1280, E.MODES8), (31, 200, 1001, E.MODES4)]


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
    return th, tw, [(y, x) for y in oy for x in ox]


@pytest.mark.parametrize("C,H,W,modes", CASES)
def test_gather_d4_is_a_bitwise_copy(C, H, W, modes):
    """batches of n + 1 items start in the middle of a pass.  A SAMPLE of them is compared, to keep the GPU suite light: every second
    batch (each spans two passes, so all passes are met) and the last, whose tail repeats the last item.  Every batch of every geometry
    is walked on the emulator (tests/test_ensemble_emu.py)."""
    from mp_hsir_amd import ops
    th, tw, origins = _plan(H, W)
    n, G = len(origins), len(modes)
    scene = torch.from_numpy(np.random.default_rng(0).random((C, H, W), dtype=np.float32))
    sd, od = scene.cuda(), _i32(origins)
    B = n + 1
    starts = list(range(0, n * G, B))
    assert (n * G) % B != 0
    out = torch.empty((B, C, th, tw), device="cuda")
    for j0 in starts[::2] + [starts[-1]]:
        out.fill_(float("nan"))
        ops.scene_gather_d4(sd, od, th, tw, j0, modes, out=out)
        assert np.array_equal(out.cpu().numpy(), E.gather_d4(scene.numpy(), origins, th, tw, j0, B, modes)), "batch at item %d" % j0


@pytest.mark.parametrize("C,H,W,modes", CASES)
def test_fold_d4_is_the_mean_whatever_the_batch_size(C, H, W, modes):
    """random y in [0, 2) for all G * n items; walked in batches of 16, n + 2 and 1 the store is bitwise the same, and the first, a middle
    and the last tile are within (G - 1) * 2^-24 * max|y| of the fp64 mean (G - 1 fp32 additions, an exact scaling)"""
    from mp_hsir_amd import ops
    th, tw, origins = _plan(H, W)
    n, G = len(origins), len(modes)
    y = torch.rand((G * n, C, th, tw), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 2
    stores = []
    for B in (16, n + 2, 1):
        store = torch.full((n, C, th, tw), float("nan"), device="cuda")
        for j0 in range(0, G * n, B):
            cnt = min(B, G * n - j0)
            ops.scene_fold_d4(y[j0:j0 + cnt], store, j0, cnt, modes)
        stores.append(store)
    assert torch.equal(stores[0], stores[1]) and torch.equal(stores[0], stores[2]), "the fold depends on the batch size"
    bound = (G - 1) * 2.0 ** -24 * float(y.max())
    for t in (0, n // 2, n - 1):
        want = sum(E.inv(y[g * n + t].cpu().numpy().astype(np.float64), modes[g]) for g in range(G)) / G
        err = np.abs(stores[0][t].cpu().numpy().astype(np.float64) - want).max()
        print("fold %s tile %d: max abs error %.3g (bound %.3g)" % ((C, H, W), t, err, bound))
        assert err <= bound
    y[n + 1, C - 1, 7, 250] = float("nan")               # pass 1 of tile 1
    store = torch.zeros((n, C, th, tw), device="cuda")
    for j0 in range(0, G * n, 16):
        cnt = min(16, G * n - j0)
        ops.scene_fold_d4(y[j0:j0 + cnt], store, j0, cnt, modes)
    bad = torch.isnan(store).nonzero().cpu().tolist()
    m = np.zeros((th, tw))
    m[7, 250] = 1
    u, v = (int(i[0]) for i in np.nonzero(E.inv(m, modes[1])))
    assert bad == [[1, C - 1, u, v]], "a NaN must poison exactly its own store element"


def _noisy_scene(C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((C, H, W), generator=g) + torch.randn((C, H, W), generator=g) * (70.0 / 255.0)).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ensemble_8_against_batch_1_forwards_of_the_transformed_scene(dtype):
    """a 256 x 256 scene is one tile: ensemble 8 with tile_batch 8 is ONE forward of the tile under its eight transforms.  Against the fp64
    mean of eight batch-1 forwards of the transformed scene, mapped back.  fp32: the project's parity bound, 1e-3 relative L2.  bf16: the
    yardstick of the tiled test (T6), what the network itself does across batch sizes without any scene code --
    net(x.repeat(8,1,1,1))[0] against net(x)[0] -- times 1.5.  Then the captured path: four calls, all equal."""
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(NATURAL_CFG, "cuda", dtype)
    scene = _noisy_scene(31, 256, 256, 3)
    ids1 = torch.ones(1, dtype=torch.long, device="cuda")
    got = SceneRestorer(net, tile_batch=8, graphed=False, ensemble=8)(scene, 1)
    assert got.shape == scene.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    acc = np.zeros((31, 256, 256))
    with torch.no_grad():
        for m in E.MODES8:
            x = torch.from_numpy(np.ascontiguousarray(E.aug(scene.cpu().numpy(), m))).cuda()
            acc += E.inv(net(x[None], ids1)[0].cpu().numpy().astype(np.float64), m)
        plain = net(scene[None], ids1)[0]
        yard = rel_l2(net(scene[None].repeat(8, 1, 1, 1), ids1.repeat(8))[0].cpu(), plain.cpu())
    dev = rel_l2(got.cpu(), torch.from_numpy(acc / 8).float())
    print("ensemble 8 %s: rel-L2 vs the mean of eight batch-1 forwards %.3g; batch-8-of-one-cube vs batch-1 yardstick %.3g; the ensemble differs "
          "from one forward by %.3g" % (str(dtype).split(".")[1], dev, yard, rel_l2(got.cpu(), plain.cpu())))
    if dtype == torch.float32:
        assert dev <= 1e-3
    else:
        assert dev <= 1.5 * yard
    graphed = SceneRestorer(net, tile_batch=8, graphed=True, ensemble=8)
    outs = [graphed(scene, 1).clone() for _ in range(4)]                # two eager warm-up calls, the capture, one more replay
    assert all(torch.equal(o, outs[0]) for o in outs)
    print("captured against eager: rel-L2 %.3g" % rel_l2(outs[0].cpu(), got.cpu()))


def _run_test_py(args, cwd):
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "test.py")] + args
    return subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)


def test_test_py_ensemble_end_to_end(tmp_path):
    """two square 31 x 200 x 200 cubes: --ensemble 4 --tile 128 keeps them whole (2 x 2 tiles); --ensemble 8 without --tile restores the
    192 x 192 crop as a one-tile scene.  A 200 x 330 cube crops to 192 x 320: --ensemble 8 ends in a message."""
    cubes, wide = tmp_path / "cubes", tmp_path / "wide"
    cubes.mkdir()
    wide.mkdir()
    rng = np.random.default_rng(5)
    for name in ("a", "b"):
        np.save(cubes / (name + ".npy"), rng.random((31, 200, 200), dtype=np.float32))
    np.save(wide / "w.npy", rng.random((31, 200, 330), dtype=np.float32))
    common = ["--allow_surrogate_clip", "1", "--mode", "0", "--save_restored", "1"]
    for args, out, shape in ((["--ensemble", "4", "--tile", "128"], "out_tiled", (31, 200, 200)), (["--ensemble", "8"], "out_crop", (31, 192, 192))):
        r = _run_test_py(common + args + ["--test_dir", str(cubes), "--output_path", str(tmp_path / out)], str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if " psnr " in ln and " ssim " in ln]
        assert len(lines) == 2 and lines[0].startswith("a ") and lines[1].startswith("b "), r.stdout
        saved = sorted((tmp_path / out).rglob("restored_*.npy"))
        assert [s.name for s in saved] == ["restored_a.npy", "restored_b.npy"]
        for s in saved:
            a = np.load(s)
            assert a.shape == shape and a.dtype == np.float32 and np.isfinite(a).all()
    r = _run_test_py(common + ["--ensemble", "8", "--test_dir", str(wide), "--output_path", str(tmp_path / "out_bad")], str(tmp_path))
    assert r.returncode != 0 and "Traceback" not in r.stderr and "--ensemble 4" in r.stderr, r.stderr[-2000:]
