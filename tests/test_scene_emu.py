"""Whole-scene inference on the CPU: the gather / blend kernels of mp-hsir_amd/csrc/scene.hip through the emulated build against the
fp64 restatement in tests/scene_ref.py, and SceneRestorer over the tiny emulated network (slow fibers: nothing larger than a batch of
four 32x32 tiles goes through the network)."""
import numpy as np
import pytest
import torch

import model_checks as M
import scene_ref as R
from emu import bind_emulator
from golden.cases import TINY_CFG
from util import rel_l2


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


def _scene(C, H, W, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).random((C, H, W), dtype=np.float32))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


@pytest.mark.parametrize("C", [1, 5, 31])
@pytest.mark.parametrize("H,W,T,ov", R.SMALL_SHAPES)
def test_gather_is_a_bitwise_copy(C, H, W, T, ov):
    from mp_hsir_amd import ops
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    origins = [(y, x) for y in oy for x in ox]
    scene = _scene(C, H, W)
    got = ops.scene_gather_tiles(scene, _i32(origins), th, tw)
    assert np.array_equal(got.numpy(), R.gather(scene.numpy(), origins, th, tw))


def test_gather_any_origin_and_repeats():
    """negative, overhanging (folded more than once: the tile is larger than the scene) and repeated origins"""
    from mp_hsir_amd import ops
    scene = _scene(5, 37, 45, 1)
    origins = [(-5, -3), (0, 0), (20, 30), (-31, 44), (36, -44), (20, 30), (20, 30), (-64, 90), (3, 7)]
    got = ops.scene_gather_tiles(scene, _i32(origins), 64, 32)
    assert np.array_equal(got.numpy(), R.gather(scene.numpy(), origins, 64, 32))


# (125,125,64,32): up to 3 x 3 tiles over a pixel, as (500,500,256,128) scaled down; PADDED_SHAPES: the geometries that have mirror padding
BLEND_SHAPES = R.SMALL_SHAPES + [(125, 125, 64, 32)] + R.PADDED_SHAPES


@pytest.mark.parametrize("C", [1, 5, 31])
@pytest.mark.parametrize("H,W,T,ov", BLEND_SHAPES)
def test_blend_matches_the_definition(C, H, W, T, ov):
    from mp_hsir_amd import ops
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    tiles = torch.from_numpy(np.random.default_rng(2).random((len(oy) * len(ox), C, th, tw), dtype=np.float32))
    got = ops.scene_blend_tiles(tiles, _i32(oy), _i32(ox), ov, H, W)
    want, cover = R.blend(tiles.numpy(), oy, ox, ov, H, W)
    if (H, W, T, ov) == (125, 125, 64, 32):
        assert cover.max() == 9
    err = np.abs(got.numpy().astype(np.float64) - want).max()
    print("blend %s C=%d: max abs error %.3g (bound %.3g), cover up to %d" % ((H, W, T, ov), C, err, R.BLEND_TOL, cover.max()))
    assert err <= R.BLEND_TOL
    again = ops.scene_blend_tiles(tiles, _i32(oy), _i32(ox), ov, H, W)
    assert np.array_equal(got.numpy(), again.numpy()), "the blend is not reproducible"
    clamped = ops.scene_blend_tiles(tiles * 3 - 1, _i32(oy), _i32(ox), ov, H, W, clamp01=True)
    assert float(clamped.min()) >= 0.0 and float(clamped.max()) <= 1.0 and float(clamped.max()) == 1.0


@pytest.mark.parametrize("H,W,T,ov", BLEND_SHAPES)
def test_round_trip_and_padding_never_leaks(H, W, T, ov):
    from mp_hsir_amd import ops
    C = 5
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    origins = [(y, x) for y in oy for x in ox]
    scene = _scene(C, H, W, 3)
    tiles = ops.scene_gather_tiles(scene, _i32(origins), th, tw)
    for t, (y, x) in enumerate(origins):                  # whatever lies outside the scene must never be read
        tiles[t, :, max(H - y, 0):, :] = float("nan")
        tiles[t, :, :, max(W - x, 0):] = float("nan")
    poisoned = int(torch.isnan(tiles[:, 0]).sum())
    assert poisoned == R.padded_positions(oy, ox, th, tw, H, W)
    assert (poisoned > 0) == ((H, W, T, ov) in R.PADDED_SHAPES), "a padded geometry must have padding to poison (and only those have)"
    back = ops.scene_blend_tiles(tiles, _i32(oy), _i32(ox), ov, H, W)
    assert torch.isfinite(back).all()
    _, cover = R.blend(np.zeros((len(origins), 1, th, tw)), oy, ox, ov, H, W)
    assert np.abs(back.numpy().astype(np.float64) - scene.numpy()).max() <= R.BLEND_TOL
    one = torch.from_numpy(cover == 1)
    assert one.any() and torch.equal(back[:, one], scene[:, one]), "a pixel under one tile must come back exactly"


def test_entry_points_refuse_bad_sizes():
    from mp_hsir_amd import ops
    scene = _scene(2, 40, 40)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.scene_gather_tiles(scene, _i32([(0, 0)]), 30, 32)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.scene_blend_tiles(torch.zeros(1, 2, 32, 30), _i32([0]), _i32([0]), 0, 32, 30)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.scene_blend_tiles(torch.zeros(1, 2, 32, 32), _i32([0]), _i32([0]), -1, 32, 32)


# ---- SceneRestorer ---------------------------------------------------------------------------------------------------------------------

def test_restorer_with_identity_network_returns_the_scene():
    """no network: a 70 x 200 scene under tile 128 is one mirror-padded tile (70 -> 128) by three tiles"""
    from mp_hsir_amd.scene import SceneRestorer
    scene = _scene(5, 70, 200, 4)
    r = SceneRestorer(lambda x, ids: x, tile=128, overlap=32, tile_batch=2)
    p = r.plan(70, 200)
    assert (p.th, p.tw, p.ny) == (128, 128, 1) and p.nx >= 2
    back, tiles = r(scene, 0, return_tiles=True)
    assert back.shape == scene.shape and tiles.shape == (len(p), 5, 128, 128)
    assert np.abs(back.numpy().astype(np.float64) - scene.numpy()).max() <= R.BLEND_TOL
    assert r(scene[None], torch.tensor([3])).shape == (1, 5, 70, 200)


def test_restorer_refuses_more_than_one_task_id():
    from mp_hsir_amd.scene import SceneRestorer
    r = SceneRestorer(lambda x, ids: x, tile=64, overlap=16)
    with pytest.raises(ValueError, match="one task id"):
        r(_scene(2, 64, 64), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        SceneRestorer(lambda x, ids: x, tile=96, overlap=16)
    with pytest.raises(ValueError):
        SceneRestorer(lambda x, ids: x, tile=64, overlap=40)
    with pytest.raises(ValueError):
        r(_scene(2, 64, 64).double(), 0)


def test_restorer_one_tile_equals_the_plain_forward_bitwise():
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(TINY_CFG, "cpu")
    scene = _scene(8, 32, 32, 5)
    with torch.no_grad():
        want = net(scene[None], torch.tensor([2]))
    got = SceneRestorer(net, tile=32, overlap=0, tile_batch=4, graphed=False, grain=32)(scene, 2)
    assert torch.equal(got, want[0])


def test_restorer_batched_tiles_equal_batch_1_forwards():
    """64 x 64 under tile 32 / overlap 0: four disjoint tiles in ONE batch of 4 (same task id: TVSP's map is that of a batch of 1);
    each quadrant against its own batch-1 forward at the project's fp32 parity bound (1e-3 relative L2)"""
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(TINY_CFG, "cpu")
    scene = _scene(8, 64, 64, 6)
    got = SceneRestorer(net, tile=32, overlap=0, tile_batch=4, graphed=False, grain=32)(scene, 4)
    assert got.shape == scene.shape
    for y in (0, 32):
        for x in (0, 32):
            with torch.no_grad():
                want = net(scene[None, :, y:y + 32, x:x + 32].contiguous(), torch.tensor([4]))[0]
            err = rel_l2(got[:, y:y + 32, x:x + 32], want)
            print("quadrant (%d,%d): rel-L2 %.3g" % (y, x, err))
            assert err <= 1e-3
