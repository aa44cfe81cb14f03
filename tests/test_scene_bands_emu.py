"""Spectral windows on the CPU: the band gather (mp-hsir_amd/csrc/scene_d4.hip) and the band blend (scene_bands.hip) through the emulated
build against the fp64 restatement in tests/scene_bands_ref.py, SceneRestorer(bands=...) over callables and over the tiny emulated
network (nothing larger than a batch of four 32x32 items goes through it), and the gather's LDS passes under the adversarial wave
schedules of tests/test_emu_schedules.py."""
import numpy as np
import pytest
import torch

import guard
import model_checks as M
import scene_bands_checks as K
import scene_bands_ref as B
import test_emu_schedules as S
from emu import bind_emulator
from golden.cases import TINY_CFG
from test_emu_schedules import emu  # noqa: F401  -- the fixture: the emulator bound, its schedule switch, reset at the end
from util import rel_l2

IDS = ["-".join(map(str, s)) for s in B.SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("shape", B.SHAPES, ids=IDS)
def test_gather_is_a_bitwise_copy_under_all_modes(shape):
    K.check_gather("cpu", shape)


def test_gather_any_origin_repeats_and_tail():
    K.check_gather_any_origin("cpu")


@pytest.mark.parametrize("shape", B.SHAPES, ids=IDS)
def test_blend_matches_the_definition(shape):
    K.check_blend("cpu", shape)


@pytest.mark.parametrize("shape", B.SHAPES, ids=IDS)
def test_round_trip_and_padding_never_leaks(shape):
    K.check_round_trip("cpu", shape)


def test_one_window_is_the_old_path_bitwise():
    K.check_one_window_is_the_old_path("cpu", B.SHAPES[6])
    K.check_same_launches_with_bands_set("cpu", B.SHAPES[6])


def test_entry_points_refuse_what_they_cannot_do():
    from mp_hsir_amd import ops
    scene = torch.zeros(7, 40, 72)
    o = torch.tensor([(0, 0, 0)], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="square tile"):
        ops.scene_gather_bands(scene, o, 5, 32, 64, 0, (0, 2), torch.empty(1, 5, 32, 64))
    with pytest.raises(RuntimeError, match="1, 2, 4 or 8"):
        ops.scene_gather_bands(scene, o, 5, 32, 32, 0, (0, 1, 4), torch.empty(1, 5, 32, 32))
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.scene_gather_bands(scene, o, 5, 30, 30, 0, (0,), torch.empty(1, 5, 30, 30))
    with pytest.raises(RuntimeError, match="outside"):
        ops.scene_gather_bands(scene, o, 5, 32, 32, 4, (0, 1, 4, 5), torch.empty(1, 5, 32, 32))
    z = torch.tensor([0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.scene_blend_bands(torch.zeros(1, 5, 32, 30), z, z, z, 0, 0, 7, 32, 30)
    with pytest.raises(RuntimeError, match="band overlap"):
        ops.scene_blend_bands(torch.zeros(1, 5, 32, 32), z, z, z, 0, -1, 7, 32, 32)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.scene_blend_bands(torch.zeros(1, 5, 32, 32), z, z, z, -1, 0, 7, 32, 32)
    with pytest.raises(AssertionError):
        ops.scene_blend_bands(torch.zeros(3, 5, 32, 32), z, z, z, 0, 0, 7, 32, 32)          # 3 items, 1 x 1 x 1 origins


# ---- SceneRestorer ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", B.SHAPES, ids=IDS)
def test_restorer_with_identity_callable_returns_the_scene(shape):
    K.check_restorer_identity("cpu", shape, 1, 4)


# two windows one band apart; a padded axis beside a multi-tile one; one mirror-padded window
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("shape", [B.SHAPES[1], B.SHAPES[2], B.SHAPES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_restorer_identity_under_the_ensemble(shape, G):
    K.check_restorer_identity("cpu", shape, G, 5)


@pytest.mark.parametrize("shape,G", [(B.SHAPES[0], 1), (B.SHAPES[1], 4), (B.SHAPES[2], 8), (B.SHAPES[4], 1), (B.SHAPES[5], 8)])
def test_restorer_with_a_band_dependent_callable(shape, G):
    K.check_restorer_band_dependent("cpu", shape, G, 4)


@pytest.mark.parametrize("G", [1, 4])
def test_restorer_does_not_depend_on_tile_batch(G):
    K.check_restorer_batch_sizes("cpu", B.SHAPES[1], G)


def test_restorer_arguments():
    from mp_hsir_amd.scene import SceneRestorer, plan_bands
    f = lambda x, ids: x          # noqa: E731
    r = SceneRestorer(f, tile=64, overlap=16)
    assert r.bands is None and r.band_overlap is None
    r = SceneRestorer(f, tile=64, overlap=16, bands=31)
    assert (r.bands, r.band_overlap) == (31, 7) and r.plan_bands(45) == plan_bands(45, 31, 7)
    for bad in (-1, 16):
        with pytest.raises(ValueError, match="band overlap"):
            SceneRestorer(f, tile=64, overlap=16, bands=31, band_overlap=bad)
    with pytest.raises(ValueError, match="band_overlap"):
        SceneRestorer(f, tile=64, overlap=16, band_overlap=4)
    net = M.build_net(TINY_CFG, "cpu")
    r = SceneRestorer(net, tile=32, overlap=0, graphed=False, grain=32)
    assert (r.bands, r.band_overlap) == (8, 2)
    r = SceneRestorer(f, tile=128, overlap=16, ensemble=8, bands=5)
    with pytest.raises(ValueError, match="ensemble=4"):
        r(torch.zeros(7, 64, 128), 0)                      # 64 x 128 tiles: the quarter turns still need square ones


def test_restorer_tiny_network_against_batch_1_forwards():
    """12 bands under the 8-band tiny network, one 32 x 32 tile, grain 32: band origins [0, 4] = two 32 x 32 items in ONE batch of 2 (the
    network is slow on the emulator); each restored item against the batch-1 forward of the same gathered item at the project's fp32
    parity bound"""
    from mp_hsir_amd import ops
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(TINY_CFG, "cpu")
    scene = torch.from_numpy(K.scene_of(12, 32, 32, 9))
    calls = []
    fwd = lambda x, ids: (calls.append(tuple(x.shape)), net(x, ids))[1]          # noqa: E731
    r = SceneRestorer(fwd, tile=32, overlap=0, tile_batch=4, graphed=False, grain=32, bands=8, band_overlap=2)
    got, store = r(scene, 2, return_tiles=True)
    assert calls == [(2, 8, 32, 32)] and r.plan_bands(12) == [0, 4]
    assert got.shape == scene.shape and torch.isfinite(got).all()
    origins3 = [(0, 0, 0), (4, 0, 0)]
    xs = ops.scene_gather_bands(scene, torch.tensor(origins3, dtype=torch.int32), 8, 32, 32, 0, (0,), torch.empty(2, 8, 32, 32))
    for s in range(2):
        with torch.no_grad():
            want = net(xs[s:s + 1], torch.tensor([2]))[0]
        err = rel_l2(store[s], want)
        print("item %d %s: rel-L2 %.3g" % (s, origins3[s], err))
        assert err <= 1e-3
    want, _ = B.blend(store.numpy(), [0, 4], [0], [0], 0, 2, 12, 32, 32)
    assert np.abs(got.numpy().astype(np.float64) - want).max() <= B.BLEND_TOL * float(store.abs().max().clamp_min(1.0))


# ---- schedules: the band gather passes tiles through LDS in the quarter-turn modes ---------------------------------------------------------

def _gather_quarter_turns():
    """C = 5, 64 x 64 tiles, the four transposing modes and a plain one"""
    from mp_hsir_amd import ops
    scene = K.scene_of(12, 70, 90, 10)
    origins3 = [(0, 0, 0), (7, 6, 26), (-2, 3, -5)]
    modes = (2, 3, 6, 7)
    out = torch.full((5, 5, 64, 64), float("nan"))
    for j0 in range(0, len(modes) * len(origins3), 5):
        ops.scene_gather_bands(torch.from_numpy(scene), torch.tensor(origins3, dtype=torch.int32), 5, 64, 64, j0, modes, out)
        assert np.array_equal(out.numpy(), B.gather(scene, origins3, 5, 64, 64, j0, 5, modes))
        guard.record(out, "band gather at item %d" % j0)


def test_gather_bits_do_not_depend_on_the_schedule(emu):  # noqa: F811
    case = ("scene_bands_gather", "scene_d4", ("scene",), _gather_quarter_turns)
    base, seen, waves = S._run(emu, case, 0, 0)
    assert base and "scene" in seen and waves > 1
    for mode, seed in S.schedules(waves):
        got, seen_s, waves_s = S._run(emu, case, mode, seed)
        assert (waves_s, seen_s) == (waves, seen) and len(got) == len(base), S.describe(mode, seed)
        for i, ((what, a), (_, b)) in enumerate(zip(base, got)):
            diff = guard.first_difference(a, b)
            assert diff is None, "under %s: recorded tensor %d (%s) is not bitwise the default schedule's: %s" % (S.describe(mode, seed), i, what, diff)
