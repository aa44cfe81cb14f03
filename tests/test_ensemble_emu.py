"""Self-ensemble on the CPU: the d4 gather / fold kernels of mp-hsir_amd/csrc/scene_d4.hip through the emulated build against the fp64
restatement in tests/ensemble_ref.py, and SceneRestorer(ensemble=4 / 8) over callables whose ensemble is known in closed form and over
the tiny emulated network."""
import numpy as np
import pytest
import torch

import ensemble_ref as E
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


def _walk_gather(scene, origins, th, tw, modes, B):
    """every batch of the item list, each against the reference (the last one repeats the last item when B does not divide it)"""
    from mp_hsir_amd import ops
    total = len(modes) * len(origins)
    out = torch.empty((B,) + (scene.shape[0], th, tw))
    for j0 in range(0, total, B):
        out.fill_(float("nan"))
        ops.scene_gather_d4(scene, _i32(origins), th, tw, j0, modes, out=out)
        want = E.gather_d4(scene.numpy(), origins, th, tw, j0, B, modes)
        assert np.array_equal(out.numpy(), want), "batch at item %d of %d (modes %s)" % (j0, total, modes)


# non-square tiles: an axis that rounds up to less than the requested tile (64 x 128), and the same with mirror padding (128 x 256)
NONSQUARE_SHAPES = [(64, 200, 128, 32), (70, 200, 256, 32)]


@pytest.mark.parametrize("C", [1, 5, 31])
@pytest.mark.parametrize("H,W,T,ov", R.SMALL_SHAPES + [R.PADDED_SHAPES[2]])
def test_gather_all_modes_square_tiles_bitwise(C, H, W, T, ov):
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    assert th == tw
    origins = [(y, x) for y in oy for x in ox]
    _walk_gather(_scene(C, H, W), origins, th, tw, E.MODES8, len(origins) + 1)       # batches start in the middle of a pass


@pytest.mark.parametrize("C", [1, 5, 31])
@pytest.mark.parametrize("H,W,T,ov", NONSQUARE_SHAPES)
def test_gather_flip_modes_nonsquare_tiles_bitwise(C, H, W, T, ov):
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    assert th != tw
    origins = [(y, x) for y in oy for x in ox]
    _walk_gather(_scene(C, H, W, 1), origins, th, tw, E.MODES4, len(origins) + 1)


def test_gather_tail_repeats_the_last_item_and_starts_mid_pass():
    """3 tiles x 8 passes = 24 items in batches of 5: batches start at items 5, 10 (mid pass), and the last one holds items 20..23 and
    the last item once more; also one mode alone, a pair, and tiles whose extent is no multiple of the 32 x 32 squares (36, 40)"""
    from mp_hsir_amd import ops
    scene = _scene(5, 50, 61, 2)
    origins = [(-3, 0), (7, 30), (20, -9)]
    for n in (32, 36, 40):
        _walk_gather(scene, origins, n, n, E.MODES8, 5)
        for m in range(8):
            _walk_gather(scene, origins, n, n, (m,), 2)
    _walk_gather(scene, origins, 36, 44, E.MODES4, 5)
    _walk_gather(scene, origins, 36, 44, (5, 1), 4)
    out = torch.empty((5, 5, 32, 32))
    ops.scene_gather_d4(scene, _i32(origins), 32, 32, 20, E.MODES8, out=out)
    assert torch.equal(out[4], out[3]) and not torch.equal(out[3], out[2])


def _fold_walk(y_all, n, modes, B):
    from mp_hsir_amd import ops
    total = len(modes) * n
    store = torch.full((n,) + tuple(y_all.shape[1:]), float("nan"))          # never read before a tile's pass 0 has been folded
    for j0 in range(0, total, B):
        cnt = min(B, total - j0)
        ops.scene_fold_d4(y_all[j0:j0 + cnt].contiguous(), store, j0, cnt, modes)
    return store


@pytest.mark.parametrize("modes,th,tw", [(E.MODES8, 32, 32), (E.MODES8, 36, 36), (E.MODES8, 64, 64), (E.MODES4, 32, 48), (E.MODES4, 64, 64),
                                         ((0, 1), 36, 32), ((3, 6), 40, 40)])
@pytest.mark.parametrize("C", [1, 5, 9])
def test_fold_is_the_mean_and_does_not_depend_on_the_batch_size(modes, th, tw, C):
    n, G = 3, len(modes)
    y = torch.from_numpy(np.random.default_rng(3).random((G * n, C, th, tw), dtype=np.float32) * 2)          # [0, 2)
    want = E.fold_mean(y.numpy(), n, modes)
    bound = (G - 1) * 2.0 ** -24 * float(y.abs().max())            # G - 1 fp32 additions; the scaling by 1 / G is exact
    stores = [_fold_walk(y, n, modes, B) for B in (1, 3, n, n + 2, 2 * n + 1, G * n)]
    err = np.abs(stores[0].numpy().astype(np.float64) - want).max()
    print("fold modes %s %dx%d C=%d: max abs error %.3g (bound %.3g)" % (modes, th, tw, C, err, bound))
    assert err <= bound
    for s in stores[1:]:
        assert torch.equal(s, stores[0]), "the fold depends on the batch size"


@pytest.mark.parametrize("modes,n_side", [(E.MODES8, 36), (E.MODES4, 32)])
def test_fold_nan_poisons_exactly_its_own_element(modes, n_side):
    n, G, C = 3, len(modes), 5
    rng = np.random.default_rng(4)
    for j in (0, 4, 7, G * n - 1):
        y = torch.from_numpy(rng.random((G * n, C, n_side, n_side), dtype=np.float32) * 2)
        y[j, 3, 5, 30] = float("nan")
        want = np.isnan(E.fold_mean(y.numpy(), n, modes))
        assert want.sum() == 1
        for B in (1, 5, G * n):
            assert np.array_equal(torch.isnan(_fold_walk(y, n, modes, B)).numpy(), want)


def test_entry_points_refuse_what_they_cannot_do():
    from mp_hsir_amd import ops
    scene = _scene(2, 40, 72)
    o = _i32([(0, 0)])
    with pytest.raises(RuntimeError, match="square tile"):
        ops.scene_gather_d4(scene, o, 32, 64, 0, E.MODES8, out=torch.empty(1, 2, 32, 64))
    with pytest.raises(RuntimeError, match="square tile"):
        ops.scene_fold_d4(torch.zeros(1, 2, 32, 64), torch.zeros(1, 2, 32, 64), 0, 1, (0, 2))
    ops.scene_gather_d4(scene, o, 32, 64, 0, E.MODES4, out=torch.empty(1, 2, 32, 64))          # the flips do not need one
    for modes in ((0, 1, 4), (0,) * 5, (0,) * 16):
        with pytest.raises(RuntimeError, match="1, 2, 4 or 8"):
            ops.scene_gather_d4(scene, o, 32, 32, 0, modes, out=torch.empty(1, 2, 32, 32))
        with pytest.raises(RuntimeError, match="1, 2, 4 or 8"):
            ops.scene_fold_d4(torch.zeros(1, 2, 32, 32), torch.zeros(1, 2, 32, 32), 0, 1, modes)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.scene_gather_d4(scene, o, 30, 30, 0, (0,), out=torch.empty(1, 2, 30, 30))
    with pytest.raises(RuntimeError, match="outside"):
        ops.scene_gather_d4(scene, o, 32, 32, 4, E.MODES4, out=torch.empty(1, 2, 32, 32))
    with pytest.raises(RuntimeError, match="outside"):
        ops.scene_fold_d4(torch.zeros(2, 2, 32, 32), torch.zeros(1, 2, 32, 32), 3, 2, E.MODES4)          # items 3, 4 of 4
    with pytest.raises(ValueError):
        ops.scene_gather_d4(scene, o, 32, 32, 0, (8,), out=torch.empty(1, 2, 32, 32))


# ---- SceneRestorer ---------------------------------------------------------------------------------------------------------------------

# (H, W, tile, overlap, tile_batch): unpadded with several tiles; one mirror-padded tile by three (70 -> 128); both axes padded
RESTORER_CASES = [(100, 131, 64, 16, 5), (70, 200, 128, 32, 4), (70, 90, 128, 32, 3)]


def _tol(G, scale=1.0):
    return (R.BLEND_TOL + (G - 1) * 2.0 ** -24) * scale


@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("H,W,T,ov,tb", RESTORER_CASES)
def test_restorer_with_identity_network_returns_the_scene(G, H, W, T, ov, tb):
    from mp_hsir_amd.scene import SceneRestorer
    scene = _scene(5, H, W, 5)
    calls = []
    r = SceneRestorer(lambda x, ids: (calls.append(1), x)[1], tile=T, overlap=ov, tile_batch=tb, ensemble=G)
    back, tiles = r(scene, 0, return_tiles=True)
    n = len(r.plan(H, W))
    assert len(calls) == -(-n * G // tb), "items are packed across passes: ceil(n G / B) forwards"
    assert back.shape == scene.shape and tiles.shape[0] == n
    err = np.abs(back.numpy().astype(np.float64) - scene.numpy()).max()
    print("identity, ensemble %d, %s: max abs error %.3g (bound %.3g)" % (G, (H, W, T, ov), err, _tol(G)))
    assert err <= _tol(G)


@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("H,W,T,ov,tb", RESTORER_CASES)
def test_restorer_with_a_position_dependent_network(G, H, W, T, ov, tb):
    """f(x)[u, v] = x[u, v] * A[u, v] + B[u, v] with random tables over the tile: the mean over the transforms depends on every inverse
    map being the right one (a linear position code would not do: its flip-average is a constant).  The scene and B are multiples of
    2^-10 in [0, 1) and A is 0.5, 1 or 2, so f is exact in fp32 and the callable and the fp64 reference apply the same function; the
    bound is that of the identity test scaled by max |f| (< 3)."""
    from mp_hsir_amd.scene import SceneRestorer
    rng = np.random.default_rng(6)
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    scene = np.floor(rng.random((5, H, W)) * 1024).astype(np.float32) / 1024
    A = rng.choice([0.5, 1.0, 2.0], size=(th, tw)).astype(np.float32)
    Bt = np.floor(rng.random((th, tw)) * 1024).astype(np.float32) / 1024
    At, Btt = torch.from_numpy(A), torch.from_numpy(Bt)
    r = SceneRestorer(lambda x, ids: x * At + Btt, tile=T, overlap=ov, tile_batch=tb, ensemble=G)
    got = r(torch.from_numpy(scene), 0)
    modes = E.MODES4 if G == 4 else E.MODES8
    want = E.restore(scene, lambda t: t * A.astype(np.float64) + Bt, (th, tw, oy, ox, ov), modes)
    err = np.abs(got.numpy().astype(np.float64) - want).max()
    fmax = float(np.abs(scene).max() * 2 + 1)
    print("x * A + B, ensemble %d, %s: max abs error %.3g (bound %.3g)" % (G, (H, W, T, ov), err, _tol(G, fmax)))
    assert err <= _tol(G, fmax)
    plain = SceneRestorer(lambda x, ids: x * At + Btt, tile=T, overlap=ov, tile_batch=tb)(torch.from_numpy(scene), 0)
    assert float((plain - got).abs().max()) > 0.05, "the ensemble of a position-dependent function must differ from one forward"


def test_restorer_pointwise_network_ensemble_equals_one_forward():
    from mp_hsir_amd.scene import SceneRestorer
    scene = _scene(5, 100, 131, 7)
    one = SceneRestorer(lambda x, ids: x * x, tile=64, overlap=16, tile_batch=4)(scene, 0)
    eight = SceneRestorer(lambda x, ids: x * x, tile=64, overlap=16, tile_batch=4, ensemble=8)(scene, 0)
    err = float((one.double() - eight.double()).abs().max())
    print("x * x, ensemble 8 against ensemble 1: max abs difference %.3g (bound %.3g)" % (err, _tol(8)))
    assert err <= _tol(8)


def test_ensemble_1_is_the_restorer_without_the_argument_bitwise():
    from mp_hsir_amd.scene import SceneRestorer
    scene = _scene(5, 100, 131, 8)
    f = lambda x, ids: x * 0.75 + 0.125          # noqa: E731
    a, ta = SceneRestorer(f, tile=64, overlap=16, tile_batch=4)(scene, 0, return_tiles=True)
    b, tb = SceneRestorer(f, tile=64, overlap=16, tile_batch=4, ensemble=1)(scene, 0, return_tiles=True)
    assert torch.equal(a, b) and torch.equal(ta, tb)


def test_restorer_refuses_bad_ensembles():
    from mp_hsir_amd.scene import SceneRestorer
    for bad in (3, 0, 2, 16, "8"):
        with pytest.raises(ValueError, match="ensemble"):
            SceneRestorer(lambda x, ids: x, tile=64, overlap=16, ensemble=bad)
    r = SceneRestorer(lambda x, ids: x, tile=128, overlap=16, ensemble=8)
    p = r.plan(64, 128)
    assert (p.th, p.tw) == (64, 128)
    with pytest.raises(ValueError, match="ensemble=4"):
        r(_scene(2, 64, 128), 0)
    back = SceneRestorer(lambda x, ids: x, tile=128, overlap=16, ensemble=4)(_scene(2, 64, 128), 0)
    assert back.shape == (2, 64, 128)


def test_restorer_tiny_network_against_batch_1_forwards():
    """32 x 32, grain 32, ensemble 4, tile_batch 4: ONE forward of batch 4 (the tile under modes 0, 1, 4, 5) against the fp64 mean of four
    batch-1 forwards of the transformed scene, mapped back; the project's fp32 parity bound, 1e-3 relative L2"""
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(TINY_CFG, "cpu")
    scene = _scene(8, 32, 32, 9)
    calls = []
    fwd = lambda x, ids: (calls.append(tuple(x.shape)), net(x, ids))[1]          # noqa: E731
    got = SceneRestorer(fwd, tile=32, overlap=0, tile_batch=4, graphed=False, grain=32, ensemble=4)(scene, 2)
    assert calls == [(4, 8, 32, 32)]
    acc = np.zeros((8, 32, 32))
    singles = []
    for m in E.MODES4:
        x = torch.from_numpy(np.ascontiguousarray(E.aug(scene.numpy(), m)))
        with torch.no_grad():
            y = net(x[None], torch.tensor([2]))[0].numpy()
        singles.append(E.inv(y, m))
        acc += singles[-1].astype(np.float64)
    err = rel_l2(got, torch.from_numpy(acc / 4).float())
    spread = rel_l2(torch.from_numpy(np.ascontiguousarray(singles[1])), torch.from_numpy(np.ascontiguousarray(singles[0])))
    print("tiny network, ensemble 4: rel-L2 against the mean of batch-1 forwards %.3g (the members differ from each other by %.3g)" % (err, spread))
    assert err <= 1e-3
