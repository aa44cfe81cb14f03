"""Spectral-window checks shared by the emulator (CPU) and GPU test files: the band gather and the band blend of
include/mphsir_bands.h against the fp64 restatement in tests/scene_bands_ref.py, and SceneRestorer(bands=...) over callables.
Every kernel check runs under tests/guard.py: inputs between NaN bands, outputs between sentinel bands and prefilled "never written"."""
import numpy as np
import torch

import ensemble_ref as E
import guard
import scene_bands_ref as B

EPS = 2.0 ** -24


def inp(dev, t):
    """a CPU tensor (or numpy array) as a guarded input on the check's device"""
    t = torch.as_tensor(t)
    G = guard.active()
    if G is not None and G.device.type == torch.device(dev).type:
        return G.input(t.detach())
    return t.to(dev)


def out_buffer(dev, shape):
    """an `out=` target: between sentinel bands and prefilled under the guard, NaN without it"""
    G = guard.active()
    if G is not None and G.device.type == torch.device(dev).type:
        return G.alloc(shape, torch.float32, torch.device(dev), "output", fill=None)
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def i32(dev, v, cols=None):
    t = torch.tensor(v, dtype=torch.int32)
    return inp(dev, t.reshape(-1, cols) if cols else t)


def scene_of(Cs, H, W, seed=0):
    return np.random.default_rng(seed).random((Cs, H, W), dtype=np.float32)


def modes_for(th, tw):
    return E.MODES8 if th == tw else E.MODES4          # the quarter turns run at square tiles only


def _walk_gather(dev, scene, origins3, C, th, tw, modes, batch):
    from mp_hsir_amd import ops
    sd, od = inp(dev, scene), i32(dev, origins3, 3)
    total = len(modes) * len(origins3)
    for j0 in range(0, total, batch):
        out = out_buffer(dev, (batch, C, th, tw))
        ops.scene_gather_bands(sd, od, C, th, tw, j0, modes, out)
        want = B.gather(scene, origins3, C, th, tw, j0, batch, modes)
        assert np.array_equal(out.cpu().numpy(), want), "batch at item %d of %d (modes %s)" % (j0, total, modes)
        guard.record(out, "gather batch at %d" % j0)


@guard.guarded
def check_gather(dev, shape, all_modes=True):
    """every batch of the pass-major item list against the restatement, bit for bit; batches of N + 1 start in the middle of a pass and
    the last one runs past the last item, which it repeats"""
    Cs, H, W, C, T, ov, ovb = shape
    th, tw, ob, oy, ox, origins3 = B.plan(*shape)
    modes = modes_for(th, tw) if all_modes else (0,)
    _walk_gather(dev, scene_of(Cs, H, W), origins3, C, th, tw, modes, len(origins3) + 1)


@guard.guarded
def check_gather_any_origin(dev):
    """negative, overhanging (folded more than once) and repeated origin triples, band origins -3 and Cs - 1 among them; non-square
    tiles under the flips, square ones under all eight modes; a tail batch whose items past the last repeat the last"""
    from mp_hsir_amd import ops
    Cs, H, W, C = 7, 37, 45, 5
    scene = scene_of(Cs, H, W, 1)
    origins3 = [(-3, -5, -3), (0, 0, 0), (Cs - 1, 20, 30), (2, -31, 44), (-3, 36, -44), (Cs - 1, 20, 30), (Cs - 1, 20, 30), (11, -64, 90), (1, 3, 7)]
    _walk_gather(dev, scene, origins3, C, 64, 32, (0,), 4)
    _walk_gather(dev, scene, origins3, C, 64, 32, E.MODES4, 7)
    _walk_gather(dev, scene, origins3, C, 36, 36, E.MODES8, 5)
    for m in range(8):
        _walk_gather(dev, scene, origins3[:3], C, 32, 32, (m,), 2)
    out = out_buffer(dev, (5, C, 32, 32))
    ops.scene_gather_bands(inp(dev, scene), i32(dev, origins3[:3], 3), C, 32, 32, 20, E.MODES8, out)       # items 20 .. 23 of 24, and the last once more
    assert torch.equal(out[4], out[3]) and not torch.equal(out[3], out[2])


@guard.guarded
def check_blend(dev, shape):
    from mp_hsir_amd import ops
    Cs, H, W, C, T, ov, ovb = shape
    th, tw, ob, oy, ox, origins3 = B.plan(*shape)
    tiles = np.random.default_rng(2).random((len(origins3), C, th, tw), dtype=np.float32)
    td, obd, oyd, oxd = inp(dev, tiles), i32(dev, ob), i32(dev, oy), i32(dev, ox)
    got = ops.scene_blend_bands(td, obd, oyd, oxd, ov, ovb, Cs, H, W)
    again = ops.scene_blend_bands(td, obd, oyd, oxd, ov, ovb, Cs, H, W)
    want, cover = B.blend(tiles, ob, oy, ox, ov, ovb, Cs, H, W)
    if shape == B.SHAPES[0]:
        assert cover.max() == B.MAX_COVER == 27
    assert cover.min() >= 1 and cover.max() <= B.MAX_COVER
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print("band blend %s: max abs error %.3g (bound %.3g), cover up to %d" % (shape, err, B.BLEND_TOL, cover.max()))
    assert err <= B.BLEND_TOL
    assert torch.equal(got, again), "the blend is not reproducible"
    clamped = ops.scene_blend_bands(inp(dev, tiles * 3 - 1), obd, oyd, oxd, ov, ovb, Cs, H, W, clamp01=True)
    assert float(clamped.min()) >= 0.0 and float(clamped.max()) <= 1.0 and float(clamped.max()) == 1.0
    guard.record(got, "blend")


@guard.guarded
def check_round_trip(dev, shape):
    """gather, poison whatever lies outside the scene on any of the three axes, blend: nothing poisoned is read, the scene comes back
    within the tolerance, and bitwise where one item covers an element"""
    from mp_hsir_amd import ops
    Cs, H, W, C, T, ov, ovb = shape
    th, tw, ob, oy, ox, origins3 = B.plan(*shape)
    scene = scene_of(Cs, H, W, 3)
    tiles = out_buffer(dev, (len(origins3), C, th, tw))
    ops.scene_gather_bands(inp(dev, scene), i32(dev, origins3, 3), C, th, tw, 0, (0,), tiles)
    B.poison_padding(tiles, origins3, Cs, H, W)
    poisoned = int(torch.isnan(tiles).sum())
    assert poisoned == B.padded_positions(ob, oy, ox, C, th, tw, Cs, H, W)
    assert (poisoned > 0) == (Cs < C or H < th or W < tw), "a padded geometry must have padding to poison (and only those have)"
    back = ops.scene_blend_bands(tiles, i32(dev, ob), i32(dev, oy), i32(dev, ox), ov, ovb, Cs, H, W)
    assert torch.isfinite(back).all()
    err = np.abs(back.cpu().numpy().astype(np.float64) - scene).max()
    print("band round trip %s: %d poisoned positions, max abs error %.3g (bound %.3g)" % (shape, poisoned, err, B.BLEND_TOL))
    assert err <= B.BLEND_TOL
    _, cover = B.blend(np.zeros((len(origins3), C, th, tw)), ob, oy, ox, ov, ovb, Cs, H, W)
    one = torch.from_numpy(cover == 1)
    assert one.any() and torch.equal(back.cpu()[one], torch.from_numpy(scene)[one]), "an element under one item must come back exactly"


@guard.guarded
def check_one_window_is_the_old_path(dev, shape):
    """Cs == C: the band blend is bitwise ops.scene_blend_tiles, the band gather with one pass bitwise ops.scene_gather_tiles"""
    from mp_hsir_amd import ops
    Cs, H, W, C, T, ov, ovb = shape
    assert Cs == C
    th, tw, ob, oy, ox, origins3 = B.plan(*shape)
    assert ob == [0]
    tiles = inp(dev, np.random.default_rng(4).random((len(origins3), C, th, tw), dtype=np.float32))
    oyd, oxd = i32(dev, oy), i32(dev, ox)
    new = ops.scene_blend_bands(tiles, i32(dev, ob), oyd, oxd, ov, ovb, Cs, H, W)
    old = ops.scene_blend_tiles(tiles, oyd, oxd, ov, H, W)
    assert torch.equal(new, old), "one window: the band blend must be the blend, bit for bit"
    scene = inp(dev, scene_of(Cs, H, W, 5))
    cut = out_buffer(dev, (len(origins3), C, th, tw))
    ops.scene_gather_bands(scene, i32(dev, origins3, 3), C, th, tw, 0, (0,), cut)
    assert torch.equal(cut, ops.scene_gather_tiles(scene, i32(dev, [o[1:] for o in origins3], 2), th, tw))


# ---- SceneRestorer over callables --------------------------------------------------------------------------------------------------------

def ensemble_tol(G, scale=1.0):
    """the blend's bound plus the G - 1 additions of the mean (tests/ensemble_ref.py: ADD_EPS each; the scaling by 1 / G is exact)"""
    return (B.BLEND_TOL + (G - 1) * E.ADD_EPS) * scale


def check_restorer_identity(dev, shape, G, tile_batch):
    from mp_hsir_amd.scene import SceneRestorer
    Cs, H, W, C, T, ov, ovb = shape
    scene = scene_of(Cs, H, W, 6)
    calls = []
    r = SceneRestorer(lambda x, ids: (calls.append(tuple(x.shape)), x)[1], tile=T, overlap=ov, tile_batch=tile_batch, ensemble=G, bands=C, band_overlap=ovb)
    back, store = r(torch.from_numpy(scene).to(dev), 0, return_tiles=True)
    th, tw, ob, oy, ox, origins3 = B.plan(*shape)
    N = len(origins3)
    assert r.plan_bands(Cs) == ob
    assert back.shape == scene.shape and store.shape == (N, C, th, tw)
    if Cs != C:
        assert len(calls) == -(-N * G // tile_batch) and set(calls) == {(min(tile_batch, N * G), C, th, tw)}, calls
    err = np.abs(back.cpu().numpy().astype(np.float64) - scene).max()
    print("identity, ensemble %d, %s: max abs error %.3g (bound %.3g)" % (G, shape, err, ensemble_tol(G)))
    assert err <= ensemble_tol(G)


def check_restorer_band_dependent(dev, shape, G, tile_batch):
    """y[:, c] = x[:, c] * (1 + c / C): wrong window-to-band mapping or a wrong item order changes the result.  The factors are rounded to
    fp32 once and the reference multiplies by the same numbers, so the callable differs from it by the rounding of one product of a value
    below 2: the ensemble bound with one more rounding, scaled by 2."""
    from mp_hsir_amd.scene import SceneRestorer
    Cs, H, W, C, T, ov, ovb = shape
    scene = scene_of(Cs, H, W, 7)
    f32 = (1.0 + np.arange(C) / C).astype(np.float32)
    fd = torch.from_numpy(f32).to(dev).reshape(1, C, 1, 1)
    r = SceneRestorer(lambda x, ids: x * fd, tile=T, overlap=ov, tile_batch=tile_batch, ensemble=G, bands=C, band_overlap=ovb)
    got = r(torch.from_numpy(scene).to(dev), 0)
    want = B.restore(scene, lambda t: t * f32.astype(np.float64)[:, None, None], Cs, H, W, C, T, ov, ovb, {1: (0,), 4: E.MODES4, 8: E.MODES8}[G])
    tol = (ensemble_tol(G) + EPS) * 2.0
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print("x * (1 + c / C), ensemble %d, %s: max abs error %.3g (bound %.3g)" % (G, shape, err, tol))
    assert err <= tol
    if Cs > C:
        assert np.abs(got.cpu().numpy() - scene).max() > 0.05, "the band-dependent function must change the scene"
    return got


def check_restorer_batch_sizes(dev, shape, G):
    outs = [check_restorer_band_dependent(dev, shape, G, tb) for tb in (1, 3, 16)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "the result depends on tile_batch"


def check_same_launches_with_bands_set(dev, shape):
    """Cs == C: the restorer with `bands` set issues the launches it issues without -- the same ops functions in the same order, the same
    ops.ACCOUNT table -- and returns the same bits"""
    from mp_hsir_amd import ops
    from mp_hsir_amd.scene import SceneRestorer
    Cs, H, W, C, T, ov, ovb = shape
    assert Cs == C
    scene = torch.from_numpy(scene_of(Cs, H, W, 8)).to(dev)
    names = [n for n in dir(ops) if n.startswith("scene_")]
    runs = []
    for G in (1, 4):
        for kw in ({}, dict(bands=C, band_overlap=ovb), dict(bands=C)):
            called, saved = [], {n: getattr(ops, n) for n in names}
            for n, fn in saved.items():
                setattr(ops, n, lambda *a, _fn=fn, _n=n, **k: (called.append(_n), _fn(*a, **k))[1])
            ops.ACCOUNT = {}
            try:
                out = SceneRestorer(lambda x, ids: x * 0.75 + 0.125, tile=T, overlap=ov, tile_batch=3, ensemble=G, **kw)(scene, 0)
                account = {k: list(v) for k, v in ops.ACCOUNT.items()}
            finally:
                ops.ACCOUNT = None
                for n, fn in saved.items():
                    setattr(ops, n, fn)
            runs.append((called, account, out))
        base = runs[-3]
        assert base[0] and "scene_gather_bands" not in base[0] and "scene_blend_bands" not in base[0]
        assert base[1] and sorted(base[1]) == ["scene"]
        for other in runs[-2:]:
            assert other[0] == base[0] and other[1] == base[1], (other[0], base[0])
            assert torch.equal(other[2], base[2])
