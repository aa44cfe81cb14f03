"""numpy restatement (fp64 where anything is added) of the self-ensemble definitions of include/mphsir.h: the eight transforms of the
training augmentation, the transform-major item list, the gather and the mean.  Written from the definitions with np.rot90 / [::-1];
it does not import mp_hsir_amd.scene.  The tile geometry and the blend are those of tests/scene_ref.py."""
import numpy as np

import scene_ref as R

MODES4, MODES8 = (0, 1, 4, 5), (0, 1, 2, 3, 4, 5, 6, 7)
TRANSPOSING = (2, 3, 6, 7)
ADD_EPS = 2.0 ** -24          # one fp32 addition of values whose sum stays below 2 |max|: half an ulp, relative to the largest term's scale


def aug(x, m):
    """mode m of data_augmentation on the last two axes: rot90 counter-clockwise m // 2 times, then an up-down flip when m is odd"""
    t = np.rot90(x, m // 2, axes=(-2, -1))
    return t[..., ::-1, :] if m % 2 else t


def inv(y, m):
    """undoes aug(., m): the flip first, then the rotation the other way"""
    t = y[..., ::-1, :] if m % 2 else y
    return np.rot90(t, -(m // 2), axes=(-2, -1))


_probe = np.arange(2 * 3 * 5, dtype=np.float64).reshape(2, 3, 5)
for _m in range(8):
    assert np.array_equal(inv(aug(_probe, _m), _m), _probe)
    assert (aug(_probe, _m).shape[-2:] == (5, 3)) == (_m in TRANSPOSING)


def item(j, n_tiles):
    """-> (pass g, tile t) of item j"""
    return j // n_tiles, j % n_tiles


def gather_d4(scene, origins, th, tw, j0, count, modes):
    """-> (count,C,th,tw): item min(j0 + i, G * n - 1) of the transform-major list, cut through the mirror map and transformed"""
    n, G = len(origins), len(modes)
    tiles = R.gather(scene, origins, th, tw)
    out = []
    for i in range(count):
        g, t = item(min(j0 + i, G * n - 1), n)
        out.append(aug(tiles[t], modes[g]))
    return np.stack(out)


def fold_mean(y_all, n_tiles, modes):
    """y_all (G * n,C,th,tw): every restored item -> (n,C,th,tw) fp64, the mean over the passes of the items mapped back"""
    G = len(modes)
    acc = np.zeros((n_tiles,) + y_all.shape[1:], np.float64)
    for j in range(G * n_tiles):
        g, t = item(j, n_tiles)
        acc[t] += inv(y_all[j].astype(np.float64), modes[g])
    return acc / G


def restore(scene, f, plan, modes):
    """blend(mean_m inv_m(f(aug_m(tile)))) in fp64; plan = (th, tw, oy, ox, ov); f maps one (C,th,tw) tile to one"""
    th, tw, oy, ox, ov = plan
    C, H, W = scene.shape
    origins = [(y, x) for y in oy for x in ox]
    tiles = R.gather(scene.astype(np.float64), origins, th, tw)
    mean = np.stack([sum(inv(f(aug(t, m)), m) for m in modes) / len(modes) for t in tiles])
    return R.blend(mean, oy, ox, ov, H, W)[0]
