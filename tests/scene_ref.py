"""numpy restatement (fp64) of the whole-scene tiling definitions: the tile plan, the mirror map of the gather and the ramp blend.
Written from the definitions, not from mp_hsir_amd.scene (which it does not import): the tests compare the two."""
import numpy as np

SHAPES = [(100, 131, 64, 16), (64, 64, 256, 32), (70, 200, 64, 0), (1000, 700, 256, 32), (307, 1280, 256, 32), (500, 500, 256, 128),
          (65, 65, 64, 32)]                                       # (H, W, T, ov)
SMALL_SHAPES = [s for s in SHAPES if s[0] * s[1] <= 70 * 200]     # what the CPU emulator runs in seconds
# geometries WITH mirror padding (an axis no longer than one tile and not a multiple of 64): both axes padded; a padded axis beside a
# multi-tile axis, each way round, with W % 4 != 0 (the blend's quads straddle the scene's right edge inside a padded tile)
PADDED_SHAPES = [(70, 90, 128, 32), (67, 67, 256, 0), (70, 203, 128, 32), (130, 65, 128, 16), (97, 301, 128, 64)]
BLEND_TOL = (2 * 9 + 1) * 2.0 ** -24      # data in [0,1], at most 9 multiply-adds (numerator and denominator) and one division in fp32


def plan_axis(H, T, ov, grain=64):
    if grain not in (32, 64) or T <= 0 or T % grain or not 0 <= ov <= T // 2 or H < grain:
        raise ValueError((H, T, ov, grain))
    th = min(T, -(-H // grain) * grain)
    if H <= th:
        return th, [0]
    n = int(np.ceil((H - ov) / (th - ov)))
    return th, [(i * (H - th)) // (n - 1) for i in range(n)]


def plan_tiles(H, W, T, ov, grain=64):
    """-> th, tw, oy, ox; tile iy * nx + ix sits at (oy[iy], ox[ix])"""
    th, oy = plan_axis(H, T, ov, grain)
    tw, ox = plan_axis(W, T, ov, grain)
    return th, tw, oy, ox


def mirror(idx, n):
    """torch `reflect` for any integer coordinates"""
    idx = np.asarray(idx)
    if n == 1:
        return np.zeros_like(idx)
    p = 2 * (n - 1)
    m = np.mod(idx, p)
    return np.where(m < n, m, p - m)


def gather(scene, origins, th, tw):
    """scene (C,H,W), origins [(oy, ox)] -> (n,C,th,tw), a copy through the mirror map"""
    C, H, W = scene.shape
    out = np.empty((len(origins), C, th, tw), scene.dtype)
    for t, (oy, ox) in enumerate(origins):
        ys, xs = mirror(oy + np.arange(th), H), mirror(ox + np.arange(tw), W)
        out[t] = scene[:, ys[:, None], xs[None, :]]
    return out


def axis_weight(o, th, H, ov):
    u = np.arange(th, dtype=np.float64)
    w = np.ones(th)
    if o > 0:
        w = np.minimum(w, (u + 1) / (ov + 1))
    if o + th < H:
        w = np.minimum(w, (th - u) / (ov + 1))
    return w


def blend(tiles, oy, ox, ov, H, W):
    """tiles (ny*nx,C,th,tw) -> (C,H,W) fp64, and the number of tiles over every pixel (H,W)"""
    n, C, th, tw = tiles.shape
    num, den, cover = np.zeros((C, H, W)), np.zeros((H, W)), np.zeros((H, W), np.int64)
    for iy, y0 in enumerate(oy):
        for ix, x0 in enumerate(ox):
            hh, ww = min(th, H - y0), min(tw, W - x0)            # positions outside the scene are ignored
            w = (axis_weight(y0, th, H, ov)[:, None] * axis_weight(x0, tw, W, ov)[None, :])[:hh, :ww]
            num[:, y0:y0 + hh, x0:x0 + ww] += w * tiles[iy * len(ox) + ix, :, :hh, :ww].astype(np.float64)
            den[y0:y0 + hh, x0:x0 + ww] += w
            cover[y0:y0 + hh, x0:x0 + ww] += 1
    return num / den, cover


def padded_positions(oy, ox, th, tw, H, W):
    """number of (tile, y, x) positions that lie outside the scene"""
    return sum(th * tw - min(th, H - y) * min(tw, W - x) for y in oy for x in ox)
