"""numpy restatement (fp64) of the spectral-window definitions of include/mphsir_bands.h: the band plan, the gather through three mirror
maps and the ramp blend over (window, tile) items, with the per-element cover.  Written from the definitions, not from
mp_hsir_amd.scene (which it does not import): the tests compare the two.  The spatial plan, the mirror map and the axis ramp are those
of tests/scene_ref.py, the transforms those of tests/ensemble_ref.py."""
import numpy as np

import ensemble_ref as E
import scene_ref as R

# (Cs, H, W, C, T, ov, ovb): the smallest shapes at which each piece can go wrong
SHAPES = [(12, 125, 125, 5, 64, 32, 2),       # cover 3 x 3 x 3 = 27: band origins [0, 2, 4, 7], spatial [0, 30, 61] each way
          (6, 70, 90, 5, 64, 0, 2),           # Cs = C + 1: two windows one band apart, both ramps saturated in the middle; W % 4 != 0
          (8, 70, 203, 5, 128, 32, 2),        # two windows sharing exactly ovb bands (Cs = 2C - ovb); a padded axis beside a multi-tile one
          (45, 70, 100, 31, 64, 16, 8),       # C and Cs no multiples of the 8-band chunk; origins [0, 14]
          (20, 70, 90, 31, 64, 16, 8),        # Cs < C: one window, bands 20..30 mirror padding
          (3, 64, 64, 5, 64, 0, 0),           # Cs < C, one tile, ovb = 0
          (31, 70, 100, 31, 64, 16, 8)]       # Cs == C: one window
GPU_SHAPES = [(210, 70, 90, 100, 64, 16, 25),         # band origins [0, 55, 110]
              (191, 300, 520, 31, 256, 32, 8)]        # 8 windows x 6 tiles
PLAN_C = (4, 5, 8, 12, 31, 100)                      # the sweep of the plan check: every legal ovb, Cs up to 4C + 2
MAX_COVER = 27

# Data in [0, 1].  The roundings of the launch's own summation (mp-hsir_amd/csrc/scene_bands.hip) for one output element under n covering
# items, each half an ulp (2^-24) relative to a value of at most about 1 (the quotient; the sums are normalised by the denominator):
#   numerator:    per item the multiply-add with the tile value, as scene_ref.BLEND_TOL counts it (2: a product and a sum on the emulator,
#                 one fma on the GPU), and the product wb * (wy * wx) (1) -- scene.hip's blend uses the very same rounded weight in
#                 numerator and denominator, where its rounding cancels; here the denominator is the factored
#                 (sum of wb) * (sum of wy * wx), which never forms that product, so its rounding stays          -> 3 n
#   denominator:  the pixel sum, one addition per spatial tile (at most 9); the band sum, one per window (at most 3); their product (1)
#                                                                                                                 -> 13
#   the division: 1
# The rounded ramp values themselves (wb, wy * wx) are the same numbers in numerator and denominator, as in scene_ref.
# n = 27: 3 * 27 + 13 + 1 = 95 roundings.  (A plain item-by-item sum with one weight per item would count 2 * 27 + 2: 3.3e-6.)
BLEND_ROUNDINGS = 3 * MAX_COVER + 13 + 1
BLEND_TOL = BLEND_ROUNDINGS * 2.0 ** -24             # 5.7e-6


def plan_bands(Cs, C, ovb):
    if Cs <= 0 or C <= 0 or not 0 <= ovb <= C // 2:
        raise ValueError((Cs, C, ovb))
    if Cs <= C:
        return [0]
    n = int(-(-(Cs - ovb) // (C - ovb)))
    return [(i * (Cs - C)) // (n - 1) for i in range(n)]


def plan(Cs, H, W, C, T, ov, ovb):
    """-> th, tw, ob, oy, ox, origins3; item (ib * ny + iy) * nx + ix sits at (ob[ib], oy[iy], ox[ix])"""
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    ob = plan_bands(Cs, C, ovb)
    return th, tw, ob, oy, ox, [(b, y, x) for b in ob for y in oy for x in ox]


def cut(scene, origin3, C, th, tw):
    """one item (C,th,tw): a copy of the scene through the mirror map on all three axes"""
    Cs, H, W = scene.shape
    b, y, x = origin3
    cs, ys, xs = R.mirror(b + np.arange(C), Cs), R.mirror(y + np.arange(th), H), R.mirror(x + np.arange(tw), W)
    return scene[cs[:, None, None], ys[None, :, None], xs[None, None, :]]


def gather(scene, origins3, C, th, tw, j0, count, modes=(0,)):
    """-> (count,C,th,tw): item min(j0 + i, G * N - 1) of the pass-major list j = g * N + s, cut and transformed"""
    N, G = len(origins3), len(modes)
    out = []
    for i in range(count):
        g, s = divmod(min(j0 + i, G * N - 1), N)
        out.append(E.aug(cut(scene, origins3[s], C, th, tw), modes[g]))
    return np.stack(out)


def band_weight(o, C, Cs, ovb):
    return R.axis_weight(o, C, Cs, ovb)          # the same ramp, ovb + 1 in place of ov + 1


def blend(tiles, ob, oy, ox, ov, ovb, Cs, H, W):
    """tiles (nb*ny*nx,C,th,tw) -> (Cs,H,W) fp64 by the definition (sum(w * item) / sum(w), w = wb * wy * wx), and the number of items
    over every element (Cs,H,W).  Item bands beyond Cs and item positions outside the scene are ignored."""
    n, C, th, tw = tiles.shape
    ny, nx = len(oy), len(ox)
    num, den, cover = np.zeros((Cs, H, W)), np.zeros((Cs, H, W)), np.zeros((Cs, H, W), np.int64)
    for ib, b0 in enumerate(ob):
        cc = min(C, Cs - b0)
        wb = band_weight(b0, C, Cs, ovb)[:cc]
        for iy, y0 in enumerate(oy):
            for ix, x0 in enumerate(ox):
                hh, ww = min(th, H - y0), min(tw, W - x0)
                w = wb[:, None, None] * (R.axis_weight(y0, th, H, ov)[None, :, None] * R.axis_weight(x0, tw, W, ov)[None, None, :])[:, :hh, :ww]
                t = tiles[(ib * ny + iy) * nx + ix, :cc, :hh, :ww].astype(np.float64)
                num[b0:b0 + cc, y0:y0 + hh, x0:x0 + ww] += w * t
                den[b0:b0 + cc, y0:y0 + hh, x0:x0 + ww] += w
                cover[b0:b0 + cc, y0:y0 + hh, x0:x0 + ww] += 1
    return num / den, cover


def padded_positions(ob, oy, ox, C, th, tw, Cs, H, W):
    """number of (item, c, y, x) positions that lie outside the scene on some axis"""
    return sum(C * th * tw - min(C, Cs - b) * min(th, H - y) * min(tw, W - x) for b in ob for y in oy for x in ox)


def poison_padding(tiles, origins3, Cs, H, W):
    """NaN into every item position outside the scene, in place (torch or numpy); -> the tiles"""
    for s, (b, y, x) in enumerate(origins3):
        tiles[s, max(Cs - b, 0):] = float("nan")
        tiles[s, :, max(H - y, 0):, :] = float("nan")
        tiles[s, :, :, max(W - x, 0):] = float("nan")
    return tiles


def restore(scene, f, Cs, H, W, C, T, ov, ovb, modes=(0,)):
    """blend(mean_m inv_m(f(aug_m(item)))) in fp64; f maps one (C,th,tw) item to one"""
    th, tw, ob, oy, ox, origins3 = plan(Cs, H, W, C, T, ov, ovb)
    s64 = scene.astype(np.float64)
    mean = np.stack([sum(E.inv(f(E.aug(cut(s64, o, C, th, tw), m)), m) for m in modes) / len(modes) for o in origins3])
    return blend(mean, ob, oy, ox, ov, ovb, Cs, H, W)[0]
