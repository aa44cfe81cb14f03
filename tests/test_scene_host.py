"""The tile plan of whole-scene inference (mp_hsir_amd.scene.plan_axis / plan_tiles): pure host arithmetic, no library."""
import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import scene_ref as R


def check_axis(H, T, ov, grain):
    from mp_hsir_amd.scene import plan_axis
    th, o = plan_axis(H, T, ov, grain)
    assert (th, o) == R.plan_axis(H, T, ov, grain)
    assert th % grain == 0 and th == min(T, -(-H // grain) * grain)
    assert (len(o) == 1) == (H <= th)
    if len(o) == 1:
        assert o == [0] and th - H < grain
        return th, o
    assert o[0] == 0 and o[-1] + th == H and all(0 <= v <= H - th for v in o)
    assert all(b > a for a, b in zip(o, o[1:]))
    assert all(a + th - b >= ov for a, b in zip(o, o[1:])), "neighbours overlap by less than ov"
    cover = np.zeros(H, np.int64)
    for v in o:
        cover[v:v + th] += 1
    assert cover.min() >= 1 and cover.max() <= 3
    return th, o


@pytest.mark.parametrize("H,W,T,ov", R.SHAPES)
def test_plan_tiles_covers_the_scene(H, W, T, ov):
    from mp_hsir_amd.scene import plan_tiles
    th, oy = check_axis(H, T, ov, 64)
    tw, ox = check_axis(W, T, ov, 64)
    p = plan_tiles(H, W, T, ov)
    assert (p.th, p.tw, p.oy, p.ox) == (th, tw, oy, ox) == R.plan_tiles(H, W, T, ov)
    assert len(p) == len(oy) * len(ox) == p.ny * p.nx
    assert p.origins == [(y, x) for y in oy for x in ox]               # tile iy * nx + ix
    cover = np.zeros((H, W), np.int64)
    for y, x in p.origins:
        cover[y:y + th, x:x + tw] += 1
    assert cover.min() >= 1 and cover.max() <= 9


def test_blending_the_tiles_of_the_products_plan_gives_the_scene_back_fp64():
    """mp_hsir_amd.scene's plan under the fp64 definitions of the gather and the blend (no kernel): cutting a scene at the plan's
    origins and blending the pieces is the identity -- for the padded geometries too"""
    from mp_hsir_amd.scene import plan_tiles
    rng = np.random.default_rng(0)
    for H, W, T, ov in R.SHAPES[:3] + R.SHAPES[-2:] + R.PADDED_SHAPES:
        p = plan_tiles(H, W, T, ov)
        assert (R.padded_positions(p.oy, p.ox, p.th, p.tw, H, W) > 0) == ((H, W, T, ov) in R.PADDED_SHAPES)
        scene = rng.random((3, H, W))
        back, _ = R.blend(R.gather(scene, p.origins, p.th, p.tw), p.oy, p.ox, p.ov, H, W)
        assert np.abs(back - scene).max() < 1e-14


@settings(max_examples=300, deadline=None)
@given(st.sampled_from([32, 64]), st.integers(1, 8), st.integers(0, 3000), st.data())
def test_plan_axis_sweep(grain, tmul, extra, data):
    T = grain * tmul
    ov = data.draw(st.integers(0, T // 2))
    check_axis(grain + extra, T, ov, grain)


def test_plan_refuses_what_it_does_not_cover():
    from mp_hsir_amd.scene import plan_axis, plan_tiles
    for args in [(63, 64, 16, 64), (31, 32, 0, 32), (100, 96, 16, 64), (100, 48, 0, 32), (100, 0, 0, 64), (100, 64, 33, 64), (100, 64, -1, 64),
                 (100, 64, 16, 16), (100, 64, 16, 8), (100, 128, 16, 128)]:
        with pytest.raises(ValueError):
            plan_axis(*args)
    with pytest.raises(ValueError):
        plan_tiles(100, 40, 64, 16)
    assert plan_axis(100, 64, 32, 64)[0] == 64 and plan_axis(40, 32, 16, 32)[0] == 32
