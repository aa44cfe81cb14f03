"""The per-slice bound of the kernel parity checks (tests/slices.py, kernel_checks.close) on the CPU: no false alarm on correctly
rounded fields at the shapes of the checks, SLICE_F re-measured against its recorded basis, and planted localised faults that the
whole-tensor comparison lets through and `close` names by axis and index."""
import pytest
import torch

import kernel_checks as K
import slices
from util import rel_l2

# (shape, geom): the shapes the checks hand to `close`, the smallest edge shapes first
FIELD_SHAPES = [((64, 16), None), ((64, 32), None), ((1, 8, 8, 32), (1, 8, 8)), ((64, 64), (1, 8, 8)), ((1, 32), None), ((1, 8, 32), (1, 1, 8)),
                ((4,), None), ((32,), None), ((170,), None), ((9, 32), None), ((9, 96), None), ((225, 4), None), ((2, 128), None),
                ((128, 96), None), ((510, 96), None), ((512, 64), (2, 16, 16)), ((2, 16, 16, 128), (2, 16, 16)), ((2, 16, 24, 128), (2, 16, 24)),
                ((8, 64), (2, 16, 16)), ((3, 40, 24, 32), (3, 40, 24)), ((8192, 128), None), ((2, 32, 32, 384), (2, 32, 32))]
STORAGE = [torch.float32, torch.bfloat16, torch.float16]
_FIELDS = {}


def field(shape, seed=0):
    """an fp64 oracle output of that shape: the token GEMM's reference expression x W^T + b (kernel_checks.check_gemm_tok), K = 32"""
    key = (tuple(shape), seed)
    if key not in _FIELDS:
        g = torch.Generator().manual_seed(1000 + seed)
        n = shape[-1]
        m = 1
        for s in shape[:-1]:
            m *= s
        x = torch.randn((m, 32), generator=g, dtype=torch.float64)
        w = torch.randn((n, 32), generator=g, dtype=torch.float64) * 32 ** -0.5
        b = torch.randn((n,), generator=g, dtype=torch.float64) * 0.1
        _FIELDS[key] = (x @ w.t() + b).reshape(shape)
    return _FIELDS[key]


def measured_ratio():
    """max over storage types and FIELD_SHAPES of slice_err / rel_l2 of the field rounded once: the basis of K.SLICE_F"""
    worst = (0.0, None)
    for dt in STORAGE:
        for shape, geom in FIELD_SHAPES:
            ref = field(shape)
            got = ref.to(dt)
            r = slices.slice_err(got, ref, geom).err / rel_l2(got.double(), ref)
            if r > worst[0]:
                worst = (r, (str(dt), shape))
    return worst


# ---- no false alarm ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", STORAGE)
def test_rounded_fields_pass_close_at_the_project_tolerance(dt):
    for shape, geom in FIELD_SHAPES:
        ref = field(shape)
        K.close(ref.to(dt), ref, K.TOL[dt], geom=geom, what=str(shape))


def test_slice_factor_matches_its_measured_basis():
    r, at = measured_ratio()
    print("slice_err / rel_l2 of once-rounded oracle fields: max %.3f at %s (recorded %.2f, SLICE_F %.2f)" % (r, at, K.SLICE_RATIO_MEASURED, K.SLICE_F))
    assert r <= K.SLICE_RATIO_MEASURED, (r, at)
    assert r > 0.8 * K.SLICE_RATIO_MEASURED, "the recorded basis is stale: re-measure and lower it"
    assert K.SLICE_F == pytest.approx(1.5 * K.SLICE_RATIO_MEASURED, rel=1e-3) and K.SLICE_F_MAX == 4 * K.SLICE_F
    for key, (factor, cause) in K.SLICE_OVERRIDES.items():
        assert K.SLICE_F < factor <= K.SLICE_F_MAX, key


# ---- planted faults ------------------------------------------------------------------------------------------------------------
BF = torch.bfloat16
BIG, BIG_GEOM = (2, 32, 32, 384), (2, 32, 32)


def rounded(shape, seed=0):
    ref = field(shape, seed)
    return ref.to(BF).double(), ref


def fails(got, ref, tol, geom, expect):
    """`close` raises, and its message names `expect`"""
    with pytest.raises(AssertionError) as e:
        K.close(got, ref, tol, geom=geom, what="planted")
    msg = str(e.value)
    assert msg.startswith("planted: ") and all(s in msg for s in ([expect] if isinstance(expect, str) else expect)), msg
    return msg


def test_last_channel_zero():
    got, ref = rounded(BIG)
    got[..., -1] = 0
    assert rel_l2(got, ref) < K.GTOL[BF]                     # 1 / sqrt(384) = 0.051: what check_pgsstb_backward_oracle lets through today
    fails(got, ref, K.GTOL[BF], BIG_GEOM, "channel 383:")


def test_one_corner_pixel_zero():
    got, ref = rounded(BIG)
    got[1, 31, 0, :] = 0
    assert rel_l2(got, ref) < 2 * K.TOL[BF] and rel_l2(got, ref) < K.GTOL[BF]
    fails(got, ref, 2 * K.TOL[BF], BIG_GEOM, "token %d:" % (1 * 1024 + 31 * 32 + 0))


def test_top_image_row_scaled():
    got, ref = rounded(BIG)
    got[:, 0] *= 0.9
    assert rel_l2(got, ref) < 2 * K.TOL[BF] and rel_l2(got, ref) < K.GTOL[BF]
    fails(got, ref, 2 * K.TOL[BF], BIG_GEOM, "image row 0:")


def test_one_tile_of_16_tokens_with_8x_the_rounding_error():
    got, ref = rounded(BIG)
    g2, r2 = got.reshape(-1, 384), ref.reshape(-1, 384)
    tile = slice(37 * 16, 38 * 16)
    g2[tile] = r2[tile] + 8 * (g2[tile] - r2[tile])
    assert rel_l2(got, ref) < K.TWIN[BF]                     # the fp32 twins' bound: 0.0021 under 4e-3
    msg = fails(got, ref, K.TWIN[BF], BIG_GEOM, "token ")
    tok = int(msg.split("token ")[1].split(":")[0])
    assert 37 * 16 <= tok < 38 * 16, msg


def test_droppath_factor_on_the_wrong_sample():
    got, ref = rounded(BIG)
    got, ref = got.reshape(32, 8, 8, 384), ref.reshape(32, 8, 8, 384)          # the same tokens as 32 samples of 8 x 8
    got[19] *= 1.25
    assert rel_l2(got, ref) < K.GTOL[BF]                     # 0.25 / sqrt(32) = 0.044
    fails(got, ref, K.GTOL[BF], (32, 8, 8), "sample 19:")


def test_one_column_of_a_tap_gradient_zero():
    got, ref = rounded((9, 384))
    got[:, 200] = 0
    assert rel_l2(got, ref) < K.GTOL[BF]
    fails(got, ref, K.GTOL[BF], None, "channel [200:202):")      # 9 taps per channel: two channels make a slice of 18


def test_one_token_row_zero_in_one_window():
    """64 tokens: a zero row is 1/8 of the whole-tensor norm, which no tolerance of the checks lets through -- what `close` adds here is
    the place"""
    got, ref = rounded((1, 8, 8, 32))
    got[0, 5, 2, :] = 0
    assert 0.06 < rel_l2(got, ref) < 0.25
    fails(got.reshape(64, 32), ref.reshape(64, 32), K.GTOL[BF], (1, 8, 8), ["whole-tensor", "token 42:"])
    # at a tolerance wide enough for the whole tensor the slice bound still refuses it
    fails(got.reshape(64, 32), ref.reshape(64, 32), 0.25, (1, 8, 8), "token 42:")


def test_a_single_nan():
    for shape, geom, at in ((BIG, BIG_GEOM, (1, 7, 30, 381)), ((1, 8, 8, 32), (1, 8, 8), (0, 0, 0, 0)), ((170,), None, (169,))):
        got, ref = rounded(shape)
        got[at] = float("nan")
        w = slices.slice_err(got, ref, geom)
        assert w.err == float("inf") and str(at) in w.name, w
        fails(got, ref, K.GTOL[BF], geom, "non-finite at index %s" % (at,))
        got[at] = float("inf")
        fails(got, ref, K.GTOL[BF], geom, "non-finite at index %s" % (at,))
    # NaN in the reference itself: the statistic is NaN, and NaN passes no `<`
    got, ref = rounded((64, 32))
    ref = ref.clone()
    ref[3, 3] = float("nan")
    assert slices.slice_err(got, ref).err != slices.slice_err(got, ref).err
    with pytest.raises(AssertionError):
        K.close(got, ref, 1.0)


# ---- quiet slices --------------------------------------------------------------------------------------------------------------
def test_an_all_zero_sample_does_not_fail():
    got, ref = rounded((2, 16, 16, 64))
    got, ref = got.clone(), ref.clone()
    got[1], ref[1] = 0, 0                                    # DropPath keep = 0 on both sides
    got[..., 60:], ref[..., 60:] = 0, 0                      # padded channels
    K.close(got, ref, K.TOL[BF], geom=(2, 16, 16), what="quiet")
    assert slices.slice_err(got, ref, (2, 16, 16)).err < 2.0 ** -8


def test_a_slice_with_tiny_reference_is_normalised_by_the_global_rms():
    ref = field((512, 64)).clone()
    ref[:, 5] *= 1e-6
    got = ref.clone()
    g_rms = float(ref.square().mean().sqrt())
    got[:, 5] += 1e-3 * g_rms                                # 1000 x the channel's own size, 1e-3 of the tensor's
    w = slices.slice_err(got, ref)
    assert (w.name, w.index) == ("channel", 5) and w.err == pytest.approx(1e-3, rel=1e-6), w
    K.close(got, ref, K.TOL[BF], what="tiny reference")


def test_small_slices_are_grouped():
    assert slices._blocks(9, 384) == ([0, 1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8, 9])
    assert slices._blocks(384, 9) == (list(range(0, 384, 2)), list(range(2, 386, 2)))
    assert slices._blocks(170, 1) == (list(range(0, 160, 16)), list(range(16, 160, 16)) + [170])          # the tail of 10 joins the block before
    assert slices._blocks(4, 1) == ([0], [4])
    w = slices.slice_err(torch.zeros(()), torch.ones(()))
    assert w.err == 1.0


def test_counters_move():
    before = list(K.SLICE_STATS.get("test_counters_move", [0, 0.0, ""]))
    ref = field((64, 32))
    K.close(ref.to(BF), ref, K.TOL[BF], what="y")
    after = K.SLICE_STATS["test_counters_move"]
    assert after[0] == before[0] + 1 and 0 < after[1] < K.SLICE_F
