"""Scene quality on the CPU: the two kernels of mp-hsir_amd/csrc/quality.hip through the emulated build against the float64 restatement in
tests/quality_ref.py, and metrics.compute_quality against the oracle's compute_psnr_ssim.  Small shapes only: the fibers are slow."""
import ctypes
import math

import numpy as np
import pytest
import torch

import quality_ref as Q
from emu import bind_emulator
from oracle import degrade_oracle as O

PSNR_FACTOR = 10.0 / math.log(10.0)          # d psnr = (10 / ln 10) d mse / mse


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


def _run(restored, clean):
    from mp_hsir_amd import ops
    p, s, a, n = ops.quality_bands(torch.from_numpy(restored), torch.from_numpy(clean))
    assert p.dtype == s.dtype == a.dtype == torch.float64 and n.dtype == torch.int64
    return p.numpy(), s.numpy(), a.numpy(), n.numpy()


def _compare(restored, clean, label):
    B, C, H, W = restored.shape
    p, s, a, n = _run(restored, clean)
    assert p.shape == s.shape == (B, C) and a.shape == n.shape == (B,)
    mse, psnr, ssim = Q.bands(restored, clean)
    bar = Q.tol(H, W)
    d_ssim = np.abs(s - ssim).max()
    d_psnr = np.abs(p - psnr).max()
    d_mse = (np.abs(10.0 ** (-p / 10.0) - mse) / mse).max()
    sam, pixels = Q.sam_half_angle(restored, clean)
    d_sam = np.abs(a - sam).max()
    print("%s %s: ssim %.3f..%.3f  |d ssim| %.3g  |d mse|/mse %.3g (bar %.3g)  |d psnr| %.3g (bar %.3g)  sam %.4g deg  |d sam| %.3g (bar %.3g)"
          % (label, (B, C, H, W), ssim.min(), ssim.max(), d_ssim, d_mse, bar, d_psnr, PSNR_FACTOR * bar, sam.mean(), d_sam, Q.SAM_TOL_DEG))
    assert d_ssim <= bar
    assert d_psnr <= PSNR_FACTOR * bar
    assert d_mse <= bar + 1e-14                      # mse recovered from the psnr output: 1e-14 for the rounding of that pow
    assert np.array_equal(n, pixels)
    assert d_sam <= Q.SAM_TOL_DEG
    return ssim, sam


# H and W not multiples of the 32 x 32 block; W % 4 != 0; an axis of exactly 7 (one window); an axis shorter than one block; B = 2; C in {1, 5, 31}
SHAPES = [(1, 5, 45, 50), (1, 31, 7, 41), (1, 1, 20, 7), (2, 5, 33, 70), (1, 31, 40, 37), (2, 1, 64, 32)]


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_noise_matches_the_definition(B, C, H, W):
    _compare(*Q.noisy_pair(B, C, H, W, seed=1), "noise")


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_smooth_cube_matches_the_definition(B, C, H, W):
    ssim, _ = _compare(*Q.smooth_pair(B, C, H, W, seed=2), "smooth")
    assert 0.1 <= ssim.mean() <= 0.6, "the smooth input is meant to sit where the structure term matters (mean ssim %.3f)" % ssim.mean()


@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_inputs_outside_01_are_clipped(B, C, H, W):
    r, c = Q.overshoot_pair(B, C, H, W, seed=3)
    assert r.min() < -0.2 and r.max() > 1.2 and c.min() < -0.2 and c.max() > 1.2
    _compare(r, c, "overshoot")


@pytest.mark.parametrize("sigma", [None, 0.1, 1e-3, 1e-4, 6e-5])
def test_spectral_angle_from_small_to_large(sigma):
    """mean angles from 0.005 to 45 degrees (sigma None: two independent cubes); the half-angle and the arccos restatements agree to
    1e-9 degrees there, which pins the definition itself"""
    B, C, H, W = 1, 31, 24, 40
    r, c = Q.noisy_pair(B, C, H, W, seed=4, sigma=sigma or 0.0)
    if sigma is None:
        r = np.random.default_rng(5).random((B, C, H, W), dtype=np.float32)
    half, n1 = Q.sam_half_angle(r, c)
    acos, n2 = Q.sam_arccos(r, c)
    assert 0.005 <= half.mean() <= 45.0, half
    assert np.array_equal(n1, n2) and np.abs(half - acos).max() <= Q.SAM_TOL_DEG
    _, _, a, n = _run(r, c)
    print("sigma %s: sam %.6g deg, kernel - half-angle %.3g, half-angle - arccos %.3g" % (sigma, half[0], np.abs(a - half).max(), np.abs(half - acos).max()))
    assert np.array_equal(n, n1) and np.abs(a - half).max() <= Q.SAM_TOL_DEG


def test_identical_inputs():
    _, c = Q.noisy_pair(2, 5, 33, 45, seed=6)
    p, s, a, n = _run(c, c)
    assert np.abs(s - 1.0).max() <= 1e-12
    assert np.all(np.isposinf(p))
    assert np.all(a == 0.0) and np.all(n == 33 * 45)


def test_pixels_without_a_spectrum_are_left_out():
    r, c = Q.noisy_pair(2, 5, 40, 37, seed=7)
    r, c = np.clip(r, 0.01, 1), np.clip(c, 0.01, 1)          # every other pixel has a norm
    r[0, :, 3:6, :] = 0
    c[1, :, 35:, :] = -0.5                                   # clipped to 0
    c[1, :, 0, 0:2] = 0
    p, s, a, n = _run(r, c)
    assert n.tolist() == [37 * 37, 35 * 37 - 2]
    sam, pixels = Q.sam_half_angle(r, c)
    assert np.array_equal(n, pixels) and np.abs(a - sam).max() <= Q.SAM_TOL_DEG
    z = np.zeros((1, 3, 9, 9), dtype=np.float32)
    p, s, a, n = _run(z, z + 0.5)
    assert n.tolist() == [0] and a.tolist() == [0.0]


def test_a_nan_poisons_its_band_and_the_angle_only():
    r, c = Q.noisy_pair(2, 5, 45, 50, seed=8)
    p0, s0, a0, n0 = _run(r, c)
    bad = r.copy()
    bad[1, 2, 40, 33] = np.nan
    p1, s1, a1, n1 = _run(bad, c)
    assert np.isnan(p1[1, 2]) and np.isnan(s1[1, 2]) and np.isnan(a1[1])
    keep = np.ones((2, 5), dtype=bool)
    keep[1, 2] = False
    assert np.array_equal(p1[keep].view(np.int64), p0[keep].view(np.int64)) and np.array_equal(s1[keep].view(np.int64), s0[keep].view(np.int64))
    assert a1[0].tobytes() == a0[0].tobytes() and np.array_equal(n1, n0)


def test_two_calls_are_bitwise_equal():
    r, c = Q.smooth_pair(2, 5, 45, 70, seed=9)
    one, two = _run(r, c), _run(r, c)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()


def test_a_cube_without_batch_axis_is_a_batch_of_one():
    r, c = Q.noisy_pair(1, 5, 20, 33, seed=10)
    from mp_hsir_amd import ops
    p, s, a, n = ops.quality_bands(torch.from_numpy(r[0]), torch.from_numpy(c[0]))
    want = _run(r, c)
    assert p.shape == (1, 5) and a.shape == (1,)
    for x, y in zip((p, s, a, n), want):
        assert x.numpy().tobytes() == y.tobytes()


# ---- metrics.compute_quality ----------------------------------------------------------------------------------------------------------
def _close(q, want, H, W):
    bar = Q.tol(H, W)
    assert q["count"] == want[2]
    assert abs(q["psnr"] - want[0]) <= PSNR_FACTOR * bar and abs(q["ssim"] - want[1]) <= bar, (q, want)


def test_compute_quality_equals_the_oracle():
    from mp_hsir_amd import metrics
    B, C, H, W = 3, 5, 20, 33
    r, c = Q.noisy_pair(B, C, H, W, seed=11)
    q = metrics.compute_quality(torch.from_numpy(r), torch.from_numpy(c))
    _close(q, O.compute_psnr_ssim(r, c), H, W)
    sam, _ = Q.sam_half_angle(r, c)
    assert abs(q["sam"] - sam.mean()) <= Q.SAM_TOL_DEG and all(type(q[k]) is float for k in ("psnr", "ssim", "sam")) and type(q["count"]) is int
    d = np.random.default_rng(12).random((B, C, H, W), dtype=np.float32) + 0.1
    d[0, 1] = 0
    d[0, 4] = 0
    d[2, 0] = 0                                              # image 1 has no zero band: it does not count
    q = metrics.compute_quality(torch.from_numpy(r), torch.from_numpy(c), torch.from_numpy(d))
    _close(q, O.compute_psnr_ssim(r, c, d), H, W)
    assert q["count"] == 2 and abs(q["sam"] - (sam[0] + sam[2]) / 2) <= Q.SAM_TOL_DEG
    r2 = c.copy()                                            # every unscored band identical (psnr +inf): it must not leak into the means
    r2[0, [1, 4]] = r[0, [1, 4]]
    r2[2, 0] = r[2, 0]
    q2 = metrics.compute_quality(torch.from_numpy(r2), torch.from_numpy(c), torch.from_numpy(d))
    assert math.isfinite(q2["psnr"])
    _close(q2, O.compute_psnr_ssim(r2, c, d), H, W)
    none = metrics.compute_quality(torch.from_numpy(r), torch.from_numpy(c), torch.from_numpy(np.abs(d) + 1))
    assert (none["psnr"], none["ssim"], none["count"]) == (0.0, 0.0, 0) and O.compute_psnr_ssim(r, c, np.abs(d) + 1) == (0.0, 0.0, 0)


# ---- refusals: an error with a message, nothing launched --------------------------------------------------------------------------------
def test_ops_refuse_what_the_kernels_do_not_take():
    from mp_hsir_amd import ops
    r, c = (torch.from_numpy(a) for a in Q.noisy_pair(1, 3, 12, 12, seed=13))
    with pytest.raises(RuntimeError, match="H, W >= 7"):
        ops.quality_bands(r[:, :, :6].contiguous(), c[:, :, :6].contiguous())
    with pytest.raises(AssertionError, match="fp32"):
        ops.quality_bands(r.double(), c.double())
    with pytest.raises(AssertionError, match="contiguous"):
        ops.quality_bands(r.transpose(2, 3), c.transpose(2, 3))
    with pytest.raises(AssertionError, match="one shape"):
        ops.quality_bands(r, c[:, :2].contiguous())


def test_the_entry_point_refuses_bad_arguments():
    import mp_hsir_amd._lib as L
    lib = L.load()
    B, C, H, W = 1, 3, 12, 12
    r, c = (torch.from_numpy(a) for a in Q.noisy_pair(B, C, H, W, seed=14))
    need = lib.mphsir_quality_workspace_bytes(B, C, H, W)
    assert need == 16 * (C + 1) * 1 * B
    assert lib.mphsir_quality_workspace_bytes(B, C, 6, W) < 0 and lib.mphsir_quality_workspace_bytes(B, C, H, 6) < 0
    assert lib.mphsir_quality_workspace_bytes(0, C, H, W) < 0 and lib.mphsir_quality_workspace_bytes(B, C, 65536, 32768) < 0
    assert lib.mphsir_quality_workspace_bytes(2, 31, 1024, 1000) == 16 * 32 * 32 * 32 * 2
    ws = torch.zeros(need // 8, dtype=torch.float64)
    outs = [torch.full((B, C), -7.0, dtype=torch.float64), torch.full((B, C), -7.0, dtype=torch.float64), torch.full((B,), -7.0, dtype=torch.float64),
            torch.full((B,), -7, dtype=torch.int64)]

    def args(**kw):
        a = L.QualityArgs(restored=r.data_ptr(), clean=c.data_ptr(), psnr=outs[0].data_ptr(), ssim=outs[1].data_ptr(), sam_deg=outs[2].data_ptr(),
                          sam_pixels=outs[3].data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need, B=B, C=C, H=H, W=W)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.mphsir_quality(ctypes.byref(a), None) == -1
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()
        assert all(float(o.double().min()) == -7.0 == float(o.double().max()) for o in outs) and float(ws.abs().max()) == 0.0, "something was launched"

    refused(args(struct_size=ctypes.sizeof(L.QualityArgs) - 8), "struct_size")
    refused(args(workspace_bytes=need - 1), "workspace")
    refused(args(H=6), "7 x 7")
    refused(args(W=6), "7 x 7")
    refused(args(psnr=None), "null pointer")
    refused(args(workspace=None), "null pointer")
    refused(args(B=65536), "bad sizes")
    assert lib.mphsir_quality(ctypes.byref(args()), None) == 0 and float(outs[0].min()) > 0
    assert lib.mphsir_kernel_name(33) == b"quality"
