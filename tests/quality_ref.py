"""TEST INFRASTRUCTURE: the scene-quality contract of include/mphsir.h (mphsir_quality) restated in numpy float64.

PSNR / SSIM come from oracle.degrade_oracle.psnr_band / ssim_band (pinned to the reference and to closed forms by tests/test_degrade.py).
The spectral angle is restated here from the formula, in the half-angle form the kernel uses and in the textbook arccos form beside it.

The tolerance rule (shared by the emulator and the GPU tests):  |d ssim| and |d mse| / mse <= max(1e-12, H W 2^-53), |d psnr| <=
(10 / ln 10) times that.  1e-12 is the project's bar for its float64 metrics (tests/test_degrade.py); H W 2^-53 is the worst-case
reordering error of a sum of H W terms.  SAM: 1e-9 degrees against the half-angle restatement (the two float64 forms themselves differ by
up to 2.6e-11 degrees at a mean angle of 0.005 degrees: the arccos form's conditioning)."""
import numpy as np

from oracle import degrade_oracle as O

SAM_TOL_DEG = 1e-9


def tol(H, W):
    return max(1e-12, H * W * 2.0 ** -53)


def clip01(a):
    """the kernel's clip: comparisons, so that a NaN stays a NaN (np.clip would keep it too; written out to mirror the contract)"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(a < 0, 0.0, np.where(a > 1, 1.0, a))


def bands(restored, clean):
    """(B,C,H,W) -> mse (B,C), psnr (B,C), ssim (B,C) in float64"""
    r, c = clip01(restored), clip01(clean)
    B, C = r.shape[:2]
    mse, psnr, ssim = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
    for b in range(B):
        for ch in range(C):
            mse[b, ch] = np.mean((r[b, ch] - c[b, ch]) ** 2)
            with np.errstate(divide="ignore"):
                psnr[b, ch] = O.psnr_band(r[b, ch], c[b, ch])
            ssim[b, ch] = O.ssim_band(r[b, ch], c[b, ch])
    return mse, psnr, ssim


def _norms(restored, clean):
    x, y = clip01(restored), clip01(clean)
    nx, ny = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))           # (B,H,W)
    return x, y, nx, ny, (nx != 0) & (ny != 0)


def _mean_deg(theta, keep):
    n = keep.reshape(keep.shape[0], -1).sum(1)
    s = np.where(keep, theta, 0.0).reshape(keep.shape[0], -1).sum(1)
    return np.where(n > 0, np.degrees(s / np.maximum(n, 1)), 0.0), n.astype(np.int64)


def sam_half_angle(restored, clean):
    """-> sam_deg (B,), sam_pixels (B,): theta = 2 atan2(sqrt(max(d2 - (nx - ny)^2, 0)), sqrt(max((nx + ny)^2 - d2, 0)))"""
    x, y, nx, ny, keep = _norms(restored, clean)
    d2 = ((x - y) ** 2).sum(1)
    theta = 2.0 * np.arctan2(np.sqrt(np.maximum(d2 - (nx - ny) ** 2, 0.0)), np.sqrt(np.maximum((nx + ny) ** 2 - d2, 0.0)))
    return _mean_deg(theta, keep)


def sam_arccos(restored, clean):
    """the same angle as arccos(<x,y> / (nx ny))"""
    x, y, nx, ny, keep = _norms(restored, clean)
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos(np.clip((x * y).sum(1) / (nx * ny), -1.0, 1.0))
    return _mean_deg(theta, keep)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def noisy_pair(B, C, H, W, seed=0, sigma=0.1):
    """uniform noise and the same plus Gaussian noise of sigma: SSIM ~0.9 at sigma 0.1, reaches outside [0,1]"""
    g = np.random.default_rng(seed)
    clean = g.random((B, C, H, W), dtype=np.float32)
    restored = (clean + sigma * g.standard_normal((B, C, H, W))).astype(np.float32)
    return restored, clean


def smooth_pair(B, C, H, W, seed=0, sigma=0.1):
    """a smooth cube (low-frequency waves, low local variance) against a noised copy: SSIM 0.1 .. 0.6 (0.37 at sigma 0.1), so that the structure term
    and the constants c1, c2 matter"""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ph = g.random((B, C, 1, 1)) * 6.28
    clean = (0.5 + 0.3 * np.sin(yy / 9.0 + ph) * np.cos(xx / 7.0 - ph)).astype(np.float32)
    restored = (clean + sigma * g.standard_normal((B, C, H, W))).astype(np.float32)
    return restored, clean


def overshoot_pair(B, C, H, W, seed=0):
    """both inputs reach well outside [0,1]: the clip decides a third of the samples"""
    g = np.random.default_rng(seed)
    clean = (g.random((B, C, H, W)) * 1.6 - 0.3).astype(np.float32)
    restored = (clean + 0.2 * g.standard_normal((B, C, H, W))).astype(np.float32)
    return restored, clean
