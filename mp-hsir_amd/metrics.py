"""Band-wise PSNR / SSIM on the device: compute_psnr_ssim / compute_psnr_ssim2 of the reference
(utils/val_utils.py:49-105) without skimage and without a host round trip per band.

The reference loops over images and bands on the CPU calling skimage's peak_signal_noise_ratio and structural_similarity
(data_range=1, defaults: 7x7 uniform window, sample covariance, mean over the interior).  Here both are batched tensor
programs over (B,C,H,W): the 7x7 window means are one avg_pool2d each ("valid" windows = exactly the interior skimage
averages over).  Accumulation in float64 like skimage.  PyTorch device ops (evaluation side of the boundary)."""
import torch
import torch.nn.functional as F


def _clip01(t):
    return t.detach().double().clamp(0, 1)


def psnr_bands(restored, clean):
    """(B,C) band-wise PSNR, data_range 1."""
    mse = ((_clip01(restored) - _clip01(clean)) ** 2).mean(dim=(-1, -2))
    return 10.0 * torch.log10(1.0 / mse)


def ssim_bands(restored, clean, win=7, k1=0.01, k2=0.03):
    """(B,C) band-wise SSIM with skimage's defaults (uniform window, sample covariance NP/(NP-1), interior mean)."""
    x, y = _clip01(restored), _clip01(clean)
    B, C, H, W = x.shape
    x, y = x.reshape(B * C, 1, H, W), y.reshape(B * C, 1, H, W)
    npx = win * win
    cov_norm = npx / (npx - 1.0)
    pool = lambda t: F.avg_pool2d(t, win, stride=1)
    ux, uy = pool(x), pool(y)
    vx = cov_norm * (pool(x * x) - ux * ux)
    vy = cov_norm * (pool(y * y) - uy * uy)
    vxy = cov_norm * (pool(x * y) - ux * uy)
    c1, c2 = k1 ** 2, k2 ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return s.mean(dim=(-1, -2, -3)).reshape(B, C)


def compute_psnr_ssim(restored, clean):
    """-> (mean PSNR, mean SSIM, B): mean over bands, then over images (val_utils.py:49-69)."""
    assert restored.shape == clean.shape
    return float(psnr_bands(restored, clean).mean(1).mean()), float(ssim_bands(restored, clean).mean(1).mean()), restored.shape[0]


def compute_psnr_ssim2(restored, clean, degraded=None):
    """compute_psnr_ssim2 (val_utils.py:71-105): with `degraded`, only bands that are entirely zero in it are scored (band
    completion, test mode 10); images without such a band do not count.  -> (psnr, ssim, count)."""
    if degraded is None:
        return compute_psnr_ssim(restored, clean)
    use = (degraded == 0).flatten(2).all(dim=2)                     # (B,C)
    p, s = psnr_bands(restored, clean), ssim_bands(restored, clean)
    n = use.sum(1)
    ok = n > 0
    count = int(ok.sum())
    if count == 0:
        return 0.0, 0.0, 0
    pm = (p * use).sum(1)[ok] / n[ok]
    sm = (s * use).sum(1)[ok] / n[ok]
    return float(pm.mean()), float(sm.mean()), count


# ---- the fused path: one HIP launch pair instead of the tensor programs above (csrc/quality.hip) --------------------------------------
def quality_bands(restored, clean):
    """-> (psnr (B,C), ssim (B,C), sam_deg (B,), sam_pixels (B,)) on the device: ops.quality_bands (definitions: include/mphsir.h)."""
    from . import ops
    return ops.quality_bands(restored, clean)


def compute_quality(restored, clean, degraded=None):
    """compute_psnr_ssim / compute_psnr_ssim2 through the fused kernel, plus the spectral angle: -> dict(psnr, ssim, sam, count) of
    Python floats (count an int).  Bands are selected and images averaged as there: with `degraded`, only the bands that are entirely
    zero in it are scored and images without one do not count (psnr = ssim = sam = 0.0 when none counts).  `sam` is the mean over
    the images that count of the mean spectral angle in degrees, always taken over all C bands.  fp32 inputs are read as they are; one
    device-to-host transfer, at the end."""
    assert restored.shape == clean.shape
    r = restored.detach()
    c = clean.detach()
    r = (r if r.dtype == torch.float32 else r.float()).contiguous()
    c = (c if c.dtype == torch.float32 else c.float()).contiguous()
    if r.dim() == 3:
        r, c = r[None], c[None]
    p, s, sam, _ = quality_bands(r, c)
    if degraded is None:
        B = r.shape[0]
        out = torch.stack([p.mean(1).mean(), s.mean(1).mean(), sam.mean()]).tolist()
        return dict(psnr=out[0], ssim=out[1], sam=out[2], count=B)
    use = (degraded == 0).flatten(2).all(dim=2)                     # (B,C)
    n = use.sum(1)
    ok = n > 0
    nd = n.clamp(min=1).double()
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    pm = torch.where(use, p, zero).sum(1) / nd                      # where, not a product: an unscored band may hold inf or NaN
    sm = torch.where(use, s, zero).sum(1) / nd
    cnt = ok.sum()
    cd = cnt.clamp(min=1).double()
    out = torch.stack([torch.where(ok, pm, zero).sum() / cd, torch.where(ok, sm, zero).sum() / cd, torch.where(ok, sam, zero).sum() / cd,
                       cnt.double()]).tolist()
    return dict(psnr=out[0], ssim=out[1], sam=out[2], count=int(out[3]))
