"""GPU-side degradation synthesiser: the reference's training / test degradations (utils/degradation_utils.py:25-284,
utils/dataset_utils.py:277-879) as batched tensor programs on the device the model runs on.

The reference degrades one (C,H,W) numpy patch at a time on DataLoader workers, drawing from the process-global
numpy / `random` state.  At thousands of patches per second per GPU that is the bottleneck, so here every
degradation is a *pure function of the clean cube and explicit random draws*:

    stripe_noise(x, bands, locs, vals)      # what the reference computes once np.random has produced bands/locs/vals

and `Draws` produces those draws on the device from a seeded torch.Generator.  The split is what makes parity
checkable: tests/golden/make_degrade_golden.py runs the REFERENCE functions under a seeded numpy state, replays the
same numpy calls to recover the draws they consumed, and stores (draws, output); the oracle restatement
(oracle/degrade_oracle.py) and these functions must reproduce the outputs from the draws (tests/test_degrade.py).

All functions take and return (B,C,H,W) float32 cubes; per-sample draws carry a leading batch axis.  PyTorch device ops
only (this is the loader side of the boundary, not the model hot path) -- except DegradationSynthesizer(fused=True), which builds a
plan of small tables with batched tensor ops, without a host synchronisation, and degrades the batch in ONE HIP launch
(csrc/degrade.hip, ops.degrade_batch; ops.degrade_planes, the tiled form, for planes beyond 128 x 128), and SceneDegrader, which does
the same for one whole cube under test.py's modes 0-10; the functions here stay the definition of every element value.
`file:line` = reference repository.
"""
import math

import torch
import torch.nn.functional as F

# ---- the degradation menu of ImageTransformDataset (utils/dataset_utils.py:112-122) -----------------------------------
DE_DICT = {
    "natural_scene": {"gaussianN": [(30, 70)], "complexN": [(10, 30, 50, 70), (0.05, 0.15), (0.1, 0.3, 0.5, 0.7), (0.05, 0.15)],
                      "blur": [(9, 15, 21)], "sr": [(2, 4, 8)], "inpaint": [(0.7, 0.8, 0.9)], "bandmiss": [(0.1, 0.2, 0.3)],
                      "motion_blur": [((15, 45),)], "cassi": [(0,)]},
    "remote_sensing": {"gaussianN": [(30, 70)], "complexN": [(10, 30, 50, 70), (0.05, 0.15), (0.1, 0.3, 0.5, 0.7), (0.05, 0.15)],
                       "blur": [(7, 11, 15)], "sr": [(2, 4, 8)], "inpaint": [(0.7, 0.8, 0.9)], "haze": [(0.5, 0.75, 1)],
                       "bandmiss": [(0.1, 0.2, 0.3)], "circle_blur": [(9,)], "poissonN": [(10,)]},
}


# ---- deterministic kernels ------------------------------------------------------------------------------------------
def gaussian_kernel2d(k):
    """(k,k) separable Gaussian of _apply_gaussian_blur (degradation_utils.py:95-102): sigma = 0.3((k-1)/2 - 1) + 0.8."""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = torch.arange(k, dtype=torch.float32)
    k1 = torch.exp(-((x - (k - 1) / 2) ** 2) / (2 * sigma ** 2))
    k1 = k1 / k1.sum()
    return k1.unsqueeze(0) * k1.unsqueeze(1)


def circle_kernel2d(k):
    """_apply_circle_blur (degradation_utils.py:114-123): Gaussian of sigma = radius inside the disc of radius k//2."""
    r = k // 2
    yy, xx = torch.meshgrid(torch.arange(k, dtype=torch.float32), torch.arange(k, dtype=torch.float32), indexing="ij")
    d = torch.sqrt((xx - r) ** 2 + (yy - r) ** 2)
    ker = torch.where(d <= r, torch.exp(-(d ** 2) / (2 * (r ** 2))), torch.zeros(()))
    return ker / ker.sum()


def square_kernel2d(k):
    return torch.full((k, k), 1.0 / (k * k))


def motion_kernel2d(k, angle):
    """_apply_motion_blur (degradation_utils.py:137-143): a horizontal line of 1/k through row (k-1)//2, rotated by `angle`
    degrees about (k/2, k/2) with cv2.getRotationMatrix2D + cv2.warpAffine (bilinear, zero border).  cv2 is not available
    offline, so this restates its published semantics: dst(x,y) = src(M^-1 (x,y)), M = [[a, b, (1-a)cx - b cy],
    [-b, a, b cx + (1-a) cy]], a = cos, b = sin.  Pinned at the angles where the warp maps pixel centres onto pixel centres (0, 90, 180,
    270: tests/test_degrade.py::test_motion_kernel_exact_angles); in between OpenCV rounds source coordinates to 1/32 pixel, which
    this float restatement does not reproduce (differences of the order of 1e-2 of a tap: unpinned, no cv2 to compare with)."""
    src = torch.zeros((k, k), dtype=torch.float64)
    src[int((k - 1) / 2), :] = 1.0 / k
    a, b = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    cx = cy = k / 2
    m = torch.tensor([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=torch.float64)
    minv = torch.linalg.inv(torch.cat([m, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)]))
    ys, xs = torch.meshgrid(torch.arange(k, dtype=torch.float64), torch.arange(k, dtype=torch.float64), indexing="ij")
    sx = minv[0, 0] * xs + minv[0, 1] * ys + minv[0, 2]
    sy = minv[1, 0] * xs + minv[1, 1] * ys + minv[1, 2]
    x0, y0 = torch.floor(sx), torch.floor(sy)
    out = torch.zeros((k, k), dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            w = (1 - (sx - x0 - dx).abs()) * (1 - (sy - y0 - dy).abs())
            ok = (xi >= 0) & (xi < k) & (yi >= 0) & (yi < k)
            out += torch.where(ok, src[yi.clamp(0, k - 1), xi.clamp(0, k - 1)] * w, torch.zeros((), dtype=torch.float64))
    return out.float()


def blur(x, kernel2d):
    """depthwise 2-D correlation with zero padding k//2 (F.conv2d, groups = bands), every *_blur of the reference."""
    C = x.shape[1]
    k = kernel2d.shape[-1]
    w = kernel2d.to(x.device, x.dtype).reshape(1, 1, k, k).expand(C, 1, k, k)
    return F.conv2d(x, w, padding=k // 2, groups=C)


def bicubic_downsample(x, factor):
    """_bicubic_downsample (degradation_utils.py:170-181): F.interpolate(bicubic, align_corners=True) to (H//f, W//f)."""
    H, W = x.shape[-2:]
    return F.interpolate(x, size=(H // factor, W // factor), mode="bicubic", align_corners=True)


def resize_nearest(x, factor):
    """_resize (degradation_utils.py:195-206): every low-resolution pixel replicated factor x factor times."""
    return x.repeat_interleave(factor, dim=-2).repeat_interleave(factor, dim=-1)


def super_resolution_input(x, factor):
    """the 'sr' degradation as the loaders emit it (single_degrade :427-428; Super_Resolution_Dataset :697-711)."""
    return resize_nearest(bicubic_downsample(x, factor), factor)


# ---- noise / masking given explicit draws ----------------------------------------------------------------------------
def gaussian_noise(x, sigma, noise):
    """_add_gaussian_noise (:25-31): x + N(0,1) * sigma, sigma (B,) already divided by 255."""
    return x + noise * sigma.reshape(-1, 1, 1, 1)


def gaussian_noise_non_iid(x, band_sigma, noise):
    """_add_gaussian_noise_non_iid (:33-39): one sigma per band, band_sigma (B,C) already divided by 255."""
    return x + noise * band_sigma[:, :, None, None]


def stripe_noise(x, band_mask, col_offset):
    """_add_stripe_noise (:41-55): in the chosen bands, the chosen columns are lowered by a per-column constant.
    band_mask (B,C) bool; col_offset (B,C,W) = the stripe value at the chosen (band, column) pairs, 0 elsewhere."""
    return x - (col_offset * band_mask[:, :, None])[:, :, None, :]


def deadline_noise(x, col_dead):
    """_add_deadline_noise (:57-68): chosen columns of chosen bands are zeroed.  col_dead (B,C,W) bool."""
    return x * (~col_dead)[:, :, None, :]


def impulse_noise(x, flipped, salted):
    """_add_impulse_noise (:70-84): where flipped, the pixel becomes 1 (salted) or 0 (peppered).  (B,C,H,W) bools, False in
    bands that were not chosen."""
    return torch.where(flipped, salted.to(x.dtype), x)


def random_mask(x, u, ratio):
    """_apply_random_mask (:235-241): keep where U[0,1) > ratio.  ratio (B,)."""
    return x * (u > ratio.reshape(-1, 1, 1, 1))


def band_loss(x, lost):
    """_simulate_band_loss (:285-293): lost (B,C) bool -> those bands are zero."""
    return x * (~lost)[:, :, None, None]


def haze(x, cirrus, omega, gamma=1.0, top_percent=0.01):
    """_simulate_haze (:243-283) given the cirrus-band map already resized to (H,W): cirrus (B,H,W), omega (B,).
    atmospheric light = mean of the top max(int(HW*top_percent/100),1) pixels per band; t1 = 1 - omega*cirrus (<= 0 -> 1e-10);
    transmission_c = t1 ** ((lambda_0/lambda_c) ** gamma) with lambda = linspace(400,1000,100) (so C <= 100)."""
    B, C, H, W = x.shape
    top_k = max(int(H * W * top_percent / 100), 1)
    atm = x.reshape(B, C, -1).topk(top_k, dim=-1).values.mean(-1)                       # (B,C)
    t1 = 1 - omega.reshape(B, 1, 1) * cirrus
    t1 = torch.where(t1 <= 0, torch.full_like(t1, 1e-10), t1)
    lam = torch.linspace(400, 1000, 100, device=x.device, dtype=torch.float64)[:C]
    ratio = ((lam[0] / lam) ** gamma).to(x.dtype)                                       # (C,)
    trans = torch.exp(ratio.reshape(1, C, 1, 1) * torch.log(t1).unsqueeze(1))
    return x * trans + atm[:, :, None, None] * (1 - trans)


def poisson_noise(x, scale, generator=None):
    """_apply_poisson (:86-89): Poisson(clip(x,0) * scale) / scale (distribution-level parity only)."""
    return torch.poisson(x.clamp_min(0) * scale, generator=generator) / scale


def cassi_measure(x, mask, origin=None, step=2):
    """_sd_cassi (:202-225), the coded-aperture snapshot measurement, and the DEFINITION of what csrc/cassi.hip computes: x (B,C,H,W) fp32,
    mask (MH,MW) fp32, origin (B,2) integer {my, mx} of the mask crop (clamped into the mask; None: (0,0)).  Every band is multiplied by the
    crop, moved `step` columns further per band and added to the measurement in ASCENDING band order (an explicit loop: the order of a
    sum(dim) is not ours to fix); band c of the result is the measurement's window at c * step; the whole sample is min-max normalised over
    its measurement.  A NaN in the measurement makes the sample NaN, a constant measurement is all NaN (0 / 0)."""
    B, C, H, W = x.shape
    MH, MW = mask.shape
    if MH < H or MW < W:
        raise ValueError("cassi: a mask of %d x %d does not hold a plane of %d x %d" % (MH, MW, H, W))
    mask = mask.to(x.device, torch.float32)
    if origin is None:
        crop = mask[:H, :W].expand(B, H, W)
    else:
        origin = torch.as_tensor(origin, device=x.device).reshape(B, 2).long()
        my, mx = origin[:, 0].clamp(0, MH - H), origin[:, 1].clamp(0, MW - W)
        rows = my[:, None] + torch.arange(H, device=x.device)
        cols = mx[:, None] + torch.arange(W, device=x.device)
        crop = mask[rows[:, :, None], cols[:, None, :]]                                   # (B,H,W)
    meas = torch.zeros((B, H, W + (C - 1) * step), dtype=x.dtype, device=x.device)
    for c in range(C):
        meas[:, :, step * c:step * c + W] += x[:, c] * crop
    out = torch.stack([meas[:, :, step * c:step * c + W] for c in range(C)], dim=1)
    lo, hi = meas.amin(dim=(1, 2)).reshape(B, 1, 1, 1), meas.amax(dim=(1, 2)).reshape(B, 1, 1, 1)
    return (out - lo) / (hi - lo)


class CassiMask:
    """The coded aperture of the cassi task, resident on the device as fp32 (cast once, here): the 'mask' entry of a .mat file (as the
    reference reads it, degradation_utils.py:209-210), a .npy file, or -- path None -- a seeded Bernoulli(0.5) binary mask of `shape`.
    origins(): the per-sample crop origins, random.randint(0, MH - H) / (0, MW - W) in the reference (:211-212), from a Draws."""

    def __init__(self, device, path=None, seed=2024, shape=(256, 256)):
        if path is None:
            g = torch.Generator().manual_seed(int(seed))
            m = (torch.rand(tuple(shape), generator=g) < 0.5).to(torch.float32)
        elif str(path).endswith(".npy"):
            import numpy as np
            m = torch.from_numpy(np.load(path).astype("float32"))
        else:
            import scipy.io as sio
            m = torch.from_numpy(sio.loadmat(path)["mask"].astype("float32"))
        if m.dim() != 2:
            raise ValueError("cassi mask %s: a 2-D array is expected, got shape %s" % (path, tuple(m.shape)))
        self.path = path
        self.mask = m.contiguous().to(device)

    @property
    def shape(self):
        return tuple(self.mask.shape)

    def check(self, H, W):
        MH, MW = self.shape
        if MH < H or MW < W:
            raise ValueError("cassi mask %s of %d x %d is smaller than the %d x %d plane it has to cover" % (self.path or "(default)", MH, MW, H, W))

    def origins(self, d, B, H, W):
        """(B,2) int32 {my, mx} on the device, from the Draws d"""
        self.check(H, W)
        MH, MW = self.shape
        return torch.stack([d.randint(0, MH - H + 1, (B,)), d.randint(0, MW - W + 1, (B,))], dim=1).to(torch.int32).contiguous()


_SCENE_MASKS = {}


def scene_cassi_mask(opts, device, H, W):
    """the CassiMask of test.py's mode 13 for a cube of H x W (made once per file / extent): --cassi_mask, or the default mask of
    max(256, H) x max(256, W) seeded by --seed.  ValueError when the file's mask is smaller than the cube."""
    path = getattr(opts, "cassi_mask", "") or None
    shape = (max(256, H), max(256, W))
    key = (path, str(device)) if path else (None, str(device), int(opts.seed), shape)
    if key not in _SCENE_MASKS:
        _SCENE_MASKS[key] = CassiMask(device, path, seed=opts.seed, shape=shape)
    _SCENE_MASKS[key].check(H, W)
    return _SCENE_MASKS[key]


def augment(x, mode):
    """data_augmentation (utils/image_utils.py:141-176) per sample: mode (B,) in 0..7 = rot90 by mode//2 (counter-clockwise,
    axes (H,W)) then an up-down flip when mode is odd.  Square patches."""
    out = torch.empty_like(x)
    for m in range(8):
        sel = (mode == m).nonzero(as_tuple=True)[0]
        if sel.numel() == 0:
            continue
        t = torch.rot90(x[sel], k=m // 2, dims=(-2, -1))
        out[sel] = t.flip(-2) if m % 2 else t
    return out


def interpolate_bands(x, target_bands):
    """interpolate_bands (utils/image_utils.py:597-619): place the C source bands at round(linspace(0, T-1, C)) and fill the
    gaps linearly between neighbouring source bands."""
    B, C, H, W = x.shape
    idx = torch.round(torch.linspace(0, target_bands - 1, C, dtype=torch.float64)).long().tolist()
    out = torch.zeros((B, target_bands, H, W), dtype=x.dtype, device=x.device)
    out[:, idx] = x
    for i in range(C - 1):
        s, e = idx[i], idx[i + 1]
        n = e - s
        for j in range(1, n):
            pos = j / n
            out[:, s + j] = x[:, i] * (1 - pos) + x[:, i + 1] * pos
    return out


# ---- draws ---------------------------------------------------------------------------------------------------------------
class Draws:
    """Random draws of the degradations on the device, from one seeded torch.Generator (replaces the reference's global
    numpy / random state).  Distributions follow the reference's calls; the streams differ."""

    def __init__(self, device, seed):
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device).manual_seed(seed)

    def rand(self, *shape):
        return torch.rand(shape, generator=self.gen, device=self.device)

    def randn(self, *shape):
        return torch.randn(shape, generator=self.gen, device=self.device)

    def randint(self, lo, hi, shape):
        return torch.randint(lo, hi, tuple(shape), generator=self.gen, device=self.device)

    def choice(self, values, n):
        v = torch.tensor(values, dtype=torch.float32, device=self.device)
        return v[self.randint(0, len(values), (n,))]

    def band_subset(self, B, C, count):
        """(B,C) bool with exactly `count` bands per sample: np.random.permutation(C)[:count]."""
        order = self.rand(B, C).argsort(dim=1)
        return order.argsort(dim=1) < count

    def column_subsets(self, B, C, W, n):
        """(B,C,W) bool with n[b,c] columns chosen uniformly without replacement per (sample, band)."""
        rank = self.rand(B, C, W).argsort(dim=2).argsort(dim=2)
        return rank < n[:, :, None]


def complex_noise(x, d, sigmas=(10, 30, 50, 70), deadline=(0.05, 0.15), impulse=(0.1, 0.3, 0.5, 0.7), stripe=(0.05, 0.15)):
    """'complexN' (:303-318): non-iid Gaussian noise, then per sample ONE of deadline / impulse / stripe noise on a random
    third of the bands.  Returns (degraded, type_idx (B,))."""
    B, C, H, W = x.shape
    nb = int(math.floor(C / 3))
    y = gaussian_noise_non_iid(x, d.choice([s / 255.0 for s in sigmas], B * C).reshape(B, C), d.randn(B, C, H, W))
    kind = d.randint(0, 3, (B,))
    bands = d.band_subset(B, C, nb)
    # deadline: n ~ randint(ceil(min W), ceil(max W)) columns zeroed
    nd = d.randint(math.ceil(deadline[0] * W), max(math.ceil(deadline[1] * W), math.ceil(deadline[0] * W) + 1), (B, C))
    dead = d.column_subsets(B, C, W, nd) & bands[:, :, None] & (kind == 0).reshape(B, 1, 1)
    y = deadline_noise(y, dead)
    # impulse: amount chosen per sample from the list, salt vs pepper 0.5
    amt = d.choice(list(impulse), B).reshape(B, 1, 1, 1)
    flipped = (d.rand(B, C, H, W) < amt) & bands[:, :, None, None] & (kind == 1).reshape(B, 1, 1, 1)
    y = impulse_noise(y, flipped, d.rand(B, C, H, W) < 0.5)
    # stripe: n ~ randint(floor(min W), floor(max W)) columns lowered by U(0,1)/2 - 1/4
    ns = d.randint(math.floor(stripe[0] * W), max(math.floor(stripe[1] * W), math.floor(stripe[0] * W) + 1), (B, C))
    cols = d.column_subsets(B, C, W, ns)
    off = (d.rand(B, C, W) * 0.5 - 0.25) * cols
    y = stripe_noise(y, bands & (kind == 2).reshape(B, 1), off)
    return y, kind


class DegradationSynthesizer:
    """ImageTransformDataset.__getitem__ (utils/dataset_utils.py:128-146) for a whole batch on the device: per sample a task
    id de_id ~ U{0..T-1}, the degradation of that task with its range from DE_DICT, one of 7 flip/rotation augmentations
    applied to both cubes; emits `degrad_patch, clean_patch, prompt (B,1) int64`.  `cirrus` (a callable (B,H,W) -> maps in
    [0,1]) supplies the haze maps the reference reads from .mat files (:245-257); default: smooth synthetic fields."""

    def __init__(self, data_type, de_types, device, seed=2024, cirrus=None, fused=False, cassi_mask=None, cassi_step=2):
        self.table, self.de_types = DE_DICT[data_type], list(de_types)
        for t in self.de_types:
            if t not in self.table:
                raise ValueError("degradation %r is not defined for %s" % (t, data_type))
        self.d = Draws(device, seed)
        self.cassi_step = int(cassi_step)
        self.cassi_mask = cassi_mask if cassi_mask is not None or "cassi" not in self.de_types else CassiMask(device, seed=seed)
        self.cirrus = cirrus or self._synthetic_cirrus
        self.fused = bool(fused)
        if self.fused:
            self._init_fused(seed)

    def _synthetic_cirrus(self, B, H, W):
        low = self.d.rand(B, 1, max(H // 16, 2), max(W // 16, 2))
        return F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)[:, 0]

    def degrade_as(self, x, de_type):
        """one degradation type for the whole batch x (B,C,H,W) -> degraded (B,C,H,W)"""
        d, rng = self.d, self.table[de_type]
        B, C, H, W = x.shape
        if de_type == "gaussianN":
            lo, hi = rng[0]
            return gaussian_noise(x, (lo + (hi - lo) * d.rand(B)) / 255.0, d.randn(B, C, H, W))
        if de_type == "complexN":
            return complex_noise(x, d, *rng)[0]
        if de_type in ("blur", "circle_blur", "motion_blur"):
            out = torch.empty_like(x)
            pick = d.randint(0, len(rng[0]), (B,))
            for i, k in enumerate(rng[0]):
                sel = (pick == i).nonzero(as_tuple=True)[0]
                if sel.numel():
                    ker = gaussian_kernel2d(k) if de_type == "blur" else circle_kernel2d(k) if de_type == "circle_blur" else motion_kernel2d(*k)
                    out[sel] = blur(x[sel], ker)
            return out
        if de_type == "sr":
            out = torch.empty_like(x)
            pick = d.randint(0, len(rng[0]), (B,))
            for i, f in enumerate(rng[0]):
                sel = (pick == i).nonzero(as_tuple=True)[0]
                if sel.numel():
                    out[sel] = super_resolution_input(x[sel], f)
            return out
        if de_type == "inpaint":
            return random_mask(x, d.rand(B, C, H, W), d.choice(list(rng[0]), B))
        if de_type == "bandmiss":
            frac = d.choice(list(rng[0]), B)
            n = (frac * C).long()                                                         # int(loss_percentage * B)
            return band_loss(x, d.rand(B, C).argsort(dim=1).argsort(dim=1) < n[:, None])
        if de_type == "haze":
            return haze(x, self.cirrus(B, H, W), d.choice(list(rng[0]), B))
        if de_type == "poissonN":
            return poisson_noise(x, float(rng[0][0]), generator=d.gen)
        if de_type == "cassi":
            return cassi_measure(x, self.cassi_mask.mask, self.cassi_mask.origins(d, B, H, W), self.cassi_step)
        raise ValueError("Invalid degradation type " + de_type)

    # ---- fused=True: a plan of small device tables (batched tensor ops, no host synchronisation) + ONE launch (csrc/degrade.hip) ----
    def _init_fused(self, seed):
        """everything that would otherwise be a host -> device copy inside the call: the value lists of DE_DICT as device tensors, the
        stencil table, the batch ordinal (a device scalar the launch reads: a captured call advances it by itself)."""
        from . import ops
        if "poissonN" in self.de_types:
            raise ValueError("poissonN has no fused form (its parity is distribution-level only): use fused=False for a menu with poissonN")
        dev = self.d.device
        self.seed = int(seed)
        self._menu = [ops.DEG_KINDS[t] for t in self.de_types]
        self._vals, self._st_base, kernels = {}, {}, []
        for name in self.de_types:
            rng = self.table[name]
            if name in ("blur", "circle_blur", "motion_blur"):
                self._st_base[name] = len(kernels)
                kernels += [gaussian_kernel2d(k) if name == "blur" else circle_kernel2d(k) if name == "circle_blur" else motion_kernel2d(*k)
                            for k in rng[0]]
            elif name == "complexN":
                self._vals["complexN/sigma"] = torch.tensor([v / 255.0 for v in rng[0]], dtype=torch.float32, device=dev)
                self._vals["complexN/amount"] = torch.tensor(list(rng[2]), dtype=torch.float32, device=dev)
            elif name in ("inpaint", "bandmiss", "haze"):
                self._vals[name] = torch.tensor(list(rng[0]), dtype=torch.float32, device=dev)
        self._ksize = [int(k.shape[-1]) for k in kernels]
        self._stencils = None
        if kernels:
            st = torch.zeros((len(kernels), 21, 21), dtype=torch.float32)
            for i, k in enumerate(kernels):
                st[i, :k.shape[0], :k.shape[1]] = k
            self._stencils = st.to(dev)
        self._factors = [int(f) for f in self.table["sr"][0]] if "sr" in self.de_types else []
        self._haze_ratio = {}
        self._ordinal = torch.full((1,), -1, dtype=torch.int64, device=dev)

    def _pick(self, key, n):
        v = self._vals[key]
        return v[self.d.randint(0, v.shape[0], (n,))]

    def fused_plan(self, clean):
        """-> (ops.DegradePlan, de_id (B,)): the draws `degrade_as` makes per type, made for the whole batch with batched tensor ops and
        merged by task id with torch.where -- no nonzero / item / boolean indexing, so nothing waits for the device."""
        from . import ops
        d = self.d
        B, C, H, W = clean.shape
        dev = clean.device
        de_id = d.randint(0, len(self.de_types), (B,))
        param = torch.zeros((B,), dtype=torch.float32, device=dev)
        sub = torch.zeros((B,), dtype=torch.int64, device=dev)
        tabs, flag, origin = {}, None, None
        for t, name in enumerate(self.de_types):
            rng, mine = self.table[name], de_id == t
            if name == "gaussianN":
                lo, hi = rng[0]
                param = torch.where(mine, (lo + (hi - lo) * d.rand(B)) / 255.0, param)
            elif name == "complexN":
                _, deadline, _, stripe = rng
                tabs["band_sigma"] = self._pick("complexN/sigma", B * C).reshape(B, C).contiguous()
                kind = d.randint(0, 3, (B,))
                bands = d.band_subset(B, C, int(math.floor(C / 3)))
                nd = d.randint(math.ceil(deadline[0] * W), max(math.ceil(deadline[1] * W), math.ceil(deadline[0] * W) + 1), (B, C))
                dead = d.column_subsets(B, C, W, nd) & bands[:, :, None] & (kind == 0).reshape(B, 1, 1)
                ns = d.randint(math.floor(stripe[0] * W), max(math.floor(stripe[1] * W), math.floor(stripe[0] * W) + 1), (B, C))
                cols = d.column_subsets(B, C, W, ns) & bands[:, :, None] & (kind == 2).reshape(B, 1, 1)
                tabs["col_dead"] = dead.to(torch.uint8)
                tabs["col_off"] = (d.rand(B, C, W) * 0.5 - 0.25) * cols
                param = torch.where(mine, self._pick("complexN/amount", B), param)
                sub = torch.where(mine, kind, sub)
                flag = bands if flag is None else torch.where(mine[:, None], bands, flag)
            elif name in ("blur", "circle_blur", "motion_blur"):
                sub = torch.where(mine, self._st_base[name] + d.randint(0, len(rng[0]), (B,)), sub)
            elif name == "sr":
                sub = torch.where(mine, d.randint(0, len(rng[0]), (B,)), sub)
            elif name == "inpaint":
                param = torch.where(mine, self._pick("inpaint", B), param)
            elif name == "bandmiss":
                n = (self._pick("bandmiss", B) * C).long()                              # int(loss_percentage * B)
                lost = d.rand(B, C).argsort(dim=1).argsort(dim=1) < n[:, None]
                flag = lost if flag is None else torch.where(mine[:, None], lost, flag)
            elif name == "haze":
                param = torch.where(mine, self._pick("haze", B), param)
                tabs["cirrus"] = self.cirrus(B, H, W).to(torch.float32).contiguous()
                top_k = max(int(H * W * 0.01 / 100), 1)
                flat = clean.reshape(B, C, -1)
                tabs["atm"] = flat.amax(dim=-1) if top_k == 1 else flat.topk(top_k, dim=-1).values.mean(-1)
                if C not in self._haze_ratio:
                    lam = torch.linspace(400, 1000, 100, device=dev, dtype=torch.float64)[:C]
                    self._haze_ratio[C] = (lam[0] / lam).to(torch.float32)
                tabs["haze_ratio"] = self._haze_ratio[C]
            elif name == "cassi":
                origin = self.cassi_mask.origins(d, B, H, W)
        if flag is not None:
            tabs["band_flag"] = flag.to(torch.uint8)
        plan = ops.DegradePlan(self._menu, self._ksize, self._factors, task=de_id.to(torch.int32), aug=d.randint(1, 8, (B,)).to(torch.int32),
                               param=param, sub=sub.to(torch.int32), stencils=self._stencils, **tabs)
        plan.cassi_origin = origin                  # not a table of the degradation launch: ops.cassi reads it (None without cassi in the menu)
        return plan, de_id

    def _call_fused(self, clean):
        from . import ops
        clean = clean.contiguous()
        plan, de_id = self.fused_plan(clean)
        cassi = self.de_types.index("cassi") if "cassi" in self.de_types else -1
        if cassi >= 0 and len(self.de_types) == 1:
            # the fine-tune menu: the cassi pair alone, which writes the augmented clean cube itself
            degraded, clean_aug = ops.cassi(clean, self.cassi_mask.mask, plan.cassi_origin, self.cassi_step, aug=plan.aug, want_clean_aug=True)
            return degraded, clean_aug, de_id.reshape(-1, 1)
        self._ordinal += 1                                                               # the batch ordinal counts calls, on the device
        # planes that fit in LDS whole keep the plane form's launch; larger ones go through the tiled form, which computes the same values
        H, W = clean.shape[-2:]
        fn = ops.degrade_batch if H * W <= 128 * 128 else ops.degrade_planes
        degraded, clean_aug = fn(clean, plan, seed=self.seed, ordinal=self._ordinal)
        if cassi >= 0:
            # cassi is kind `none` in that launch's menu (its samples left it as augmented copies); the pair overwrites exactly them,
            # selected on the device by the task table: no nonzero / item / boolean indexing
            ops.cassi(clean, self.cassi_mask.mask, plan.cassi_origin, self.cassi_step, aug=plan.aug, task=plan.task, task_id=cassi,
                      out=(degraded, None))
        return degraded, clean_aug, de_id.reshape(-1, 1)

    def __call__(self, clean):
        """clean (B,C,H,W) on the device -> (degraded, clean_augmented, prompt (B,1) int64)"""
        if self.fused:
            return self._call_fused(clean)
        B = clean.shape[0]
        de_id = self.d.randint(0, len(self.de_types), (B,))
        degraded = torch.empty_like(clean)
        for t, name in enumerate(self.de_types):
            sel = (de_id == t).nonzero(as_tuple=True)[0]
            if sel.numel():
                degraded[sel] = self.degrade_as(clean[sel], name)
        mode = self.d.randint(1, 8, (B,))                                                 # random.randint(1, 7)
        return augment(degraded, mode), augment(clean, mode), de_id.reshape(B, 1)


class SceneDegrader:
    """test.py's degradation modes 0-10 for one whole cube (1,C,H,W), any H and W, in ONE HIP launch (ops.degrade_planes): no cube-sized
    temporary, no library convolution, and a result that depends on (seed, cube ordinal, the plan) only -- the per-element draws are the
    launch's Philox draws keyed by the seed and the ordinal, which counts calls; the plan's small tables (per-band sigmas, band and column
    subsets, the cirrus map) come from a seeded torch.Generator with the expressions of test.py::degrade_for_mode.  `opts`: test.py's
    parsed flags.  Mode 11 (Poisson) has no fused form, mode 12 degrades nothing.  Mode 13 (the CASSI measurement) is the launch pair of
    ops.cassi with the mask of scene_cassi_mask and the origin test.py::degrade_for_mode draws: the tensor form's values."""
    PROMPT = {0: 0, 1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 0, 7: 3, 8: 4, 9: 5, 10: 5}

    def __init__(self, model, device, seed):
        self.model, self.device, self.seed = model, torch.device(device), int(seed)
        self.d = Draws(device, seed)
        self.ordinal = -1
        self._stencils, self._haze_ratio, self._consts = {}, {}, {}

    def prompt_id(self, mode):
        if mode == 13:
            return 0
        return 6 if mode == 10 and self.model != "natural_scene" else self.PROMPT[mode]

    def _const(self, shape, dtype, value, dev):
        """a constant table, made once (the launch only reads its tables): a plan of mode 0 or 1 costs no fill launches"""
        key = (tuple(shape), dtype, value)
        if key not in self._consts:
            self._consts[key] = torch.full(tuple(shape), value, dtype=dtype, device=dev)
        return self._consts[key]

    def _choice(self, values, n, dev):
        """Draws.choice with the value list kept on the device (no host -> device copy per cube)"""
        key = ("choice",) + tuple(values)
        if key not in self._consts:
            self._consts[key] = torch.tensor(values, dtype=torch.float32, device=dev)
        return self._consts[key][self.d.randint(0, len(values), (n,))]

    def _stencil(self, key, make):
        if key not in self._stencils:
            k = make()
            st = torch.zeros((1, 21, 21), dtype=torch.float32)
            if k.shape[-1] <= 21:
                st[0, :k.shape[0], :k.shape[1]] = k
            self._stencils[key] = (st.to(self.device), int(k.shape[-1]))               # a side beyond 21 (or even) is refused by the launch
        return self._stencils[key]

    def plan(self, clean, mode, opts):
        """-> ops.DegradePlan for one cube: one task, mode 0 of the augmentation (aug=None), the tables of `mode`"""
        from . import ops
        d, o, dev = self.d, opts, clean.device
        B, C, H, W = clean.shape
        assert B == 1, "SceneDegrader degrades one cube per call"
        if mode == 11:
            raise ValueError("mode 11 is Poisson noise, which has no fused form (poissonN: distribution-level parity only)")
        if mode not in self.PROMPT:
            raise ValueError("SceneDegrader: modes 0-10, got %r" % (mode,))
        nb = int(math.floor(C / 3))
        f32 = lambda v: self._const((B,), torch.float32, float(v), dev)                  # noqa: E731
        zero = lambda *shape, dt=torch.float32: self._const(shape, dt, 0, dev)           # noqa: E731
        task, tabs = zero(B, dt=torch.int32), {}
        kind, ksize, factors, param, sub = "none", [], [], 0.0, 0
        if mode == 0:
            kind, param = "gaussianN", f32(o.gaussian_noise_sigma / 255.0)
        elif mode <= 4:
            kind = "complexN"
            sigmas = o.gaussian_noise_sigmas if mode == 1 else (10, 30, 50, 70)
            tabs["band_sigma"] = self._choice([s / 255.0 for s in sigmas], B * C, dev).reshape(B, C)
            flag, dead, off = zero(B, C, dt=torch.uint8), zero(B, C, W, dt=torch.uint8), zero(B, C, W)
            if mode == 2:
                lo, hi = o.stripe_nosie_ratio
                bands = d.band_subset(B, C, nb)
                n = d.randint(int(lo * W), max(int(hi * W), int(lo * W) + 1), (B, C))
                cols = d.column_subsets(B, C, W, n) & bands[:, :, None]
                off, sub = (d.rand(B, C, W) * 0.5 - 0.25) * cols, 2
            elif mode == 3:
                lo, hi = o.deadline_nosie_ratio
                bands = d.band_subset(B, C, nb)
                n = d.randint(int(math.ceil(lo * W)), max(int(math.ceil(hi * W)), int(math.ceil(lo * W)) + 1), (B, C))
                dead = d.column_subsets(B, C, W, n) & bands[:, :, None]
            elif mode == 4:
                flag, sub = d.band_subset(B, C, nb), 1
                param = self._choice(list(o.impulse_nosie_ratio), B, dev)
            tabs.update(band_flag=flag.to(torch.uint8), col_dead=dead.to(torch.uint8), col_off=off.contiguous())
        elif mode in (5, 6):
            kind = "blur"
            if mode == 5:
                st, k = self._stencil(("gaussian", o.gaussian_blur_radius), lambda: gaussian_kernel2d(o.gaussian_blur_radius))
            else:
                st, k = self._stencil(("motion",) + tuple(o.motion_blur_radius), lambda: motion_kernel2d(*o.motion_blur_radius))
            tabs["stencils"], ksize = st, [k]
        elif mode == 7:
            kind, factors = "sr", [int(o.downsample_factor)]
        elif mode == 8:
            kind, param = "inpaint", f32(o.mask_ratio)
        elif mode == 9:
            kind, param = "haze", f32(o.haze_omega)
            low = d.rand(B, 1, max(H // 16, 2), max(W // 16, 2))
            tabs["cirrus"] = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)[:, 0].contiguous()
            top_k = max(int(H * W * 0.01 / 100), 1)
            flat = clean.reshape(B, C, -1)
            tabs["atm"] = flat.amax(dim=-1) if top_k == 1 else flat.topk(top_k, dim=-1).values.mean(-1)
            if C not in self._haze_ratio:
                lam = torch.linspace(400, 1000, 100, device=dev, dtype=torch.float64)[:C]
                self._haze_ratio[C] = (lam[0] / lam).to(torch.float32)
            tabs["haze_ratio"] = self._haze_ratio[C]
        else:
            kind = "bandmiss"
            n = int(o.bandmis_ratio * C)
            tabs["band_flag"] = (d.rand(B, C).argsort(dim=1).argsort(dim=1) < n).to(torch.uint8)
        param = param if torch.is_tensor(param) else f32(param)
        return ops.DegradePlan([ops.DEG_KINDS[kind]], ksize, factors, task=task, aug=None, param=param.to(torch.float32).contiguous(),
                               sub=self._const((B,), torch.int32, sub, dev), **tabs)

    def __call__(self, clean, mode, opts):
        """clean (1,C,H,W) fp32 on the device -> (degraded, prompt id): the plan, then one launch; no copy of the clean cube is written"""
        from . import ops
        clean = clean.contiguous()
        if mode == 13:
            B, _, H, W = clean.shape
            mask = scene_cassi_mask(opts, clean.device, H, W)
            return ops.cassi(clean, mask.mask, mask.origins(self.d, B, H, W), opts.cassi_step)[0], 0
        plan = self.plan(clean, mode, opts)
        self.ordinal += 1
        return ops.degrade_planes(clean, plan, seed=self.seed, ordinal=self.ordinal, want_clean=False)[0], self.prompt_id(mode)
