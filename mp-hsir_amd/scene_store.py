"""The training set as a scene pyramid resident in HBM, and the patch records cut out of it on the device.

The reference prepares its training patches offline (utils/lmdb_patch.py:39-71, 120-224, utils/image_utils.py:416-448): every cube is
band-adapted, cropped to a multiple of 256 (128 for remote sensing), resampled with scipy.ndimage.zoom at 1 / 0.5 / 0.25, cut into grid
patches whose window touches no mask pixel, and every patch is min-max normalised and stored.  Here the three LEVELS of every scene are
kept instead (1.31 x the scene bytes against 2.25 x for the patches: stride 32 at the lower scales stores every pixel four times) in one
fp32 arena on the device, next to a table of the grid records (level, y, x) in the reference's order, and a batch is cut out and normalised
by one launch pair (ops.patch_sample, csrc/patch_sample.hip).  Building the store is tensor programs in float64, run once.

The zoom levels are exact matrices: scipy.ndimage.zoom(order=3, mode='constant', prefilter=True) is, per axis of length n -> m = round(n s),
R = W A^-1 with A the cubic B-spline collocation matrix (1/6, 4/6, 1/6) under whole-sample mirror at both ends and W the four B-spline
weights of coordinate o (n - 1) / (m - 1), indices outside [0, n) mirrored the same way; level = R_y x R_x^T.  The mask level is the mask
at rows / columns floor(o (n - 1) / (m - 1) + 0.5) (zoom order 0).
"""
import os

import numpy as np
import torch

from . import degrade, ops

# lmdb_patch.py:159-168: source name (the file name up to the first '_') -> (first wavelength, last wavelength, bands)
REMOTE_SENSING_BANDS = {"Xiongan": (400, 1000, 256), "WDC": (400, 2400, 191), "PaviaC": (430, 860, 102), "PaviaU": (430, 860, 103),
                        "Houston": (364, 1046, 144), "Chikusei": (343, 1018, 128), "Eagle": (401, 999, 248), "BerlinUrGrad": (455, 2447, 111)}
REMOTE_SENSING_TARGET = (400, 1000, 100)                 # lmdb_patch.py:170
CROP_MULTIPLE = {"natural_scene": 256, "remote_sensing": 128}      # lmdb_patch.py:47-48, 128-129


def band_matrix(lo, hi, n, target=REMOTE_SENSING_TARGET):
    """(T, n) float64 with two entries per row: scipy.interpolate.interp1d(linspace(lo, hi, n), ., kind='linear',
    fill_value='extrapolate') evaluated at linspace(*target) -- the end segments extend outside [lo, hi]."""
    src = np.linspace(lo, hi, n)
    dst = np.linspace(*target)
    k = np.clip(np.searchsorted(src, dst, side="left") - 1, 0, n - 2)       # interp1d: x_new between src[k] and src[k + 1], clipped to the end segments
    w = (dst - src[k]) / (src[k + 1] - src[k])
    M = np.zeros((dst.shape[0], n), dtype=np.float64)
    rows = np.arange(dst.shape[0])
    M[rows, k] = 1.0 - w
    M[rows, k + 1] += w
    return M


def _mirror(i, n):
    """whole-sample mirror of any integer index into [0, n): -1 -> 1, n -> n - 2"""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def zoom_out_len(n, s):
    return int(round(n * s))


def zoom_coords(n, m):
    """the input coordinate of every output sample of scipy.ndimage.zoom (grid_mode=False): o * ((n - 1) / (m - 1))"""
    step = (n - 1) / (m - 1) if m > 1 else 1.0
    return np.arange(m, dtype=np.float64) * step


def spline_zoom_matrix(n, s):
    """(m, n) float64 R with zoom(x, s, order=3, mode='constant')[o] = sum_i R[o, i] x[i] along an axis of length n (needs n >= 2)"""
    m = zoom_out_len(n, s)
    A = np.zeros((n, n), dtype=np.float64)
    i = np.arange(n)
    A[i, i] = 4.0 / 6.0
    for d in (-1, 1):
        np.add.at(A, (i, _mirror(i + d, n)), 1.0 / 6.0)
    t = zoom_coords(n, m)
    outside = t > n - 1          # scipy's mode 'constant': a coordinate past the last sample gives cval = 0, and (m - 1) * ((n - 1) / (m - 1))
    t = np.minimum(t, float(n - 1))      # can round to just above n - 1 (n = 384, s = 0.5): the reference's level then ends in a zero row
    f = np.floor(t)
    x = t - f
    w = np.stack([(1 - x) ** 3 / 6.0, (3 * x ** 3 - 6 * x ** 2 + 4) / 6.0, (-3 * x ** 3 + 3 * x ** 2 + 3 * x + 1) / 6.0, x ** 3 / 6.0], axis=1)
    W = np.zeros((m, n), dtype=np.float64)
    rows = np.arange(m)
    for k in range(4):
        np.add.at(W, (rows, _mirror(f.astype(np.int64) - 1 + k, n)), w[:, k])       # a tap outside [0, n) is folded back, never dropped
    W[outside] = 0.0
    return np.linalg.solve(A.T, W.T).T


def nearest_zoom_index(n, s):
    """(m,) int64: zoom(mask, s, order=0) along an axis of length n is mask[index]; -1: a coordinate that rounded to above n - 1, where
    scipy gives cval = 0 (see spline_zoom_matrix)"""
    m = zoom_out_len(n, s)
    t = zoom_coords(n, m)
    return np.where(t > n - 1, -1, np.minimum(np.floor(t + 0.5).astype(np.int64), n - 1))


def zoom_level(x, s):
    """x (C,H,W) float64 tensor -> the level scipy.ndimage.zoom(x, (1, s, s)) gives, float64, on x's device"""
    Ry = torch.from_numpy(spline_zoom_matrix(x.shape[1], s)).to(x.device)
    Rx = torch.from_numpy(spline_zoom_matrix(x.shape[2], s)).to(x.device)
    return torch.matmul(torch.matmul(Ry, x), Rx.t())


def zoom_mask(mask, s):
    """mask (H,W) numpy -> scipy.ndimage.zoom(mask, (s, s), order=0)"""
    iy, ix = nearest_zoom_index(mask.shape[0], s), nearest_zoom_index(mask.shape[1], s)
    out = mask[np.maximum(iy, 0)][:, np.maximum(ix, 0)].copy()
    out[iy < 0, :] = 0
    out[:, ix < 0] = 0
    return out


def load_scene(path):
    """-> (cube (C,H,W) numpy, mask (H,W) or None).  .mat as test.py reads them (key `data`, stored H x W x C, optional `mask`); .npy (C,H,W)"""
    if path.endswith(".npy"):
        return np.load(path), None
    with open(path, "rb") as f:
        head = f.read(128)
    if head.startswith(b"MATLAB 7.3"):
        raise RuntimeError("%s is a MATLAB v7.3 (HDF5) file: reading it needs h5py, which this project does not use -- save the cube with "
                           "scipy.io.savemat (v5) or as a (C,H,W) .npy" % path)
    import scipy.io
    m = scipy.io.loadmat(path)
    return m["data"].transpose(2, 0, 1), m.get("mask", None)


def grid_origins(mask, patch, stride):
    """(n, 2) int32 (y, x): the origins range(0, n - patch + 1, stride) per axis, y-major, whose window touches no mask pixel"""
    H, W = mask.shape
    sat = np.zeros((H + 1, W + 1), dtype=np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(mask != 0, axis=0, dtype=np.int64), axis=1)
    ys, xs = np.arange(0, H - patch + 1, stride), np.arange(0, W - patch + 1, stride)
    if ys.size == 0 or xs.size == 0:
        return np.zeros((0, 2), dtype=np.int32)
    Y, X = np.meshgrid(ys, xs, indexing="ij")
    hit = sat[Y + patch, X + patch] - sat[Y, X + patch] - sat[Y + patch, X] + sat[Y, X]
    keep = hit == 0
    return np.stack([Y[keep], X[keep]], axis=1).astype(np.int32)


class SceneStore:
    """paths_or_arrays: .mat / .npy paths, (C,H,W) arrays, or (array, mask) pairs.  sources: the source-file name of every scene (default:
    the file's base name, `scene_%04d` for arrays); for remote_sensing the name up to the first '_' selects the band adaptation
    (REMOTE_SENSING_BANDS; an unknown name is accepted only when the cube already has 100 bands).  len(store) records in the reference's order
    (scene, scale, y, x); store.names[i] is record i's source name.  store.degenerate counts the records whose window is constant or
    holds a NaN -- the reference turns them into NaN patches; they are kept unless drop_degenerate.  adapt_bands=False keeps every cube's
    own bands (the reference's natural-scene script stores them as they are and its loader adapts them per sample).  While it is built, the
    fp32 levels stay on the device until the arena has been allocated and filled: the peak is about 2 x nbytes plus one float64 scene."""

    def __init__(self, paths_or_arrays, data_type, device, patch=64, scales=(1, .5, .25), strides=(64, 32, 32), crop_multiple=None,
                 sources=None, drop_degenerate=False, adapt_bands=True):
        assert len(scales) == len(strides) and patch % 4 == 0, "one stride per scale; the patch side is a multiple of 4"
        self.data_type, self.device, self.patch = data_type, torch.device(device), patch
        self.scales, self.strides = tuple(scales), tuple(int(s) for s in strides)
        cm = CROP_MULTIPLE[data_type] if crop_multiple is None else int(crop_multiple)
        levels, masks, records, names, level_stride = [], [], [], [], []
        cubes = []
        total = 0
        for si, item in enumerate(paths_or_arrays):
            mask = None
            if isinstance(item, str):
                cube, mask = load_scene(item)
                name = os.path.basename(item)
            else:
                if isinstance(item, (tuple, list)):
                    item, mask = item
                cube = item.detach().cpu().numpy() if torch.is_tensor(item) else np.asarray(item)
                name = "scene_%04d" % si
            if sources is not None:
                name = sources[si]
            x = torch.from_numpy(np.ascontiguousarray(cube, dtype=np.float64)).to(self.device)
            if adapt_bands:
                x = self._adapt_bands(x, name)
            H, W = (x.shape[1] // cm) * cm, (x.shape[2] // cm) * cm
            if H < patch or W < patch:
                raise ValueError("scene %s: %d x %d after the crop to multiples of %d holds no %d x %d patch" % (name, H, W, cm, patch, patch))
            x = x[:, :H, :W]
            mask = np.zeros((H, W), dtype=bool) if mask is None else np.asarray(mask)[:H, :W]
            if cubes and x.shape[0] != cubes[0].shape[0]:
                raise ValueError("scene %s has %d bands after adaptation, the store holds %d" % (name, x.shape[0], cubes[0].shape[0]))
            for s, stride in zip(self.scales, self.strides):
                lv, mk = (x, mask) if s == 1 else (zoom_level(x, s), zoom_mask(mask, s))
                if lv.shape[1] < patch or lv.shape[2] < patch:
                    continue                                     # a level no window fits into holds no record (and the kernel refuses it)
                lv = lv.to(torch.float32).contiguous()
                org = grid_origins(mk, patch, stride)
                l = len(levels)
                levels.append((total, lv.shape[1], lv.shape[2]))
                total += (lv.numel() + 3) // 4 * 4                   # every level starts 16-byte aligned
                cubes.append(lv)
                masks.append(mk != 0)
                level_stride.append(stride)
                records.append(np.concatenate([np.full((org.shape[0], 1), l, dtype=np.int32), org], axis=1))
                names += [name] * org.shape[0]
        if not cubes:
            raise ValueError("SceneStore: no scenes")
        self.C = cubes[0].shape[0]
        self.arena = torch.empty((total,), dtype=torch.float32, device=self.device)
        for (off, H, W), lv in zip(levels, cubes):
            self.arena[off:off + lv.numel()].copy_(lv.reshape(-1))
        del cubes
        self.levels_host = torch.tensor(levels, dtype=torch.int64).reshape(-1, 3)
        self.levels = self.levels_host.to(self.device)
        self.level_stride = torch.tensor(level_stride, dtype=torch.int32, device=self.device)
        self.masks = masks
        self._sat = None
        self._set_records(np.concatenate(records, axis=0), names)
        if len(self) == 0:
            raise ValueError("SceneStore: every grid window touches the mask: no records")
        bad = self._degenerate_records()
        self.degenerate = int(bad.sum())
        if drop_degenerate and self.degenerate:
            keep = ~bad
            self._set_records(self.records_host[keep], [n for n, k in zip(self.names, keep) if k])

    def _adapt_bands(self, x, name):
        if self.data_type == "remote_sensing":
            src = REMOTE_SENSING_BANDS.get(name.split("_")[0])
            if src is None:
                if x.shape[0] != REMOTE_SENSING_TARGET[2]:
                    raise ValueError("scene %s: source %r is none of %s and the cube has %d bands, not %d" %
                                     (name, name.split("_")[0], sorted(REMOTE_SENSING_BANDS), x.shape[0], REMOTE_SENSING_TARGET[2]))
                return x
            if x.shape[0] != src[2]:
                raise ValueError("scene %s: %d bands, source %s has %d" % (name, x.shape[0], name.split("_")[0], src[2]))
            M = torch.from_numpy(band_matrix(*src)).to(x.device)
            return torch.matmul(M, x.reshape(x.shape[0], -1)).reshape(M.shape[0], x.shape[1], x.shape[2])
        if x.shape[0] != 31:
            return degrade.interpolate_bands(x[None], 31)[0]
        return x

    def _set_records(self, rec, names):
        self.records_host = np.ascontiguousarray(rec, dtype=np.int32)
        self.records = torch.from_numpy(self.records_host).to(self.device)
        self.names = list(names)

    def __len__(self):
        return self.records_host.shape[0]

    @property
    def nbytes(self):
        return self.arena.numel() * 4

    def sample(self, index, out=None, workspace=None):
        """index (B,) int64 on the device -> (B,C,P,P) normalised patches of those records: one launch pair, no synchronisation"""
        return ops.patch_sample(self.arena, self.levels, self.levels_host, self.records, index, self.C, self.patch, out=out, workspace=workspace)

    def sample_at(self, triples, out=None, workspace=None):
        """triples (B,3) int32 on the device {level, y, x}: the windows at those origins (clamped into their level by the kernel)"""
        return ops.patch_sample(self.arena, self.levels, self.levels_host, triples, None, self.C, self.patch, out=out, workspace=workspace)

    def patches(self, batch=256):
        """every record's patch in order, in batches of (<= batch, C, P, P) on the device"""
        idx = torch.arange(len(self), dtype=torch.int64, device=self.device)
        for i in range(0, len(self), batch):
            yield self.sample(idx[i:i + batch].contiguous())

    def _degenerate_records(self):
        bad = [torch.isnan(p[:, 0, 0, 0]) for p in self.patches()]
        return torch.cat(bad).cpu().numpy()

    def mask_sat(self):
        """(sat, offsets): the integral images of the mask levels, each (H + 1) x (W + 1) int32, in one flat device tensor, and the (n_levels,)
        int64 offset of each; built on first use (the jitter of data.SceneStoreSource)"""
        if self._sat is None:
            parts, offs, total = [], [], 0
            for mk in self.masks:
                s = np.zeros((mk.shape[0] + 1, mk.shape[1] + 1), dtype=np.int32)
                s[1:, 1:] = np.cumsum(np.cumsum(mk, axis=0, dtype=np.int64), axis=1).astype(np.int32)
                parts.append(s.reshape(-1))
                offs.append(total)
                total += s.size
            self._sat = (torch.from_numpy(np.concatenate(parts)).to(self.device), torch.tensor(offs, dtype=torch.int64, device=self.device))
        return self._sat


def scene_files(scene_dir):
    """the .mat / .npy files of a directory, sorted by name"""
    fs = sorted(f for f in os.listdir(scene_dir) if f.endswith(".mat") or f.endswith(".npy"))
    if not fs:
        raise ValueError("%s holds no .mat / .npy scene" % scene_dir)
    return [os.path.join(scene_dir, f) for f in fs]
