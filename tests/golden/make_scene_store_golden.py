#!/usr/bin/env python3
"""Generate tests/golden/scene_store.npz: the training patches the REFERENCE's preprocessing cuts out of one synthetic cube.

The reference's `create_lmdb` (/root/reference/utils/lmdb_patch.py:39-71) cannot run here (`lmdb` is absent), so this script does what
its `preprocess` does, with the reference's own `Data2Volume` (utils/image_utils.py:416-448) and the same scipy `zoom` calls: crop to
multiples of 256, `zoom(data, (1, s, s))` and `zoom(mask, (s, s), order=0)` per scale s != 1, grid patches whose window touches no mask
pixel, per-patch min-max, float32.  Data2Volume does not say where a patch came from, so the origin list is replayed with the same loop
and checked against its output patch by patch.  The fixture holds data only: the cube as uint8 codes (cube = codes / 255.0 in float64,
so that the file stays small), the mask, the ordered origins {scale index, y, x} and the float32 patches.  Runs only in the build
container (imports /root/reference through tests/golden/refshim, as make_degrade_golden.py does)."""
import os
import sys
from itertools import product

import numpy as np
from scipy.ndimage import zoom

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "refshim"))
sys.path.insert(1, "/root/reference")
import utils.image_utils as RI  # noqa: E402  (the reference)

SCALES, KSIZE, STRIDES = (1, 0.5, 0.25), 16, (64, 32, 16)


def make_cube():
    rs = np.random.RandomState(2024)
    C, H, W = 4, 256, 300
    y, x = np.mgrid[0:H, 0:W]
    cube = np.stack([0.5 + 0.3 * np.sin(x / (17.0 + 3 * c) + c) * np.cos(y / (23.0 - 2 * c)) for c in range(C)]) + 0.15 * rs.rand(C, H, W)
    codes = np.clip(np.round(cube * 255.0), 0, 255).astype(np.uint8)
    mask = np.zeros((H, W), dtype=bool)
    mask[(y - 100) ** 2 + (x - 110) ** 2 < 45 ** 2] = True          # a blob that kills some, not all, patches at every scale
    mask[200:204, 230:260] = True
    return codes, mask


def main():
    codes, mask = make_cube()
    data = codes.astype(np.float64) / 255.0
    C = data.shape[0]
    nh, nw = (data.shape[1] // 256) * 256, (data.shape[2] // 256) * 256
    data_c, mask_c = data[..., :nh, :nw], mask[:nh, :nw]
    patches, origins = [], []
    for i, s in enumerate(SCALES):
        if s != 1:
            td, tm = zoom(data_c, zoom=(1, s, s)), zoom(mask_c, zoom=(s, s), order=0)
        else:
            td, tm = data_c, mask_c
        V = RI.Data2Volume(td, tm, ksizes=(C, KSIZE, KSIZE), strides=[C, STRIDES[i], STRIDES[i]])
        here = [(i, y0, x0) for _, y0, x0 in product(*[range(0, td.shape[k] - (C, KSIZE, KSIZE)[k] + 1, (C, STRIDES[i], STRIDES[i])[k]) for k in range(3)])
                if not np.any(tm[y0:y0 + KSIZE, x0:x0 + KSIZE])]
        total = len(range(0, td.shape[1] - KSIZE + 1, STRIDES[i])) * len(range(0, td.shape[2] - KSIZE + 1, STRIDES[i]))
        assert len(here) == V.shape[0] and 0 < len(here) < total, (i, len(here), V.shape, total)
        for (_, y0, x0), v in zip(here, V):
            p = td[:, y0:y0 + KSIZE, x0:x0 + KSIZE]
            assert np.array_equal((p - p.min()) / (p.max() - p.min()), v)
        patches.extend(V)
        origins.extend(here)
    patches = np.stack(patches).astype(np.float32)          # preprocess: new_data.astype(np.float32)
    assert not np.isnan(patches).any()
    out = os.path.join(HERE, "scene_store.npz")
    np.savez_compressed(out, cube_u8=codes, mask=mask, origins=np.array(origins, dtype=np.int32), patches=patches,
                        scales=np.array(SCALES), strides=np.array(STRIDES), ksize=np.array(KSIZE))
    print(out, os.path.getsize(out), "bytes,", patches.shape[0], "patches", [sum(1 for o in origins if o[0] == i) for i in range(3)])


if __name__ == "__main__":
    main()
