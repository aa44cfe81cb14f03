#!/usr/bin/env python3
"""Generate tests/golden/cassi.npz by running the REFERENCE's Degradation._sd_cassi (utils/degradation_utils.py:202-225) itself.

    python tests/golden/make_cassi_golden.py <root of the reference repository>

The function lists a folder of .mat DATA files, picks one with random.choice, reads its 'mask' entry and crops it at an origin from
random.randint.  The files are not part of the reference, so -- as make_degrade_golden.py::haze_entries does for the cirrus maps -- the
folder listing and sio.loadmat are answered with a seeded synthetic mask; `random` is seeded before the call and the same calls are
replayed afterwards to recover the origin the function drew.  The fixture holds data only: per case the mask, the origin and the
function's output; the clean cubes are re-creatable from their seeds (tests/cassi_ref.py::golden_clean)."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (seed, (C, H, W), (MH, MW), binary mask?, dtype sio.loadmat hands the mask back in)
CASES = {"c9": (1, (9, 32, 32), (48, 40), True, np.float32),
         "c5": (2, (5, 16, 24), (16, 24), False, np.float64),
         "c31": (3, (31, 20, 12), (64, 64), False, np.float32)}


def golden_clean(seed, shape):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


def golden_mask(seed, shape, binary):
    m = np.random.RandomState(1000 + seed).rand(*shape)
    return (m < 0.5).astype(np.float32) if binary else m.astype(np.float32)


def main(reference_root):
    sys.path.insert(0, os.path.join(HERE, "refshim"))
    sys.path.insert(1, reference_root)
    import utils.degradation_utils as RD          # the reference
    D = RD.Degradation(None)
    out = {}
    real_listdir, real_loadmat = RD.os.listdir, RD.sio.loadmat
    try:
        for name, (seed, shape, mshape, binary, dtype) in CASES.items():
            x, mask = golden_clean(seed, shape), golden_mask(seed, mshape, binary)
            RD.os.listdir = lambda folder: ["synthetic.mat"]
            RD.sio.loadmat = lambda path, m=mask.astype(dtype): {"mask": m}
            random.seed(seed)
            y = D._sd_cassi(x.copy())
            random.seed(seed)
            random.choice(["synthetic.mat"])
            origin = (random.randint(0, mshape[0] - shape[1]), random.randint(0, mshape[1] - shape[2]))
            assert y.dtype == np.float32 and y.shape == shape
            out.update({name + "/mask": mask, name + "/origin": np.array(origin, dtype=np.int32), name + "/out": y,
                        name + "/seed_shape": np.array((seed,) + shape, dtype=np.int32)})
    finally:
        RD.os.listdir, RD.sio.loadmat = real_listdir, real_loadmat
    np.savez_compressed(os.path.join(HERE, "cassi.npz"), **out)
    print("wrote cassi.npz with", len(out), "entries")


if __name__ == "__main__":
    main(sys.argv[1])
