"""The CASSI launch pair (mp-hsir_amd/csrc/cassi.hip, ops.cassi) beside its traffic floor and beside the tensor form, and what a whole
SyntheticPatchSource.next() of the fine-tune menu costs either way.  Timing as bench_scene.py (device events, the median of REGIONS
regions, with min .. max); inputs are COLD by rotation: every call works on the next of a ring of input / output sets whose total size
exceeds the 256 MB of last-level cache several times, so no call finds its cube in cache.

    python tools/bench/bench_cassi.py [pair] [next] [account]          (no argument: all legs)

pair     ops.cassi with clean_aug at 32 x 31 x 64 x 64 (a training batch, random modes and origins) and 1 x 31 x 1024 x 1024 (a scene,
         mode 0), beside a copy_ of its algorithmic traffic (read clean, write degraded and clean_aug: 12 bytes per element) over the same
         kind of ring, beside the tensor form (degrade.cassi_measure + degrade.augment of both cubes), and what each of the two launches
         takes by the library's launch timer.
next     SyntheticPatchSource(31, 64, 32, 1, de_types=["cassi"]).next(), fused against tensor, host clock with a final synchronise.
account  the launch list (ops.ACCOUNT) of one next() for the default six-task menu, a mixed menu with cassi and the fine-tune menu.
"""
import ctypes
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from bench_degrade import wall  # noqa: E402
from bench_scene import dev, fmt, timed  # noqa: E402
from mp_hsir_amd import _lib, ops  # noqa: E402
from mp_hsir_amd import degrade as D  # noqa: E402
from mp_hsir_amd.data import SyntheticPatchSource  # noqa: E402

SHAPES = [("training batch", (32, 31, 64, 64), 24, True), ("scene", (1, 31, 1024, 1024), 4, False)]     # label, shape, ring length, modes?


class Ring:
    def __init__(self, n, make):
        self.items, self.i = [make(k) for k in range(n)], -1

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


def leg_pair():
    lib = _lib.load()
    kids = [k for k in range(64) if lib.mphsir_kernel_name(k) in (b"cassi_measure", b"cassi_emit")]
    g = torch.Generator(device=dev).manual_seed(3)
    for label, shape, n, modes in SHAPES:
        B, C, H, W = shape
        numel = B * C * H * W
        nb = 12.0 * numel
        mask = D.CassiMask(dev, seed=1, shape=(max(256, H), max(256, W)))
        origin = mask.origins(D.Draws(dev, 5), B, H, W)
        aug = torch.randint(0, 8, (B,), generator=g, device=dev).int() if modes else None
        ws = torch.empty((lib.mphsir_cassi_workspace_bytes(B, C, H, W, 2) // 4,), device=dev)
        ring = Ring(n, lambda k: (torch.rand(shape, generator=g, device=dev), torch.empty(shape, device=dev), torch.empty(shape, device=dev)))
        copies = Ring(n, lambda k: (torch.rand(numel * 3 // 2, generator=g, device=dev), torch.empty(numel * 3 // 2, device=dev)))
        print("%s %s: ring of %d sets = %.0f MB, workspace %.1f MB" % (label, " x ".join(map(str, shape)), n, n * nb / 1e6, ws.numel() * 4e-6), flush=True)

        def copy():
            a, b = copies.next()
            b.copy_(a)

        def pair():
            x, d, c = ring.next()
            ops.cassi(x, mask.mask, origin, 2, aug=aug, out=(d, c), workspace=ws)

        def tensor():
            x, _, _ = ring.next()
            y = D.cassi_measure(x, mask.mask, origin, 2)
            return (D.augment(y, aug), D.augment(x, aug)) if aug is not None else (y, x.clone())

        cp, t, tf = timed(copy, 20), timed(pair, 20), timed(tensor, 3, warm=1)
        share = []
        for kid in kids:
            lib.mphsir_prof_enable(kid)
            for _ in range(20):
                pair()
            cnt, ms = ctypes.c_int(0), ctypes.c_float(0)
            lib.mphsir_prof_read(ctypes.byref(cnt), ctypes.byref(ms))
            lib.mphsir_prof_enable(-1)
            share.append("%s %.4f ms over %d launches" % (lib.mphsir_kernel_name(kid).decode(), ms.value / max(cnt.value, 1), cnt.value))
        print("  copy_ of 12 B / element %s" % fmt(cp, nb), flush=True)
        print("  launch pair            %s, copy / pair %.2f (launch timer: %s)" % (fmt(t, nb), cp[0] / t[0], ", ".join(share)), flush=True)
        print("  tensor form            %s, tensor / pair %.1f" % (fmt(tf), tf[0] / t[0]), flush=True)
        x, d, c = ring.next()
        ops.cassi(x, mask.mask, origin, 2, aug=aug, out=(d, c), workspace=ws)
        want = D.cassi_measure(x, mask.mask, origin, 2)
        assert torch.equal(d, D.augment(want, aug) if aug is not None else want), "the timed launch pair differs from the tensor form"
        del ring, copies


def leg_next():
    srcs = {"fused": SyntheticPatchSource(31, 64, 32, 1, dev, de_types=["cassi"], fused_degrade=True),
            "tensor": SyntheticPatchSource(31, 64, 32, 1, dev, de_types=["cassi"], fused_degrade=False)}
    for s in srcs.values():
        for _ in range(3):
            s.next()
    w = {k: wall(s.next) for k, s in srcs.items()}
    print("next() of the fine-tune menu, 32 x 31 x 64 x 64: fused %.3f ms [%.3f .. %.3f] | tensor %.3f ms [%.3f .. %.3f] = %.2f x"
          % (w["fused"] + w["tensor"] + (w["tensor"][0] / w["fused"][0],)), flush=True)


def leg_account():
    for menu in (["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"], ["gaussianN", "cassi", "blur"], ["cassi"]):
        src = SyntheticPatchSource(31, 64, 32, 6, dev, de_types=menu, fused_degrade=True)
        src.next()
        ops.ACCOUNT = {}
        src.next()
        print("launch list of next() for %s: %s" % (menu, {k: v[0] for k, v in sorted(ops.ACCOUNT.items())}), flush=True)
        ops.ACCOUNT = None


if __name__ == "__main__":
    lib = _lib.load()
    lib.mphsir_kernel_name.restype = ctypes.c_char_p
    for leg in sys.argv[1:] or ["pair", "next", "account"]:
        {"pair": leg_pair, "next": leg_next, "account": leg_account}[leg]()
