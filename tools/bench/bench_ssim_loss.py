"""The SSIM term of the training loss (the ssim_loss kernels of mp-hsir_amd/csrc/arena.hip, ops.ssim_loss_grad, engine.SpectralLoss(ssim=)):
what the launch pair costs alone and what it does to the training step.

    python tools/bench/bench_ssim_loss.py [pair] [step]          (no argument: both)

pair     ops.ssim_loss_grad(y, c, 0.2) at 32 x 31 x 64 x 64, 32 x 100 x 64 x 64 and 4 x 31 x 256 x 256, inputs COLD by rotation (a ring of
         input sets several times the 256 MB of last-level cache), beside ops.quality_bands on the same ring (the existing kernel that
         forms the same five float64 window sums, without a gradient), beside ops.spectral_loss_grad, beside a copy_ of the pair's
         algorithmic traffic (read y and c, write grad: 12 B per element), and what each of the two launches takes by the library's launch
         timer.
step     bench.py's workload through the engine directly (natural-scene model, bf16, batch 32, 64 x 64 patches, graph mode): the default loss
         against SpectralLoss(ssim=0.2), three alternating pairs in the same process.
(The default step against another commit: tools/bench/bench_spectral_loss.py default, in alternating processes.)
Every time is the median of REGIONS timed regions (device events around several calls each), printed with min and max."""
import ctypes
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from bench_optim import dev, engine, fmt, timed  # noqa: E402
from bench_spectral_loss import SHAPES, Ring  # noqa: E402
from mp_hsir_amd import _lib, ops  # noqa: E402


def leg_pair():
    lib = _lib.load()
    lib.mphsir_kernel_name.restype = ctypes.c_char_p
    kids = [k for k in range(64) if lib.mphsir_kernel_name(k) in (b"spectral_loss", b"spectral_loss_finish")]
    g = torch.Generator(device=dev).manual_seed(3)
    for shape, n in SHAPES:
        numel = shape[0] * shape[1] * shape[2] * shape[3]
        nb = 12.0 * numel

        def make(k):
            c = torch.rand(shape, generator=g, device=dev)
            return c + 0.1 * torch.randn(shape, generator=g, device=dev), c
        ring = Ring(n, make)
        copies = Ring(n, lambda k: (torch.rand(numel * 3 // 2, generator=g, device=dev), torch.empty(numel * 3 // 2, device=dev)))
        print("%s: ring of %d sets = %.0f MB" % (" x ".join(map(str, shape)), n, n * nb / 1e6), flush=True)

        def copy():
            a, b = copies.next()
            b.copy_(a)

        def pair():
            y, c = ring.next()
            return ops.ssim_loss_grad(y, c, 0.2)

        def quality():
            y, c = ring.next()
            return ops.quality_bands(y, c)

        def spectral():
            y, c = ring.next()
            return ops.spectral_loss_grad(y, c, 0.1, 0.3)

        rows = {}
        for rnd in range(2):                                # alternate: two rounds of each, the second is reported
            rows = {"copy": timed(copy, 20), "pair": timed(pair, 20), "quality": timed(quality, 20), "spectral": timed(spectral, 20)}
        share = []
        for kid in kids:
            lib.mphsir_prof_enable(kid)
            for _ in range(20):
                pair()
            cnt, ms = ctypes.c_int(0), ctypes.c_float(0)
            lib.mphsir_prof_read(ctypes.byref(cnt), ctypes.byref(ms))
            lib.mphsir_prof_enable(-1)
            share.append("%s %.4f ms over %d launches" % (lib.mphsir_kernel_name(kid).decode(), ms.value / max(cnt.value, 1), cnt.value))
        print("  copy_ of 12 B / element     %s" % fmt(rows["copy"], nb), flush=True)
        print("  ssim_loss launch pair       %s, pair / copy %.2f (launch timer: %s)" % (fmt(rows["pair"], nb), rows["pair"][0] / rows["copy"][0], ", ".join(share)), flush=True)
        print("  quality_bands               %s, pair / quality %.2f" % (fmt(rows["quality"], nb), rows["pair"][0] / rows["quality"][0]), flush=True)
        print("  spectral_loss launch pair   %s, pair / spectral %.2f" % (fmt(rows["spectral"], nb), rows["pair"][0] / rows["spectral"][0]), flush=True)
        del ring, copies
        torch.cuda.empty_cache()


def leg_step():
    from mp_hsir_amd.engine import SpectralLoss
    off, step_off = engine()
    on, step_on = engine(loss_fn=SpectralLoss(ssim=0.2))
    for _ in range(6):                                      # eager steps, the capture, a few replays
        step_off()
        step_on()
    torch.cuda.synchronize()
    for pair in range(3):
        a = timed(step_off, 10)
        b = timed(step_on, 10)
        print("pair %d: default loss %s = %.1f patches/s | SpectralLoss(ssim=0.2) %s = %.1f patches/s | on - off %.4f ms, on / off %.4f"
              % (pair + 1, fmt(a), 32e3 / a[0], fmt(b), 32e3 / b[0], b[0] - a[0], b[0] / a[0]), flush=True)
    print("the terms after the run: %s" % on.loss_components())


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["pair", "step"]:
        {"pair": leg_pair, "step": leg_step}[leg]()
