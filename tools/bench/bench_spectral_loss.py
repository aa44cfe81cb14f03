"""The training loss with spectral terms (mp-hsir_amd/csrc/spectral_loss.hip, ops.spectral_loss_grad, engine.SpectralLoss): what the launch
pair costs alone and what it does to the training step.

    python tools/bench/bench_spectral_loss.py [pair] [step] [default]          (no argument: pair and step)

pair     ops.spectral_loss_grad(y, c, 0.1, 0.3) at 32 x 31 x 64 x 64, 32 x 100 x 64 x 64 and 4 x 31 x 256 x 256, inputs COLD by rotation (a ring
         of input / gradient sets several times the 256 MB of last-level cache), beside ops.l1_clamp_loss_grad on the same ring, beside a
         copy_ of the launches' algorithmic traffic (read y and c, write grad: 12 B per element; the gradient walk re-reads y and c, 8 B per
         element more, from cache) and what each of the two launches takes by the library's launch timer.
step     bench.py's workload through the engine directly (natural-scene model, bf16, batch 32, 64 x 64 patches, graph mode): the default loss
         against SpectralLoss(0.1, 0.1), three alternating pairs in the same process.
default  the default step alone (three timings) and its launch list from ops.ACCOUNT, printed sorted: to be run from two commits in
         alternating processes.
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
from mp_hsir_amd import _lib, ops  # noqa: E402

SHAPES = [((32, 31, 64, 64), 24), ((32, 100, 64, 64), 8), ((4, 31, 256, 256), 12)]     # shape, ring length


class Ring:
    def __init__(self, n, make):
        self.items, self.i = [make(k) for k in range(n)], -1

    def next(self):
        self.i = (self.i + 1) % len(self.items)
        return self.items[self.i]


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
            return ops.spectral_loss_grad(y, c, 0.1, 0.3)

        def l1():
            y, c = ring.next()
            return ops.l1_clamp_loss_grad(y, c)

        rows = {}
        for rnd in range(2):                                # alternate: two rounds of each, the second is reported
            rows = {"copy": timed(copy, 20), "pair": timed(pair, 20), "l1": timed(l1, 20)}
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
        print("  spectral_loss launch pair   %s, pair / copy %.2f (launch timer: %s)" % (fmt(rows["pair"], nb), rows["pair"][0] / rows["copy"][0], ", ".join(share)), flush=True)
        print("  l1_clamp_loss + reduce      %s, pair / l1 %.2f" % (fmt(rows["l1"], nb), rows["pair"][0] / rows["l1"][0]), flush=True)
        del ring, copies
        torch.cuda.empty_cache()


def leg_step():
    from mp_hsir_amd.engine import SpectralLoss
    off, step_off = engine()
    on, step_on = engine(loss_fn=SpectralLoss(0.1, 0.1))
    for _ in range(6):                                      # eager steps, the capture, a few replays
        step_off()
        step_on()
    torch.cuda.synchronize()
    for pair in range(3):
        a = timed(step_off, 10)
        b = timed(step_on, 10)
        print("pair %d: default loss %s = %.1f patches/s | SpectralLoss(0.1, 0.1) %s = %.1f patches/s | on - off %.4f ms, on / off %.4f"
              % (pair + 1, fmt(a), 32e3 / a[0], fmt(b), 32e3 / b[0], b[0] - a[0], b[0] / a[0]), flush=True)
    print("the terms after the run: %s" % on.loss_components())


def leg_default():
    eng, step = engine()
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    for k in range(3):
        t = timed(step, 10)
        print("default step %d: %s = %.1f patches/s" % (k + 1, fmt(t), 32e3 / t[0]), flush=True)
    del eng, step
    torch.cuda.empty_cache()
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    from bench_optim import CFG
    torch.manual_seed(2024)
    net = MP_HSIR_Net(**CFG, compute_dtype=torch.bfloat16, clip_prompt="surrogate").to(dev).train()
    src = SyntheticPatchSource(CFG["in_channel"], 64, 32, CFG["task_classes"], dev, 2024, 0, pool=8).prefill()
    fresh = DataParallelEngine(net, lr=2e-4, use_graph=False)
    for k in range(2):
        if k == 1:
            ops.ACCOUNT = {}
        _, x, c, p = src.next()
        fresh.train_step(x, c, p)                           # the second: an eager step with the arenas in place, its launches by name
    acct, ops.ACCOUNT = ops.ACCOUNT, None
    print("launches of a default step (ops.ACCOUNT): %s" % sorted((k, v[0]) for k, v in acct.items()))


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["pair", "step"]:
        {"pair": leg_pair, "step": leg_step, "default": leg_default}[leg]()
