"""Clip + EMA on the optimizer arenas (mp-hsir_amd/csrc/optim.hip, engine.DataParallelEngine(grad_clip=, ema_decay=)): what the launches cost
and what they do to the training step.

    python tools/bench/bench_optim.py [launches] [step]          (no argument: both legs)

launches  at the arena length of the natural-scene model (taken from an engine that has built its arenas, not from a constant), alternating
          in the same run: flat_adamw, flat_adamw_ex without EMA, flat_adamw_ex with EMA, grad_norm, and a device-to-device copy_ of the
          bytes each of them moves (28 / 28 / 36 / 4 B per element) -- the project's yardstick for a streaming kernel.
step      bench.py's workload through the engine directly (natural-scene model, bf16, batch 32, 64 x 64 patches, graph mode): both flags off
          against grad_clip=1.0 + ema_decay=0.999, three alternating pairs in the same process, and the launch list of a default step from
          ops.ACCOUNT (printed sorted, to be compared with another commit's).
Every time is the median of REGIONS timed regions (device events around several calls each), printed with min and max.
"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from mp_hsir_amd import ops  # noqa: E402
from mp_hsir_amd.data import SyntheticPatchSource  # noqa: E402
from mp_hsir_amd.engine import DataParallelEngine  # noqa: E402
from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net  # noqa: E402

dev = torch.device("cuda")
REGIONS = 7
CFG = dict(in_channel=31, out_channel=31, dim=64, task_classes=6)


def timed(fn, per_region, warm=2):
    """-> (median, min, max) milliseconds per call over REGIONS regions of per_region calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REGIONS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(per_region):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / per_region)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(t, nbytes=None):
    s = "%.4f ms [%.4f .. %.4f]" % t
    return s + (" = %.2f TB/s" % (nbytes / t[0] / 1e9) if nbytes else "")


def engine(batch=32, **kw):
    torch.manual_seed(2024)
    net = MP_HSIR_Net(**CFG, compute_dtype=torch.bfloat16, clip_prompt="surrogate").to(dev).train()
    src = SyntheticPatchSource(CFG["in_channel"], 64, batch, CFG["task_classes"], dev, 2024, 0, pool=8).prefill()
    eng = DataParallelEngine(net, lr=2e-4, use_graph=True, **kw)

    def step():
        _, x, c, p = src.next()
        return eng.train_step(x, c, p)
    return eng, step


def leg_launches():
    eng, step = engine(batch=4)
    step()                                                  # the first step builds the arenas
    n = eng.flat_p.numel()
    del eng, step
    torch.cuda.empty_cache()
    print("arena: %d fp32 elements = %.1f MB" % (n, 4e-6 * n))
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    g, ema = torch.randn(n, device=dev) * 1e-3, p.clone()
    stats, ws = ops.new_optim_stats(dev), ops.grad_norm_workspace(g)
    ops.grad_norm(g, stats, 1.0, workspace=ws)
    src, dst = torch.empty(9 * n, device=dev), torch.empty(9 * n, device=dev)     # a copy_ of k n floats moves 8 k n bytes
    calls = {
        "flat_adamw": (lambda: ops.flat_adamw(p, g, m, v, 2e-4, 10), 28),
        "flat_adamw_ex": (lambda: ops.flat_adamw_ex(p, g, m, v, 2e-4, 10, stats=stats), 28),
        "flat_adamw_ex + ema": (lambda: ops.flat_adamw_ex(p, g, m, v, 2e-4, 10, stats=stats, ema=ema, ema_decay=0.999), 36),
        "grad_norm": (lambda: ops.grad_norm(g, stats, 1.0, workspace=ws), 4),
    }
    rows = {}
    for rnd in range(2):                                    # alternate: two rounds of each, the second is reported
        for name, (fn, bpe) in calls.items():
            k = bpe * n // 8
            rows[name] = (timed(fn, 20), timed(lambda: dst[:k].copy_(src[:k]), 20))
    for name, (fn, bpe) in calls.items():
        t, c = rows[name]
        print("  %-20s %s | copy_ of the same %2d B per element %s | kernel / copy time %.2f"
              % (name, fmt(t, bpe * n), bpe, fmt(c, bpe * n), t[0] / c[0]), flush=True)


def leg_step():
    off, step_off = engine()
    on, step_on = engine(grad_clip=1.0, ema_decay=0.999)
    for _ in range(6):                                      # eager steps, the capture, a few replays
        step_off()
        step_on()
    torch.cuda.synchronize()
    for pair in range(3):
        a = timed(step_off, 10)
        b = timed(step_on, 10)
        print("pair %d: flags off %s = %.1f patches/s | clip + ema %s = %.1f patches/s | on / off %.4f"
              % (pair + 1, fmt(a), 32e3 / a[0], fmt(b), 32e3 / b[0], b[0] / a[0]), flush=True)
    print("clip + ema after the run: %s" % on.grad_stats())
    del on, step_on
    torch.cuda.empty_cache()
    fresh, step = engine()
    step()
    ops.ACCOUNT = {}
    step()                                                  # an eager step with the arenas in place: its launches, by name
    acct, ops.ACCOUNT = ops.ACCOUNT, None
    print("launches of a default step (ops.ACCOUNT): %s" % sorted((k, v[0]) for k, v in acct.items()))


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["launches", "step"]:
        {"launches": leg_launches, "step": leg_step}[leg]()
