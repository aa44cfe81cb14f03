"""Fused training-batch degradation (mp-hsir_amd/degrade.py DegradationSynthesizer(fused=True), csrc/degrade.hip): what one synthesiser
call costs by the tensor programs and by plan + one launch, and what that does to a train.py-shaped loop.  Timing as bench_scene.py (the
median of REGIONS regions of device events, with min .. max); both paths run in the same process, alternating.

    python tools/bench/bench_degrade.py [call] [loop]          (no argument: both legs)

call   one DegradationSynthesizer call at the natural-scene (32 x 31 x 64 x 64) and the remote-sensing (32 x 100 x 64 x 64) training shape:
       the default menu of the shape and every kind of it alone, tensor path (fused=False: the parent commit's code, untouched) against
       fused=True (plan + launch), then the launch alone on a prepared plan beside a copy_ of three cubes' bytes (one read, two writes:
       the launch's traffic floor).  Wall time per call is taken too (host clock around a synchronised call): the tensor path's blocking
       nonzero() calls cost host time that device events between two records do not show when the queue runs empty.
loop   src.next() + eng.train_step(), natural-scene model, bf16, captured step, batch 32: the pooled source (bench.py's situation), the
       tensor source and the fused source, in steps per second (host clock over synchronised regions of STEPS steps).
"""
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from bench_scene import REGIONS, dev, fmt, timed  # noqa: E402
from mp_hsir_amd import degrade as D  # noqa: E402
from mp_hsir_amd import ops  # noqa: E402

MENUS = {"natural_scene": (31, ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"]),
         "remote_sensing": (100, ["gaussianN", "complexN", "blur", "sr", "inpaint", "haze", "bandmiss"])}
STEPS = 20


def wall(fn, n=10):
    """-> (median, min, max) milliseconds of host time per synchronised call"""
    ts = []
    for _ in range(REGIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def leg_call():
    for data_type, (C, menu) in MENUS.items():
        clean = torch.rand((32, C, 64, 64), device=dev)
        nb = 12.0 * clean.numel()
        src3, dst3 = torch.rand(clean.numel() * 3 // 2, device=dev), torch.empty(clean.numel() * 3 // 2, device=dev)
        cp = timed(lambda: dst3.copy_(src3), 20)
        print("%s 32 x %d x 64 x 64 (%.0f MB per cube): copy_ of three cubes' bytes %s" % (data_type, C, clean.numel() * 4e-6, fmt(cp, nb)), flush=True)
        extra = ["motion_blur"] if data_type == "natural_scene" else ["circle_blur"]
        for types in [menu] + [[t] for t in menu + extra]:
            tens = D.DegradationSynthesizer(data_type, types, dev, seed=1)
            fus = D.DegradationSynthesizer(data_type, types, dev, seed=1, fused=True)
            a, b = timed(lambda: tens(clean), 5), timed(lambda: fus(clean), 5)
            wa, wb = wall(lambda: tens(clean)), wall(lambda: fus(clean))
            plan, _ = fus.fused_plan(clean)
            out = (torch.empty_like(clean), torch.empty_like(clean))
            k = timed(lambda: ops.degrade_batch(clean, plan, seed=1, ordinal=0, out=out), 10)
            print("  %-22s tensor %s (wall %.3f) | fused %s (wall %.3f) = %.2f x (wall %.2f x) | launch alone %s, copy / launch %.2f"
                  % ("menu" if types is menu else types[0], fmt(a), wa[0], fmt(b), wb[0], a[0] / b[0], wa[0] / wb[0], fmt(k, nb), cp[0] / k[0]), flush=True)
        # the all-blur batch at k = 21: 441 LDS reads per element
        fus = D.DegradationSynthesizer("natural_scene", ["blur"], dev, seed=1, fused=True)
        plan, _ = fus.fused_plan(clean)
        plan.sub.fill_(2)
        out = (torch.empty_like(clean), torch.empty_like(clean))
        k = timed(lambda: ops.degrade_batch(clean, plan, seed=1, ordinal=0, out=out), 10)
        ker = D.gaussian_kernel2d(21)
        t = timed(lambda: D.blur(clean, ker), 5)
        print("  all samples blur k = 21: launch alone %s | F.conv2d of the tensor path %s = %.2f x" % (fmt(k, nb), fmt(t), t[0] / k[0]), flush=True)


def leg_loop():
    from bench import MODELS
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    cfg = MODELS["natural_scene"]
    torch.manual_seed(2024)
    net = MP_HSIR_Net(**cfg, compute_dtype=torch.bfloat16, clip_prompt="surrogate").to(dev).train()
    eng = DataParallelEngine(net, lr=2e-4, use_graph=True)
    types = MENUS["natural_scene"][1]
    mk = lambda **kw: SyntheticPatchSource(31, 64, 32, cfg["task_classes"], dev, 2024, 0, de_types=types, **kw)      # noqa: E731
    srcs = {"pooled": mk(pool=8).prefill(), "tensor": mk(), "fused": mk(fused_degrade=True)}

    def step(src):
        _, x, c, p = src.next()
        return eng.train_step(x, c, p)
    for _ in range(4):
        for s in srcs.values():
            step(s)
    rates = {k: [] for k in srcs}
    for _ in range(REGIONS):
        for name, s in srcs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                step(s)
            torch.cuda.synchronize()
            rates[name].append(STEPS / (time.perf_counter() - t0))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    for k, v in rates.items():
        print("loop %-7s %.2f steps/s [%.2f .. %.2f] = %.0f patches/s, %.3f ms per step" % (k, med[k], min(v), max(v), 32 * med[k], 1e3 / med[k]), flush=True)
    gap = 1e3 / med["tensor"] - 1e3 / med["pooled"]
    print("gap tensor - pooled %.3f ms per step; fused closes %.3f ms of it = %.0f%%" % (gap, 1e3 / med["tensor"] - 1e3 / med["fused"],
          100.0 * (1e3 / med["tensor"] - 1e3 / med["fused"]) / gap if gap > 0 else float("nan")), flush=True)
    eng.finish()


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["call", "loop"]:
        {"call": leg_call, "loop": leg_loop}[leg]()
