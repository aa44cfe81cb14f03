"""In-training validation (mp-hsir_amd/validate.py, ops.quality_meter, mp-hsir_amd/csrc/quality_meter.hip): what the meter launch costs
beside the tail of metrics.compute_quality it replaces, and what one validation pass costs.

    python tools/bench/bench_validate.py [meter] [pass]          (no argument: both)

meter    ops.quality_meter at (B, C) = (4, 31), (16, 31), (4, 100) on the outputs of a quality_bands call, beside the tail of
         metrics.compute_quality on the same outputs: its framework launches after quality_bands plus the .tolist() (the plain form and
         the band-completion form with a `use` mask).  Two clocks: the host clock around CALLS calls that end in a synchronise (what a
         loop pays per batch: the tail's .tolist() synchronises every call, the meter never does), and device events around ONE meter
         launch whose inputs are cold (a 512 MB fill runs between the calls; the inputs are a few KB, so rotation cannot evict them).
pass     the natural-scene net, bf16, 8 crops of 31 x 256 x 256, modes 0, 1, 5, 7, 8, 10 (prompt ids 0..5), batch 4: Validator.run() with
         the eager forward, beside the same crops scored the existing way (metrics.compute_quality and its read-back per batch), beside
         Validator(forward="graphed") -- its first pass (two eager calls and a capture per input shape) and a later pass over unchanged
         weights (replays; between two passes of a training run the weights change and every pass is a first pass).  The shares of a
         pass: the forwards alone, forwards + quality_bands, forwards + quality_bands + quality_meter (each loop ends in a synchronise).
Every time is the median of REGIONS timed regions, printed with min and max."""
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from bench_optim import CFG, REGIONS, dev, fmt  # noqa: E402
from mp_hsir_amd import metrics, ops, validate  # noqa: E402
from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net  # noqa: E402

CALLS = 50


def host_timed(fn, calls=CALLS, warm=3):
    """-> (median, min, max) milliseconds per call by the host clock: `calls` calls, then a synchronise"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / calls)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def tail_plain(p, s, sam):
    """metrics.compute_quality after quality_bands, degraded=None"""
    return torch.stack([p.mean(1).mean(), s.mean(1).mean(), sam.mean()]).tolist()


def tail_masked(p, s, sam, use):
    """metrics.compute_quality after quality_bands, with the band mask (the mask itself, a reduction over the degraded cube, is not timed)"""
    n = use.sum(1)
    ok = n > 0
    nd = n.clamp(min=1).double()
    zero = torch.zeros((), dtype=torch.float64, device=p.device)
    pm = torch.where(use, p, zero).sum(1) / nd
    sm = torch.where(use, s, zero).sum(1) / nd
    cnt = ok.sum()
    cd = cnt.clamp(min=1).double()
    return torch.stack([torch.where(ok, pm, zero).sum() / cd, torch.where(ok, sm, zero).sum() / cd, torch.where(ok, sam, zero).sum() / cd, cnt.double()]).tolist()


def leg_meter():
    g = torch.Generator(device=dev).manual_seed(5)
    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)          # 512 MB: twice the last-level cache
    for B, C in ((4, 31), (16, 31), (4, 100)):
        c = torch.rand((B, C, 64, 64), generator=g, device=dev)
        p, s, sam, px = ops.quality_bands(c + 0.05 * torch.randn((B, C, 64, 64), generator=g, device=dev), c)
        use = torch.rand((B, C), generator=g, device=dev) < 0.3
        use[:, 0] = True
        use8 = use.to(torch.uint8)
        table = torch.zeros((6, 8), dtype=torch.float64, device=dev)
        rows = {"meter": host_timed(lambda: ops.quality_meter(table, 2, p, s, sam, px)),
                "meter + use": host_timed(lambda: ops.quality_meter(table, 2, p, s, sam, px, use=use8)),
                "tail": host_timed(lambda: tail_plain(p, s, sam)), "tail + use": host_timed(lambda: tail_masked(p, s, sam, use))}
        cold = []
        for _ in range(21):
            flush.fill_(1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.quality_meter(table, 2, p, s, sam, px, use=use8)
            b.record()
            torch.cuda.synchronize()
            cold.append(a.elapsed_time(b))
        cold.sort()
        print("(B, C) = (%d, %d), host clock, %d calls then a synchronise, per call:" % (B, C, CALLS), flush=True)
        for k in ("meter", "meter + use", "tail", "tail + use"):
            print("  %-12s %s" % (k, fmt(rows[k])), flush=True)
        print("  tail / meter %.1f, (tail + use) / (meter + use) %.1f" % (rows["tail"][0] / rows["meter"][0], rows["tail + use"][0] / rows["meter + use"][0]))
        print("  one meter launch, inputs cold, device events: %.4f ms [%.4f .. %.4f] (median of 21)" % (cold[10], cold[0], cold[-1]), flush=True)


def leg_pass():
    torch.manual_seed(2024)
    net = MP_HSIR_Net(**CFG, compute_dtype=torch.bfloat16, clip_prompt="surrogate").to(dev).train()
    crops = torch.rand((8, 31, 256, 256), generator=torch.Generator().manual_seed(6))
    modes = (0, 1, 5, 7, 8, 10)
    vset = validate.ValidationSet.from_crops(crops, "natural_scene", dev, modes=modes, seed=2025, net=net)
    val = validate.Validator(net, vset, batch=4)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def timed_pass(fn, warm=1):
        for _ in range(warm):
            fn()
        ts = sorted(once(fn)[0] for _ in range(REGIONS))
        return ts[len(ts) // 2], ts[0], ts[-1]

    def old_way():
        net.eval()
        out = {}
        with torch.no_grad():
            for m in modes:
                ps = ss = sa = 0.0
                n = 0
                for i0 in range(0, 8, 4):
                    y = net(vset.degraded[m][i0:i0 + 4], val._prompt[m]).float()
                    q = metrics.compute_quality(y, vset.clean[i0:i0 + 4], vset.degraded[m][i0:i0 + 4] if m == 10 else None)
                    ps, ss, sa, n = ps + q["psnr"] * q["count"], ss + q["ssim"] * q["count"], sa + q["sam"] * q["count"], n + q["count"]
                out[m] = (ps / max(n, 1), ss / max(n, 1), sa / max(n, 1), n)
        net.train()
        return out

    def partial(upto):
        def run():
            net.eval()
            with torch.no_grad():
                for r, m in enumerate(modes):
                    for j, i0 in enumerate(range(0, 8, 4)):
                        y = net(vset.degraded[m][i0:i0 + 4], val._prompt[m]).float().contiguous()
                        if upto >= 1:
                            q = ops.quality_bands(y, vset.clean[i0:i0 + 4], out=val._q)
                        if upto >= 2:
                            ops.quality_meter(val.table, r, *q[:4], use=None if vset.use[m] is None else vset.use[m][i0:i0 + 4], reset=j == 0)
            net.train()
        return run

    new = timed_pass(val.run)
    old = timed_pass(old_way)
    res, ref = val.run(), old_way()
    print("one pass, 8 crops of 31 x 256 x 256, 6 modes, batch 4, bf16 (host clock around the pass, synchronised):")
    print("  Validator.run(), eager forward        %s" % fmt(new))
    print("  compute_quality + read-back per batch %s, old / new %.3f" % (fmt(old), old[0] / new[0]), flush=True)
    for m in modes:
        print("    mode %2d psnr %.6f | %.6f  ssim %.6f | %.6f  sam %.5f | %.5f  n %d | %d" % (m, res[m]["psnr"], ref[m][0], res[m]["ssim"], ref[m][1],
                                                                                             res[m]["sam"], ref[m][2], res[m]["n"], ref[m][3]))
    f, fq, fqm = timed_pass(partial(0)), timed_pass(partial(1)), timed_pass(partial(2))
    print("  shares: forwards alone %s; + quality_bands %s; + quality_meter %s -> forward %.1f %%, quality %.1f %%, meter %.1f %% of the last"
          % (fmt(f), fmt(fq), fmt(fqm), 100 * f[0] / fqm[0], 100 * (fq[0] - f[0]) / fqm[0], 100 * (fqm[0] - fq[0]) / fqm[0]), flush=True)
    gval = validate.Validator(net, vset, batch=4, forward="graphed")
    first = once(gval.run)[0]
    steady = timed_pass(gval.run, warm=0)         # every batch of every mode has one shape: the first pass held the two eager calls and the capture
    print("  Validator(forward='graphed'): first pass %.1f ms (two eager calls, the capture, 9 replays), then %s per pass over unchanged weights; "
          "eager / replayed %.3f, first graphed / eager %.3f" % (first, fmt(steady), new[0] / steady[0], first / new[0]), flush=True)


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["meter", "pass"]:
        {"meter": leg_meter, "pass": leg_pass}[leg]()
