"""Scene quality (mp-hsir_amd/metrics.py, csrc/quality.hip): the fused PSNR / SSIM / SAM kernel against the tensor-program path it stands beside.

    python tools/bench/bench_quality.py [sizes] [share]          (no argument: both legs)

sizes   on 31 x 512 x 512, 31 x 1024 x 1024, 100 x 1024 x 1024 and 100 x 2048 x 2048 (noisy restored cube against a clean one), alternating in
        the same run:
          1. metrics.compute_psnr_ssim   the tensor programs in float64 (PSNR / SSIM only): the yardstick
          2. metrics.compute_quality     the fused kernel pair + the band / image means + the one transfer to the host
          3. ops.quality_bands           the launch pair alone, with the bytes it has to read (two fp32 cubes) per second
          4. a device-to-device copy_ of 2 B C H W 4 bytes: the project's yardstick for a streaming kernel
        and the rise of the peak of allocated memory around one call of 1 and of 2, in units of one input cube.
share   what part of a test.py --tile 256 scene (31 x 1024 x 1024, bf16, the restorer's defaults) the scoring is: SceneRestorer alone, then
        each scoring path alone, all as wall time per scene (the scores come back as Python floats, so each call ends synchronised).
Every time is the median of REGIONS timed regions (device events around several calls each), printed with min and max.
"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from mp_hsir_amd import metrics, ops  # noqa: E402

dev = torch.device("cuda")
REGIONS = 7


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
    s = "%.3f ms [%.3f .. %.3f]" % t
    return s + (" = %.2f TB/s" % (nbytes / t[0] / 1e9) if nbytes else "")


def peak_rise(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def leg_sizes():
    for C, H, W in ((31, 512, 512), (31, 1024, 1024), (100, 1024, 1024), (100, 2048, 2048)):
        clean = torch.rand((1, C, H, W), device=dev)
        restored = clean + torch.randn_like(clean) * 0.05
        cube = clean.numel() * 4
        n = 20 if cube < 2e8 else 5
        a = metrics.compute_psnr_ssim(restored, clean)
        q = metrics.compute_quality(restored, clean)
        print("C=%d %dx%d (one cube %.0f MB): torch psnr %.6f ssim %.8f | fused psnr %.6f ssim %.8f sam %.4f deg"
              % (C, H, W, cube * 1e-6, a[0], a[1], q["psnr"], q["ssim"], q["sam"]))
        src = torch.empty(2 * clean.numel(), device=dev)
        dst = torch.empty_like(src)
        rows = {}
        for rnd in range(2):                                   # alternate: two rounds of each, the second is reported
            rows["torch"] = timed(lambda: metrics.compute_psnr_ssim(restored, clean), max(n // 5, 1))
            rows["fused"] = timed(lambda: metrics.compute_quality(restored, clean), n)
            rows["kernels"] = timed(lambda: ops.quality_bands(restored, clean), n)
            rows["copy"] = timed(lambda: dst.copy_(src), n)
        del src, dst
        torch.cuda.empty_cache()
        m_torch = peak_rise(lambda: metrics.compute_psnr_ssim(restored, clean))
        m_fused = peak_rise(lambda: metrics.compute_quality(restored, clean))
        print("  1 compute_psnr_ssim %s | peak memory rise %.2f cubes" % (fmt(rows["torch"]), m_torch / cube))
        print("  2 compute_quality   %s | peak memory rise %.4f cubes (%d bytes) | torch / fused %.1f x"
              % (fmt(rows["fused"]), m_fused / cube, m_fused, rows["torch"][0] / rows["fused"][0]))
        print("  3 quality_bands     %s | 4 copy_ of 2 cubes %s (counted as the 2 cubes it reads) | kernels / copy time %.2f"
              % (fmt(rows["kernels"], 2.0 * cube), fmt(rows["copy"], 2.0 * cube), rows["kernels"][0] / rows["copy"][0]), flush=True)
        del clean, restored
        torch.cuda.empty_cache()


def leg_share():
    from golden.cases import NATURAL_CFG
    from golden.detfill import det_fill_, surrogate_clip_prompt
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    from mp_hsir_amd.scene import SceneRestorer
    net = MP_HSIR_Net(**NATURAL_CFG, clip_prompt=surrogate_clip_prompt(NATURAL_CFG["task_classes"])).eval()
    det_fill_(net)
    net = net.to(dev).set_compute_dtype(torch.bfloat16)
    C, H, W = 31, 1024, 1024
    clean = torch.rand((1, C, H, W), device=dev)
    noisy = clean + torch.randn_like(clean) * (70.0 / 255.0)
    r = SceneRestorer(net, tile=256, overlap=32)
    restored = r(noisy, 0)
    t_r = timed(lambda: r(noisy, 0), 2, warm=4)
    t_t = timed(lambda: metrics.compute_psnr_ssim(restored, clean), 4)
    t_f = timed(lambda: metrics.compute_quality(restored, clean), 20)
    print("31x1024x1024 bf16, tile 256: restore %s | score (torch) %s = %.1f%% of restore + score | score (fused) %s = %.2f%% of restore + score"
          % (fmt(t_r), fmt(t_t), 100.0 * t_t[0] / (t_r[0] + t_t[0]), fmt(t_f), 100.0 * t_f[0] / (t_r[0] + t_f[0])), flush=True)


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["sizes", "share"]:
        {"sizes": leg_sizes, "share": leg_share}[leg]()
