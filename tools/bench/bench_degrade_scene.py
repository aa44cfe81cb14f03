"""Degradation of whole cubes (mp-hsir_amd/degrade.py SceneDegrader, csrc/degrade.hip degrade_planes_kernel): what degrading one scene
costs under each of test.py's modes 0-10 by the tensor programs and by plan + one launch.  Timing as bench_degrade.py (the median of
REGIONS regions of device events, with min .. max); each region walks a ring of distinct cubes whose bytes exceed the 256 MB cache, so no
call finds its input there.

    python tools/bench/bench_degrade_scene.py [scene] [synth]          (no argument: both legs)

scene  per mode, at 31 x 1024 x 1024, 100 x 1024 x 1024 and 31 x 1000 x 700 (no multiple of 64; mode 7 by 4 there, 8 does not divide 700):
       (a) test.py::degrade_for_mode, the tensor programs (the parent commit's path, untouched); (b) SceneDegrader: plan + launch;
       (c) the launch alone on a prepared plan; (d) a copy_ of one cube into another: one read and one write, the launch's traffic floor.
       Peak extra memory of (a) and (b): torch.cuda.max_memory_allocated over one call, less what was allocated before it.
synth  one DegradationSynthesizer call at 32 x 31 x 192 x 192, beyond the plane form: the tensor path against plan + launch.
"""
import importlib
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from bench_scene import REGIONS, dev, fmt, timed  # noqa: E402
from mp_hsir_amd import degrade as D  # noqa: E402
from mp_hsir_amd import ops  # noqa: E402

T = importlib.import_module("mp_hsir_amd.test")
SHAPES = [("natural_scene", 31, 1024, 1024), ("remote_sensing", 100, 1024, 1024), ("natural_scene", 31, 1000, 700)]
CACHE = 256e6


def ring(fn, cubes):
    """fn(cube) over the ring: one region = one pass, so per-call time with every input cold"""
    def once():
        for c in cubes:
            fn(c)
    t = timed(once, 1, warm=1)
    return tuple(v / len(cubes) for v in t)


def peak_extra(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def leg_scene():
    for model, C, H, W in SHAPES:
        nbytes = 4.0 * C * H * W
        n = int(CACHE // nbytes) + 2
        cubes = [torch.rand((1, C, H, W), device=dev) for _ in range(n)]
        dst = torch.empty_like(cubes[0])
        cp = ring(lambda c: dst.copy_(c), cubes)
        print("%s %d x %d x %d (%.0f MB per cube, ring of %d): (d) copy_ of one cube %s" % (model, C, H, W, nbytes * 1e-6, n, fmt(cp, 2 * nbytes)), flush=True)
        print("  mode | (a) tensor programs | (b) plan + launch | (a) / (b) | (c) launch alone | (d) / (c) | peak extra MB (a) | (b)", flush=True)
        for mode in range(11):
            o = T.build_parser().parse_args(["--mode", str(mode), "--model", model] + (["--downsample_factor", "4"] if W % 8 else []))
            draws, sd = D.Draws(dev, 1), D.SceneDegrader(model, dev, 1)
            a = ring(lambda c: T.degrade_for_mode(o, c, draws, model), cubes)
            b = ring(lambda c: sd(c, mode, o), cubes)
            plan = sd.plan(cubes[0], mode, o)
            out = (dst, None)
            k = ring(lambda c: ops.degrade_planes(c, plan, seed=1, ordinal=0, out=out), cubes)
            ma, mb = peak_extra(lambda: T.degrade_for_mode(o, cubes[0], draws, model)), peak_extra(lambda: sd(cubes[0], mode, o))
            print("  %4d | %s | %s | %.2f x | %s | %.2f | %.0f | %.0f" % (mode, fmt(a), fmt(b), a[0] / b[0], fmt(k, 2 * nbytes), cp[0] / k[0], ma * 1e-6, mb * 1e-6),
                  flush=True)
        del cubes, dst
        torch.cuda.empty_cache()


def leg_synth():
    menu = ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"]
    n = 4
    cubes = [torch.rand((32, 31, 192, 192), device=dev) for _ in range(n)]
    tens = D.DegradationSynthesizer("natural_scene", menu, dev, seed=1)
    fus = D.DegradationSynthesizer("natural_scene", menu, dev, seed=1, fused=True)
    a, b = ring(lambda c: tens(c), cubes), ring(lambda c: fus(c), cubes)
    plan, _ = fus.fused_plan(cubes[0])
    out = (torch.empty_like(cubes[0]), torch.empty_like(cubes[0]))
    k = ring(lambda c: ops.degrade_planes(c, plan, seed=1, ordinal=0, out=out), cubes)
    print("synthesiser 32 x 31 x 192 x 192 (%.0f MB per batch, ring of %d), natural-scene menu: tensor %s | fused (plan + tiled launch) %s = %.2f x | "
          "launch alone %s" % (cubes[0].numel() * 4e-6, n, fmt(a), fmt(b), a[0] / b[0], fmt(k, 12.0 * cubes[0].numel())), flush=True)


if __name__ == "__main__":
    assert REGIONS == 7
    for leg in sys.argv[1:] or ["scene", "synth"]:
        {"scene": leg_scene, "synth": leg_synth}[leg]()
