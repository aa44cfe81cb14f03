"""Self-ensemble (mp-hsir_amd/scene.py ensemble = 4 / 8, csrc/scene_d4.hip): what the two launches cost per transform and what the ensemble
costs per scene.  The sibling of bench_scene.py, whose timing method it uses (the median of REGIONS regions of device events).

    python tools/bench/bench_ensemble.py [kernels] [path]          (no argument: both legs)

kernels  31 x 1024 x 1024, tile 256, overlap 32 (25 tiles): mphsir_scene_gather_d4 and mphsir_scene_fold_d4 alone, one pass (G = 1) under
         each of the eight modes, beside a device-to-device copy_ of the same number of bytes timed in the same run.  Bytes are the
         algorithm's: gather 2 x tiles (read + write); fold 2 x tiles for a first pass (read y, write the store -- G = 1 reads no store)
         and 3 x tiles for a later one (read y, read and write the store: timed as pass 1 of G = 2, where a copy of 2 x has one access
         per element less); the later pass also with a transposing mode among the G, where every mode uses the 32 x 32 ownership of
         store elements.  The existing scene_gather is timed alongside as the mode-0 yardstick.
path     SceneRestorer on a 31 x 1024 x 1024 scene, bf16, tile_batch 16, ensemble 1 / 4 / 8, three repeats each, alternating: time per
         scene against G x the ensemble-1 time of the same run, the number of forwards, and the same restorer around an identity
         "network" (gather + fold + blend, nothing else) for the share of the scene code.
"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from bench_scene import dev, fmt, natural_net, timed  # noqa: E402
from mp_hsir_amd import ops  # noqa: E402
from mp_hsir_amd.scene import SceneRestorer, plan_tiles  # noqa: E402


def leg_kernels():
    C, H, W = 31, 1024, 1024
    p = plan_tiles(H, W, 256, 32)
    n = len(p)
    scene = torch.rand((C, H, W), device=dev)
    origins = torch.tensor(p.origins, dtype=torch.int32, device=dev)
    tiles = torch.empty((n, C, p.th, p.tw), device=dev)
    y = torch.rand((n, C, p.th, p.tw), device=dev)
    store = torch.zeros_like(tiles)
    nb = 4.0 * tiles.numel()
    src, dst = torch.rand(tiles.numel() * 3 // 2, device=dev), torch.empty(tiles.numel() * 3 // 2, device=dev)
    c2 = timed(lambda: dst[:tiles.numel()].copy_(src[:tiles.numel()]), 20)
    c3 = timed(lambda: dst.copy_(src), 20)
    g0 = timed(lambda: ops.scene_gather_tiles(scene, origins, p.th, p.tw, out=tiles), 20)
    print("C=%d %dx%d, %d tiles of %dx%d = %.0f MB | copy_ of 2 x tiles %s | copy_ of 3 x tiles %s | scene_gather %s, kernel / copy bandwidth %.2f"
          % (C, H, W, n, p.th, p.tw, nb * 1e-6, fmt(c2, 2 * nb), fmt(c3, 3 * nb), fmt(g0, 2 * nb), c2[0] / g0[0]), flush=True)
    for m in range(8):
        g = timed(lambda: ops.scene_gather_d4(scene, origins, p.th, p.tw, 0, (m,), out=tiles), 20)
        f1 = timed(lambda: ops.scene_fold_d4(y, store, 0, n, (m,)), 20)
        f2 = timed(lambda: ops.scene_fold_d4(y, store, n, n, (0, m)), 20)
        f3 = timed(lambda: ops.scene_fold_d4(y, store, n, n, (3, m)), 20)           # beside a transposing pass: the 32 x 32 ownership
        print("  mode %d: gather_d4 %s, / copy %.2f | fold_d4 first pass %s, / copy %.2f | fold_d4 later pass (read-modify-write) %s, / copy of 3 x %.2f"
              " | the same within an ensemble that transposes %s, / copy of 3 x %.2f"
              % (m, fmt(g, 2 * nb), c2[0] / g[0], fmt(f1, 2 * nb), c2[0] / f1[0], fmt(f2, 3 * nb), c3[0] / f2[0], fmt(f3, 3 * nb), c3[0] / f3[0]), flush=True)


def leg_path():
    net = natural_net(torch.bfloat16)
    C, H, W, tb = 31, 1024, 1024, 16
    scene = torch.rand((C, H, W), device=dev)
    rs = {G: SceneRestorer(net, tile=256, overlap=32, tile_batch=tb, graphed=True, ensemble=G) for G in (1, 4, 8)}
    ids = {G: SceneRestorer(lambda x, i: x, tile=256, overlap=32, tile_batch=tb, ensemble=G) for G in (1, 4, 8)}
    n = len(rs[1].plan(H, W))
    for G in rs:
        for _ in range(4):
            rs[G](scene, 0)
    times = {G: [] for G in rs}
    for rep in range(3):
        for G in rs:
            times[G].append(timed(lambda: rs[G](scene, 0), 2, warm=1))
    base = sorted(t[0] for t in times[1])
    print("ensemble 1 (%d tiles, %d forwards): scene %s ms over three repeats, spread %.3f ms" % (n, -(-n // tb), ["%.3f" % t for t in base], base[-1] - base[0]))
    for G in (1, 4, 8):
        ident = timed(lambda: ids[G](scene, 0), 5)
        med = sorted(t[0] for t in times[G])
        print("ensemble %d: %d forwards; scene %s ms, median %.3f = %.3f x ensemble 1 (G x ensemble 1 = %.3f ms) | gather + fold + blend %s = %.2f%% of "
              "the scene" % (G, -(-n * G // tb), ["%.3f" % t for t in med], med[1], med[1] / base[1], G * base[1], fmt(ident), 100.0 * ident[0] / med[1]), flush=True)


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["kernels", "path"]:
        {"kernels": leg_kernels, "path": leg_path}[leg]()
