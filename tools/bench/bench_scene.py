"""Whole-scene inference (mp-hsir_amd/scene.py, csrc/scene.hip): what the two launches cost and what share of a restored scene they are.

    python tools/bench/bench_scene.py [kernels] [path] [quality]          (no argument: all three legs)

kernels  scene_gather / scene_blend alone at 31 and 100 bands x 1024 x 1024 (5 x 5 tiles, origins multiples of 4) and 31 / 100 x 1000 x 700 (5 x 3
         tiles, origins 0 / 222 / 444 across: the blend's dword path), tile 256, overlap 32: time per launch and
         bytes moved / time, beside a device-to-device torch copy_ of the same number of bytes timed in the same run (the yardstick
         of a streaming kernel) and the torch composite the launch replaces (F.pad(reflect) + slices + stack; a per-tile weighted
         accumulation loop + one division).  Bytes are the algorithm's: gather 2 x tiles, blend tiles + scene.
path     SceneRestorer on a 31 x 1024 x 1024 scene, bf16, tile_batch 1 / 4 / 16: scenes/s and Mpixel/s; the same restorer around an
         identity "network" (gather + tile-store copies + blend, nothing else) for the share of the new code in the wall time; and
         the GraphedForward replay of one tile batch times the number of batches, which is the forward time alone.
quality  for information: relative L2 between SceneRestorer(tile=256) and the whole-cube forward on the 512 x 512 x 31 test cube input
         with the seeded stand-in weights -- two different functions of the input (per-tile spectral Gram, per-tile prompt stretch).
Every time is the median of REGIONS timed regions (device events around several launches each), printed with min and max.
"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore")
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mp_hsir_amd import ops  # noqa: E402
from mp_hsir_amd.scene import SceneRestorer, plan_tiles  # noqa: E402

dev = torch.device("cuda")
REGIONS = 7


def timed(fn, per_region, warm=3):
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


def axis_w(o, th, H, ov):
    u = torch.arange(th, device=dev, dtype=torch.float32)
    w = torch.ones(th, device=dev)
    if o > 0:
        w = torch.minimum(w, (u + 1) / (ov + 1))
    if o + th < H:
        w = torch.minimum(w, (th - u) / (ov + 1))
    return w


def torch_gather(scene, p):
    C, H, W = scene.shape
    padded = F.pad(scene[None], (0, max(p.tw - W, 0), 0, max(p.th - H, 0)), mode="reflect")[0] if (p.th > H or p.tw > W) else scene
    return torch.stack([padded[:, y:y + p.th, x:x + p.tw] for y, x in p.origins])


def torch_blend(tiles, p, weights):
    C = tiles.shape[1]
    num = torch.zeros((C, p.H, p.W), device=dev)
    den = torch.zeros((p.H, p.W), device=dev)
    for t, (y, x) in enumerate(p.origins):
        hh, ww = min(p.th, p.H - y), min(p.tw, p.W - x)
        w = weights[t][:hh, :ww]
        num[:, y:y + hh, x:x + ww] += w * tiles[t, :, :hh, :ww]
        den[y:y + hh, x:x + ww] += w
    return num / den


def leg_kernels():
    # 1024 x 1024: origins are multiples of 192, every tile read of the blend is a 16-byte vector; 1000 x 700: ox = 0, 222, 444, so the
    # tiles of two of three columns are read as dwords (x - ox is not a multiple of 4) and scene rows are not 16-byte aligned either
    for C, H, W in ((31, 1024, 1024), (100, 1024, 1024), (31, 1000, 700), (100, 1000, 700)):
        p = plan_tiles(H, W, 256, 32)
        scene = torch.rand((C, H, W), device=dev)
        origins = torch.tensor(p.origins, dtype=torch.int32, device=dev)
        oy, ox = torch.tensor(p.oy, dtype=torch.int32, device=dev), torch.tensor(p.ox, dtype=torch.int32, device=dev)
        tiles = torch.empty((len(p), C, p.th, p.tw), device=dev)
        out = torch.empty_like(scene)
        weights = [axis_w(y, p.th, H, p.ov)[:, None] * axis_w(x, p.tw, W, p.ov)[None, :] for y, x in p.origins]
        gb, bb = 8.0 * tiles.numel(), 4.0 * (tiles.numel() + scene.numel())
        print("C=%d %dx%d, %d tiles of %dx%d: tile store %.0f MB, scene %.0f MB" % (C, H, W, len(p), p.th, p.tw, tiles.numel() * 4e-6, scene.numel() * 4e-6))
        g = timed(lambda: ops.scene_gather_tiles(scene, origins, p.th, p.tw, out=tiles), 20)
        src = torch.rand(tiles.numel(), device=dev)
        dst = torch.empty_like(src)
        gc = timed(lambda: dst.copy_(src), 20)
        gt = timed(lambda: torch_gather(scene, p), 10)
        print("  gather   %s | copy_ of the same bytes %s | kernel / copy bandwidth %.2f | torch composite %s" % (fmt(g, gb), fmt(gc, gb), gc[0] / g[0], fmt(gt)))
        b = timed(lambda: ops.scene_blend_tiles(tiles, oy, ox, p.ov, H, W, out=out), 20)
        n2 = (tiles.numel() + scene.numel()) // 2
        bc = timed(lambda: dst[:n2].copy_(src[:n2]), 20)
        bt = timed(lambda: torch_blend(tiles, p, weights), 10)
        print("  blend    %s | copy_ of the same bytes %s | kernel / copy bandwidth %.2f | torch composite %s" % (fmt(b, bb), fmt(bc, bb), bc[0] / b[0], fmt(bt)))
        assert torch.equal(torch_gather(scene, p), tiles)
        print("  torch composite blend vs kernel: max abs difference %.3g" % float((torch_blend(tiles, p, weights) - out).abs().max()), flush=True)
        del scene, tiles, out, src, dst, weights
        torch.cuda.empty_cache()


def natural_net(dtype):
    from golden.cases import NATURAL_CFG
    from golden.detfill import det_fill_, surrogate_clip_prompt
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    net = MP_HSIR_Net(**NATURAL_CFG, clip_prompt=surrogate_clip_prompt(NATURAL_CFG["task_classes"])).eval()
    det_fill_(net)
    return net.to(dev).set_compute_dtype(dtype)


def leg_path():
    from mp_hsir_amd.engine import GraphedForward
    net = natural_net(torch.bfloat16)
    C, H, W = 31, 1024, 1024
    scene = torch.rand((C, H, W), device=dev)
    for tb in (1, 4, 16):
        r = SceneRestorer(net, tile=256, overlap=32, tile_batch=tb, graphed=True)
        n = len(r.plan(H, W))
        nb = -(-n // tb)
        whole = timed(lambda: r(scene, 0), 2, warm=4)
        rid = SceneRestorer(lambda x, ids: x, tile=256, overlap=32, tile_batch=tb)
        ident = timed(lambda: rid(scene, 0), 5)
        fwd = GraphedForward(net)
        x, ids = torch.rand((tb, C, 256, 256), device=dev), torch.zeros(tb, dtype=torch.long, device=dev)
        one = timed(lambda: fwd(x, ids), 5, warm=4)
        print("tile_batch %2d (%d tiles, %d forwards): scene %s = %.2f scenes/s, %.1f Mpixel/s | gather + store copies + blend %s = %.1f%% of the scene"
              " | %d x replay of one tile batch %.3f ms = %.1f ms" % (tb, n, nb, fmt(whole), 1e3 / whole[0], H * W * 1e-3 / whole[0], fmt(ident),
                                                                   100.0 * ident[0] / whole[0], nb, one[0], nb * one[0]), flush=True)
        del r, fwd
        torch.cuda.empty_cache()


def leg_quality():
    from golden.cases import cube_inputs
    from util import rel_l2
    c, clean, degraded = cube_inputs("nat512")
    x = degraded.to(dev)
    for dtype in (torch.float32, torch.bfloat16):
        net = natural_net(dtype)
        with torch.no_grad():
            whole = net(x, torch.zeros(1, dtype=torch.long, device=dev))
        tiled = SceneRestorer(net, tile=256, overlap=32, tile_batch=4, graphed=False)(x, 0)
        print("512x512x31 cube, %s, seeded stand-in weights: SceneRestorer(tile=256) vs whole-cube forward rel-L2 %.3g (of the outputs), "
              "%.3g (of the residuals output - input)" % (str(dtype).split(".")[1], rel_l2(tiled.cpu(), whole.cpu()),
                                                           rel_l2((tiled - x).cpu(), (whole - x).cpu())), flush=True)


if __name__ == "__main__":
    legs = sys.argv[1:] or ["kernels", "path", "quality"]
    for leg in legs:
        {"kernels": leg_kernels, "path": leg_path, "quality": leg_quality}[leg]()
