"""Spectral windows (mp-hsir_amd/scene.py bands=..., csrc/scene_d4.hip bands_gather, csrc/scene_bands.hip): what the two launches cost
beside a copy, what the band axis costs where it is not needed, and the scene time of a scene that needs no windows.  The sibling of
bench_scene.py and bench_ensemble.py, whose timing method it uses (the median of REGIONS regions of device events, min and max shown).

    python tools/bench/bench_scene_bands.py [--root CHECKOUT] [kernels] [one_window] [scene]          (no leg named: all three)

kernels     191 x 1024 x 1024 under C = 31 (ovb 7: 8 windows x 25 tiles) and 210 x 1024 x 1024 under C = 100 (ovb 25: 3 windows x 25 tiles),
            tile 256, overlap 32: mphsir_scene_gather_bands (one pass, mode 0; and mode 2, through LDS) and mphsir_scene_blend_bands alone,
            each beside a device-to-device copy_ of the same number of bytes timed in the same run.  Bytes are the algorithm's, from the
            plan: gather 2 x items (read + write); blend the item bands that map into the scene (mirror padding is never read) + the scene.
            The blend's traffic per output band is printed from the plan as well: the mean number of items read per scene element.
one_window  31 x 1024 x 1024, C = 31: the band blend with one window against mphsir_scene_blend on the same tiles, alternating in one
            process, and the band gather against mphsir_scene_gather_d4 -- what the band axis costs where it is not needed (the restorer
            never takes that path: a scene of the model's band count issues the old launches).
scene       SceneRestorer on the default 31 x 1024 x 1024 scene, bf16, tile 256, overlap 32, tile_batch 16, ensemble 1 and 8: time per scene,
            three repeats each, alternating.  --root CHECKOUT imports the package (and loads the library) of another checkout of the
            project: run the leg in alternating processes with and without it to compare two commits.  The launch list of such a
            scene does not involve the band kernels.
"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGS = sys.argv[1:]
PKG_ROOT = os.path.abspath(ARGS.pop(ARGS.index("--root") + 1)) if "--root" in ARGS else ROOT
ARGS = [a for a in ARGS if a != "--root"]
sys.path.insert(0, PKG_ROOT)          # the package of --root's checkout (the `scene` leg); the golden fixtures are this checkout's
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

import mp_hsir_amd  # noqa: E402,F401  -- first, from PKG_ROOT: bench_scene puts this checkout in front of sys.path and would import its own
from bench_scene import dev, fmt, natural_net, timed  # noqa: E402
from mp_hsir_amd import ops  # noqa: E402
from mp_hsir_amd.scene import SceneRestorer, plan_tiles  # noqa: E402


def leg_kernels():
    from mp_hsir_amd.scene import plan_bands
    H = W = 1024
    for Cs, C, ovb in ((191, 31, 7), (210, 100, 25)):
        p = plan_tiles(H, W, 256, 32)
        ob = plan_bands(Cs, C, ovb)
        rows = [(b, y, x) for b in ob for (y, x) in p.origins]
        N = len(rows)
        scene = torch.rand((Cs, H, W), device=dev)
        origins3 = torch.tensor(rows, dtype=torch.int32, device=dev)
        obd, oyd, oxd = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (ob, p.oy, p.ox))
        tiles = torch.empty((N, C, p.th, p.tw), device=dev)
        out = torch.empty_like(scene)
        gb = 8.0 * tiles.numel()
        read = sum(min(C, Cs - b) for b in ob) * len(p) * p.th * p.tw          # item elements that map into the scene (nothing spatial is padded here)
        bb = 4.0 * (read + scene.numel())
        src = torch.rand(tiles.numel(), device=dev)
        dst = torch.empty_like(src)
        print("Cs=%d under C=%d (ovb %d): band origins %s x %d tiles = %d items of %dx%dx%d: store %.0f MB, scene %.0f MB; the blend reads %.2f item "
              "elements per scene element" % (Cs, C, ovb, ob, len(p), N, C, p.th, p.tw, tiles.numel() * 4e-6, scene.numel() * 4e-6, read / scene.numel()))
        gc = timed(lambda: dst.copy_(src), 10)
        for m in (0, 2):
            g = timed(lambda: ops.scene_gather_bands(scene, origins3, C, p.th, p.tw, 0, (m,), tiles), 10)
            print("  gather mode %d  %s | copy_ of the same bytes %s | kernel / copy bandwidth %.2f" % (m, fmt(g, gb), fmt(gc, gb), gc[0] / g[0]))
        b = timed(lambda: ops.scene_blend_bands(tiles, obd, oyd, oxd, p.ov, ovb, Cs, H, W, out=out), 10)
        n2 = int(bb / 8)
        bc = timed(lambda: dst[:n2].copy_(src[:n2]), 10)
        print("  blend          %s | copy_ of the same bytes %s | kernel / copy bandwidth %.2f" % (fmt(b, bb), fmt(bc, bb), bc[0] / b[0]), flush=True)
        del scene, tiles, out, src, dst
        torch.cuda.empty_cache()


def leg_one_window():
    C, H, W = 31, 1024, 1024
    p = plan_tiles(H, W, 256, 32)
    n = len(p)
    scene = torch.rand((C, H, W), device=dev)
    tiles = torch.rand((n, C, p.th, p.tw), device=dev)
    out_a, out_b = torch.empty_like(scene), torch.empty_like(scene)
    origins = torch.tensor(p.origins, dtype=torch.int32, device=dev)
    origins3 = torch.tensor([(0, y, x) for y, x in p.origins], dtype=torch.int32, device=dev)
    zero, oyd, oxd = (torch.tensor(v, dtype=torch.int32, device=dev) for v in ([0], p.oy, p.ox))
    bb = 4.0 * (tiles.numel() + scene.numel())
    for rep in range(3):
        old = timed(lambda: ops.scene_blend_tiles(tiles, oyd, oxd, p.ov, H, W, out=out_a), 20)
        new = timed(lambda: ops.scene_blend_bands(tiles, zero, oyd, oxd, p.ov, 7, C, H, W, out=out_b), 20)
        print("one window, blend:  scene_blend %s | scene_blend_bands %s | bands / plain time %.2f" % (fmt(old, bb), fmt(new, bb), new[0] / old[0]))
    assert torch.equal(out_a, out_b)
    cut = torch.empty_like(tiles)
    for rep in range(3):
        old = timed(lambda: ops.scene_gather_d4(scene, origins, p.th, p.tw, 0, (0,), out=cut), 20)
        new = timed(lambda: ops.scene_gather_bands(scene, origins3, C, p.th, p.tw, 0, (0,), cut), 20)
        print("one window, gather: scene_gather_d4 %s | scene_gather_bands %s | bands / d4 time %.2f"
              % (fmt(old, 8.0 * cut.numel()), fmt(new, 8.0 * cut.numel()), new[0] / old[0]), flush=True)


def leg_scene():
    net = natural_net(torch.bfloat16)
    C, H, W, tb = 31, 1024, 1024, 16
    scene = torch.rand((C, H, W), device=dev)
    rs = {G: SceneRestorer(net, tile=256, overlap=32, tile_batch=tb, graphed=True, ensemble=G) for G in (1, 8)}
    for G in rs:
        for _ in range(4):
            rs[G](scene, 0)
    times = {G: [] for G in rs}
    for rep in range(3):
        for G in rs:
            times[G].append(timed(lambda: rs[G](scene, 0), 2, warm=1))
    for G in rs:
        med = sorted(t[0] for t in times[G])
        print("scene 31x1024x1024 bf16, ensemble %d (%s): %s ms over three repeats, median %.3f, spread %.3f"
              % (G, "this checkout" if PKG_ROOT == ROOT else PKG_ROOT, ["%.3f" % t for t in med], med[1], med[-1] - med[0]), flush=True)


if __name__ == "__main__":
    for leg in ARGS or ["kernels", "one_window", "scene"]:
        {"kernels": leg_kernels, "one_window": leg_one_window, "scene": leg_scene}[leg]()
