"""The HBM-resident scene store as a training source (mp-hsir_amd/scene_store.py, data.SceneStoreSource, csrc/patch_sample.hip): what the
launch pair costs beside its traffic floor, what a whole next() costs beside PatchDBSource's, and what that does to a train.py-shaped loop.
Timing as bench_scene.py (the median of REGIONS regions, with min .. max).

    python tools/bench/bench_patch_source.py [pair] [next] [loop] [build]          (no argument: all legs)

pair   ops.patch_sample alone at 32 x 31 x 64 x 64 and 32 x 100 x 64 x 64 beside a copy_ of 1.5 x the batch bytes (two reads, one write:
       the pair's traffic), grid origins (16-byte rows) and jittered origins (element-wise rows) apart, and what each of the two launches takes by the
       library's launch timer (a kernel id each: patch_sample = min / max, patch_normalise).
next   src.next() end to end, host clock with a final synchronise: PatchDBSource (its database exported from the same store to a
       temporary directory on local disk, read once before: page-cache warm) against SceneStoreSource, both fused_degrade=True.
loop   bench_degrade.py's loop leg with the two real-data sources beside bench.py's pooled batches, in patches per second.
build  store build time and resident bytes for a stand-in set of 8 scenes of 31 x 1280 x 1280.
"""
import os
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from bench_degrade import MENUS, STEPS, wall  # noqa: E402
from bench_scene import REGIONS, dev, fmt, timed  # noqa: E402
from make_patch_db import export_patch_db  # noqa: E402
from mp_hsir_amd.data import PatchDB, PatchDBSource, SceneStoreSource, SyntheticPatchSource  # noqa: E402
from mp_hsir_amd.scene_store import SceneStore  # noqa: E402

SHAPES = {"natural_scene": (31, 512, 2), "remote_sensing": (100, 256, 2)}         # bands, scene side, scenes of the timing stores


def make_store(data_type):
    C, side, n = SHAPES[data_type]
    g = torch.Generator().manual_seed(7)
    return SceneStore([torch.rand((C, side, side), generator=g).numpy() for _ in range(n)], data_type, dev,
                      sources=["ICVL_%d.mat" % i if data_type == "natural_scene" else "Synthetic_%d.mat" % i for i in range(n)])


def leg_pair():
    import ctypes
    from mp_hsir_amd import _lib
    lib = _lib.load()
    lib.mphsir_kernel_name.restype = ctypes.c_char_p
    kids = [k for k in range(64) if lib.mphsir_kernel_name(k) in (b"patch_sample", b"patch_normalise")]      # launch 1, launch 2
    for data_type in SHAPES:
        st = make_store(data_type)
        C, B, P = st.C, 32, st.patch
        nb = 12.0 * B * C * P * P
        a, b = torch.rand(B * C * P * P * 3 // 2, device=dev), torch.empty(B * C * P * P * 3 // 2, device=dev)
        cp = timed(lambda: b.copy_(a), 20)
        g = torch.Generator(device=dev).manual_seed(3)
        idx = torch.randint(0, len(st), (B,), generator=g, device=dev)
        rec = st.records.index_select(0, idx)
        jit = rec.clone()
        jit[:, 1:] += torch.randint(1, 4, (B, 2), generator=g, device=dev, dtype=torch.int32)      # origins off the 16-byte grid; the kernel clamps
        out = torch.empty((B, C, P, P), device=dev)
        ws = torch.empty((2 * B * C,), device=dev)
        print("%s 32 x %d x 64 x 64 (%d records, %.0f MB resident): copy_ of 1.5 x the batch bytes %s" % (data_type, C, len(st), st.nbytes / 1e6, fmt(cp, nb)), flush=True)
        for name, fn in (("grid origins", lambda: st.sample(idx, out=out, workspace=ws)), ("jittered origins", lambda: st.sample_at(jit, out=out, workspace=ws))):
            t = timed(fn, 20)
            share = []
            for kid in kids:                                  # the timer follows one kernel id at a time: the two launches have one each
                lib.mphsir_prof_enable(kid)
                for _ in range(20):
                    fn()
                n, ms = ctypes.c_int(0), ctypes.c_float(0)
                lib.mphsir_prof_read(ctypes.byref(n), ctypes.byref(ms))
                lib.mphsir_prof_enable(-1)
                share.append("%s %.4f ms over %d launches" % (lib.mphsir_kernel_name(kid).decode(), ms.value / max(n.value, 1), n.value))
            print("  %-17s pair %s, copy / pair %.2f (launch timer: %s)" % (name, fmt(t, nb), cp[0] / t[0], ", ".join(share)), flush=True)


def leg_next():
    for data_type, (C, menu) in MENUS.items():
        st = make_store(data_type)
        with tempfile.TemporaryDirectory() as tmp:
            export_patch_db(st, tmp)
            db = PatchDB(tmp, dataset_names=None)
            with open(os.path.join(tmp, "data.bin"), "rb") as f:
                while f.read(1 << 24):
                    pass
            a = PatchDBSource(db, 32, menu, data_type, dev, seed=5, fused_degrade=True)
            b = SceneStoreSource(st, 32, menu, data_type, dev, seed=5, fused_degrade=True)
            c = SceneStoreSource(st, 32, menu, data_type, dev, seed=5, fused_degrade=True, jitter=True)
            for s in (a, b, c):
                for _ in range(3):
                    s.next()
            wa, wb, wc = wall(a.next), wall(b.next), wall(c.next)
            print("%s next(): PatchDBSource %.3f ms [%.3f .. %.3f] | SceneStoreSource %.3f ms [%.3f .. %.3f] = %.2f x | with jitter %.3f ms [%.3f .. %.3f]"
                  % ((data_type,) + wa + wb + (wa[0] / wb[0],) + wc), flush=True)
            del a, db


def leg_loop():
    from bench import MODELS
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    cfg = MODELS["natural_scene"]
    torch.manual_seed(2024)
    net = MP_HSIR_Net(**cfg, compute_dtype=torch.bfloat16, clip_prompt="surrogate").to(dev).train()
    eng = DataParallelEngine(net, lr=2e-4, use_graph=True)
    types = MENUS["natural_scene"][1]
    st = make_store("natural_scene")
    with tempfile.TemporaryDirectory() as tmp:
        export_patch_db(st, tmp)
        db = PatchDB(tmp, dataset_names=None)
        srcs = {"pooled": SyntheticPatchSource(31, 64, 32, cfg["task_classes"], dev, 2024, 0, de_types=types, pool=8).prefill(),
                "patch_db": PatchDBSource(db, 32, types, "natural_scene", dev, seed=5, fused_degrade=True),
                "scene_store": SceneStoreSource(st, 32, types, "natural_scene", dev, seed=5, fused_degrade=True)}

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
        for k, v in rates.items():
            m = sorted(v)[len(v) // 2]
            print("loop %-11s %.2f steps/s [%.2f .. %.2f] = %.0f patches/s, %.3f ms per step" % (k, m, min(v), max(v), 32 * m, 1e3 / m), flush=True)
        eng.finish()
        del srcs, db


def leg_build():
    g = torch.Generator().manual_seed(9)
    scenes = [torch.rand((31, 1280, 1280), generator=g).numpy() for _ in range(8)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = SceneStore(scenes, "natural_scene", dev)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    raw = sum(s.size for s in scenes) * 4
    print("build: 8 scenes of 31 x 1280 x 1280 (%.2f GB fp32) -> %d records, %.2f GB resident (%.2f x), %d degenerate, %.1f s"
          % (raw / 1e9, len(st), st.nbytes / 1e9, st.nbytes / raw, st.degenerate, dt), flush=True)


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["pair", "next", "loop", "build"]:
        {"pair": leg_pair, "next": leg_next, "loop": leg_loop, "build": leg_build}[leg]()
