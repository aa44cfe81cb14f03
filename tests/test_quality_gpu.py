"""Scene quality on a real MI355X: the fused kernel (mp-hsir_amd/csrc/quality.hip) at scene sizes against the float64 restatement of
tests/quality_ref.py, on SceneRestorer output against the tensor-program path, its memory use, and test.py --quality fused end to end.
The bars are those of tests/test_quality_emu.py (quality_ref.tol: 7.8e-11 at 1000 x 700)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import model_checks as M
import quality_ref as Q
from golden.cases import TINY_CFG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = [(31, 1000, 700), (100, 307, 1280)]          # the shapes of tests/test_scene_gpu.py
PSNR_FACTOR = 10.0 / math.log(10.0)


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


@pytest.mark.parametrize("C,H,W", SCENES)
def test_scene_sizes_match_the_definition(C, H, W):
    """noise reaching outside [0,1] on one half of the scene, a smooth cube on the other; two rows without a spectrum; the reference
    (scipy's uniform_filter over the whole cube: seconds of host time) is evaluated once per shape"""
    from mp_hsir_amd import ops
    r, c = Q.noisy_pair(1, C, H, W, seed=C)
    rs, cs = Q.smooth_pair(1, C, H, W // 2, seed=C + 1)
    r[..., :W // 2], c[..., :W // 2] = rs, cs
    r[0, :, 5:7, :] = 0
    rd, cd = torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda()
    p, s, a, n = (t.cpu().numpy() for t in ops.quality_bands(rd, cd))
    p2, s2, a2, n2 = (t.cpu().numpy() for t in ops.quality_bands(rd, cd))
    assert p.tobytes() == p2.tobytes() and s.tobytes() == s2.tobytes() and a.tobytes() == a2.tobytes() and np.array_equal(n, n2), "not reproducible"
    mse, psnr, ssim = Q.bands(r, c)
    sam, pixels = Q.sam_half_angle(r, c)
    bar = Q.tol(H, W)
    d_ssim, d_psnr = np.abs(s - ssim).max(), np.abs(p - psnr).max()
    d_mse = (np.abs(10.0 ** (-p / 10.0) - mse) / mse).max()
    d_sam = np.abs(a - sam).max()
    print("%s: ssim %.3f..%.3f  |d ssim| %.3g  |d mse|/mse %.3g (bar %.3g)  |d psnr| %.3g (bar %.3g)  sam %.4g deg over %d pixels  |d sam| %.3g (bar %.3g)"
          % ((C, H, W), ssim.min(), ssim.max(), d_ssim, d_mse, bar, d_psnr, PSNR_FACTOR * bar, sam[0], n[0], d_sam, Q.SAM_TOL_DEG))
    assert d_ssim <= bar and d_psnr <= PSNR_FACTOR * bar and d_mse <= bar + 1e-14
    assert n.tolist() == [(H - 2) * W] and np.array_equal(n, pixels)
    assert d_sam <= Q.SAM_TOL_DEG


def test_identical_and_poisoned_scenes():
    from mp_hsir_amd import ops
    _, c = Q.noisy_pair(1, 31, 300, 333, seed=3)
    cd = torch.from_numpy(c).cuda()
    p, s, a, n = ops.quality_bands(cd, cd)
    assert torch.isposinf(p).all() and float((s - 1).abs().max()) <= 1e-12 and a.tolist() == [0.0] and n.tolist() == [300 * 333]
    r = torch.from_numpy(Q.noisy_pair(1, 31, 300, 333, seed=4)[0]).cuda()
    p0, s0, a0, _ = ops.quality_bands(r, cd)
    r[0, 7, 150, 200] = float("nan")
    p1, s1, a1, _ = ops.quality_bands(r, cd)
    keep = torch.ones(31, dtype=torch.bool, device="cuda")
    keep[7] = False
    assert torch.isnan(p1[0, 7]) and torch.isnan(s1[0, 7]) and torch.isnan(a1[0])
    assert torch.equal(p1[0, keep], p0[0, keep]) and torch.equal(s1[0, keep], s0[0, keep])


def test_restorer_output_scores_the_same_on_both_paths():
    """the tiny network's restoration of a 150 x 200 scene through SceneRestorer: compute_quality == compute_psnr_ssim at the same bar"""
    from mp_hsir_amd import metrics
    from mp_hsir_amd.scene import SceneRestorer
    net = M.build_net(TINY_CFG, "cuda", torch.float32)
    C, H, W = TINY_CFG["in_channel"], 150, 200
    g = torch.Generator().manual_seed(11)
    clean = torch.rand((C, H, W), generator=g)
    noisy = (clean + torch.randn((C, H, W), generator=g) * (30.0 / 255.0)).cuda()
    clean = clean.cuda()
    restored = SceneRestorer(net, tile=64, overlap=16, tile_batch=4, graphed=False)(noisy, 0)
    assert restored.shape == clean.shape and torch.isfinite(restored).all()
    q = metrics.compute_quality(restored[None], clean[None])
    p, s, cnt = metrics.compute_psnr_ssim(restored[None], clean[None])
    bar = Q.tol(H, W)
    print("restorer output: psnr %.6f / %.6f (|d| %.3g, bar %.3g)  ssim %.8f / %.8f (|d| %.3g, bar %.3g)  sam %.4f deg"
          % (q["psnr"], p, abs(q["psnr"] - p), PSNR_FACTOR * bar, q["ssim"], s, abs(q["ssim"] - s), bar, q["sam"]))
    assert q["count"] == cnt == 1 and abs(q["psnr"] - p) <= PSNR_FACTOR * bar and abs(q["ssim"] - s) <= bar
    assert 0.0 < q["sam"] < 90.0


def test_no_cube_sized_temporary():
    """around one call on a 31 x 1024 x 1024 pair the peak of allocated memory rises by less than ONE input cube (the tensor-program
    path needs four for its two float64 copies alone); the fused path allocates its outputs and the workspace, 16 (C + 1) bytes per block"""
    from mp_hsir_amd import ops
    B, C, H, W = 1, 31, 1024, 1024
    r = torch.rand((B, C, H, W), device="cuda")
    c = torch.rand((B, C, H, W), device="cuda")
    ops.quality_bands(r, c)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.quality_bands(r, c)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak memory rise of one quality_bands call: %d bytes (one cube: %d)" % (rise, r.numel() * 4))
    assert rise < r.numel() * 4
    assert torch.isfinite(out[0]).all()


def _test_py(args):
    cmd = ["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "test.py")] + args
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _scores(out, fused):
    """[(psnr, ssim)] as printed: the per-cube lines, then the summary line"""
    tail = r" sam (-?[\d.]+)$" if fused else "$"
    cubes = [m.groups() for m in (re.match(r"^\S+ psnr (-?[\d.]+|inf|nan) ssim (-?[\d.]+|nan)" + tail, ln) for ln in out.splitlines()) if m]
    tail = r", sam: (-?[\d.]+)$" if fused else "$"
    summary = [m.groups() for m in (re.search(r": psnr: (-?[\d.]+|inf|nan), ssim: (-?[\d.]+|nan)" + tail, ln) for ln in out.splitlines()) if m]
    assert len(summary) == 1, out
    return cubes + summary


def test_test_py_quality_fused_prints_the_same_scores_and_a_sam_column(tmp_path):
    """test.py --quality fused against --quality torch of the same command (same seed: the same degraded cubes), modes 0 and 10, with
    --tile 256 and without: psnr / ssim equal to the printed digits (one unit of the last digit allowed), and a sam field is there.
    Eight fresh child processes, each under its own timeout, running side by side."""
    configs = [(mode, tile) for mode in ("0", "10") for tile in (["--tile", "256"], [])]
    procs = {}
    for mode, tile in configs:
        for quality in ("torch", "fused"):
            args = ["--mode", mode, "--size", "320", "--cubes", "2", "--allow_surrogate_clip", "1", "--quality", quality] + tile
            procs[(mode, bool(tile), quality)] = _test_py(args)
    outs = {}
    for k, pr in procs.items():
        o, e = pr.communicate()
        assert pr.returncode == 0, "%s: %s %s" % (k, o[-2000:], e[-4000:])
        outs[k] = o
    for mode, tile in configs:
        t, f = _scores(outs[(mode, bool(tile), "torch")], False), _scores(outs[(mode, bool(tile), "fused")], True)
        print("mode %s tile %s: torch %s | fused %s" % (mode, bool(tile), t, f))
        assert len(t) == len(f) == 3, (outs[(mode, bool(tile), "torch")], outs[(mode, bool(tile), "fused")])
        for a, b in zip(t, f):
            assert abs(float(a[0]) - float(b[0])) <= 0.01 + 1e-9 and abs(float(a[1]) - float(b[1])) <= 0.0001 + 1e-9, (a, b)
            assert 0.0 <= float(b[2]) < 90.0
        assert " sam " not in outs[(mode, bool(tile), "torch")] and "sam:" not in outs[(mode, bool(tile), "torch")]
