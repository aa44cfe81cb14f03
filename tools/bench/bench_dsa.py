#!/usr/bin/env python3
"""The d_sa part of a PGSSTB attention backward per shape, replayed from a captured graph: the three launches
(combine_bwd with d_sa -> gemm_tok epi 1 -> win_attn_bwd) against the two (combine_bwd without d_sa -> win_attn_bwd branch=...).

    python tools/bench/bench_dsa.py            # C, heads, B, H, W of the table below; prints us per sequence and the head split

Shapes on both sides of the library's head split (one workgroup per window from 512 windows on): DESIGN.md section 5."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mp_hsir_amd import _lib, ops  # noqa: E402

SHAPES = [(256, 8, 32, 16, 16), (256, 8, 128, 16, 16), (256, 8, 256, 16, 16),
          (128, 4, 8, 32, 32), (128, 4, 16, 32, 32), (128, 4, 32, 32, 32),
          (128, 2, 32, 64, 64), (64, 2, 32, 64, 64)]


def replay_us(fn, n=40):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(5):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(3):
        a.record()
        for _ in range(n):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) * 1e3 / n
        best = t if best is None else min(best, t)
    return best


def main():
    dt = torch.bfloat16
    r = lambda *shape, **kw: torch.randn(*shape, device="cuda", dtype=kw.get("dtype", dt)) * kw.get("scale", 1.0)
    for C, heads, B, H, W in SHAPES:
        M = B * H * W
        x, dy, sa = r(B, H, W, C), r(B, H, W, C), r(B, H, W, C)
        gate, dmu = r(M // 64, C, dtype=torch.float32), r(M // 64, C, dtype=torch.float32)
        keep = torch.full((B,), 1.0 / 0.9, device="cuda")
        lnw, lnb = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        wqkv, bqkv = r(3 * C, C, scale=C ** -0.5), r(3 * C, dtype=torch.float32, scale=0.1)
        rpb, wprojT = r(225, heads, dtype=torch.float32, scale=0.2), r(C, C, scale=C ** -0.5)
        dt3, wsT = r(M, 3 * C), r(C, 3 * C, scale=(3 * C) ** -0.5)
        tail = (lnw, lnb, wqkv, bqkv, rpb, wprojT, heads, 4)

        def three():
            d_out, d_sa, _ = ops.combine_bwd(dy, sa, gate, keep, 4)
            d_sa = ops.gemm_tok(dt3, wsT, epi=1, res=d_sa.reshape(M, C)).reshape(B, H, W, C)
            ops.win_attn_bwd(x, d_sa, dmu, *tail)

        def two():
            d_out, _, _ = ops.combine_bwd(dy, sa, gate, keep, 4, want_dsa=False)
            ops.win_attn_bwd(x, None, dmu, *tail, branch=dict(dt3=dt3, wsT=wsT, d_out=d_out.reshape(M, C), gate=gate))

        hs = _lib.load().mphsir_win_attn_bwd_head_split(B, H, W, heads)
        t3, t2 = replay_us(three), replay_us(two)
        print("C=%3d heads=%d B=%3d %dx%d windows=%5d head_split=%d: three launches %7.1f us, two %7.1f us (%+.1f)" %
              (C, heads, B, H, W, M // 64, hs, t3, t2, t2 - t3), flush=True)


if __name__ == "__main__":
    main()
