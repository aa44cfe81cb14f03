"""TEST INFRASTRUCTURE: the quality meter (mp-hsir_amd/csrc/quality_meter.hip, ops.quality_meter) against a numpy float64 restatement.

The meter only adds float64 values in a fixed order and divides once per image: IEEE add and divide are correctly rounded on the GPU,
in the emulated build and in numpy alike, and no transcendental function is involved, so every comparison here is BITWISE -- no
tolerance.  The checks run on the device they are given: the emulated build (tests/test_quality_meter_emu.py) or an MI355X
(tests/test_validate_gpu.py), under tests/guard.py's guard bands."""
import ctypes

import numpy as np
import torch

import guard
from util import bits  # noqa: F401  (the tests reach it through this module)

SHAPES = [(1, 1), (3, 8), (5, 31), (64, 100)]        # (B, C): one value; fewer images than a wave; the natural-scene bands; B * C = 6400
USES = ["null", "ones", "random", "zero_row"]
INIT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, 0.0])


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def meter_ref(row, psnr, ssim, sam, use=None, n=None, reset=False):
    """the row after one launch: per image the sum over its used bands in ascending band order divided by their number, images added in
    ascending order onto `row` (numpy float64 scalars: one rounding per add, as the kernel)"""
    r = INIT.copy() if reset else np.array(row, dtype=np.float64)
    B, C = psnr.shape
    for b in range(B if n is None else n):
        ap, as_, cnt = np.float64(0.0), np.float64(0.0), 0
        for c in range(C):
            if use is None or use[b, c]:
                ap, as_, cnt = ap + psnr[b, c], as_ + ssim[b, c], cnt + 1
        if cnt == 0:
            r[7] += 1.0
            continue
        with np.errstate(invalid="ignore"):
            ap, as_ = ap / np.float64(cnt), as_ / np.float64(cnt)
        if not (np.isfinite(ap) and np.isfinite(as_) and np.isfinite(sam[b])):
            r[4] += 1.0
            continue
        r[0] += 1.0
        r[1] += ap
        r[2] += as_
        r[3] += sam[b]
        r[5] = min(r[5], ap)
        r[6] = max(r[6], ap)
    return r


def make_values(B, C, seed=0):
    """per-band values of the magnitudes mphsir_quality writes: psnr 15..45 dB, ssim 0.2..1, sam 0.5..30 degrees"""
    g = np.random.default_rng(9100 + seed + 131 * B + C)
    return 15.0 + 30.0 * g.random((B, C)), 0.2 + 0.8 * g.random((B, C)), 0.5 + 29.5 * g.random(B), g.integers(1, 4096, B).astype(np.int64)


def make_use(kind, B, C, seed=0):
    if kind == "null":
        return None
    if kind == "ones":
        return np.ones((B, C), dtype=np.uint8)
    g = np.random.default_rng(9200 + seed + 131 * B + C)
    u = (g.random((B, C)) < 0.4).astype(np.uint8)
    if kind == "zero_row":
        u[B // 2] = 0                                 # an image without a used band
        if B > 1:
            u[0, 0] = 1
    return u


# ---- device plumbing: guarded inputs and tables while a guard is active ----------------------------------------------------------------------
def put(a, dev, seed=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    G = guard.active()
    if G is not None and G.device.type == torch.device(dev).type:
        return G.input(t, seed)
    return t.to(dev)


def new_table(rows, dev, fill=-7.0):
    G = guard.active()
    if G is not None and G.device.type == torch.device(dev).type:
        return G.alloc((rows, 8), torch.float64, dev, "output", fill=fill)
    return torch.full((rows, 8), fill, dtype=torch.float64).to(dev)


def launch(table, row, vals, use, dev, n=None, reset=False, seed=0):
    from mp_hsir_amd import ops
    p, s, a, px = vals
    return ops.quality_meter(table, row, put(p, dev, seed + 1), put(s, dev, seed + 2), put(a, dev, seed + 3), put(px, dev, seed + 4),
                             use=put(use, dev, seed + 5), n=n, reset=reset)


# ---- checks ---------------------------------------------------------------------------------------------------------------------------------
@guard.guarded
def check_values(dev, B, C, use_kind):
    """n over {1, B - 1, B} (and 0 where that is B - 1), with reset and onto a row that holds something; rows 0 and 2 of the table stay"""
    vals, use = make_values(B, C), make_use(use_kind, B, C)
    for n in sorted({1, B - 1, B}):
        table = new_table(3, dev)
        before = table.detach().cpu().numpy().copy()
        launch(table, 1, vals, use, dev, n=n, reset=True)
        want = meter_ref(None, *vals[:3], use=use, n=n, reset=True)
        got = table.detach().cpu().numpy().copy()
        assert bits(got[1]) == bits(want), (B, C, use_kind, n, got[1], want)
        assert bits(got[[0, 2]]) == bits(before[[0, 2]]), "reset / the update touched another row"
        more = make_values(B, C, seed=1)
        launch(table, 1, more, use, dev, n=n, reset=False, seed=10)                      # onto what the row holds
        want2 = meter_ref(want, *more[:3], use=use, n=n)
        got2 = table.detach().cpu().numpy().copy()
        assert bits(got2[1]) == bits(want2), (B, C, use_kind, n, got2[1], want2)
        assert bits(got2[[0, 2]]) == bits(before[[0, 2]])
        if use_kind == "zero_row" and n == B:
            assert got[1][7] >= 1.0, "the image without a used band was not counted as skipped"
        if n is not None and n >= 1 and use_kind in ("null", "ones"):
            assert got[1][0] == float(n) and got[1][4] == got[1][7] == 0.0 and got[1][5] <= got[1][1] / n <= got[1][6]


@guard.guarded
def check_split_invariance(dev, C=31):
    """the same 13 images in launches of (13), (4, 4, 4, 1) and (1, ..., 1): bitwise the same row, which is the restatement's"""
    N = 13
    p, s, a, px = make_values(N, C, seed=2)
    use = make_use("random", N, C, seed=2)
    use[5] = 0
    p[7, 3] = np.nan
    use[7, 3] = 1
    rows = []
    for sizes in ((13,), (4, 4, 4, 1), (1,) * 13):
        table = new_table(1, dev)
        i0 = 0
        for j, k in enumerate(sizes):
            B = max(sizes)                                                               # one buffer size per cut: the last batch is padded
            pad = lambda v: np.concatenate([v[i0:i0 + k], np.repeat(v[i0 + k - 1:i0 + k], B - k, axis=0)])       # noqa: E731
            launch(table, 0, (pad(p), pad(s), pad(a), pad(px)), pad(use), dev, n=k, reset=j == 0, seed=20 * j)
            i0 += k
        rows.append(bits(table))
    want = meter_ref(None, p, s, a, use=use, reset=True)
    assert rows[0] == rows[1] == rows[2] == bits(want), [np.frombuffer(r, dtype=np.float64) for r in rows] + [want]
    assert want[0] == 11.0 and want[4] == 1.0 and want[7] == 1.0


@guard.guarded
def check_reproducible(dev, B=64, C=100):
    vals, use = make_values(B, C, seed=3), make_use("random", B, C, seed=3)
    one, two = new_table(1, dev), new_table(1, dev)
    launch(one, 0, vals, use, dev, reset=True)
    launch(two, 0, vals, use, dev, reset=True, seed=10)
    assert bits(one) == bits(two)


@guard.guarded
def check_edges(dev):
    """image 0 clean; 1 a NaN psnr band; 2 a psnr band of +inf; 3 a NaN ssim; 4 a NaN sam; 5 a NaN and an inf in UNUSED bands only (scored);
    6 no used band (skipped, though its sam is NaN)"""
    B, C = 7, 8
    p, s, a, px = make_values(B, C, seed=4)
    use = np.ones((B, C), dtype=np.uint8)
    p[1, 2] = np.nan
    p[2, 7] = np.inf
    s[3, 0] = np.nan
    a[4] = np.nan
    use[5, 1] = use[5, 6] = 0
    p[5, 1], s[5, 6], p[5, 6] = np.nan, np.nan, np.inf
    use[6] = 0
    a[6] = np.nan
    table = new_table(1, dev)
    launch(table, 0, (p, s, a, px), use, dev, reset=True)
    got = table.detach().cpu().numpy()[0].copy()
    want = meter_ref(None, p, s, a, use=use, reset=True)
    assert bits(got) == bits(want), (got, want)
    assert got[0] == 2.0 and got[4] == 4.0 and got[7] == 1.0 and np.all(np.isfinite(got[:5]))
    m0, m5 = (meter_ref(None, p[i:i + 1], s[i:i + 1], a[i:i + 1], use=use[i:i + 1], reset=True)[1] for i in (0, 5))
    assert got[5] == min(m0, m5) and got[6] == max(m0, m5), "the unused bands of image 5 leaked into it, or the extremes are off"
    # use = NULL: every band counts, so image 5 is now non-finite and image 6 is judged by its NaN sam
    launch(table, 0, (p, s, a, px), None, dev, reset=True, seed=10)
    got = table.detach().cpu().numpy()[0].copy()
    assert bits(got) == bits(meter_ref(None, p, s, a, reset=True)) and got[0] == 1.0 and got[4] == 6.0 and got[7] == 0.0
    # nothing scored at all: the sums stay 0 and the extremes stay at +inf / -inf
    launch(table, 0, (p, s, a, px), np.zeros((B, C), dtype=np.uint8), dev, reset=True, seed=20)
    got = table.detach().cpu().numpy()[0].copy()
    assert bits(got) == bits(np.array([0, 0, 0, 0, 0, np.inf, -np.inf, 7.0])), got


@guard.guarded
def check_refusals(dev):
    """EINVAL and a message, nothing launched: the table and ops.ACCOUNT are unchanged"""
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    lib = L.load()
    B, C = 3, 8
    p, s, a, px = (put(v, dev, i) for i, v in enumerate(make_values(B, C, seed=5)))
    use = put(make_use("random", B, C, seed=5), dev, 9)
    table = new_table(2, dev)
    keep = bits(table)
    stream = ops._stream(table)

    def args(**kw):
        q = L.QualityMeterArgs(psnr=p.data_ptr(), ssim=s.data_ptr(), sam_deg=a.data_ptr(), sam_pixels=px.data_ptr(), use=use.data_ptr(),
                               table=table.data_ptr(), B=B, C=C, n=B, rows=2, row=1, reset=1)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def refused(q, text):
        assert lib.mphsir_quality_meter(ctypes.byref(q), stream) == -1, text
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()

    ops.ACCOUNT = {}
    try:
        refused(args(struct_size=ctypes.sizeof(L.QualityMeterArgs) - 8), "struct_size")
        refused(args(struct_size=ctypes.sizeof(L.QualityMeterArgs) + 8), "struct_size")
        for name in ("psnr", "ssim", "sam_deg", "sam_pixels", "table"):
            refused(args(**{name: None}), "null pointer")
        refused(args(n=B + 1), "outside [0, B")
        refused(args(n=-1), "outside [0, B")
        refused(args(row=2), "row 2 outside")
        refused(args(row=-1), "row -1 outside")
        refused(args(B=0, n=0), "bad sizes")
        refused(args(C=0), "bad sizes")
        refused(args(rows=0, row=0), "bad sizes")
        assert lib.mphsir_quality_meter(None, stream) == -1
        for call in (lambda: ops.quality_meter(table, 2, p, s, a, px), lambda: ops.quality_meter(table, 0, p, s, a, px, n=B + 1),
                     lambda: ops.quality_meter(table.float(), 0, p, s, a, px), lambda: ops.quality_meter(table, 0, p.float(), s.float(), a, px),
                     lambda: ops.quality_meter(table, 0, p, s[:, :4], a, px), lambda: ops.quality_meter(table, 0, p, s, a, px, use=use[:2]),
                     lambda: ops.quality_meter(table[:, :4], 0, p, s, a, px)):
            try:
                call()
            except (RuntimeError, AssertionError):
                pass
            else:
                raise AssertionError("the wrapper accepted what the entry point refuses")
        assert not ops.ACCOUNT, ("launched before refusing", sorted(ops.ACCOUNT))
        assert bits(table) == keep, "something was launched"
        assert lib.mphsir_quality_meter(ctypes.byref(args()), stream) == 0               # the same arguments, nothing wrong: it runs
        assert lib.mphsir_quality_meter(ctypes.byref(args(use=None, reset=0)), stream) == 0      # use is optional
    finally:
        ops.ACCOUNT = None
    got = table.detach().cpu().numpy().copy()
    hp, hs, ha, hu = (t.detach().cpu().numpy() for t in (p, s, a, use))
    want = meter_ref(meter_ref(None, hp, hs, ha, use=hu, reset=True), hp, hs, ha)
    assert bits(got[1]) == bits(want) and bits(got[0]) == keep[:64]
