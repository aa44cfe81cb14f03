"""TEST INFRASTRUCTURE for the SSIM term of the training loss (mphsir_ssim_loss, the ssim_loss kernels of mp-hsir_amd/csrc/arena.hip;
ops.ssim_loss, engine.SpectralLoss(ssim=)): the float64 numpy restatement of the definition in include/mphsir.h and the checks,
parametrised by device and run under tests/guard.py (guard bands, NaN-prefilled outputs, inputs compared bitwise afterwards).
tests/test_ssim_loss_emu.py runs them through the CPU-emulated build, tests/test_ssim_loss_gpu.py on the GPU.

Bars.
  SSIM and the loss: every sum is float64 in the kernel and in the restatement, only the order of the additions differs (far below an
    fp32 ulp), then one rounding to fp32: 2 fp32 ulps.
  gradient, element-wise, no element left out (SSIM has no kinks, and the clamp mask is decided on the fp32 y both sides read):
    |g - g64| <= 8 ulp32(mag_p),  mag_p = |g_base,p| + w / (49 B C Nw) sum over w holding p of (|d_w| + |b_w| |x_p - ux_w| + |c_w| |c_p - uy_w|)
    -- one fp32 rounding of the term, one fp32 addition onto the base: about 2 ulps of that magnitude; 8 is the spectral-loss bar.
    Measured worst: DESIGN.md §5.
The weight crosses the C ABI as fp32, so the restatement starts from the fp32 value."""
import ctypes
import math

import numpy as np
import torch

import guard
from optim_ex_ref import as_f32, f64
from spectral_loss_ref import ConvNet, batch, make_engine, put, run_engine  # noqa: F401  (the tests reach them through this module)
from util import bits, ulp32  # noqa: F401

C1, C2, COV, NWIN = 1e-4, 9e-4, 49.0 / 48.0, 49.0
T = (16, 32)                        # the tile of ssim_loss_kernel (rows, columns)
# one window; one window row; every pixel's window set clipped on both sides; extents of T + 1 and T + 6 / T + 7 in rows and in columns;
# several tiles with an odd width; the natural-scene band count at a 16-byte multiple
SHAPES = [(2, 3, 7, 7), (1, 1, 7, 20), (2, 3, 13, 13), (1, 2, 17, 39), (1, 2, 22, 33), (1, 2, 23, 38), (1, 3, 45, 70), (2, 31, 16, 16)]
SHAPE_GPU = (4, 31, 64, 64)         # GPU only: the training patch, eight tiles an image
FAMILIES = ("noise", "smooth", "flat", "dark")
W_SSIM = 0.2


def make_inputs(shape, family="noise", seed=0):
    """(y, c) CPU masters.  noise: c uniform, y = c + 0.3 N(0, 1): both clamp sides occur; smooth: a ramp from 0.2 to 0.8 plus 0.01 N;
    flat: 0.5 plus 0.002 N; dark: c <= 0.004, y = c + 0.001 N.  smooth and flat look like well-restored images: where an uncentred or
    fp32 sum loses digits"""
    g = torch.Generator().manual_seed(8100 + seed + sum(shape) + 17 * FAMILIES.index(family))
    B, C, H, W = shape
    n = lambda: torch.randn(shape, generator=g)         # noqa: E731
    if family == "noise":
        c = torch.rand(shape, generator=g)
        return c + 0.3 * n(), c
    if family == "smooth":
        ramp = torch.linspace(0.2, 0.8, H * W).view(1, 1, H, W).expand(shape)
        c = ramp + 0.01 * n()
        return c + 0.01 * n(), c.contiguous()
    if family == "flat":
        return 0.5 + 0.002 * n(), 0.5 + 0.002 * n()
    c = 0.004 * torch.rand(shape, generator=g)
    return c + 0.001 * n(), c


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _win(a):
    """7 x 7 window sums: (B,C,H,W) -> (B,C,H-6,W-6)"""
    return np.lib.stride_tricks.sliding_window_view(a, (7, 7), axis=(2, 3)).sum((-1, -2))


def _shifted(m, i, j, H, W):
    """for every pixel p the entry of window map m (B,C,H-6,W-6) of the window whose top-left corner is p - (i, j); 0 where there is none"""
    P = np.pad(m, ((0, 0), (0, 0), (6, 6), (6, 6)))
    return P[:, :, 6 - i:6 - i + H, 6 - j:6 - j + W]


def reference(y, c, w, g_base=None, base=None):
    """float64, from the definition: -> dict(ssim, loss, g, mag); g = g_base - w d SSIM / d y, loss = base + w (1 - SSIM)"""
    w = as_f32(w)
    y, c = f64(y), f64(c)
    B, C, H, W = y.shape
    n = B * C * (H - 6) * (W - 6)
    with np.errstate(all="ignore"):
        x = np.where(y < 0, 0.0, np.where(y > 1, 1.0, y))
        m = ((y >= 0) & (y <= 1)).astype(np.float64)
        ux, uy = _win(x) / NWIN, _win(c) / NWIN
        vx, vy, vxy = COV * (_win(x * x) / NWIN - ux * ux), COV * (_win(c * c) / NWIN - uy * uy), COV * (_win(x * c) / NWIN - ux * uy)
        A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux * ux + uy * uy + C1, vx + vy + C2
        S = A1 * A2 / (B1 * B2)
        ssim = S.sum() / n
        bw, cw = -2 * COV * S / B2, 2 * COV * A1 / (B1 * B2)
        dw = 2 * uy * A2 / (B1 * B2) - 2 * ux * S / B1
        acc, mag = np.zeros_like(y), np.zeros_like(y)
        has = np.ones_like(S)
        for i in range(7):
            for j in range(7):
                sh = lambda q: _shifted(q, i, j, H, W)      # noqa: E731
                h = sh(has)
                dx, dc = (x - sh(ux)) * h, (c - sh(uy)) * h
                acc += sh(dw) + sh(bw) * dx + sh(cw) * dc
                mag += np.abs(sh(dw)) + np.abs(sh(bw)) * np.abs(dx) + np.abs(sh(cw)) * np.abs(dc)
        scale = w / (NWIN * n)
        g_ssim = -scale * m * acc
    gb = np.zeros_like(y) if g_base is None else f64(g_base)
    b0 = 0.0 if base is None else float(base)
    return dict(ssim=ssim, loss=b0 + w * (1.0 - ssim), g=gb + g_ssim, g_ssim=g_ssim, mag=np.abs(gb) + scale * mag)


def torch_ssim(y, c):
    """the same SSIM as a float64 torch composite (five avg_pool2d passes): autograd through it is the independent check of the closed form"""
    import torch.nn.functional as F
    x = torch.clamp(y, 0, 1)
    pool = lambda t: F.avg_pool2d(t, 7, 1)            # noqa: E731
    ux, uy = pool(x), pool(c)
    vx, vy, vxy = COV * (pool(x * x) - ux * ux), COV * (pool(c * c) - uy * uy), COV * (pool(x * c) - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.mean()


def torch_loss(y, c, sam, sdiff, ssim):
    """base loss (L1 [+ spectral terms]) + ssim (1 - SSIM) in float64 torch, for the host test"""
    import spectral_loss_ref as SL
    import torch.nn.functional as F
    base = SL.torch_loss(y, c, sam, sdiff) if (sam > 0 or sdiff > 0) else F.l1_loss(torch.clamp(y, 0, 1), c)
    return base + as_f32(ssim) * (1.0 - torch_ssim(y, c))


def check_restatement(shape, family):
    """the closed form against float64 autograd through the composite, and its SSIM against metrics.ssim_bands: 1e-12 relative"""
    from mp_hsir_amd import metrics
    y, c = make_inputs(shape, family)
    ref = reference(y, c, 1.0)
    yt = y.double().requires_grad_(True)
    s = torch_ssim(yt, c.double())
    (1.0 - s).backward()
    ga = f64(yt.grad)
    err_s, err_g = abs(float(s.detach()) - ref["ssim"]), float(np.abs(ga - ref["g"]).max())
    bands = float(metrics.ssim_bands(y.double(), c.double()).mean())
    print("%s %s: restatement vs float64 autograd: SSIM %.3g, gradient %.3g absolute (max |g| %.3g); vs metrics.ssim_bands %.3g"
          % (shape, family, err_s, err_g, float(np.abs(ga).max()), abs(bands - ref["ssim"])))
    assert err_s <= 1e-12 * abs(ref["ssim"]) and err_g <= 1e-12 * float(np.abs(ga).max())
    assert abs(bands - ref["ssim"]) <= 1e-12 * abs(ref["ssim"])


# ---- kernel checks --------------------------------------------------------------------------------------------------------------------------
def assert_within_bars(out, g, ref, what):
    """bars of the module docstring; -> the worst gradient error in ulps of the magnitude"""
    got = [float(v) for v in out.detach().cpu().tolist()]
    for name, val in zip(("loss", "ssim"), got):
        want = ref[name]
        print("%s %s: %.9g want %.9g (%.2f ulp, bar 2)" % (what, name, val, want, abs(val - want) / float(ulp32(want))))
        assert math.isfinite(val) and abs(val - want) <= 2 * float(ulp32(want)), (what, name, val, want)
    if g is None:
        return 0.0
    gg = f64(g)
    assert np.isfinite(gg).all(), what
    err = np.abs(gg - ref["g"])
    unit = ulp32(ref["mag"])
    worst = float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0
    print("%s gradient: worst %.3f ulp of the magnitude (bar 8), max |g| %.3g" % (what, worst, float(np.abs(ref["g"]).max())))
    assert worst <= 8.0 and bool((err[unit == 0] == 0).all()), (what, worst)
    return worst


@guard.guarded
def check_values(dev, shape, family="noise", offset=False):
    """SSIM, loss and gradient against the restatement: the term alone; on a base (accumulate onto a base gradient, base_loss set), which is
    bitwise base + the term alone; without a gradient; the autograd form"""
    from mp_hsir_amd import ops
    ym, cm = make_inputs(shape, family)
    y, c = put(ym, dev, 1, offset), put(cm, dev, 2, offset)
    what = "%s %s%s" % (shape, family, " offset" if offset else "")
    loss, g, out = ops.ssim_loss_grad(y, c, W_SSIM)
    assert g.shape == y.shape and g.dtype == torch.float32 and bits(loss) == bits(out[0]) and out.shape == (2,)
    worst = assert_within_bars(out, g, reference(ym, cm, W_SSIM), what)
    # on a base, as the engine does it: the L1 loss and its gradient (l1_clamp_loss asks for 16-byte alignment: the spectral pair otherwise)
    lb, gb = ops.spectral_loss_grad(y, c, 0.1, 0.3)[:2] if offset else ops.l1_clamp_loss_grad(y, c)
    gb0 = gb.clone()
    loss2, g2, out2 = ops.ssim_loss_grad(y, c, W_SSIM, base_loss=lb.reshape(1), grad=gb)
    assert g2 is gb and bits(g2) == bits(gb0 + g), "accumulate is one fp32 addition onto the base gradient"
    assert bits(out2[1]) == bits(out[1])
    worst = max(worst, assert_within_bars(out2, g2, reference(ym, cm, W_SSIM, g_base=gb0, base=float(lb)), what + " on a base"))
    # the value alone (grad = NULL) and the autograd form
    with torch.no_grad():
        assert bits(ops.ssim_loss(y, c, W_SSIM)) == bits(loss)
    out_v, g_v = ops._ssim_loss_launch(y, c, W_SSIM, None, None, False)
    assert g_v is None and bits(out_v) == bits(out), "grad == NULL gives bitwise the same {loss, SSIM}"
    out_b, _ = ops._ssim_loss_launch(y, c, W_SSIM, lb.reshape(1), None, False)
    assert bits(out_b) == bits(out2), "and the same on a base"
    ya = y.detach().clone().requires_grad_(True)
    la = ops.ssim_loss(ya, c, W_SSIM)
    la.backward()
    assert bits(la) == bits(loss) and bits(ya.grad) == bits(g)
    return worst


@guard.guarded
def check_reproducible_and_alignment(dev, shape=(2, 31, 16, 16)):
    """two runs give the same bits, and so does the same cube one element past a 16-byte boundary (one path for every alignment)"""
    from mp_hsir_amd import ops
    ym, cm = make_inputs(shape)
    y, c = put(ym, dev, 1), put(cm, dev, 2)
    a, b = ops.ssim_loss_grad(y, c, W_SSIM), ops.ssim_loss_grad(y, c, W_SSIM)
    assert bits(a[2]) == bits(b[2]) and bits(a[1]) == bits(b[1])
    o = ops.ssim_loss_grad(put(ym, dev, 3, offset=True), put(cm, dev, 4, offset=True), W_SSIM)
    assert bits(a[2]) == bits(o[2]) and bits(a[1]) == bits(o[1])


@guard.guarded
def check_quality_agrees(dev, shape):
    """out[1] against the SSIM ops.quality_bands reports, averaged over bands and images in float64: 2 fp32 ulps"""
    from mp_hsir_amd import ops
    ym, cm = make_inputs(shape, "smooth")
    y, c = put(ym, dev, 1), put(cm, dev, 2)
    out = ops.ssim_loss_grad(y, c, W_SSIM)[2]
    want = float(ops.quality_bands(y, c)[1].double().mean())
    print("%s: SSIM %.9g, quality_bands %.9g" % (shape, float(out[1]), want))
    assert abs(float(out[1]) - want) <= 2 * float(ulp32(want))


@guard.guarded
def check_edges(dev):
    from mp_hsir_amd import ops
    shape = (2, 3, 9, 12)
    ym, cm = make_inputs(shape, seed=11)
    # y == c (inside [0, 1]): SSIM within 2 ulp of 1, the gradient within its bar (it need not be exactly 0)
    loss, g, out = ops.ssim_loss_grad(put(cm, dev, 1), put(cm, dev, 2), W_SSIM)
    assert_within_bars(out, g, reference(cm, cm, W_SSIM), "y == c")
    assert abs(float(out[1]) - 1.0) <= 2 * float(ulp32(1.0))
    # all-zero planes: every denominator is C1 C2, S = 1
    z = torch.zeros(shape)
    loss, g, out = ops.ssim_loss_grad(put(z, dev, 3), put(z, dev, 4), W_SSIM)
    assert_within_bars(out, g, reference(z, z, W_SSIM), "all zero")
    # y all outside [0, 1]: the gradient is exactly 0
    yo = torch.where(ym > 0.5, ym + 1.0, ym - 1.0)
    loss, g, out = ops.ssim_loss_grad(put(yo, dev, 5), put(cm, dev, 6), W_SSIM)
    assert bool(((yo < 0) | (yo > 1)).all()) and bool((g == 0).all())
    assert_within_bars(out, g, reference(yo, cm, W_SSIM), "y outside [0, 1]")
    # y at exactly 0 and 1 passes gradient; +-inf clamps like any value outside and gets 0
    ye = ym.clone()
    ye[1, 0, 4, 4], ye[1, 1, 4, 4], ye[1, 2, 4, 5], ye[1, 2, 4, 6] = 0.0, 1.0, float("inf"), float("-inf")
    loss, g, out = ops.ssim_loss_grad(put(ye, dev, 7), put(cm, dev, 8), W_SSIM)
    assert_within_bars(out, g, reference(ye, cm, W_SSIM), "bounds and infinities")
    gc = g.cpu()
    assert float(gc[1, 0, 4, 4]) != 0.0 and float(gc[1, 1, 4, 4]) != 0.0 and float(gc[1, 2, 4, 5]) == 0.0 and float(gc[1, 2, 4, 6]) == 0.0
    # a NaN in y, a NaN in c: both outputs NaN; planes without it keep their gradient bits
    clean_run = ops.ssim_loss_grad(put(ym, dev, 9), put(cm, dev, 10), W_SSIM)[1].cpu()
    for which in (0, 1):
        yn, cn = ym.clone(), cm.clone()
        (yn, cn)[which][1, 2, 3, 5] = float("nan")
        loss, g, out = ops.ssim_loss_grad(put(yn, dev, 11 + which), put(cn, dev, 13 + which), W_SSIM)
        assert math.isnan(float(out[0])) and math.isnan(float(out[1])) and math.isnan(float(loss))
        gc = g.cpu()
        assert torch.equal(gc[0], clean_run[0]) and torch.equal(gc[1, :2], clean_run[1, :2])


@guard.guarded
def check_refusals(dev):
    """an error (EINVAL, a message that names the cause), nothing launched: ops.ACCOUNT stays empty and no output loses its poison"""
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    lib = L.load()
    shape = (2, 3, 9, 40)
    ym, cm = make_inputs(shape)
    y, c = put(ym, dev, 1), put(cm, dev, 2)
    need = lib.mphsir_ssim_loss_workspace_bytes(*shape)
    assert need == 8 * 2 * 2 and lib.mphsir_ssim_loss_workspace_bytes(32, 31, 64, 64) == 8 * 32 * 8
    for bad in ((2, 0, 9, 40), (0, 3, 9, 40), (2, 3, 6, 40), (2, 3, 9, 6), (1, 1, 65536, 32768)):
        assert lib.mphsir_ssim_loss_workspace_bytes(*bad) < 0, bad
    g = torch.full(shape, -7.0, device=dev)
    base = torch.full((1,), 0.25, device=dev)
    out, ws = torch.full((2,), -7.0, device=dev), torch.full((need // 8,), -7.0, dtype=torch.float64, device=dev)
    keep = [bits(t) for t in (g, out, ws)]
    stream = ops._stream(y)

    def args(**kw):
        a = L.SsimLossArgs(y=y.data_ptr(), clean=c.data_ptr(), grad=g.data_ptr(), base_loss=base.data_ptr(), out=out.data_ptr(),
                           workspace=ws.data_ptr(), workspace_bytes=need, B=shape[0], C=shape[1], H=shape[2], W=shape[3], w_ssim=W_SSIM, accumulate=0)
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def refused(a, text):
        assert lib.mphsir_ssim_loss(ctypes.byref(a), stream) == -1, text
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()

    ops.ACCOUNT = {}
    try:
        refused(args(struct_size=ctypes.sizeof(L.SsimLossArgs) - 8), "struct_size")
        refused(args(struct_size=ctypes.sizeof(L.SsimLossArgs) + 8), "struct_size")
        for name in ("y", "clean", "out", "workspace"):
            refused(args(**{name: None}), "null pointer")
        refused(args(H=6), "no 7 x 7 window")
        refused(args(W=6), "no 7 x 7 window")
        refused(args(C=0), "bad sizes")
        refused(args(B=0), "bad sizes")
        refused(args(B=2 ** 31 - 1), "bad sizes")                       # too many workgroups
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            refused(args(w_ssim=bad), "weight")
        refused(args(workspace_bytes=need - 1), "workspace")
        refused(args(workspace=ws.data_ptr() + 4, workspace_bytes=need + 8), "workspace")
        refused(args(accumulate=2), "accumulate")
        refused(args(accumulate=1, grad=None), "accumulate")
        for call in (lambda: ops.ssim_loss_grad(y, c, 0.0), lambda: ops.ssim_loss_grad(y, c, -1.0), lambda: ops.ssim_loss_grad(y, c, float("nan")),
                     lambda: ops.ssim_loss_grad(y.double(), c.double(), W_SSIM), lambda: ops.ssim_loss_grad(y, c[:1], W_SSIM),
                     lambda: ops.ssim_loss_grad(y[0], c[0], W_SSIM), lambda: ops.ssim_loss_grad(y[..., :6], c[..., :6], W_SSIM),
                     lambda: ops.ssim_loss_grad(y, c, W_SSIM, grad=g[:1]), lambda: ops.ssim_loss(y, c, 0.0)):
            try:
                call()
            except (RuntimeError, AssertionError):
                pass
            else:
                raise AssertionError("a wrapper accepted what the entry point refuses")
        assert not ops.ACCOUNT, ("launched before refusing", sorted(ops.ACCOUNT))
        assert [bits(t) for t in (g, out, ws)] == keep, "something was launched"
        assert lib.mphsir_ssim_loss(ctypes.byref(args()), stream) == 0                    # the same arguments, nothing wrong: it runs
        assert_within_bars(out, g, reference(ym, cm, W_SSIM, base=0.25), "after the refusals")
        assert lib.mphsir_ssim_loss(ctypes.byref(args(grad=None, base_loss=None)), stream) == 0     # both optional
        assert_within_bars(out, None, reference(ym, cm, W_SSIM), "value alone")
    finally:
        ops.ACCOUNT = None


# ---- engine checks (the engines of tests/spectral_loss_ref.py: "tiny" on the GPU, "conv" through the emulator) ------------------------------
LOSSES = [dict(ssim=0.2), dict(sam=0.1, sdiff=0.1, ssim=0.2)]


def check_engine_eager_vs_graph(dev, kw, kind="tiny", dtype=torch.float32):
    """three steps eager and in graph mode: bitwise-equal losses, gradient arenas and parameters; loss_components() reads the replayed buffers"""
    from mp_hsir_amd.engine import SpectralLoss
    e0, l0, p0, _ = run_engine(dev, kind, 3, False, dtype, loss_fn=SpectralLoss(**kw))
    e1, l1, p1, _ = run_engine(dev, kind, 3, True, dtype, loss_fn=SpectralLoss(**kw))
    assert e1.captured and not e0.captured, "the graph-mode engine never captured"
    print("losses eager %s graph %s; parameters equal: %s" % ([float(a) for a in l0], [float(b) for b in l1], p0 == p1))
    lc = e1.loss_components()
    assert lc["loss"] == float(l1[-1]) and -1.0 < lc["ssim"] < 1.0 and lc == e0.loss_components()
    assert [bits(a) for a in l0] == [bits(b) for b in l1] and e0.g_bits == e1.g_bits and p0 == p1


def check_engine_loss_and_components(dev, kw, kind="tiny", dtype=torch.float32):
    """the loss a step returns is the SSIM kernel's out[0] on the same `restored` and base; loss_components() is consistent with it"""
    from mp_hsir_amd import ops
    from mp_hsir_amd.engine import SpectralLoss
    fn = SpectralLoss(**kw)
    net, eng = make_engine(dev, kind, False, dtype, loss_fn=fn)
    assert eng.loss_components() is None and eng._eager_hyper
    x, c, task = batch(0, dev, kind)
    with torch.no_grad():
        restored = net(x, task).float()
    if fn.spectral:
        lb, gb, _ = ops.spectral_loss_grad(restored, c, fn.sam, fn.sdiff)
    else:
        lb, gb = ops.l1_clamp_loss_grad(restored, c)
    want = ops.ssim_loss_grad(restored, c, fn.ssim, base_loss=lb.reshape(1), grad=gb)
    ops.ACCOUNT = {}
    try:
        got = eng.train_step(x, c, task)
        acct = {k: v[0] for k, v in ops.ACCOUNT.items()}
    finally:
        ops.ACCOUNT = None
    assert acct["ssim_loss"] == 1 and acct.get("spectral_loss", 0) == int(fn.spectral) and acct.get("l1_clamp_loss", 0) == int(not fn.spectral), acct
    assert bits(got) == bits(want[0])
    lc = eng.loss_components()
    assert lc["loss"] == float(got) and lc["ssim"] == float(want[2][1]) and -1.0 < lc["ssim"] < 1.0
    assert sorted(lc) == ["l1", "loss", "sam_deg", "sdiff", "ssim"] and lc["l1"] > 0
    assert (lc["sam_deg"] > 0 and lc["sdiff"] > 0) if fn.spectral else (lc["sam_deg"] == 0 and lc["sdiff"] == 0)
    total = lc["l1"] + as_f32(fn.sam) * math.radians(lc["sam_deg"]) + as_f32(fn.sdiff) * lc["sdiff"] + as_f32(fn.ssim) * (1.0 - lc["ssim"])
    assert abs(lc["loss"] - total) <= 4 * float(ulp32(lc["loss"])), (lc, total)
    # the loss_fn as a plain callable (another caller's autograd): the same value within the fp32 addition that joins the two terms
    assert abs(float(fn(restored, c)) - float(got)) <= 2 * float(ulp32(float(got)))


def check_engine_without_the_term(dev, kind="tiny"):
    """ssim = 0: no ssim_loss launch, the launch list and the parameters of SpectralLoss(0.1, 0.3) as ever; _loss_parts stays fp32[4]"""
    from mp_hsir_amd.engine import SpectralLoss
    e0, _, p0, a0 = run_engine(dev, kind, 2, account=True, loss_fn=SpectralLoss(0.1, 0.3))
    e1, _, p1, a1 = run_engine(dev, kind, 2, account=True, loss_fn=SpectralLoss(0.1, 0.3, 0.0))
    e2, _, p2, a2 = run_engine(dev, kind, 2, account=True)
    assert a0 == a1 and p0 == p1 and "ssim_loss" not in a0 and "ssim_loss" not in a2 and e2.loss_components() is None
    assert e1._loss_parts.shape == (4,) and e1._ssim_parts is None and sorted(e1.loss_components()) == ["l1", "loss", "sam_deg", "sdiff"]
    e3, _, p3, a3 = run_engine(dev, kind, 2, account=True, loss_fn=SpectralLoss(0.1, 0.3, 0.2))
    rest = dict(a3)
    assert rest.pop("ssim_loss") == 1 and rest == a0 and p3 != p0, "with the term on the list gains the one ssim_loss entry and nothing else"


def check_engine_fp16_scaler(dev, kind="tiny"):
    """the fp16 path: the summed gradient goes through the loss scale, the optimizer divides it out; parameters stay finite and move"""
    from mp_hsir_amd.engine import SpectralLoss
    kw = dict(loss_scaling=True) if kind == "conv" else {}
    net, eng = make_engine(dev, kind, False, torch.float16 if kind != "conv" else torch.float32, loss_fn=SpectralLoss(ssim=0.2), init_scale=1024.0, **kw)
    for s in range(3):
        loss = eng.train_step(*batch(s, dev, kind))
        if s == 0:
            start = eng.flat_p.clone()
    assert eng.scaler is not None and float(eng.scaler[3]) >= 2.0, "the scaler counted optimizer steps"
    assert bool(torch.isfinite(eng.flat_p).all()) and math.isfinite(float(loss)) and not torch.equal(start, eng.flat_p)
    assert -1.0 < eng.loss_components()["ssim"] < 1.0
