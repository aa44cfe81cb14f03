"""TEST INFRASTRUCTURE for the training loss with spectral terms (mphsir_spectral_loss, mp-hsir_amd/csrc/spectral_loss.hip; ops.spectral_loss,
engine.SpectralLoss): the float64 numpy restatement of the definition in include/mphsir.h and the checks, parametrised by device and run
under tests/guard.py (guard bands, NaN-prefilled outputs, inputs compared bitwise afterwards).  tests/test_spectral_loss_emu.py runs them
through the CPU-emulated build, tests/test_spectral_loss_gpu.py on the GPU.

Bars.
  loss and components: every sum is float64 in the kernel and in the restatement, only the order of at most 2^24 additions differs
    (<= 2^24 2^-53 = 2e-9 relative, far below an fp32 ulp), then one rounding to fp32: 2 fp32 ulps.
  gradient, element-wise: |g - g64| <= 8 ulp32(|g_L1| + |g_SDIFF| + w_sam (|a c_k| + |b x_k|) / P) -- the kernel rounds the two SAM scalars
    and the constants of L1 and SDIFF to fp32 (half an ulp each), forms a c - b x in fp32 (two products, one difference) and joins the terms
    with two fp32 additions: about 4 ulps of that magnitude in the worst case, 8 leaves a factor of two.  Measured worst: DESIGN.md §5.
The weights cross the C ABI as fp32, so the restatement starts from the fp32 values (tests/optim_ex_ref.py does the same for AdamW's)."""
import ctypes
import gc
import math

import numpy as np
import torch

import guard
from optim_ex_ref import ConvNet, as_f32, f64
from util import bits, ulp32  # noqa: F401  (the tests reach them through this module)

MIN_SIN = 1e-6                      # MPHSIR_SAM_MIN_SIN of include/mphsir.h (tests/test_spectral_loss_meta.py compares the two)
WEIGHTS = [(0.1, 0.0), (0.0, 0.3), (0.1, 0.3)]
# C = 1 (no band difference, theta = 0); W % 4 != 0 twice (the scalar path); the natural-scene band count; the remote-sensing band counts
# (100 = 4 x 25, 172 = 4 x 43, and 3 / 8 / 31 split unevenly over the four waves); the training patch: several workgroups per image
SHAPES = [(1, 1, 4, 4), (1, 3, 4, 5), (3, 8, 5, 7), (2, 31, 16, 16), (2, 100, 8, 8), (1, 172, 4, 8), (2, 31, 64, 64)]
SHAPE_GPU = (4, 31, 64, 64)         # GPU only, 4 bytes past a 16-byte boundary: the scalar path at a size the 16-byte path is built for


def make_inputs(shape, seed=0):
    """c = rand, y = c + 0.1 randn (CPU masters): about a tenth of y falls outside [0, 1]; theta >= 6e-3 for these seeds"""
    g = torch.Generator().manual_seed(7100 + seed + sum(shape))
    c = torch.rand(shape, generator=g)
    return c + 0.1 * torch.randn(shape, generator=g), c


def put(t, dev, seed=None, offset=False):
    """the CPU master on the check's device: a guarded input while a guard is active; offset: one fp32 element past a 16-byte boundary"""
    G = guard.active()
    if offset:
        flat = torch.cat([torch.zeros(1), t.reshape(-1)])
        flat = G.input(flat, seed) if G is not None and G.device.type == torch.device(dev).type else flat.to(dev)
        v = flat[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4
        return v
    if G is not None and G.device.type == torch.device(dev).type:
        return G.input(t.detach(), seed)
    return t.to(dev)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _sign(v):
    return (v > 0).astype(np.float64) - (v < 0).astype(np.float64)          # 0 for 0 and for a NaN


def reference(y, c, w_sam, w_sdiff):
    """float64, from the definition: -> dict(loss, l1, sam, sdiff, g, mag) with g = d loss / d y and mag the magnitude the gradient bar is
    taken of; a weight of 0 leaves its term out (component 0)"""
    w_sam, w_sdiff = as_f32(w_sam), as_f32(w_sdiff)
    y, c = f64(y), f64(c)
    B, C, H, W = y.shape
    P, n = B * H * W, B * C * H * W
    with np.errstate(all="ignore"):
        x = np.where(y < 0, 0.0, np.where(y > 1, 1.0, y))                   # a NaN stays a NaN
        m = ((y >= 0) & (y <= 1)).astype(np.float64)
        d = x - c
        l1 = np.abs(d).sum() / n
        g_l1 = _sign(d) * m / n
        sam, g_sam, mag_sam = 0.0, np.zeros_like(y), np.zeros_like(y)
        if w_sam != 0.0:
            nx, ny, d2 = np.sqrt((x * x).sum(1)), np.sqrt((c * c).sum(1)), (d * d).sum(1)
            has = (nx != 0) & (ny != 0)
            s = np.sqrt(np.maximum(d2 - (nx - ny) ** 2, 0.0))
            t = np.sqrt(np.maximum((nx + ny) ** 2 - d2, 0.0))
            theta = np.where(has, 2.0 * np.arctan2(s, t), 0.0)
            sam = theta.sum() / P
            sn, cs = np.sin(theta), np.cos(theta)
            ok = has & np.isfinite(nx * nx) & np.isfinite(ny * ny) & np.isfinite(d2) & (sn >= MIN_SIN)
            a = np.where(ok, 1.0 / (sn * nx * ny), 0.0)[:, None]
            b = np.where(ok, cs / (sn * nx * nx), 0.0)[:, None]
            xs, cc = np.where(np.isnan(x), 0.0, x), c                        # m is 0 at a NaN element: keep 0 * NaN out of the product
            g_sam = -(a * cc - b * xs) * m * (w_sam / P)
            mag_sam = (np.abs(a * cc) + np.abs(b * xs)) * (w_sam / P)
        sdiff, g_sd = 0.0, np.zeros_like(y)
        if w_sdiff != 0.0 and C > 1:
            e = (x[:, 1:] - x[:, :-1]) - (c[:, 1:] - c[:, :-1])
            nsd = B * (C - 1) * H * W
            sdiff = np.abs(e).sum() / nsd
            se = _sign(e)
            g_sd[:, 1:] += se
            g_sd[:, :-1] -= se
            g_sd *= m * (w_sdiff / nsd)
    return dict(loss=l1 + w_sam * sam + w_sdiff * sdiff, l1=l1, sam=sam, sdiff=sdiff, g=g_l1 + g_sam + g_sd,
                mag=np.abs(g_l1) + np.abs(g_sd) + mag_sam, g_l1=g_l1, g_sd=g_sd)


def torch_loss(y, c, w_sam, w_sdiff):
    """the same loss as a float64 torch expression (atan2 form, F.l1_loss of band differences): autograd through it is the independent
    check of the closed-form gradient (well-conditioned inputs with C >= 3 only: acos-free, but NaN at theta = 0)"""
    import torch.nn.functional as F
    x = torch.clamp(y, 0, 1)
    nx, ny, d2 = x.norm(dim=1), c.norm(dim=1), ((x - c) ** 2).sum(1)
    theta = 2.0 * torch.atan2(torch.sqrt(torch.clamp(d2 - (nx - ny) ** 2, min=0)), torch.sqrt(torch.clamp((nx + ny) ** 2 - d2, min=0)))
    return F.l1_loss(x, c) + as_f32(w_sam) * theta.mean() + as_f32(w_sdiff) * F.l1_loss(x[:, 1:] - x[:, :-1], c[:, 1:] - c[:, :-1])


def check_restatement_vs_autograd(shape):
    y, c = make_inputs(shape)
    ref = reference(y, c, 0.1, 0.3)
    yt = y.double().requires_grad_(True)
    loss = torch_loss(yt, c.double(), 0.1, 0.3)
    loss.backward()
    err_l, err_g = abs(float(loss.detach()) - ref["loss"]), float(np.abs(f64(yt.grad) - ref["g"]).max())
    print("%s: restatement vs float64 autograd: loss %.3g, gradient %.3g (bar 1e-12)" % (shape, err_l, err_g))
    assert err_l <= 1e-12 and err_g <= 1e-12


# ---- kernel checks --------------------------------------------------------------------------------------------------------------------------
def assert_within_bars(out, g, ref, what):
    """bars 1 and 2 of the module docstring; -> the worst gradient error in units of the bar's ulp"""
    got = [float(v) for v in out.detach().cpu().tolist()]
    for name, val in zip(("loss", "l1", "sam", "sdiff"), got):
        want = ref[name]
        err = abs(val - want) / float(ulp32(want)) if math.isfinite(want) else 0.0
        print("%s %s: %.9g want %.9g (%.2f ulp, bar 2)" % (what, name, val, want, err))
        assert math.isfinite(val) and abs(val - want) <= 2 * float(ulp32(want)), (what, name, val, want)
    gg = f64(g)
    assert np.isfinite(gg).all(), what
    unit = ulp32(ref["mag"])
    worst = float((np.abs(gg - ref["g"]) / unit).max())
    print("%s gradient: worst %.3f ulp of the magnitude (bar 8), max |g| %.3g" % (what, worst, float(np.abs(ref["g"]).max())))
    assert worst <= 8.0, (what, worst)
    return worst


@guard.guarded
def check_values(dev, shape, offset=False):
    """loss, components and gradient against the restatement for the three weight pairs; the autograd form gives the same loss and, after
    backward(), the same gradient bits"""
    from mp_hsir_amd import ops
    ym, cm = make_inputs(shape)
    y, c = put(ym, dev, 1, offset), put(cm, dev, 2, offset)
    worst = 0.0
    for w_sam, w_sd in WEIGHTS:
        loss, g, out = ops.spectral_loss_grad(y, c, w_sam, w_sd)
        assert g.shape == y.shape and g.dtype == torch.float32 and bits(loss) == bits(out[0])
        ref = reference(ym, cm, w_sam, w_sd)
        worst = max(worst, assert_within_bars(out, g, ref, "%s w (%g, %g)%s" % (shape, w_sam, w_sd, " offset" if offset else "")))
        if w_sam == 0.0:
            assert float(out[2]) == 0.0
        if w_sd == 0.0 or shape[1] == 1:
            assert float(out[3]) == 0.0
        ya = y.detach().clone().requires_grad_(True)
        la = ops.spectral_loss(ya, c, w_sam, w_sd)
        la.backward()
        assert bits(la) == bits(loss) and bits(ya.grad) == bits(g)
    return worst


@guard.guarded
def check_paths_agree(dev, shape=(2, 31, 16, 16)):
    """the 16-byte path and the scalar path (the same cube one element past a 16-byte boundary) give the same bits"""
    from mp_hsir_amd import ops
    ym, cm = make_inputs(shape)
    a = ops.spectral_loss_grad(put(ym, dev, 1), put(cm, dev, 2), 0.1, 0.3)
    b = ops.spectral_loss_grad(put(ym, dev, 3, offset=True), put(cm, dev, 4, offset=True), 0.1, 0.3)
    assert bits(a[2]) == bits(b[2]) and bits(a[1]) == bits(b[1])


@guard.guarded
def check_edges(dev):
    from mp_hsir_amd import ops
    shape = (2, 5, 4, 8)
    ym, cm = make_inputs(shape, seed=11)
    # y == c everywhere (inside [0, 1]): all three terms 0, gradient exactly 0, no NaN
    loss, g, out = ops.spectral_loss_grad(put(cm, dev, 1), put(cm, dev, 2), 0.1, 0.3)
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0] and bool((g == 0).all())
    # a pixel of all-zero c, one of all y < 0, y at exactly 0 and 1, y outside [0, 1], +-inf
    ym, cm = ym.clone(), cm.clone()
    cm[0, :, 1, 2] = 0.0
    ym[0, :, 2, 3] = -0.25
    ym[1, 0, 0, 0], ym[1, 1, 0, 0], ym[1, 2, 0, 1], ym[1, 3, 0, 1] = 0.0, 1.0, float("inf"), float("-inf")
    y, c = put(ym, dev, 3), put(cm, dev, 4)
    for w in WEIGHTS:
        loss, g, out = ops.spectral_loss_grad(y, c, *w)
        ref = reference(ym, cm, *w)
        assert_within_bars(out, g, ref, "edges w %s" % (w,))
        gc = g.cpu()
        outside = (ym < 0) | (ym > 1)
        assert bool((gc[outside] == 0).all()), "y outside [0, 1] gets gradient 0 from all three terms"
        assert float(gc[1, 0, 0, 0]) != 0.0 and float(gc[1, 1, 0, 0]) != 0.0, "y at exactly 0 and 1 passes gradient"
    # no angle and no SAM gradient at the two pixels: their gradient is bitwise that of the run without the SAM term
    with_sam, without = ops.spectral_loss_grad(y, c, 0.1, 0.3)[1].cpu(), ops.spectral_loss_grad(y, c, 0.0, 0.3)[1].cpu()
    for (b, i, j) in ((0, 1, 2), (0, 2, 3)):
        assert torch.equal(with_sam[b, :, i, j], without[b, :, i, j])
    assert not torch.equal(with_sam[0, :, 0, 0], without[0, :, 0, 0])
    # one NaN in y: the loss is NaN, the gradient finite everywhere and 0 at the NaN element; the other pixels keep their gradient bits
    clean_run = ops.spectral_loss_grad(y, c, 0.1, 0.3)[1].cpu()
    yn = ym.clone()
    yn[1, 2, 3, 5] = float("nan")
    loss, g, out = ops.spectral_loss_grad(put(yn, dev, 5), c, 0.1, 0.3)
    gc = g.cpu()
    assert math.isnan(float(loss)) and math.isnan(float(out[1])) and bool(torch.isfinite(gc).all()) and float(gc[1, 2, 3, 5]) == 0.0
    keep = torch.ones(shape, dtype=torch.bool)
    keep[1, :, 3, 5] = False
    assert torch.equal(gc[keep], clean_run[keep])
    assert bool((gc[1, :, 3, 5] == torch.from_numpy((reference(yn, cm, 0.0, 0.3)["g"])[1, :, 3, 5].astype(np.float32))).all()), \
        "inside the NaN pixel: L1 + SDIFF only (signs of a NaN difference are 0)"


@guard.guarded
def check_zero_weight(dev):
    """a weight of 0 leaves its term out: bitwise the result of a run with that weight on and inputs on which the term is identically 0 with
    a zero gradient -- SAM: c = 0 everywhere (no pixel has an angle); SDIFF: x - c constant along the bands of every pixel, exactly (all
    values on a 2^-10 grid inside [0, 1])"""
    from mp_hsir_amd import ops
    shape = (2, 7, 4, 8)
    g = torch.Generator().manual_seed(7200)
    y0, c0 = put(torch.rand(shape, generator=g) * 1.2 - 0.1, dev, 1), put(torch.zeros(shape), dev, 2)
    on, off = ops.spectral_loss_grad(y0, c0, 0.1, 0.3), ops.spectral_loss_grad(y0, c0, 0.0, 0.3)
    assert bits(on[2]) == bits(off[2]) and bits(on[1]) == bits(off[1]) and float(on[2][2]) == 0.0 and float(on[2][3]) > 0.0
    cg = torch.randint(256, 512, shape, generator=g).float() / 1024.0
    yg = cg + (torch.randint(-64, 65, (2, 1, 4, 8), generator=g).float() / 1024.0)
    y1, c1 = put(yg, dev, 3), put(cg, dev, 4)
    on, off = ops.spectral_loss_grad(y1, c1, 0.1, 0.3), ops.spectral_loss_grad(y1, c1, 0.1, 0.0)
    assert bits(on[2]) == bits(off[2]) and bits(on[1]) == bits(off[1]) and float(on[2][3]) == 0.0 and float(on[2][2]) > 0.0


@guard.guarded
def check_reproducible(dev, shape):
    from mp_hsir_amd import ops
    ym, cm = make_inputs(shape)
    y, c = put(ym, dev, 1), put(cm, dev, 2)
    a, b = ops.spectral_loss_grad(y, c, 0.1, 0.3), ops.spectral_loss_grad(y, c, 0.1, 0.3)
    assert bits(a[2]) == bits(b[2]) and bits(a[1]) == bits(b[1])


@guard.guarded
def check_refusals(dev):
    """an error (EINVAL, a message), nothing launched: ops.ACCOUNT stays empty and no output changes"""
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    lib = L.load()
    shape = (2, 3, 4, 8)
    ym, cm = make_inputs(shape)
    y, c = put(ym, dev, 1), put(cm, dev, 2)
    need = lib.mphsir_spectral_loss_workspace_bytes(*shape)
    assert need == 24 * 2 and lib.mphsir_spectral_loss_workspace_bytes(32, 31, 64, 64) == 24 * 512
    assert lib.mphsir_spectral_loss_workspace_bytes(2, 0, 4, 8) < 0 and lib.mphsir_spectral_loss_workspace_bytes(0, 3, 4, 8) < 0
    g = torch.full(shape, -7.0, device=dev)
    out, ws = torch.full((4,), -7.0, device=dev), torch.full((need // 8,), -7.0, dtype=torch.float64, device=dev)
    keep = [bits(t) for t in (g, out, ws)]
    stream = ops._stream(y)

    def args(**kw):
        a = L.SpectralLossArgs(y=y.data_ptr(), clean=c.data_ptr(), grad=g.data_ptr(), out=out.data_ptr(), workspace=ws.data_ptr(),
                               workspace_bytes=need, B=shape[0], C=shape[1], H=shape[2], W=shape[3], w_sam=0.1, w_sdiff=0.3)
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def refused(a, text):
        assert lib.mphsir_spectral_loss(ctypes.byref(a), stream) == -1, text
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()

    ops.ACCOUNT = {}
    try:
        refused(args(w_sam=0.0, w_sdiff=0.0), "mphsir_l1_clamp_loss")
        refused(args(struct_size=ctypes.sizeof(L.SpectralLossArgs) - 8), "struct_size")
        refused(args(struct_size=ctypes.sizeof(L.SpectralLossArgs) + 8), "struct_size")
        refused(args(C=0), "bad sizes")
        refused(args(B=0), "bad sizes")
        for name in ("y", "clean", "out", "workspace"):
            refused(args(**{name: None}), "null pointer")
        refused(args(workspace_bytes=need - 1), "workspace")
        refused(args(workspace=ws.data_ptr() + 4, workspace_bytes=need + 8), "workspace")
        for bad in (-0.1, float("nan"), float("inf")):
            refused(args(w_sam=bad), "weights")
            refused(args(w_sdiff=bad), "weights")
        for call in (lambda: ops.spectral_loss_grad(y, c, 0.0, 0.0), lambda: ops.spectral_loss_grad(y, c, -1.0, 0.3),
                     lambda: ops.spectral_loss_grad(y.double(), c.double(), 0.1, 0.3), lambda: ops.spectral_loss_grad(y.half(), c.half(), 0.1, 0.3),
                     lambda: ops.spectral_loss_grad(y, c[:1], 0.1, 0.3), lambda: ops.spectral_loss_grad(y[0], c[0], 0.1, 0.3),
                     lambda: ops.spectral_loss(y, c, 0.0, 0.0)):
            try:
                call()
            except (RuntimeError, AssertionError):
                pass
            else:
                raise AssertionError("a wrapper accepted what the entry point refuses")
        other = torch.zeros(shape) if torch.device(dev).type == "cuda" else None      # a CPU tensor while the GPU library is bound
        if other is not None:
            try:
                ops.spectral_loss_grad(other, other, 0.1, 0.3)
            except RuntimeError as e:
                assert "no CPU fallback" in str(e)
            else:
                raise AssertionError("CPU tensors accepted")
        assert not ops.ACCOUNT, ("launched before refusing", sorted(ops.ACCOUNT))
        assert [bits(t) for t in (g, out, ws)] == keep, "something was launched"
        assert lib.mphsir_spectral_loss(ctypes.byref(args()), stream) == 0                 # the same arguments, nothing wrong: it runs
        assert_within_bars(out, g, reference(ym, cm, 0.1, 0.3), "after the refusals")
        assert lib.mphsir_spectral_loss(ctypes.byref(args(grad=None)), stream) == 0        # grad is optional
    finally:
        ops.ACCOUNT = None
    assert lib.mphsir_kernel_name(39) == b"spectral_loss" and lib.mphsir_kernel_name(40) == b"spectral_loss_finish"


# ---- engine checks --------------------------------------------------------------------------------------------------------------------------
# "tiny": model_checks.build_net(TINY_CFG) through the HIP forward / backward, batch (2, 8, 32, 32) -- the GPU tests; "conv": the
# two-convolution network of tests/optim_ex_ref.py -- the emulator tests (a step of the tiny net takes 75 s through the emulator)
def make_net(kind, dev, dtype=torch.float32):
    if kind == "conv":
        torch.manual_seed(690)
        return ConvNet().to(dev)
    import model_checks as M
    from golden.cases import TINY_CFG
    return M.build_net(TINY_CFG, dev, dtype)


def batch(step, dev, kind):
    from golden.detfill import seeded_input
    shape = (4, 3, 8, 8) if kind == "conv" else (2, 8, 32, 32)
    return (seeded_input("sl_x%d" % step, shape).to(dev), seeded_input("sl_c%d" % step, shape).to(dev), torch.tensor([[1], [3]]).to(dev))


def make_engine(dev, kind, use_graph=False, dtype=torch.float32, **kw):
    from mp_hsir_amd.engine import DataParallelEngine
    gc.collect()          # dead engines of earlier tests go now, not at a moment of the collector's choosing (see run_engine)
    net = make_net(kind, dev, dtype)
    return net, DataParallelEngine(net, lr=2e-3, use_graph=use_graph, graph_warmup=0 if use_graph else 2, **kw)


def run_engine(dev, kind, steps, use_graph=False, dtype=torch.float32, account=False, **kw):
    """-> (engine, [loss per step], flat_p bits after the last step, the ops.ACCOUNT launch counts of the LAST step when asked)"""
    from mp_hsir_amd import ops
    net, eng = make_engine(dev, kind, use_graph, dtype, **kw)
    losses, acct = [], None
    eng.g_bits = []                                       # the gradient arena after every step
    for s in range(steps):
        if account and s == steps - 1:
            ops.ACCOUNT = {}
        try:
            losses.append(eng.train_step(*batch(s, dev, kind)).clone())
            eng.g_bits.append(bits(eng.flat_g))
        finally:
            if ops.ACCOUNT is not None:
                acct = {k: v[0] for k, v in ops.ACCOUNT.items()}
                ops.ACCOUNT = None
    # The captured graph is destroyed HERE.  An engine that dies inside a reference cycle (the frames of a failed assertion hold it) is
    # freed whenever the collector next runs, possibly in the middle of another engine's capture, and destroying a graph while a stream
    # is capturing aborts the process (this torch no longer collects at the start of a capture).  Its buffers outlive it.
    eng.captured = eng._graph is not None
    if eng.captured:
        torch.cuda.synchronize()
        eng._graph = None
    return eng, losses, bits(eng.flat_p), acct


def check_engine_eager_vs_graph(dev, kind="tiny", dtype=torch.float32):
    """three steps with SpectralLoss(0.1, 0.3), eager and in graph mode: bitwise-equal losses, gradient arenas and parameters (under this
    loss the eager step stages Adam's bias corrections on the device as the replayed step reads them: DataParallelEngine._eager_hyper);
    loss_components() reads the replayed buffer"""
    from mp_hsir_amd.engine import SpectralLoss
    e0, l0, p0, _ = run_engine(dev, kind, 3, False, dtype, loss_fn=SpectralLoss(0.1, 0.3))
    e1, l1, p1, _ = run_engine(dev, kind, 3, True, dtype, loss_fn=SpectralLoss(0.1, 0.3))
    assert e1.captured and not e0.captured, "the graph-mode engine never captured"
    print("losses eager %s graph %s; parameters equal: %s; gradient arenas equal per step: %s"
          % ([float(a) for a in l0], [float(b) for b in l1], p0 == p1, [a == b for a, b in zip(e0.g_bits, e1.g_bits)]))
    lc = e1.loss_components()
    assert lc["loss"] == float(l1[-1]) and lc["l1"] > 0 and lc["sam_deg"] > 0 and lc["sdiff"] > 0
    assert [bits(a) for a in l0] == [bits(b) for b in l1] and e0.g_bits == e1.g_bits and p0 == p1


def check_engine_loss_and_components(dev, kind="tiny", dtype=torch.float32):
    """the loss a step returns is ops.spectral_loss_grad's on the same `restored`; loss_components() reports it and its three terms"""
    from mp_hsir_amd import ops
    from mp_hsir_amd.engine import SpectralLoss
    net, eng = make_engine(dev, kind, False, dtype, loss_fn=SpectralLoss(0.1, 0.3))
    assert eng.loss_components() is None
    x, c, task = batch(0, dev, kind)
    with torch.no_grad():
        restored = net(x, task).float()
    want = ops.spectral_loss_grad(restored, c, 0.1, 0.3)
    got = eng.train_step(x, c, task)
    assert bits(got) == bits(want[0])
    lc = eng.loss_components()
    assert lc["loss"] == float(got) and [lc["l1"], math.radians(lc["sam_deg"]), lc["sdiff"]] == pytest_approx(want[2][1:].tolist())
    assert lc["l1"] > 0 and lc["sam_deg"] > 0 and lc["sdiff"] > 0
    assert abs(lc["loss"] - (lc["l1"] + as_f32(0.1) * math.radians(lc["sam_deg"]) + as_f32(0.3) * lc["sdiff"])) <= 4 * float(ulp32(lc["loss"]))


def pytest_approx(vals):
    import pytest
    return pytest.approx(vals, rel=1e-12)


def check_engine_off_by_default(dev, kind="tiny", use_graph=False):
    """no loss_fn == loss_fn=l1_after_clamp given explicitly: the same launch list and bitwise the same parameters after two steps; with
    the loss on the list differs in l1_clamp_loss -> spectral_loss and in nothing else"""
    from mp_hsir_amd.engine import SpectralLoss, l1_after_clamp
    n = 3 if use_graph else 2
    e0, _, p0, a0 = run_engine(dev, kind, n, use_graph, account=True)
    e1, _, p1, a1 = run_engine(dev, kind, n, use_graph, account=True, loss_fn=l1_after_clamp)
    assert p0 == p1 and a0 == a1 and e0.loss_components() is None
    if use_graph:
        return                                                # a replayed step issues no launches the account could see
    assert a0["l1_clamp_loss"] == 1 and "spectral_loss" not in a0
    e2, _, p2, a2 = run_engine(dev, kind, n, use_graph, account=True, loss_fn=SpectralLoss(0.1, 0.3))
    assert p2 != p0 and a2["spectral_loss"] == 1 and "l1_clamp_loss" not in a2
    rest0, rest2 = dict(a0), dict(a2)
    del rest0["l1_clamp_loss"], rest2["spectral_loss"]
    # l1_clamp_loss hands its block partials (one per 1024 elements) to a reduce_parts launch of its own when there is more than one:
    # that launch is part of the default loss and leaves with it; the spectral loss sums its partials in its second launch
    if batch(0, dev, kind)[0].numel() > 1024:
        rest0["reduce_parts"] -= 1
    assert rest0 == rest2, (a0, a2)


def check_engine_fp16_scaler(dev, kind="tiny"):
    """the fp16 path: the gradient goes through the loss scale (g.mul_), the optimizer divides it out; parameters stay finite and move"""
    from mp_hsir_amd.engine import SpectralLoss
    kw = dict(loss_scaling=True) if kind == "conv" else {}
    net, eng = make_engine(dev, kind, False, torch.float16 if kind != "conv" else torch.float32, loss_fn=SpectralLoss(0.1, 0.3), init_scale=1024.0, **kw)
    for s in range(3):
        loss = eng.train_step(*batch(s, dev, kind))
        if s == 0:
            start = eng.flat_p.clone()
    assert eng.scaler is not None and float(eng.scaler[3]) >= 2.0, "the scaler counted optimizer steps"
    assert bool(torch.isfinite(eng.flat_p).all()) and math.isfinite(float(loss)) and not torch.equal(start, eng.flat_p)
