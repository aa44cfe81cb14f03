"""Global-norm clipping and EMA weights (mp-hsir_amd/csrc/optim.hip: grad_sqnorm_kernel, grad_norm_finish_kernel, flat_adamw_ex_kernel;
engine.DataParallelEngine(grad_clip=, ema_decay=)): a float64 numpy restatement of clip + AdamW + EMA and the checks, parametrised by
device.  tests/test_optim_ex_emu.py runs them through the CPU-emulated build, tests/test_optim_ex_gpu.py on the GPU.

Bars.  The norm: every square is exact in float64 and only the order of at most 2^22 additions differs from numpy's, so the float64 sum
of the block partials is within n 2^-53 <= 1e-10 (relative) of the reference and stats[0] within one fp32 ulp of its rounding.  The clip
factor: one fp32 ulp of the float64 rule.  Arenas after clipped steps: rel-L2 < 2e-6 per arena and step, the bar tests/kernel_checks.py
check_loss_scaler holds mphsir_flat_adamw_scaled to."""
import ctypes
import math

import numpy as np
import torch

from util import bits, rel_l2, ulp32  # noqa: F401  (the tests reach them through this module)

# one vector; less than a full block plus a tail vector; just past a block multiple; many blocks, still small enough for the emulator
SIZES = [4, 1028, 3 * 1024 + 4, 2 ** 16 + 8]
SIZE_GPU = 2 ** 21 + 2 ** 12 + 4          # past the 2048-block cap: the grid-stride loops run twice
def as_f32(x):
    return float(np.float32(x))


# The hyper-parameters cross the C ABI as fp32 (the parameter lists of mphsir_flat_adamw and the float members of the args struct), so the
# restatement starts from the values the kernel is GIVEN: 1 - (float)0.999 is 4.7e-5 away from 0.001, which is a property of the
# interface (and of mphsir_flat_adamw, whose bits the new kernel must keep), not a rounding error of the kernel.
B1, B2, EPS, WD = as_f32(0.9), as_f32(0.999), as_f32(1e-8), as_f32(1e-2)
BAR = 2e-6


def normals(n, seed, dev="cpu", scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dev)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def ref_norm(g, grad_scale=1.0, loss_scale=1.0):
    return math.sqrt(float(np.sum(f64(g) ** 2))) * grad_scale / loss_scale


def ref_coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))            # torch.nn.utils.clip_grad_norm_


def ema_decay_at(decay, t, warmup):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class RefState:
    """p, m, v (and ema) in float64, stepped by clip + AdamW (decoupled decay, torch.optim.AdamW's update) + EMA"""

    def __init__(self, p, m=None, v=None, ema=None):
        self.p = f64(p)
        self.m = np.zeros_like(self.p) if m is None else f64(m)
        self.v = np.zeros_like(self.p) if v is None else f64(v)
        self.ema = None if ema is None else f64(ema)

    def step(self, g, lr, t, max_norm=None, grad_scale=1.0, loss_scale=1.0, decay=None, bc=None):
        """-> (norm, coef) used; t: the 1-based step of the bias corrections; bc: (1 - beta1^t, sqrt(1 - beta2^t)) as staged by the caller
        of the hyper form (the engine computes them from 0.9 / 0.999 in double), default: from the betas the kernel is given"""
        lr, decay = as_f32(lr), None if decay is None else as_f32(decay)
        bc1, bc2_sqrt = (as_f32(b) for b in bc) if bc is not None else (1.0 - B1 ** t, math.sqrt(1.0 - B2 ** t))
        g = f64(g) * (grad_scale / loss_scale)
        norm = math.sqrt(float(np.sum(g ** 2)))
        coef = 1.0 if max_norm is None else ref_coef(norm, max_norm)
        g = g * coef
        self.p *= 1.0 - lr * WD
        self.m = B1 * self.m + (1.0 - B1) * g
        self.v = B2 * self.v + (1.0 - B2) * g * g
        self.p -= (lr / bc1) * self.m / (np.sqrt(self.v) / bc2_sqrt + EPS)
        if decay is not None:
            self.ema += (1.0 - decay) * (self.p - self.ema)
        return norm, coef

    def compare(self, p, m, v, ema=None, what=""):
        errs = {"p": rel_l2(p.cpu(), self.p), "m": rel_l2(m.cpu(), self.m), "v": rel_l2(v.cpu(), self.v)}
        if ema is not None:
            errs["ema"] = rel_l2(ema.cpu(), self.ema)
        print("%s rel-L2 %s (bar %.1g)" % (what, {k: "%.3g" % e for k, e in errs.items()}, BAR))
        assert all(e < BAR for e in errs.values()), (what, errs)


# ---- kernel checks --------------------------------------------------------------------------------------------------------------------------
def norm_inputs(n, dev):
    """seeded normals; the same with one entry 1e30 (its square overflows fp32, not float64); all entries 1e-30 (their squares vanish in fp32)"""
    g = normals(n, 601 + n % 97)
    big = g.clone()
    big[n // 2] = 1e30
    return [("normal", g.to(dev)), ("one 1e30", big.to(dev)), ("all 1e-30", torch.full((n,), 1e-30).to(dev))]


def check_norm(dev, n):
    from mp_hsir_amd import ops
    for label, g in norm_inputs(n, dev):
        for grad_scale, loss_scale in ((1.0, None), (0.5, None), (1.0, 1024.0)):
            scaler = None if loss_scale is None else ops.new_loss_scaler(dev, loss_scale)
            stats, ws = ops.new_optim_stats(dev), ops.grad_norm_workspace(g)
            ops.grad_norm(g, stats, float("inf"), grad_scale, scaler=scaler, workspace=ws)
            S, want_S = math.fsum(ws.cpu().tolist()), float(np.sum(f64(g) ** 2))
            want = ref_norm(g, grad_scale, loss_scale or 1.0)
            got = float(stats[0])
            print("n %d %s gs %g scale %s: S rel err %.3g, norm %.9g want %.9g" % (n, label, grad_scale, loss_scale, abs(S - want_S) / want_S, got, want))
            assert want_S > 0 and abs(S - want_S) / want_S <= 1e-10
            assert math.isfinite(got) and got > 0 and abs(got - float(np.float32(want))) <= ulp32(want), (label, got, want)
            assert stats.tolist()[1:] == [1.0, 0.0, 0.0]


def _fresh(n, dev, seed=611):
    return normals(n, seed, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)


def check_coef(dev, n):
    """max_norm above the norm and +inf: coef == 1 exactly and p / m / v bitwise those of flat_adamw; below: one fp32 ulp of the rule"""
    from mp_hsir_amd import ops
    g = normals(n, 620, dev)
    norm = ref_norm(g)
    p0, m0, v0 = _fresh(n, dev)
    ops.flat_adamw(p0, g, m0, v0, 1e-2, 1)
    for max_norm in (norm * 1.5, float("inf")):
        stats = ops.new_optim_stats(dev)
        ops.grad_norm(g, stats, max_norm)
        assert float(stats[1]) == 1.0 and float(stats[3]) == 0.0
        p, m, v = _fresh(n, dev)
        ops.flat_adamw_ex(p, g, m, v, 1e-2, 1, stats=stats)
        assert bits(p) == bits(p0) and bits(m) == bits(m0) and bits(v) == bits(v0), max_norm
    for frac in (0.5, 0.01):
        stats = ops.new_optim_stats(dev)
        ops.grad_norm(g, stats, norm * frac)
        want = ref_coef(norm, float(np.float32(norm * frac)))
        print("n %d: coef %.9g want %.9g" % (n, float(stats[1]), want))
        assert float(stats[1]) < 1.0 and abs(float(stats[1]) - float(np.float32(want))) <= ulp32(want)


def check_bitwise_link(dev, n):
    """three steps of flat_adamw_ex without stats and without ema == flat_adamw (host-lr form and hyper form) and, with a scaler,
    == scaled_adamw_step including its overflow step"""
    from mp_hsir_amd import ops
    a, b = _fresh(n, dev), _fresh(n, dev)
    for form in ("host", "hyper"):
        for t in (1, 2, 3):
            g = normals(n, 630 + t, dev)
            lr = 1e-2 / t
            if form == "host":
                ops.flat_adamw(a[0], g, a[1], a[2], lr, t, grad_scale=0.5)
                ops.flat_adamw_ex(b[0], g, b[1], b[2], lr, t, grad_scale=0.5)
            else:
                hyper = torch.tensor([lr, 1.0 - B1 ** t, math.sqrt(1.0 - B2 ** t)], dtype=torch.float32, device=dev)
                ops.flat_adamw(a[0], g, a[1], a[2], 0.0, 0, grad_scale=0.5, hyper=hyper)
                ops.flat_adamw_ex(b[0], g, b[1], b[2], 0.0, 0, grad_scale=0.5, hyper=hyper)
            assert all(bits(x) == bits(y) for x, y in zip(a, b)), (form, t)
    a, b = _fresh(n, dev), _fresh(n, dev)
    sa, sb = ops.new_loss_scaler(dev, 1024.0), ops.new_loss_scaler(dev, 1024.0)
    for t in range(4):
        g = normals(n, 640 + t, dev) * float(sa[0])
        if t == 1:
            g[n // 3] = float("inf")
        ops.scaled_adamw_step(a[0], g, a[1], a[2], sa, 1e-2, interval=2)
        ops.grad_check(g, sb)
        ops.flat_adamw_ex(b[0], g, b[1], b[2], 1e-2, 1, scaler=sb)
        ops.scaler_update(sb, interval=2)
        assert all(bits(x) == bits(y) for x, y in zip(a, b)) and bits(sa) == bits(sb), t
    assert float(sb[3]) == 3.0


def check_clipped_ema_steps(dev, n, warmup, steps=5, decay=0.9):
    """five clipped steps with EMA against the restatement: p, m, v and ema each within the bar at every step"""
    from mp_hsir_amd import ops
    p, m, v = _fresh(n, dev, 650)
    ema, stats = p.clone(), ops.new_optim_stats(dev)
    ref = RefState(p, ema=p)
    clipped = 0
    for t in range(1, steps + 1):
        g = normals(n, 650 + t, dev, scale=1.0 + t)
        max_norm = 0.7 * math.sqrt(n)                      # below the norm of every step (about (1 + t) sqrt(n))
        d = ema_decay_at(decay, t, warmup)
        ops.grad_norm(g, stats, max_norm, 0.5)
        ops.flat_adamw_ex(p, g, m, v, 1e-2, t, grad_scale=0.5, stats=stats, ema=ema, ema_decay=d)
        norm, coef = ref.step(g, 1e-2, t, max_norm=max_norm, grad_scale=0.5, decay=d)
        clipped += coef < 1.0
        assert abs(float(stats[0]) - norm) <= 2 * ulp32(norm) and abs(float(stats[1]) - coef) <= 2 * ulp32(coef)
        ref.compare(p, m, v, ema, "n %d warmup %s step %d (decay %.3f, coef %.3f)" % (n, warmup, t, d, coef))
    assert clipped == steps and rel_l2(ema.cpu(), f64(p)) > 1e-4, "the test is meant to clip every step and to leave the EMA behind p"


def check_nonfinite(dev, n, bad, with_scaler):
    """an inf / a NaN at element 17: p, m, v, ema bitwise unchanged, the skip flag set, the skip count up by one; the next finite step
    proceeds and clears the flag"""
    from mp_hsir_amd import ops
    assert n > 17
    p, m, v = _fresh(n, dev, 660)
    ema, stats = p.clone(), ops.new_optim_stats(dev)
    scaler = ops.new_loss_scaler(dev, 1024.0) if with_scaler else None

    def step(g, t):
        if scaler is not None:
            ops.grad_check(g, scaler)
        ops.grad_norm(g, stats, 1.0, scaler=scaler)
        ops.flat_adamw_ex(p, g, m, v, 1e-2, t, scaler=scaler, stats=stats, ema=ema, ema_decay=0.9)
        if scaler is not None:
            ops.scaler_update(scaler, interval=1000)

    scale = 1024.0 if with_scaler else 1.0
    step(normals(n, 661, dev) * scale, 1)
    assert stats.tolist()[2:] == [0.0, 0.0] and float((ema - p).abs().max()) > 0
    before = [bits(x) for x in (p, m, v, ema)]
    g = normals(n, 662, dev) * scale
    g[17] = bad
    step(g, 2)
    assert [bits(x) for x in (p, m, v, ema)] == before
    assert float(stats[1]) == 0.0 and stats.tolist()[2:] == [1.0, 1.0] and not math.isfinite(float(stats[0]))
    if scaler is not None:
        assert float(scaler[0]) == 512.0 and float(scaler[3]) == 1.0
    step(normals(n, 663, dev) * (float(scaler[0]) if with_scaler else 1.0), 2)
    assert stats.tolist()[2:] == [1.0, 0.0] and 0.0 < float(stats[1]) <= 1.0 and math.isfinite(float(stats[0]))
    assert bits(p) != before[0] and bits(ema) != before[3] and bool(torch.isfinite(p).all())


def check_reproducible(dev, n):
    from mp_hsir_amd import ops
    outs = []
    for _ in range(2):
        p, m, v = _fresh(n, dev, 670)
        ema, stats = p.clone(), ops.new_optim_stats(dev)
        for t in (1, 2):
            g = normals(n, 670 + t, dev)
            ops.grad_norm(g, stats, 0.5 * math.sqrt(n))
            ops.flat_adamw_ex(p, g, m, v, 1e-2, t, stats=stats, ema=ema, ema_decay=0.9)
        outs.append([bits(x) for x in (stats, p, m, v, ema)])
    assert outs[0] == outs[1]


def check_refusals(dev):
    """an error (EINVAL, a message), nothing launched: ops.ACCOUNT stays empty and no output changes"""
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    lib = L.load()
    n = 1024
    base = normals(n + 4, 680, dev)
    g = base[:n]
    p, m, v = _fresh(n, dev, 681)
    ema, stats, ws = p.clone(), ops.new_optim_stats(dev), ops.grad_norm_workspace(g)
    ws.fill_(-7.0)
    need = lib.mphsir_grad_norm_workspace_bytes(n)
    assert need == 8 * 1 and lib.mphsir_grad_norm_workspace_bytes(SIZE_GPU) == 8 * 2048 and lib.mphsir_grad_norm_workspace_bytes(6) < 0
    keep = [bits(x) for x in (p, m, v, ema, stats, ws)]
    stream = ops._stream(g)

    def norm_args(**kw):
        a = L.GradNormArgs(g=g.data_ptr(), n=n, grad_scale=1.0, max_norm=1.0, scaler=None, workspace=ws.data_ptr(), workspace_bytes=need,
                           stats=stats.data_ptr())
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def adam_args(**kw):
        a = L.FlatAdamwExArgs(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), ema=ema.data_ptr(), n=n, lr=1e-2, beta1=B1,
                              beta2=B2, eps=EPS, weight_decay=WD, grad_scale=1.0, step=1, ema_decay=0.9, hyper=None, scaler=None,
                              stats=stats.data_ptr())
        for k, val in kw.items():
            setattr(a, k, val)
        return a

    def refused(fn, a, text):
        assert fn(ctypes.byref(a), stream) == -1, text
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()

    ops.ACCOUNT = {}
    try:
        refused(lib.mphsir_grad_norm, norm_args(struct_size=ctypes.sizeof(L.GradNormArgs) - 8), "struct_size")
        refused(lib.mphsir_grad_norm, norm_args(n=n - 2), "multiple of 4")
        refused(lib.mphsir_grad_norm, norm_args(g=base.data_ptr() + 4), "alignment")
        refused(lib.mphsir_grad_norm, norm_args(workspace_bytes=need - 1), "workspace")
        for bad in (0.0, -1.0, float("nan")):
            refused(lib.mphsir_grad_norm, norm_args(max_norm=bad), "max_norm")
        refused(lib.mphsir_grad_norm, norm_args(stats=None), "null pointer")
        refused(lib.mphsir_flat_adamw_ex, adam_args(struct_size=ctypes.sizeof(L.FlatAdamwExArgs) + 8), "struct_size")
        refused(lib.mphsir_flat_adamw_ex, adam_args(n=n - 2), "multiple of 4")
        refused(lib.mphsir_flat_adamw_ex, adam_args(g=base.data_ptr() + 4), "alignment")
        refused(lib.mphsir_flat_adamw_ex, adam_args(ema=base.data_ptr() + 8), "alignment")
        for bad in (1.0, -0.1, float("nan")):
            refused(lib.mphsir_flat_adamw_ex, adam_args(ema_decay=bad), "ema_decay")
        # the wrappers refuse the same before any launch
        for call in (lambda: ops.grad_norm(base[:6].clone(), stats, 1.0), lambda: ops.grad_norm(base[1:n + 1], stats, 1.0, workspace=ws),
                     lambda: ops.grad_norm(g, stats, 0.0, workspace=ws), lambda: ops.grad_norm(g, stats, 1.0, workspace=ws[:0]),
                     lambda: ops.flat_adamw_ex(p, g, m, v, 1e-2, 1, ema=ema, ema_decay=1.0),
                     lambda: ops.flat_adamw_ex(p, base[1:n + 1], m, v, 1e-2, 1)):
            try:
                call()
            except (RuntimeError, AssertionError):
                pass
            else:
                raise AssertionError("a wrapper accepted what the entry point refuses")
        assert not ops.ACCOUNT, ("launched before refusing", sorted(ops.ACCOUNT))
        assert [bits(x) for x in (p, m, v, ema, stats, ws)] == keep, "something was launched"
        assert lib.mphsir_grad_norm(ctypes.byref(norm_args()), stream) == 0 and lib.mphsir_flat_adamw_ex(ctypes.byref(adam_args()), stream) == 0
        assert float(stats[0]) > 0 and bits(p) != keep[0]
    finally:
        ops.ACCOUNT = None


# ---- engine checks --------------------------------------------------------------------------------------------------------------------------
# Two networks.  "tiny": model_checks.build_net(TINY_CFG) through the HIP forward / backward -- the GPU tests.  "conv": two torch
# convolutions (the net of tests/test_host_logic.py's gloo worker) -- the emulator tests: a step of the tiny net through the emulated
# kernels takes 75 s (measured: 24 minutes for the three engine tests), and what these checks are about is the engine's optimizer path,
# which runs through the emulated optim.hip kernels with either network.
class ConvNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.b = torch.nn.Conv2d(8, 3, 3, padding=1)
        self.unused = torch.nn.Linear(5, 5)              # never receives a gradient: stays out of the arenas
        self.register_buffer("stamp", torch.arange(3.0))

    def forward(self, x, prompt):
        return self.b(torch.nn.functional.gelu(self.a(x))) + x


def make_net(kind, dev):
    if kind == "conv":
        torch.manual_seed(690)
        return ConvNet().to(dev)
    import model_checks as M
    from golden.cases import TINY_CFG
    return M.build_net(TINY_CFG, dev, torch.float32)


def _batch(step, dev, kind="tiny"):
    from golden.detfill import seeded_input
    shape = (4, 3, 8, 8) if kind == "conv" else (2, 8, 32, 32)
    return (seeded_input("ox_x%d" % step, shape).to(dev), seeded_input("ox_c%d" % step, shape).to(dev), torch.tensor([[1], [3]]).to(dev))


def make_engine(dev, use_graph=False, lr=2e-3, kind="tiny", **kw):
    from mp_hsir_amd.engine import DataParallelEngine
    net = make_net(kind, dev)
    return net, DataParallelEngine(net, lr=lr, use_graph=use_graph, graph_warmup=0 if use_graph else 2, **kw)


def run_engine(dev, use_graph, steps, snapshots=False, kind="tiny", **kw):
    """-> (net, engine, per-step records): grad_stats() of every step and, with snapshots, the arenas before the optimizer ran (p, m, v of
    the step before, g of this step) and flat_p after it"""
    net, eng = make_engine(dev, use_graph, kind=kind, **kw)
    init = {id(p): p.detach().clone() for p in net.parameters()}
    rec = []
    for s in range(steps):
        before = None if eng.arena is None or not snapshots else [x.clone() for x in (eng.flat_p, eng.flat_m, eng.flat_v)]
        eng.train_step(*_batch(s, dev, kind))
        r = dict(eng.grad_stats(), p=eng.flat_p.clone(), before=before, g=eng.flat_g.clone())
        if eng.flat_ema is not None:
            r["ema"] = eng.flat_ema.clone()
        if s == 0:                                      # the arenas exist now: the parameters the run (and its EMA) started from, in arena order
            r["p0"] = torch.zeros_like(eng.flat_p)
            for p, o in zip(*eng.arena[:2]):
                r["p0"][o:o + p.numel()] = init[id(p)].reshape(-1)
        rec.append(r)
    return net, eng, rec


def check_engine_off(dev, use_graph=False, kind="tiny"):
    """both features off: a step's ops.ACCOUNT holds neither new name, no EMA arena, no stats"""
    from mp_hsir_amd import ops
    net, eng = make_engine(dev, use_graph, kind=kind)
    ops.ACCOUNT = {}
    try:
        for s in range(2):
            eng.train_step(*_batch(s, dev, kind))
        assert "grad_norm" not in ops.ACCOUNT and "flat_adamw_ex" not in ops.ACCOUNT, sorted(ops.ACCOUNT)
    finally:
        ops.ACCOUNT = None
    assert eng.flat_ema is None and eng.optim_stats is None and eng.grad_stats() == {"norm": 0.0, "coef": 1.0, "skipped": 0}
    net2, eng2 = make_engine(dev, use_graph, kind=kind, grad_clip=1.0, ema_decay=0.9)
    ops.ACCOUNT = {}
    try:
        eng2.train_step(*_batch(0, dev, kind))
        assert ops.ACCOUNT["grad_norm"][0] == 1 and ops.ACCOUNT["flat_adamw_ex"][0] == 1, sorted(ops.ACCOUNT)
    finally:
        ops.ACCOUNT = None


def check_engine_measure_and_ema(dev, use_graph=False, steps=3, decay=0.9, kind="tiny"):
    """grad_clip=1e9 (never clips) + EMA: parameters bitwise those of a default engine; flat_ema follows the recurrence applied to the
    per-step parameter snapshots.  -> the norm reported at step 1"""
    _, eng0, rec0 = run_engine(dev, use_graph, steps, kind=kind)
    _, eng1, rec1 = run_engine(dev, use_graph, steps, kind=kind, grad_clip=1e9, ema_decay=decay)
    ema = f64(rec1[0]["p0"])
    for s, (r0, r1) in enumerate(zip(rec0, rec1)):
        assert bits(r0["p"]) == bits(r1["p"]), "step %d: measuring the norm / keeping an EMA changed the parameters" % s
        assert r1["coef"] == 1.0 and r1["skipped"] == 0 and r1["norm"] > 0
        want = math.sqrt(float(np.sum(f64(r1["g"]) ** 2)))
        assert abs(r1["norm"] - want) <= 2 * ulp32(want), (s, r1["norm"], want)
        d = ema_decay_at(decay, s + 1, True)
        ema = ema + (1.0 - d) * (f64(r1["p"]) - ema)
        e = rel_l2(r1["ema"].cpu(), ema)
        print("step %d: norm %.6g, ema rel-L2 %.3g" % (s + 1, r1["norm"], e))
        assert e < BAR
    return rec1[0]["norm"]


def check_engine_active_clip(dev, norm1, use_graph=False, steps=3, kind="tiny"):
    """grad_clip = half the norm measured at step 1: coef < 1 there, and the float64 optimizer replayed from the snapshots of
    flat_p / flat_g / flat_m / flat_v reproduces flat_p of every step"""
    lr = 2e-3
    _, eng, rec = run_engine(dev, use_graph, steps, snapshots=True, kind=kind, lr=lr, grad_clip=0.5 * norm1)
    assert rec[0]["coef"] < 1.0 and abs(rec[0]["coef"] - 0.5) < 1e-3, rec[0]["coef"]
    for s, r in enumerate(rec):
        if r["before"] is None:
            continue                                    # the first step builds the arenas: no snapshot of the state before it
        ref = RefState(*r["before"])
        bc = None if not use_graph else (1.0 - 0.9 ** (s + 1), math.sqrt(1.0 - 0.999 ** (s + 1)))     # graph mode: staged by the engine
        norm, coef = ref.step(r["g"], lr, s + 1, max_norm=0.5 * norm1, bc=bc)
        e = rel_l2(r["p"].cpu(), ref.p)
        print("step %d: norm %.6g coef %.4f (engine %.6g %.4f), p rel-L2 %.3g" % (s + 1, norm, coef, r["norm"], r["coef"], e))
        assert abs(r["coef"] - coef) <= 2 * ulp32(coef) and e < BAR


def check_engine_ema_weights(dev, use_graph=False, kind="tiny"):
    """inside ema_weights() the forward is bitwise that of a fresh net loaded with ema_state_dict(); after exit the parameters are bitwise
    restored and two further steps are bitwise those of an engine that never entered the context"""
    kw = dict(grad_clip=1e9, ema_decay=0.9, kind=kind)
    net_a, eng_a = make_engine(dev, use_graph, **kw)
    net_b, eng_b = make_engine(dev, use_graph, **kw)
    for s in range(2):
        eng_a.train_step(*_batch(s, dev, kind))
        eng_b.train_step(*_batch(s, dev, kind))
    assert bits(eng_a.flat_p) == bits(eng_b.flat_p)
    x, _, task = _batch(7, dev, kind)
    sd = {k: v.detach().clone() for k, v in eng_a.ema_state_dict().items()}
    live = {k: v.detach().clone() for k, v in net_a.state_dict().items()}
    assert set(sd) == set(live) and any(not torch.equal(sd[k], live[k]) for k in sd)
    names = {id(p): k for k, p in net_a.named_parameters()}
    arena = {names[id(p)] for p in eng_a.arena[0]}
    assert all(torch.equal(sd[k], live[k]) for k in sd if k not in arena), "buffers and parameters without a gradient keep their live values"
    fresh = make_net(kind, dev)
    fresh.load_state_dict(sd)
    p_before, e_before = bits(eng_a.flat_p), bits(eng_a.flat_ema)
    with torch.no_grad():
        want = fresh(x, task)
        with eng_a.ema_weights():
            assert bits(eng_a.flat_p) == e_before and bits(eng_a.flat_ema) == p_before
            got = net_a(x, task)
        assert bits(got) == bits(want)
        assert bits(eng_a.flat_p) == p_before and bits(eng_a.flat_ema) == e_before
        assert bits(net_a(x, task)) != bits(want)
    for s in range(2, 4):
        eng_a.train_step(*_batch(s, dev, kind))
        eng_b.train_step(*_batch(s, dev, kind))
        assert bits(eng_a.flat_p) == bits(eng_b.flat_p) and bits(eng_a.flat_ema) == bits(eng_b.flat_ema), s
