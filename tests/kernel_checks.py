"""Kernel parity checks shared by the CPU-emulator tests (tests/test_emu_kernels.py) and the real
MI355X tests (tests/test_gpu_kernels.py): each check drives the C ABI through mp_hsir_amd.ops on
device `dev` and compares with the fp64 oracle on the same (dtype-rounded) weights."""
import sys

import torch

import guard
import slices
from guard import guarded
from oracle import mp_hsir_oracle as O
from util import params_from_manifest, rel_l2 as _rel

DTYPES = [torch.float32, torch.bfloat16]
# fp32: exact-f32 MFMA / fp32 VALU vs fp64 oracle.  bf16: storage rounding of activations (2^-9 per
# element per stage) -- the reference's own bf16 autocast deviates 1e-2 from its fp32.
TOL = {torch.float32: 2e-6, torch.bfloat16: 1.5e-2, torch.float16: 2e-3}      # fp16: 11-bit significand (2^-11 per rounding)

GEMM_CASES = [(64, 64, 32, False, 0), (128, 96, 96, True, 0), (64, 48, 192, False, 1), (128, 32, 64, True, 1)]
MLP_CASES = [(32, 85), (96, 255), (128, 340)]
WIN_CASES = [
    ("tiny", "encoder_level1.blocks.1.", 1, 4, (1, 16, 24, 32)),
    ("natural_mode0", "encoder_level1.blocks.1.", 2, 4, (2, 16, 16, 64)),
    ("natural_mode0", "refinement.blocks.0.", 2, 0, (1, 8, 16, 128)),
    ("remote_mode8", "encoder_level1.blocks.1.", 2, 4, (1, 16, 8, 96)),
]
SPEC_CASES = [(32, 2, (2, 8, 16), 1), (64, 2, (1, 16, 16), 2), (96, 2, (1, 8, 8), 1), (128, 2, (1, 8, 16), 2)]

_DEV = ["cpu"]


def rel_l2(a, b):
    return _rel(torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu())


# ---- per-slice bounds (tests/slices.py) -----------------------------------------------------------------------------------------
# A whole-tensor rel-L2 under TOL / GTOL lets a wrong channel, halo row, tile or sample through.  `close` asserts the whole-tensor
# bound AND, for every axis and index, slice_err < SLICE_F * tol.  SLICE_F is a property of the statistic and of rounding, not of a
# kernel: SLICE_RATIO_MEASURED is the largest slice_err / rel_l2 of an fp64 oracle field rounded once to fp32 / bf16 / fp16, over the
# shapes of the checks (64x16, 64x32, one window ... 8192x128; the worst are 16-element token rows); tests/test_slices_host.py
# measures it again.  x 1.5 because the accumulated roundings of a real kernel are less even across slices than one rounding.
SLICE_RATIO_MEASURED = 1.56         # fp32 at (3, 40, 24, 32): 2880 token rows of 32 elements; bf16 peaks at 1.51 ((9, 96) and 64x16), fp16 at 1.49
SLICE_F = 2.34                      # 1.5 * SLICE_RATIO_MEASURED
SLICE_F_MAX = 4 * SLICE_F           # no override goes beyond: a slice above it is a kernel defect

# (check function, what) -> (factor, arithmetic cause: about magnitudes, never about position alone).  Read by tests/test_slices_meta.py.
SLICE_OVERRIDES = {
    ("check_gated_mlp_wgrad", "dW1 vs operands"): (
        6.5, "the wgrad kernel recomputes dval / dgate; its fp32 pre-activations differ from the data-gradient kernel's in the last bits, so about 3 "
             "elements per million round to the neighbouring 16-bit value (measured on the MI355X: the worst rows differ from the fp64 product of "
             "the stored operands by exactly +-1 ulp16(d) x LN(x) of ONE token, cosine 1.0000; every other row is at 1.2e-7).  One such element "
             "moves its row by ulp16(d) |LN(x)_t| against a row of sqrt(M) rms(d) rms(LN(x)): fp16 at the M >= 2048 where a million elements "
             "occur, |d| <= 6 rms(d): 2^-10 * 6 / sqrt(2048) = 1.3e-4 = 6.5 tol (seen: 3.2 tol at M = 16384, 2.6 tol at M = 2048)"),
    ("check_gated_mlp_wgrad", "dW2 vs operands"): (
        6.5, "the same for the recomputed h = value * gelu(gate) in dW2 = dm^T h: one h that rounds to the neighbouring 16-bit value moves column j "
             "of dW2 by ulp16(h) x dm of that token against a column of sqrt(M) rms(h) rms(dm): 2^-10 * 6 / sqrt(2048) = 1.3e-4 = 6.5 tol "
             "(seen: 2.8 tol at M = 2048 and M = 4160, fp16)"),
}

# tolerance comparisons of rel_l2 that stay whole-tensor: check function -> (how many, why).  tests/test_slices_meta.py counts them.
SLICE_SKIP = {
    "check_spectral_attention_chain": (2, "the fold launch's reduced Gram / norm partials against the fp64 sum of the same fp32 partials at 3e-7: an ordered "
                                          "sum of a handful of terms, bound at fp32 rounding itself, not a kernel's arithmetic under a 16-bit tolerance"),
    "check_reduce_parts": (1, "ordered sums of partials against their fp64 sum at 3e-7 (and bitwise against the ordered fp32 sum further down)"),
    "check_reduce_block": (6, "sub-blocks of an ordered sum of five partials against the fp64 sum at 3e-7; the untouched columns are compared with 0 exactly"),
    "check_gdfn_fused": (1, "the inequality 'the fused form is no further from fp64 than the three-launch chain': two whole-tensor values compared "
                            "with each other, not a tensor with a tolerance; both tensors pass `close` against the oracle above it"),
}
# comparisons that never went through rel_l2 and stay as they are: bitwise ones (torch.equal), scalars (the L1 loss value, the scaler
# state), exact zeros of padded columns, and the `<=` inequalities between two already-bounded whole-tensor values (ln_bwd_*_dxn,
# spectral_dqkv_bwd, dsa_prologue, check_block's fused-vs-unfused margin)

# Headroom on the MI355X (worst slice_err / tol per check over tests/test_gpu_kernels.py + tests/test_branch_bwd_gpu.py, allowed 2.34):
# wgrad vs operands 3.20 (override 6.5), resamplers 1.29 (fp32 y: the source coordinate's rounding grows with the coordinate), the fp32
# twins 1.02 / 1.15 / 0.64, conv3x3 0.73, fold_bwd 0.61 / 0.30, dwconv_gate_bwd 0.51, dwconv_plain 0.51, gemm_tn 0.50, ln_bwd_tok_dxn
# 0.49, pgsstb_backward_oracle 0.42, fused_pass_a 0.41, gdfn_fused 0.38, spectral chain 0.36, gated_mlp 0.34, win_attn 0.32, every other
# check <= 0.25.  `test_slice_bounds_were_active` prints the table of the run.
SLICE_STATS = {}                    # check function -> [close calls, worst slice_err / tol, where that was]


def slice_report():
    """one line per check: how many tensors went through `close` and the worst slice_err / tol seen (allowed: SLICE_F, or the override)"""
    return ["slices: %-44s %4d comparisons, worst slice_err / tol %.3f at %s" % (name, calls, ratio, at)
            for name, (calls, ratio, at) in sorted(SLICE_STATS.items())]


def _calling_check():
    f = sys._getframe(2)
    first = f.f_code.co_name
    while f is not None:
        if f.f_code.co_name.startswith("check_") or f.f_code.co_name == "run_block":
            return f.f_code.co_name
        f = f.f_back
    return first


def close(got, ref, tol, geom=None, what="", whole=None):
    """assert rel_l2(got, ref) < tol (what the checks always asserted) and slice_err(got, ref, geom) < SLICE_F * tol; geom = (B, H, W)
    views an (M, C) token tensor as (B, H, W, C) so that image rows, image columns and samples are axes of their own.  Returns the
    whole-tensor value (`whole`: that value where the caller has computed it already)."""
    name = _calling_check()
    guard.record(got, "close " + what)           # a no-op unless guard.recording() is active
    g, r = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    if whole is None:
        whole = _rel(g, r)
    w = slices.slice_err(g, r, geom)
    factor = SLICE_OVERRIDES[(name, what)][0] if (name, what) in SLICE_OVERRIDES else SLICE_F
    st = SLICE_STATS.setdefault(name, [0, 0.0, ""])
    st[0] += 1
    if not w.err / tol <= st[1]:
        st[1], st[2] = w.err / tol, "%s: %s" % (what, slices.where(w))
    if (name, what) in _PENDING:                 # a comparison under an input profile (yard_bar): its yardstick, bar and measured error
        prof, dt, yard, bar = _PENDING.pop((name, what))
        key = (name, prof, dt, what)
        if key not in PROFILE_STATS or whole / bar > PROFILE_STATS[key][2] / PROFILE_STATS[key][1]:
            PROFILE_STATS[key] = [yard, bar, whole]          # the case of this key with the worst measured / bar
        print("profile: %s [%s, %s] %s: yardstick %.3g, bar %.3g, measured %.3g (worst slice %.3g, allowed %.3g)" % (
            name, prof, dt, what, yard, bar, whole, w.err, factor * tol))
    assert whole < tol, "%s: whole-tensor rel-L2 %.3g (bound %.3g; worst slice %s: %.3g)" % (what, whole, tol, slices.where(w), w.err)
    assert w.err < factor * tol, "%s: %s: %.3g (whole %.3g; bound %.2f x %.3g)" % (what, slices.where(w), w.err, whole, factor, tol)
    return whole


# ---- input profiles: the checks off the unit Gaussian --------------------------------------------------------------------------------
# Every `rnd` draw is shift + scale N(0, 1): unit-variance zero-mean rows, LayerNorm weights near 1, pre-activations near N(0, 1), logits
# of order 1 -- data on which the LayerNorm epsilon, the GELU clamp, the softmax max-subtraction and the F.normalize clamp change nothing
# that a 16-bit tolerance sees.  A check with an `inputs=` keyword applies one of these to its fresh draws ON THE CPU, before `inp`, so the
# result is a guarded input like any other; "unit" (the default) leaves every draw byte-identical.  All factors are powers of two (exact
# in bf16 and fp16).  A "row" is a token: the last axis is the channel axis, every axis before it counts tokens.
OFFSETS = (-8.0, -4.0, 0.0, 4.0, 8.0)                                    # `offset`: by token index mod 5
FLAT_STD = (1.0, 2.0 ** -4, 2.0 ** -8, 2.0 ** -9, 2.0 ** -12, 0.0)      # `flat`: by token index mod 6 -- variance above, at (2^-8, 2^-9: 1.5e-5, 3.8e-6) and below epsilon, and 0
FLAT_CONST = (-0.5, 0.0, 0.5)                                            # the zero-variance rows are constant at one of these, in turn
INPUT_PROFILES = {
    "unit": "the draw as it is",
    "offset": "N(0, 1) plus a row offset from OFFSETS by token index mod 5 (never combined with `flat`: an fp32 mean of 8 carries 5e-7)",
    "flat": "row standard deviation from FLAT_STD by token index mod 6; the zero rows constant at one of FLAT_CONST: inside every 16-row tile and window",
    "outlier": "channel 5 x 64; the tokens with index mod 17 == 3 x 32.  fp16 draws: x 8 and x 4 -- torch's own fp16 evaluation of the variance squares "
               "x - mean in fp16 and overflows from 256 on (the yardstick came out at 0.24 with 64 and 32: not a test), 32 x 4 sigma = 128 stays below",
    "gain": "gated MLP / GDFN: fc1 / project_in weights x 3 (about a third of the gate pre-activations beyond +-3); the activations stay unit",
    "peaked": "window attention / prompt gate: q and k rows of the qkv weight x 4 (logits x 16); spectral attention: temperature x 8, one k channel "
              "x 2^-10 through its qkv and depthwise rows and, forward only, the qkv row of q channel 0 zeroed (its norm is exactly 0: the 1e-12 "
              "clamp decides); the activations stay unit",
    "saturated": "window attention only: q and k rows of the qkv weight x 8 (logits x 64, up to +-95: exp overflows fp32 from 88.7 on, so the softmax "
                 "stands on its max-subtraction; `peaked` reaches +-24, where dropping the subtraction changes nothing -- found with mutant 4 of DESIGN 4)",
}
ROW_PROFILES = ("offset", "flat", "outlier")          # the ones that reshape the activation rows; `gain` / `peaked` act on weights inside the checks
GAIN = 3.0
YARD_F = 3.0          # bar = max(present tolerance, YARD_F x yardstick): the factor model_checks.block_grad_bars gives the reference's own deviation
YARD_CAP = 4.0        # a case whose bar comes out above YARD_CAP x the present tolerance is not a test: change the profile
PROFILE_STATS = {}    # (check, inputs, dtype, what) -> [yardstick, bar, measured] of the case with the worst measured / bar


OUTLIER = {torch.float16: (8.0, 4.0)}          # (channel factor, token factor); every other dtype: (64, 32)


def apply_profile(t, profile, dtype=torch.float32):
    """the profile applied to a CPU fp32 draw of shape (..., C) that will be stored as `dtype`; "unit", "gain" and "peaked" leave rows alone"""
    assert profile in INPUT_PROFILES, profile
    if profile not in ROW_PROFILES:
        return t
    C = t.shape[-1]
    r = t.reshape(-1, C).clone()
    tok = torch.arange(r.shape[0])
    if profile == "offset":
        r += torch.tensor(OFFSETS)[tok % 5][:, None]
    elif profile == "flat":
        r *= torch.tensor(FLAT_STD)[tok % 6][:, None]
        zero = tok % 6 == 5
        r[zero] = torch.tensor(FLAT_CONST)[(tok[zero] // 6) % 3][:, None].expand(-1, C)
    else:
        fc, ft = OUTLIER.get(dtype, (64.0, 32.0))
        if C > 5:
            r[:, 5] *= fc
        r[tok % 17 == 3] *= ft
    return r.reshape(t.shape)


def rnd(shape, seed, dtype=torch.float32, scale=1.0, shift=0.0, profile="unit", edit=None):
    """a seeded input `shift + scale * N(0, 1)` on the check's device; while a guard is active (tests/guard.py) it lies between NaN bands
    and its CPU master is kept for the bitwise comparison after the check.  Scale and shift are applied here, not by arithmetic on the
    result, so that LayerNorm weights, biases and tables are guarded too.  `profile`: an INPUT_PROFILES entry applied to the draw; `edit`: a
    function that changes the CPU draw in place"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    if shift:
        t = shift + t
    if profile != "unit":
        t = apply_profile(t, profile, dtype)
    if edit is not None:          # a `peaked` case scaling or zeroing rows of a weight: on the CPU draw, in place
        edit(t)
    return inp(t.to(dtype), seed)


def peaked_qkv_edit(C, k_scale, k_channel=3, zero_q0=False, k_row0=None):
    """`peaked` for spectral attention, on a (3C, ...) qkv or depthwise weight draw (k_row0 = 0: a (2C, ...) kv draw of the cross form): the row of
    one k channel scaled, the row of q channel 0 zeroed"""
    def edit(t):
        t[(C if k_row0 is None else k_row0) + k_channel] *= k_scale
        if zero_q0:
            t[0] = 0.0
    return edit


def row_profile(inputs):
    """the profile an activation draw gets under `inputs`"""
    assert inputs in INPUT_PROFILES, inputs
    return inputs if inputs in ROW_PROFILES else "unit"


def yard_bar(inputs, dtype, tol, what, ref, in_dtype, required=True):
    """the bar of one comparison under an input profile: max(tol, YARD_F x yardstick).  The yardstick is the error against fp64 (`ref`, the
    check's own reference) of the ORACLE's expression evaluated by torch on the CPU in the compute dtype (`in_dtype(cast)`, cast taking each
    operand to that dtype: fp32 throughout, or inputs, weights and every op result in the 16-bit type) -- it never touches the code under
    test.  "unit": tol itself, nothing evaluated.  The measured error is printed by `close` beside the yardstick and the bar.
    required=False (one tensor among many of a whole-block check): a bar above the cap returns None -- the caller leaves that tensor out,
    by a figure that comes from torch alone -- where required=True fails the case as "not a test"."""
    if inputs == "unit":
        return tol
    name = _calling_check_of_bar()
    with torch.no_grad():
        got = in_dtype(lambda t: t.detach().cpu().to(dtype))
    yard = _rel(torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu())
    bar = max(tol, YARD_F * yard)
    if not required and not bar <= YARD_CAP * tol:
        print("profile: %s [%s, %s] %s: yardstick %.3g: the bar %.3g would exceed %g x %.3g -- not a test, left out" % (name, inputs, dtype, what, yard, bar, YARD_CAP, tol))
        return None
    _PENDING[(name, what)] = (inputs, str(dtype).replace("torch.", ""), yard, bar)
    assert bar <= YARD_CAP * tol, "%s [%s] %s: torch's own %s evaluation is %.3g from fp64: the bar %.3g would exceed %g x the tolerance %.3g -- not a test" % (
        name, inputs, what, dtype, yard, bar, YARD_CAP, tol)
    return bar


_PENDING = {}


def _calling_check_of_bar():
    f = sys._getframe(2)
    while f is not None:
        if f.f_code.co_name.startswith("check_"):
            return f.f_code.co_name
        f = f.f_back
    return "?"


def profile_report():
    return ["profile: %-32s %-8s %-9s %-28s yardstick %.3g, bar %.3g, measured %.3g" % (k + tuple(v)) for k, v in sorted(PROFILE_STATS.items())]


def inp(t, seed=None):
    """a CPU tensor the check built itself (DropPath factors, index tables, fixture parameters) as a guarded input on the check's device"""
    G = guard.active()
    if G is not None and G.device.type == torch.device(_DEV[0]).type:
        return G.input(t.detach(), seed)
    return t.to(_DEV[0])


as_input = inp          # for a check that has a local of that name


def alloc(shape, dtype=torch.float32, device=None, fill=0, role="output"):
    """a buffer the check itself hands to a kernel (an `out=` target, a padded weight, a partly filled operand): through the active
    guard like everything ops.py allocates.  fill=None: torch.empty (prefilled "never written" under the guard); role "input": a
    buffer the check fills and a kernel only reads (NaN bands)"""
    device = torch.device(device if device is not None else _DEV[0])
    G = guard.active()
    if G is not None and G.device.type == device.type:
        return G.alloc(shape, dtype, device, role, fill=fill)
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=device)
    return torch.full(shape, fill, dtype=dtype, device=device)


def _use(dev):
    _DEV[0] = dev


class tok_form:
    """`with tok_form(f):` runs the token GEMMs in kernel form f (1 = workgroup per tile, 2 = persistent ring form where it applies)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from mp_hsir_amd import ops
        self.prev, ops.TOK_FORM = ops.TOK_FORM, self.form

    def __exit__(self, *exc):
        from mp_hsir_amd import ops
        ops.TOK_FORM = self.prev
        return False


@guarded
def check_gemm_tok_ring(dev, dtype, M, N, K, epi, per_sample=0, ldx=None, ldy=None):
    """the ring form of the token GEMM (persistent workgroups, loader wave + LDS-DMA ring) against the workgroup-per-tile form
    (bitwise: same products, same accumulation order per output) and the fp64 product: plain / residual / branch-sum epilogues,
    per-sample weights, strided input and output views, K tails of 32, N tails, more tiles than workgroups and fewer."""
    _use(dev)
    from mp_hsir_amd import ops
    ldx, ldy = ldx or K, ldy or N
    xw = rnd((M, ldx), 11, dtype)
    x = xw[:, :K]
    w = rnd((per_sample, N, K) if per_sample else (N, K), 12, dtype, K ** -0.5)
    bias = rnd((N,), 13) if epi < 2 else None
    res = rnd((M, N), 14, dtype) if epi else None
    H = W_ = 16
    sa = rnd((M, N), 15, dtype) if epi == 2 else None
    gate = rnd((M // 64, N), 16) if epi == 2 else None
    keep = (rnd((M // (H * W_),), 17, scale=0.25, shift=1.0)) if epi == 2 else None
    outs = []
    for form in (1, 2):
        yw = alloc((M, ldy), dtype)
        with tok_form(form):
            ops.gemm_tok(x, w, bias=bias, epi=epi, res=res, sa=sa, gate=gate, keep=keep, geom=(H, W_, 4) if epi == 2 else None, out=yw[:, :N])
        outs.append(yw)
    assert torch.equal(outs[0].cpu(), outs[1].cpu()), rel_l2(outs[1], outs[0].double().cpu())
    if epi < 2:
        wd = w.double().cpu()
        xd = x.double().cpu()
        acc = torch.einsum("bnk,bck->bnc", xd.reshape(per_sample, M // per_sample, K), wd).reshape(M, N) if per_sample else xd @ wd.t()
        ref = acc + bias.double().cpu() + (res.double().cpu() if epi else 0)
        close(outs[1][:, :N], ref, TOL[dtype], what="y")
        if ldy > N:
            assert float(outs[1][:, N:].abs().max()) == 0.0


@guarded
def check_gemm_tok(dev, dtype, M, N, K, ln, epi, inputs="unit"):
    _use(dev)
    from mp_hsir_amd import ops
    x, w = rnd((M, K), 1, dtype, profile=row_profile(inputs)), rnd((N, K), 2, dtype, K ** -0.5)
    bias = rnd((N,), 3)
    lnw, lnb = rnd((K,), 4, scale=0.1, shift=1), rnd((K,), 5, scale=0.1)
    res = rnd((M, N), 6, dtype)
    y = ops.gemm_tok(x, w, bias=bias, ln=(lnw, lnb) if ln else None, epi=epi, res=res if epi else None)
    xd = x.double().cpu()
    if ln:
        xd = O.layer_norm_c(xd, lnw.double().cpu(), lnb.double().cpu())
        if dtype != torch.float32:
            xd = xd.to(dtype).double().cpu()
    ref = xd @ w.double().cpu().t() + bias.double().cpu() + (res.double().cpu() if epi else 0)
    tol = yard_bar(inputs, dtype, TOL[dtype], "y", ref, lambda c: (O.layer_norm_c(c(x), c(lnw), c(lnb)) if ln else c(x)) @ c(w).t() + c(bias) + (c(res) if epi else 0))
    close(y, ref, tol, what="y")


@guarded
def check_gemm_tok_per_sample_combine(dev, dtype):
    """epi 2 with a per-sample weight: the folded channel attention + PGSSTB branch sum."""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W, C, shift = 2, 16, 16, 32, 4
    M = B * H * W
    v, Wb = rnd((M, C), 1, dtype), rnd((B, C, C), 2, dtype, C ** -0.5)
    res, sa = rnd((M, C), 3, dtype), rnd((M, C), 4, dtype)
    gate = rnd((B * (H // 8) * (W // 8), C), 5)
    keep = inp(torch.tensor([1.25, 0.0]))
    y = ops.gemm_tok(v, Wb, epi=2, res=res, sa=sa, gate=gate, keep=keep, geom=(H, W, shift))
    acc = torch.einsum("bnk,bck->bnc", v.double().cpu().reshape(B, H * W, C), Wb.double().cpu()).reshape(B, H, W, C)
    # gate lives in the shifted window frame: expand to windows, un-window, roll back
    gw = gate.double().cpu()[:, None, :].expand(-1, 64, -1)
    gimg = torch.roll(O.from_windows(gw, B, H, W), shifts=(shift, shift), dims=(1, 2))
    ref = res.double().cpu().reshape(B, H, W, C) + keep.double().cpu().reshape(B, 1, 1, 1) * (sa.double().cpu().reshape(B, H, W, C) * gimg + acc)
    close(y.reshape(B, H, W, C), ref, TOL[dtype], geom=(B, H, W), what="y")


@guarded
def check_gated_mlp(dev, dtype, C, hid, tpw=0, M=128, hsplit=None, res=False, inputs="unit"):
    _use(dev)
    from mp_hsir_amd import ops
    x = rnd((M, C), 1, dtype, profile=row_profile(inputs))
    r2 = rnd((M, C + 8), 8, dtype)[:, :C] if res else None          # second residual (BaseBlock skip), a strided view
    P = {"fc1.weight": rnd((2 * hid, C), 2, scale=C ** -0.5 * (GAIN if inputs == "gain" else 1.0)), "fc1.bias": rnd((2 * hid,), 3, scale=0.1),
         "fc2.weight": rnd((C, hid), 4, scale=hid ** -0.5), "fc2.bias": rnd((C,), 5, scale=0.1)}
    lnw, lnb = rnd((C,), 6, scale=0.1, shift=1), rnd((C,), 7, scale=0.1)
    keep = inp(torch.tensor([1.0, 1.5]))
    W1, b1, W2 = ops.pack_gated_mlp(P["fc1.weight"], P["fc1.bias"], P["fc2.weight"], dtype)
    y = ops.gated_mlp_fwd(x, lnw, lnb, W1, b1, W2, P["fc2.bias"], keep=keep, rows_per_batch=M // 2, tiles_per_wave=tpw, hsplit=hsplit, res=r2)
    Pd = {k: (v.to(dtype) if k.endswith("weight") else v).double().cpu() for k, v in P.items()}
    xn = O.layer_norm_c(x.double().cpu(), lnw.double().cpu(), lnb.double().cpu())
    ref = x.double().cpu() + keep.double().cpu().repeat_interleave(M // 2)[:, None] * O.gated_mlp(Pd, "", xn)
    if res:
        ref = ref + r2.double().cpu()
        if dtype == torch.float32:      # (x + keep mlp) + res in that order: bitwise what the separate add of the unfused path gives
            y0 = ops.gated_mlp_fwd(x, lnw, lnb, W1, b1, W2, P["fc2.bias"], keep=keep, rows_per_batch=M // 2, tiles_per_wave=tpw, hsplit=hsplit)
            assert torch.equal((y0 + r2).cpu(), y.cpu())
    tol = yard_bar(inputs, dtype, TOL[dtype], "y", ref, lambda c: c(x) + c(keep).repeat_interleave(M // 2)[:, None] * O.gated_mlp(
        {k: c(v) for k, v in P.items()}, "", O.layer_norm_c(c(x), c(lnw), c(lnb))) + (c(r2) if res else 0))
    close(y, ref, tol, geom=(2, M // 2, 1), what="y")         # two samples of M // 2 tokens, each with its own DropPath factor


@guarded
def check_gated_mlp_branch_sum(dev, dtype, C, hid, B=2, H=8, W=16, shift=0, keep=True, want_y=True, res=False):
    """mphsir_gated_mlp_fwd with PV (the block's branch sum formed inside the launch) against the two launches it replaces
    (gemm_tok epi 2, then the plain gated MLP in the same kernel form): the same arithmetic in the same order -> bitwise equal."""
    _use(dev)
    from mp_hsir_amd import ops
    M = B * H * W
    x = rnd((M, C), 1, dtype)
    v = rnd((M, 3 * C), 11, dtype)[:, 2 * C:]                        # a strided view, as pass A hands it over
    sa = rnd((M, C), 12, dtype)
    Mb = rnd((B, C, C), 13, scale=C ** -0.5).to(dtype)
    gate = rnd((B * (H * W // 64), C), 14)
    k1 = inp(torch.tensor(([1.0, 1.25, 0.0, 1.5] * B)[:B])) if keep else None
    k2 = inp(torch.tensor(([1.5, 1.0, 1.25, 0.0] * B)[:B])) if keep else None
    r2 = rnd((M, C + 8), 8, dtype)[:, :C] if res else None
    fc1w, fc1b = rnd((2 * hid, C), 2, scale=C ** -0.5), rnd((2 * hid,), 3, scale=0.1)
    fc2w, fc2b = rnd((C, hid), 4, scale=hid ** -0.5), rnd((C,), 5, scale=0.1)
    lnw, lnb = rnd((C,), 6, scale=0.1, shift=1), rnd((C,), 7, scale=0.1)
    W1, b1, W2 = ops.pack_gated_mlp(fc1w, fc1b, fc2w, dtype)
    y0 = ops.gemm_tok(v, Mb, epi=2, res=x, sa=sa, gate=gate, keep=k1, geom=(H, W, shift))
    z0 = ops.gated_mlp_fwd(y0, lnw, lnb, W1, b1, W2, fc2b, keep=k2, rows_per_batch=H * W, tiles_per_wave=3, res=r2)
    z1, y1 = ops.gated_mlp_fwd(x, lnw, lnb, W1, b1, W2, fc2b, keep=k2, rows_per_batch=H * W, res=r2,
                               branch=dict(v=v, Mb=Mb, sa=sa, gate=gate, keep=k1, geom=(H, W, shift), want_y=want_y))
    assert (y1 is not None) == want_y
    if want_y:
        assert torch.equal(y0.cpu(), y1.cpu()), rel_l2(y1, y0.double().cpu())
    assert torch.equal(z0.cpu(), z1.cpu()), rel_l2(z1, z0.double().cpu())


# ---- fp32 twins of the forms that exist in 16 bits only (round-3 review, weak point 13) ------------------------------------------
# The oracle comparisons above allow TOL[bf16] = 1.5e-2: wide enough for a wrong small term.  Here the SAME operation runs through the
# fp32 kernels on the 16-bit-rounded inputs and weights, so that what is left is the 16-bit rounding of the stored intermediates and
# of the output (bf16: 2^-9 per rounding): the bounds are ~3x tighter.
TWIN = {torch.bfloat16: 4e-3, torch.float16: 5e-4}      # measured: 1.1e-3 ... 2.6e-3 / 1.4e-4 ... 3.2e-4


@guarded
def check_gated_mlp_fp32_twin(dev, dtype, C=128, hid=340, M=1024, tpw=3, hsplit=None):
    _use(dev)
    from mp_hsir_amd import ops
    x = rnd((M, C), 1, dtype)
    fc1w, fc1b = rnd((2 * hid, C), 2, scale=C ** -0.5), rnd((2 * hid,), 3, scale=0.1)
    fc2w, fc2b = rnd((C, hid), 4, scale=hid ** -0.5), rnd((C,), 5, scale=0.1)
    lnw, lnb = rnd((C,), 6, scale=0.1, shift=1), rnd((C,), 7, scale=0.1)
    W1, b1, W2 = ops.pack_gated_mlp(fc1w, fc1b, fc2w, dtype)
    y = ops.gated_mlp_fwd(x, lnw, lnb, W1, b1, W2, fc2b, tiles_per_wave=tpw, hsplit=hsplit)
    W1f, b1f, W2f = ops.pack_gated_mlp(fc1w.to(dtype).float(), fc1b, fc2w.to(dtype).float(), torch.float32)
    y32 = ops.gated_mlp_fwd(x.float(), lnw, lnb, W1f, b1f, W2f, fc2b)
    return close(y, y32, TWIN[dtype], what="y")


@guarded
def check_pass_a_rows_fp32_twin(dev, dtype, C=64, heads=2, shape=(1, 32, 64), row_segments=2):
    """the row-walking fused pass A (16-bit only) against gemm_tok -> dwconv_gram in fp32 on the rounded inputs: v and the summed
    Gram / norm partials"""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    assert ops.qkv_dwconv_gram_rows_fits(C, heads, H, W, dtype, False)
    x = rnd((B, H, W, C), 61, dtype)
    wq = rnd((3 * C, C), 62, scale=C ** -0.5).to(dtype).contiguous()
    w9 = ops.pack_dw(rnd((3 * C, 1, 3, 3), 63, scale=1 / 3))
    x2 = x.reshape(-1, C)
    v, gp, sp, _ = ops.qkv_dwconv_gram(x2, wq, w9, B, H, W, C, heads, row_segments=row_segments, nsplit=(W // 32) * row_segments)
    t = ops.gemm_tok(x2.float(), wq.float())
    v0, gp0, sp0, _ = ops.dwconv_gram(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], w9[:, :C], w9[:, C:2 * C], w9[:, 2 * C:], 3 * C, B, H, W, C, heads)
    ev = close(v, v0, TWIN[dtype], geom=(B, H, W), what="v")
    eg = close(gp.double().sum(1), gp0.double().sum(1), 2 * TWIN[dtype], geom=(B, H, W), what="gram")
    es = close(sp.double().sum(1), sp0.double().sum(1), 2 * TWIN[dtype], geom=(B, H, W), what="norms")
    return ev, eg, es


@guarded
def check_gdfn_fused_fp32_twin(dev, dtype, D=64, hid=170, shape=(1, 16, 32)):
    """the fused GDFN (16-bit only) against the three-launch chain in fp32 on the rounded inputs and weights"""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    HP = ops.round_up(hid, 32)
    assert ops.gdfn_fused_fits(D, HP, H, W, dtype)
    x = rnd((B, H, W, D), 41, dtype)
    wi, wd, wo = rnd((2 * hid, D), 42, scale=D ** -0.5), rnd((2 * hid, 1, 3, 3), 43, scale=1 / 3), rnd((D, hid), 44, scale=hid ** -0.5)
    lnw, lnb = rnd((D,), 45, scale=0.1, shift=1), rnd((D,), 46, scale=0.1)
    w_in = alloc((2 * HP, D), dtype, role="input")
    w_in[:hid], w_in[HP:HP + hid] = wi[:hid].to(dtype), wi[hid:].to(dtype)
    w9 = alloc((9, 2 * HP), role="input")
    w9s = ops.pack_dw(wd)
    w9[:, :hid], w9[:, HP:HP + hid] = w9s[:, :hid], w9s[:, hid:]
    w_out = alloc((D, HP), dtype, role="input")
    w_out[:, :hid] = wo.to(dtype)
    x2 = x.reshape(-1, D)
    y = ops.gdfn_fused(x2, (lnw, lnb), w_in, w9, w_out, B, H, W)
    t = ops.gemm_tok(x2.float(), w_in.float(), ln=(lnw, lnb))
    y32 = ops.gemm_tok(ops.dwconv_gate(t, w9, B, H, W), w_out.float(), epi=1, res=x2.float())
    return close(y, y32, TWIN[dtype], geom=(B, H, W), what="y")


def _block_params(manifest_entry, prefix):
    return {k: inp(v) for k, v in params_from_manifest(manifest_entry, prefix, dtype=torch.float32).items()}


@guarded
def check_win_attn(dev, dtype, man, prefix, heads, shift, shape, manifest, inputs="unit"):
    _use(dev)
    from mp_hsir_amd import ops
    P = _block_params(manifest[man], prefix)
    B, H, W, C = shape
    assert inputs in ("unit", "flat", "peaked", "saturated")
    if inputs in ("peaked", "saturated"):          # q and k rows of the qkv weight x 4: logits x 16; x 8: logits x 64
        wpk = P["attn.qkv.weight"].detach().cpu().clone()
        wpk[:2 * C] *= 4.0 if inputs == "peaked" else 8.0
        P["attn.qkv.weight"] = inp(wpk)
    x = rnd(shape, 11, dtype, profile=row_profile(inputs))
    wq = P["attn.qkv.weight"].to(dtype)
    wp = P["attn.proj.weight"].to(dtype)
    pg = {k[len("local_spectral_attn."):]: v.contiguous() for k, v in P.items() if k.startswith("local_spectral_attn.")}
    pg["prompt_param"] = pg["prompt_param"].reshape(128, -1).contiguous()
    sa, gate = ops.win_attn_fwd(x, P["norm1.weight"], P["norm1.bias"], wq, P["attn.qkv.bias"],
                                P["attn.relative_position_bias_table"], ops.pack_win_proj(P["attn.proj.weight"], heads, dtype),
                                P["attn.proj.bias"], pg, heads, shift)
    # oracle on the same (dtype-rounded) weights, fp64 arithmetic
    Pd = {k: v.double().cpu() for k, v in P.items()}
    Pd["attn.qkv.weight"], Pd["attn.proj.weight"] = wq.double().cpu(), wp.double().cpu()
    xn = O.layer_norm_c(x.double().cpu(), Pd["norm1.weight"], Pd["norm1.bias"])
    if shift:
        xn = torch.roll(xn, (-4, -4), (1, 2))
    mask = O.shift_mask(H, W, torch.float64) if shift else None
    saw = O.spatial_attention(Pd, "attn.", O.to_windows(xn), heads, mask)
    g_ref = O.pg_spectral_gate(Pd, "local_spectral_attn.", saw)
    sa_ref = O.from_windows(saw, B, H, W)
    if shift:
        sa_ref = torch.roll(sa_ref, (4, 4), (1, 2))
    own = {}

    def in_dtype(what):
        def f(c):
            if not own:
                Pc = {k: c(v) for k, v in Pd.items()}
                xc = O.layer_norm_c(c(x), Pc["norm1.weight"], Pc["norm1.bias"])
                if shift:
                    xc = torch.roll(xc, (-4, -4), (1, 2))
                sw = O.spatial_attention(Pc, "attn.", O.to_windows(xc), heads, c(mask) if shift else None)
                own["gate"] = O.pg_spectral_gate(Pc, "local_spectral_attn.", sw)
                own["sa"] = O.from_windows(sw, B, H, W)
                if shift:
                    own["sa"] = torch.roll(own["sa"], (4, 4), (1, 2))
            return own[what]
        return f
    close(sa, sa_ref, yard_bar(inputs, dtype, TOL[dtype] * (2 if dtype != torch.float32 else 1), "sa", sa_ref, in_dtype("sa")), geom=(B, H, W), what="sa")
    close(gate, g_ref, yard_bar(inputs, dtype, TOL[dtype] * (4 if dtype != torch.float32 else 1), "gate", g_ref, in_dtype("gate")), geom=(B, H, W), what="gate")        # window-major: one row per window


@guarded
def check_spectral_attention_chain(dev, dtype, C, heads, shape, nsplit, inputs="unit"):
    """gemm_tok (1x1 qkv) -> dwconv_gram -> spectral_fold -> gemm_tok (per-sample M) == oracle spectral_attention"""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    x = rnd((B, H, W, C), 21, dtype)
    pk = inputs == "peaked"          # temperature x 8; k channel 3 x 2^-10 (2^-5 in its qkv row, 2^-5 in its depthwise row); q channel 0 exactly 0
    assert inputs in ("unit", "peaked")
    P = {"qkv.weight": rnd((3 * C, C, 1, 1), 22, scale=C ** -0.5, edit=peaked_qkv_edit(C, 2.0 ** -5, zero_q0=True) if pk else None),
         "qkv_dwconv.weight": rnd((3 * C, 1, 3, 3), 23, scale=1 / 3, edit=peaked_qkv_edit(C, 2.0 ** -5) if pk else None),
         "project_out.weight": rnd((C, C, 1, 1), 24, scale=C ** -0.5), "temperature": rnd((heads, 1, 1), 25, scale=0.3 * (8 if pk else 1), shift=8 if pk else 1)}
    wqkv = P["qkv.weight"].reshape(3 * C, C).to(dtype)
    t = ops.gemm_tok(x.reshape(-1, C), wqkv)
    w9 = ops.pack_dw(P["qkv_dwconv.weight"])
    v, gp, sp, ns = ops.dwconv_gram(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], w9[:, :C], w9[:, C:2 * C], w9[:, 2 * C:],
                                    3 * C, B, H, W, C, heads, nsplit=nsplit)
    Mb = ops.spectral_fold(gp, sp, P["temperature"].reshape(heads).contiguous(),
                           P["project_out.weight"].reshape(C, C).contiguous(), dtype)
    y = ops.gemm_tok(v, Mb)
    # training form: also M^T and the reduced partials (what the backward kernel reads)
    Mb2, MbT, gsum, ssum = ops.spectral_fold(gp, sp, P["temperature"].reshape(heads).contiguous(),
                                             P["project_out.weight"].reshape(C, C).contiguous(), dtype, transposed=True)
    assert torch.equal(Mb2.cpu(), Mb.cpu()) and torch.equal(MbT.cpu(), Mb.transpose(1, 2).cpu())
    assert rel_l2(gsum[:, 0], gp.double().sum(1)) < 3e-7 and rel_l2(ssum[:, 0], sp.double().sum(1)) < 3e-7
    Pd = {k: v_.double().cpu() for k, v_ in P.items()}
    Pd["qkv.weight"] = wqkv.double().cpu().reshape(3 * C, C, 1, 1)
    ref = O.spectral_attention(Pd, "", x.double().cpu(), heads)
    if pk:          # the clamp of F.normalize decides q channel 0: its norm partials are exactly 0, and it is a row of zeros in M's softmax input
        assert float(sp.double().sum(1)[:, 0, 0].abs().max()) == 0.0, "q channel 0 is not exactly zero: the profile does not reach the 1e-12 clamp"
    tol = yard_bar(inputs, dtype, TOL[dtype] * (2 if dtype != torch.float32 else 1), "y", ref, lambda c: O.spectral_attention({k: c(v_) for k, v_ in Pd.items()}, "", c(x), heads))
    close(y.reshape(B, H, W, C), ref, tol, geom=(B, H, W), what="y")


FUSED_CASES = [(32, 1, (1, 8, 16), 1, False), (32, 2, (2, 16, 32), 2, True), (64, 2, (1, 24, 32), 3, False), (64, 4, (1, 16, 16), 1, True)]
# (…, head_groups): 1 = all heads in one workgroup, g > 1 = heads split over g workgroups per tile set
# heads wider than one channel slab (two slabs of 32 per head): 16-bit only
FUSED_SLAB_CASES = [(64, 1, (1, 16, 32), 2, False), (64, 1, (1, 8, 16), 1, True)]
FUSED_HG_CASES = [(64, 4, (1, 16, 32), 2, False, 1), (64, 4, (1, 16, 32), 2, True, 2), (64, 4, (1, 8, 16), 1, False, 4)]


# the row-walking form (spectral_rows.hip): (C, heads, (B, H, W), row segments per strip, ln); W % 32 == 0, 16-bit
ROWS_CASES = [(64, 2, (1, 8, 32), 1, False), (64, 2, (2, 16, 64), 2, False), (128, 4, (1, 8, 32), 2, False), (128, 2, (1, 12, 32), 1, False),
              (64, 1, (1, 8, 64), 2, False), (96, 2, (1, 8, 32), 1, False), (192, 4, (1, 4, 32), 1, False),
              (64, 2, (1, 24, 96), 2, False),
              # with the LayerNorm prologue (the `Attention` of PromptFusion: 32-wide heads): rows normalised in place in the ring
              (64, 2, (1, 8, 32), 1, True), (128, 4, (1, 12, 64), 1, True), (128, 4, (2, 8, 32), 2, True),
              # C = 256 (the latent level, fusion2's Attention): four-slot ring, four head groups per strip
              (256, 8, (1, 8, 32), 1, False), (256, 8, (1, 12, 32), 2, True)]


# larger ones for the GPU only: the widths / resolutions of both nets' levels 1-2 at 64x64 and 128x128 inputs
ROWS_CASES_GPU = [(64, 2, (2, 64, 64), 4, False), (128, 4, (2, 32, 32), 2, False), (128, 2, (2, 64, 64), 8, False), (128, 4, (1, 64, 64), 1, False),
                  (96, 2, (2, 64, 64), 2, False), (192, 4, (2, 32, 32), 4, False), (64, 2, (1, 128, 128), 8, False),
                  (128, 4, (2, 64, 64), 4, True), (128, 4, (1, 128, 128), 8, True), (64, 2, (2, 64, 64), 2, True),
                  (256, 8, (1, 128, 128), 8, False), (256, 8, (2, 32, 32), 2, False), (256, 8, (1, 64, 64), 4, True)]


@guarded
def check_fused_pass_a(dev, dtype, C, heads, shape, nsplit, ln, hgroups=None, row_segments=0, inputs="unit"):
    """qkv_dwconv_gram (LN + 1x1 qkv + depthwise 3x3 + Gram / norms in one launch) == gemm_tok -> dwconv_gram, and the
    chain through spectral_fold / pass B == oracle spectral_attention (ref :96-114; with ln: norm1 of :476 first)."""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    if row_segments:
        assert ops.qkv_dwconv_gram_rows_fits(C, heads, H, W, dtype, ln)
        nsplit = (W // 32) * row_segments
    else:
        assert ops.qkv_dwconv_gram_fits(C, heads, H, W, dtype)
    x = rnd((B, H, W, C), 61, dtype, profile=row_profile(inputs))
    P = {"qkv.weight": rnd((3 * C, C, 1, 1), 62, scale=C ** -0.5), "qkv_dwconv.weight": rnd((3 * C, 1, 3, 3), 63, scale=1 / 3),
         "project_out.weight": rnd((C, C, 1, 1), 64, scale=C ** -0.5), "temperature": rnd((heads, 1, 1), 65, scale=0.3, shift=1)}
    lnp = (rnd((C,), 66, scale=0.2, shift=1), rnd((C,), 67, scale=0.1)) if ln else None
    wqkv = P["qkv.weight"].reshape(3 * C, C).to(dtype).contiguous()
    w9 = ops.pack_dw(P["qkv_dwconv.weight"])
    x2 = x.reshape(-1, C)
    v, gp, sp, ns = ops.qkv_dwconv_gram(x2, wqkv, w9, B, H, W, C, heads, ln=lnp, nsplit=nsplit, head_groups=hgroups, row_segments=row_segments)
    assert gp.shape == (B, nsplit, heads, C // heads, C // heads) and sp.shape == (B, nsplit, 2, C)
    # the two-kernel path on the same inputs: same rounding points (t and q,k,v in the compute dtype), different
    # accumulation order in the 1x1 conv only
    t = ops.gemm_tok(x2, wqkv, ln=lnp)
    v0, gp0, sp0, _ = ops.dwconv_gram(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], w9[:, :C], w9[:, C:2 * C], w9[:, 2 * C:], 3 * C, B, H, W, C, heads)
    tol = TOL[dtype]
    close(v, v0, tol, geom=(B, H, W), what="v")
    close(gp.double().sum(1), gp0.double().sum(1), tol, geom=(B, H, W), what="gram")
    close(sp.double().sum(1), sp0.double().sum(1), tol, geom=(B, H, W), what="norms")
    # training form: the same launch also keeps t and q|k; v and the partials must not change (bitwise)
    v2, gp2, sp2, _, tk, qk = ops.qkv_dwconv_gram(x2, wqkv, w9, B, H, W, C, heads, ln=lnp, nsplit=nsplit, head_groups=hgroups, keep=True,
                                                  row_segments=row_segments)
    assert torch.equal(v2.cpu(), v.cpu()) and torch.equal(gp2.cpu(), gp.cpu()) and torch.equal(sp2.cpu(), sp.cpu())
    close(tk, t, tol, geom=(B, H, W), what="t")
    _, _, _, _, qk0 = ops.dwconv_gram(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], w9[:, :C], w9[:, C:2 * C], w9[:, 2 * C:], 3 * C, B, H, W, C, heads,
                                      keep_qk=True)
    if qk0 is not None:
        close(qk, qk0, tol, geom=(B, H, W), what="qk")
    temp, wo = P["temperature"].reshape(heads).contiguous(), P["project_out.weight"].reshape(C, C).contiguous()
    y = ops.gemm_tok(v, ops.spectral_fold(gp, sp, temp, wo, dtype))
    Pd = {k: v_.double().cpu() for k, v_ in P.items()}
    Pd["qkv.weight"] = wqkv.double().cpu().reshape(3 * C, C, 1, 1)
    xin = x.double().cpu()
    if ln:
        xin = torch.nn.functional.layer_norm(xin, (C,), lnp[0].double().cpu(), lnp[1].double().cpu(), 1e-5)
    ref = O.spectral_attention(Pd, "", xin, heads)
    ytol = yard_bar(inputs, dtype, tol * (2 if dtype != torch.float32 else 1), "y", ref, lambda c: O.spectral_attention(
        {k: c(v_) for k, v_ in Pd.items()}, "", O.layer_norm_c(c(x), c(lnp[0]), c(lnp[1])) if ln else c(x), heads))
    close(y.reshape(B, H, W, C), ref, ytol, geom=(B, H, W), what="y")


@guarded
def check_gdfn_chain(dev, dtype):
    """gemm_tok(LN + project_in) -> dwconv_gate -> gemm_tok(project_out + residual) == x + gdfn(LN(x))"""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W, C, hid = 1, 8, 16, 64, 170
    HP = ops.round_up(hid, 32)
    x = rnd((B, H, W, C), 31, dtype)
    P = {"project_in.weight": rnd((2 * hid, C, 1, 1), 32, scale=C ** -0.5), "dwconv.weight": rnd((2 * hid, 1, 3, 3), 33, scale=1 / 3),
         "project_out.weight": rnd((C, hid, 1, 1), 34, scale=hid ** -0.5)}
    lnw, lnb = rnd((C,), 35, scale=0.1, shift=1), rnd((C,), 36, scale=0.1)
    w_in = alloc((2 * HP, C), dtype, role="input")
    w_in[:hid], w_in[HP:HP + hid] = P["project_in.weight"].reshape(2 * hid, C)[:hid].to(dtype), P["project_in.weight"].reshape(2 * hid, C)[hid:].to(dtype)
    w9 = alloc((9, 2 * HP), role="input")
    w9s = ops.pack_dw(P["dwconv.weight"])
    w9[:, :hid], w9[:, HP:HP + hid] = w9s[:, :hid], w9s[:, hid:]
    w_out = alloc((C, HP), dtype, role="input")
    w_out[:, :hid] = P["project_out.weight"].reshape(C, hid).to(dtype)
    x2 = x.reshape(-1, C)
    t = ops.gemm_tok(x2, w_in, ln=(lnw, lnb))
    u = ops.dwconv_gate(t, w9, B, H, W)
    y = ops.gemm_tok(u, w_out, epi=1, res=x2)
    Pd = {"project_in.weight": P["project_in.weight"].to(dtype).double().cpu(), "dwconv.weight": P["dwconv.weight"].double().cpu(),
          "project_out.weight": P["project_out.weight"].to(dtype).double().cpu()}
    ref = x.double().cpu() + O.gdfn(Pd, "", O.layer_norm_c(x.double().cpu(), lnw.double().cpu(), lnb.double().cpu()))
    close(y.reshape(B, H, W, C), ref, TOL[dtype] * (2 if dtype != torch.float32 else 1), geom=(B, H, W), what="y")


GDFN_FUSED_CASES = [(64, 170, (1, 8, 16), None), (64, 170, (2, 16, 32), 2), (128, 340, (1, 16, 16), 1), (192, 510, (1, 8, 16), None),
                    (256, 680, (1, 16, 16), 2)]
GDFN_FUSED_CASES_GPU = [(128, 340, (1, 64, 64), None), (256, 680, (2, 32, 32), None), (192, 510, (1, 32, 48), None), (64, 170, (2, 64, 64), None)]


@guarded
def check_gdfn_fused(dev, dtype, D, hid, shape, nsplit, inputs="unit"):
    """mphsir_gdfn_fused == x + gdfn(LN(x)) (oracle, fp64) and == the three-launch chain gemm_tok -> dwconv_gate -> gemm_tok
    (which rounds t to the storage type between the 1x1 and the depthwise conv; the fused kernel keeps it in fp32)."""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    HP = ops.round_up(hid, 32)
    assert ops.gdfn_fused_fits(D, HP, H, W, dtype)
    x = rnd((B, H, W, D), 41, dtype, profile=row_profile(inputs))
    P = {"project_in.weight": rnd((2 * hid, D, 1, 1), 42, scale=D ** -0.5 * (GAIN if inputs == "gain" else 1.0)), "dwconv.weight": rnd((2 * hid, 1, 3, 3), 43, scale=1 / 3),
         "project_out.weight": rnd((D, hid, 1, 1), 44, scale=hid ** -0.5)}
    lnw, lnb = rnd((D,), 45, scale=0.1, shift=1), rnd((D,), 46, scale=0.1)
    w_in = alloc((2 * HP, D), dtype, role="input")
    wi = P["project_in.weight"].reshape(2 * hid, D)
    w_in[:hid], w_in[HP:HP + hid] = wi[:hid].to(dtype), wi[hid:].to(dtype)
    w9 = alloc((9, 2 * HP), role="input")
    w9s = ops.pack_dw(P["dwconv.weight"])
    w9[:, :hid], w9[:, HP:HP + hid] = w9s[:, :hid], w9s[:, hid:]
    w_out = alloc((D, HP), dtype, role="input")
    w_out[:, :hid] = P["project_out.weight"].reshape(D, hid).to(dtype)
    x2 = x.reshape(-1, D)
    y = ops.gdfn_fused(x2, (lnw, lnb), w_in, w9, w_out, B, H, W, nsplit=nsplit)
    t = ops.gemm_tok(x2, w_in, ln=(lnw, lnb))
    y3 = ops.gemm_tok(ops.dwconv_gate(t, w9, B, H, W), w_out, epi=1, res=x2)
    Pd = {"project_in.weight": P["project_in.weight"].to(dtype).double().cpu(), "dwconv.weight": P["dwconv.weight"].double().cpu(),
          "project_out.weight": P["project_out.weight"].to(dtype).double().cpu()}
    ref = x.double().cpu() + O.gdfn(Pd, "", O.layer_norm_c(x.double().cpu(), lnw.double().cpu(), lnb.double().cpu()))
    tol = yard_bar(inputs, dtype, TOL[dtype] * 2, "y", ref, lambda c: c(x) + O.gdfn({k: c(v) for k, v in P.items()}, "", O.layer_norm_c(c(x), c(lnw), c(lnb))))
    close(y.reshape(B, H, W, D), ref, tol, geom=(B, H, W), what="y")
    close(y, y3, TOL[dtype] * 2, geom=(B, H, W), what="y vs chain")          # kernel against kernel: the yardstick against fp64 has no say here
    # the fused form is the more accurate of the two (no rounding of t)
    assert rel_l2(y.reshape(B, H, W, D), ref) <= rel_l2(y3.reshape(B, H, W, D), ref) * 1.05 + 1e-6
    # training form: the same y (bitwise) plus t = project_in(LN(x)) as the three-launch chain's first GEMM writes it
    yk, tk = ops.gdfn_fused(x2, (lnw, lnb), w_in, w9, w_out, B, H, W, nsplit=nsplit, keep=True)
    assert torch.equal(yk, y)
    assert tk.shape == t.shape
    close(tk, t, TOL[dtype] * 0.5, geom=(B, H, W), what="t")
    assert float((tk.float() - t.float()).abs().max()) <= float(t.float().abs().max()) * 2.0 ** -7


@guarded
def check_dwconv_gate_bwd(dev, dtype, shape=(2, 16, 32), hid=85):
    """dwconv_gate_bwd (depthwise conv recomputed inside the gate backward) vs fp64 autograd of u = gelu(dw(t)[:hid]) * dw(t)[hid:],
    and vs the two launches dwconv3x3 -> gdfn_gate_bwd (which round the conv output to the storage type in between)."""
    _use(dev)
    import torch.nn.functional as F
    from mp_hsir_amd import ops
    B, H, W = shape
    HP = ops.round_up(hid, 32)
    M = B * H * W
    t = alloc((M, 2 * HP), dtype, role="input")
    tv = rnd((M, 2 * hid), 81, dtype)
    t[:, :hid], t[:, HP:HP + hid] = tv[:, :hid], tv[:, hid:]
    du = alloc((M, HP), dtype, role="input")
    du[:, :hid] = rnd((M, hid), 82, dtype)
    w = rnd((2 * hid, 1, 3, 3), 83, scale=1 / 3)
    w9 = alloc((9, 2 * HP), role="input")
    w9s = ops.pack_dw(w)
    w9[:, :hid], w9[:, HP:HP + hid] = w9s[:, :hid], w9s[:, hid:]
    u, dtd = ops.dwconv_gate_bwd(t, w9, du, B, H, W)
    u2, dtd2 = ops.gdfn_gate_bwd(ops.dwconv3x3(t.reshape(B, H, W, 2 * HP), w9).reshape(M, 2 * HP), du)
    tr = tv.double().cpu().reshape(B, H, W, 2 * hid).permute(0, 3, 1, 2)
    xr = F.conv2d(tr, w.double().cpu(), None, 1, 1, 1, 2 * hid).requires_grad_(True)
    ur = F.gelu(xr[:, :hid]) * xr[:, hid:]
    ur.backward(du[:, :hid].double().cpu().reshape(B, H, W, hid).permute(0, 3, 1, 2))
    g = xr.grad.permute(0, 2, 3, 1).reshape(M, 2 * hid)
    close(u[:, :hid], ur.detach().permute(0, 2, 3, 1).reshape(M, hid), TOL[dtype], geom=(B, H, W), what="u")
    close(dtd[:, :hid], g[:, :hid], TOL[dtype], geom=(B, H, W), what="dt gelu half")
    close(dtd[:, HP:HP + hid], g[:, hid:], TOL[dtype], geom=(B, H, W), what="dt gate half")
    close(u, u2, TOL[dtype], geom=(B, H, W), what="u vs two launches")
    close(dtd, dtd2, TOL[dtype], geom=(B, H, W), what="dt vs two launches")
    assert float(dtd[:, hid:HP].abs().max()) == 0.0 and float(dtd[:, HP + hid:].abs().max()) == 0.0      # padded channels stay zero


@guarded
def check_dwconv_plain(dev, dtype, shape):
    """forward, backward-data (flipped taps) and weight gradient of the depthwise 3x3 vs torch autograd (fp64)."""
    _use(dev)
    import torch.nn.functional as F
    from mp_hsir_amd import ops
    B, H, W, C = shape
    x, dy = rnd(shape, 41, dtype), rnd(shape, 42, dtype)
    w = rnd((C, 1, 3, 3), 43, scale=1 / 3)
    w9 = ops.pack_dw(w)
    y = ops.dwconv3x3(x, w9)
    dx = ops.dwconv3x3(dy, w9, flip=True)
    dw = ops.dwconv3x3_wgrad(x, dy, nblk=3)
    xr = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.double().cpu().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, 1, 1, 1, C)
    yr.backward(dy.double().cpu().permute(0, 3, 1, 2))
    close(y, yr.detach().permute(0, 2, 3, 1), TOL[dtype], geom=(B, H, W), what="y")
    close(dx, xr.grad.permute(0, 2, 3, 1), TOL[dtype], geom=(B, H, W), what="dx")
    close(dw, wr.grad.reshape(C, 9).t(), TOL[dtype], geom=(B, H, W), what="dw")


DW_BWD_CASES = [(1, 8, 16, 32), (2, 16, 32, 96), (1, 24, 16, 128), (2, 8, 32, 352)]
DW_BWD_CASES_GPU = [(32, 64, 64, 384), (4, 64, 64, 704), (2, 128, 128, 192)]


@guarded
def check_dwconv_bwd(dev, dtype, shape):
    """mphsir_dwconv3x3_bwd (dX and dW of one depthwise conv in one launch) vs the two launches (dX bitwise: the same tap order)
    and vs torch autograd in fp64; the parameter-layout output (col_ranges) as well."""
    _use(dev)
    import torch.nn.functional as F
    from mp_hsir_amd import ops
    B, H, W, C = shape
    assert ops.dwconv3x3_bwd_fits(H, W, C, dtype)
    x, dy = rnd(shape, 51, dtype), rnd(shape, 52, dtype)
    w = rnd((C, 1, 3, 3), 53, scale=1 / 3)
    w9 = ops.pack_dw(w)
    dx, dw = ops.dwconv3x3_bwd(x, dy, w9)
    assert torch.equal(dx, ops.dwconv3x3(dy, w9, flip=True))
    xr = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.double().cpu().requires_grad_(True)
    F.conv2d(xr, wr, None, 1, 1, 1, C).backward(dy.double().cpu().permute(0, 3, 1, 2))
    close(dx, xr.grad.permute(0, 2, 3, 1), TOL[dtype], geom=(B, H, W), what="dx")
    close(dw, wr.grad.reshape(C, 9).t(), TOL[dtype], geom=(B, H, W), what="dw")
    close(dw, ops.dwconv3x3_wgrad(x, dy), 1e-5, geom=(B, H, W), what="dw vs wgrad launch")
    half = C // 2 // 8 * 8
    _, dwp = ops.dwconv3x3_bwd(x, dy, w9, col_ranges=[(0, half - 2), (half, C - half)])
    ref = wr.grad.reshape(C, 9)
    close(dwp, torch.cat([ref[:half - 2], ref[half:]], dim=0), TOL[dtype], geom=(B, H, W), what="dw parameter layout")
    # strided views (a channel range of a wider tensor), as the backward of pass A passes them
    wide_x, wide_dy = rnd((B, H, W, C + 32), 54, dtype), rnd((B, H, W, C + 32), 55, dtype)
    dx2, dw2 = ops.dwconv3x3_bwd(wide_x[..., 32:], wide_dy[..., :C], w9)
    dx2r, dw2r = ops.dwconv3x3_bwd(wide_x[..., 32:].contiguous(), wide_dy[..., :C].contiguous(), w9)
    assert torch.equal(dx2, dx2r) and torch.equal(dw2, dw2r)


@guarded
def check_gated_mlp_bwd(dev, dtype, C, hid, variant=0, hsplit=None, M=128, inputs="unit"):
    """HIP data-gradient kernel + token-reduction GEMMs vs autograd of the fp64 oracle; M tokens = M // 64 samples of 64 rows, each with
    its own DropPath factor."""
    _use(dev)
    from mp_hsir_amd import ops
    x, dy = rnd((M, C), 1, dtype, profile=row_profile(inputs)), rnd((M, C), 9, dtype)
    P = {"fc1.weight": rnd((2 * hid, C), 2, scale=C ** -0.5 * (GAIN if inputs == "gain" else 1.0)), "fc1.bias": rnd((2 * hid,), 3, scale=0.1),
         "fc2.weight": rnd((C, hid), 4, scale=hid ** -0.5), "fc2.bias": rnd((C,), 5, scale=0.1)}
    lnw, lnb = rnd((C,), 6, scale=0.1, shift=1), rnd((C,), 7, scale=0.1)
    keep = inp(torch.tensor(([1.0, 1.5] * (M // 64))[:M // 64]))
    W1, b1, W2 = ops.pack_gated_mlp(P["fc1.weight"], P["fc1.bias"], P["fc2.weight"], dtype)
    HP = W2.shape[1]
    dm = (dy.float() * keep.repeat_interleave(64)[:, None]).to(dtype)
    dx, xn, h, dpre, part = ops.gated_mlp_bwd(x, dy, dm, lnw, lnb, W1, b1, W1.t().contiguous(), W2.t().contiguous(), variant=variant, hsplit=hsplit)
    # DropPath scaling fused into the kernel: same results, dm produced by the kernel
    r2 = ops.gated_mlp_bwd(x, dy, None, lnw, lnb, W1, b1, W1.t().contiguous(), W2.t().contiguous(), variant=variant, keep=keep, rows_per_batch=64,
                           hsplit=hsplit)
    assert torch.equal(r2[5].cpu(), dm.cpu()) and torch.equal(r2[0].cpu(), dx.cpu()) and torch.equal(r2[3].cpu(), dpre.cpu())
    dW2 = (dm.float().t() @ h.float())[:, :hid]
    dW1p = dpre.float().t() @ xn.float()
    dW1 = torch.cat([dW1p[:hid], dW1p[HP:HP + hid]], 0)
    db1p = dpre.float().sum(0)
    db1 = torch.cat([db1p[:hid], db1p[HP:HP + hid]])
    db2 = dm.float().sum(0)
    dln = part.sum(0)
    # oracle autograd
    Pd = {k: (v.to(dtype) if k.endswith("weight") else v).double().cpu().requires_grad_(True) for k, v in P.items()}
    xd = x.double().cpu().requires_grad_(True)
    lw, lb = lnw.double().cpu().requires_grad_(True), lnb.double().cpu().requires_grad_(True)
    y = xd + keep.double().cpu().repeat_interleave(64)[:, None] * O.gated_mlp(Pd, "", O.layer_norm_c(xd, lw, lb))
    y.backward(dy.double().cpu())
    tol = TOL[dtype] * (2 if dtype != torch.float32 else 5)
    own = {}          # the yardstick: autograd of the same oracle expression with every operand and op result in the compute dtype

    def in_dtype(what):
        def f(c):
            if not own:
                with torch.enable_grad():
                    Pc = {k: c(v).requires_grad_(True) for k, v in P.items()}
                    xc, lwc, lbc = c(x).requires_grad_(True), c(lnw).requires_grad_(True), c(lnb).requires_grad_(True)
                    yc = xc + c(keep).repeat_interleave(64)[:, None] * O.gated_mlp(Pc, "", O.layer_norm_c(xc, lwc, lbc))
                    yc.backward(c(dy))
                own.update(dx=xc.grad, dW2=Pc["fc2.weight"].grad, dW1=Pc["fc1.weight"].grad, db1=Pc["fc1.bias"].grad, db2=Pc["fc2.bias"].grad,
                           dgamma=lwc.grad, dbeta=lbc.grad)
            return own[what]
        return f
    close(dx, xd.grad, yard_bar(inputs, dtype, tol, "dx", xd.grad, in_dtype("dx")), geom=(M // 64, 64, 1), what="dx")          # samples of 64 tokens, each with its own DropPath factor
    for what, got, ref in (("dW2", dW2, Pd["fc2.weight"].grad), ("dW1", dW1, Pd["fc1.weight"].grad), ("db1", db1, Pd["fc1.bias"].grad),
                           ("db2", db2, Pd["fc2.bias"].grad), ("dgamma", dln[0], lw.grad), ("dbeta", dln[1], lb.grad)):
        close(got, ref, yard_bar(inputs, dtype, tol, what, ref, in_dtype(what)), what=what)


@guarded
def check_gated_mlp_wgrad(dev, dtype, C, hid, M=256, nch=1, ranges=8, keep=True):
    """mphsir_gated_mlp_wgrad (parameter gradients by recomputation, fp32 accumulators per hidden slab and token range) against
    (a) autograd of the fp64 oracle and (b) the token-reduction GEMMs of the operands the data-gradient kernel writes (the path
    it replaces: same 16-bit roundings of h / dval / dgate but for a few elements per million whose recomputed fp32 value falls on the
    other side of a rounding boundary -- SLICE_OVERRIDES -- so the two agree to fp32 summation order); the data-gradient kernel
    without operand outputs must give the dx / LN(x) / dm it gives with them, bitwise; a second launch repeats bitwise."""
    _use(dev)
    from mp_hsir_amd import ops
    x, dy = rnd((M, C), 1, dtype), rnd((M, C), 9, dtype)
    P = {"fc1.weight": rnd((2 * hid, C), 2, scale=C ** -0.5), "fc1.bias": rnd((2 * hid,), 3, scale=0.1),
         "fc2.weight": rnd((C, hid), 4, scale=hid ** -0.5), "fc2.bias": rnd((C,), 5, scale=0.1)}
    lnw, lnb = rnd((C,), 6, scale=0.1, shift=1), rnd((C,), 7, scale=0.1)
    nb = M // 64
    kf = inp((1.0 + 0.25 * torch.arange(nb) / nb).float()) if keep else None
    W1, b1, W2 = ops.pack_gated_mlp(P["fc1.weight"], P["fc1.bias"], P["fc2.weight"], dtype)
    W1T, W2T = W1.t().contiguous(), W2.t().contiguous()
    HP = W2.shape[1]
    if keep:
        dx, xn, h, dpre, part, dm = ops.gated_mlp_bwd(x, dy, None, lnw, lnb, W1, b1, W1T, W2T, keep=kf, rows_per_batch=64)
        dx2, xn2, h2, dpre2, part2, dm2 = ops.gated_mlp_bwd(x, dy, None, lnw, lnb, W1, b1, W1T, W2T, keep=kf, rows_per_batch=64, operands=False)
    else:
        dm = dy
        dx, xn, h, dpre, part = ops.gated_mlp_bwd(x, dy, dm, lnw, lnb, W1, b1, W1T, W2T)
        dx2, xn2, h2, dpre2, part2 = ops.gated_mlp_bwd(x, dy, dm, lnw, lnb, W1, b1, W1T, W2T, operands=False)
        dm2 = dm
    assert h2 is None and dpre2 is None
    assert torch.equal(dx.cpu(), dx2.cpu()) and torch.equal(xn.cpu(), xn2.cpu()) and torch.equal(dm.cpu(), dm2.cpu()) and torch.equal(part.cpu(), part2.cpu())
    dW1, db1, dW2, db2 = ops.gated_mlp_wgrad(xn, dm, W1, b1, W2T, hid, nch=nch, ranges=ranges)
    again = ops.gated_mlp_wgrad(xn, dm, W1, b1, W2T, hid, nch=nch, ranges=ranges)
    for u, v in zip((dW1, db1, dW2, db2), again):
        assert torch.equal(u.cpu(), v.cpu())
    # (b) the operands path
    dW2r = (dm.float().t() @ h.float())[:, :hid]
    dW1p = dpre.float().t() @ xn.float()
    dW1r = torch.cat([dW1p[:hid], dW1p[HP:HP + hid]], 0)
    db1p = dpre.float().sum(0)
    db1r = torch.cat([db1p[:hid], db1p[HP:HP + hid]])
    db2r = dm.float().sum(0)
    for what, got, ref in (("dW1 vs operands", dW1, dW1r), ("db1 vs operands", db1, db1r), ("dW2 vs operands", dW2, dW2r), ("db2 vs operands", db2, db2r)):
        assert got.shape == ref.shape
        close(got, ref.double().cpu(), 2e-5, what=what)
    # (a) oracle autograd
    Pd = {k: (v.to(dtype) if k.endswith("weight") else v).double().cpu().requires_grad_(True) for k, v in P.items()}
    xd = x.double().cpu().requires_grad_(True)
    lw, lb = lnw.double().cpu(), lnb.double().cpu()
    kd = kf.double().cpu().repeat_interleave(64)[:, None] if keep else 1.0
    y = xd + kd * O.gated_mlp(Pd, "", O.layer_norm_c(xd, lw, lb))
    y.backward(dy.double().cpu())
    tol = TOL[dtype] * 2
    for what, got, ref in (("dW2", dW2, Pd["fc2.weight"].grad), ("dW1", dW1, Pd["fc1.weight"].grad), ("db1", db1, Pd["fc1.bias"].grad),
                           ("db2", db2, Pd["fc2.bias"].grad)):
        close(got, ref, tol, what=what)


@guarded
def check_l1_clamp_loss(dev):
    """mphsir_l1_clamp_loss (loss + gradient in one pass) vs the oracle's clamp + L1 and torch autograd through it (train.py:58-61),
    incl. values exactly on the clamp bounds / equal to the target, a length that is not a multiple of 4, and an upstream factor."""
    _use(dev)
    from mp_hsir_amd import ops
    for shape in ((2, 8, 32, 32), (1, 3, 5, 7), (4, 31, 64, 64)):
        y = (rnd(shape, 901) * 0.7 + 0.5)
        c = rnd(shape, 902).abs().clamp(0, 1)
        with torch.no_grad():
            y.view(-1)[:4] = torch.tensor([0.0, 1.0, -0.0, float(c.view(-1)[3])])
        y.requires_grad_(True)
        loss = ops.l1_clamp_loss(y, c)
        (loss * 3.0).backward()
        yr = y.detach().double().cpu().requires_grad_(True)
        lr = O.l1_after_clamp(yr, c.double().cpu())
        (lr * 3.0).backward()
        assert abs(float(loss.detach()) - float(lr.detach())) < 1e-6 * abs(float(lr.detach())) + 1e-9
        close(y.grad, yr.grad, 1e-6, what="dy")
        assert float((y.grad.double().cpu() - yr.grad).abs().max()) < 1e-7 * 3.0 / y.numel() + 1e-12
    # non-finite outputs: torch.clamp propagates NaN (the loss becomes NaN: a diverged run must not log a finite loss) and clamps the
    # infinities; the gradient is 0 at all three, as torch's
    for bad, loss_nan in ((float("nan"), True), (float("inf"), False), (float("-inf"), False)):
        y = (rnd((2, 8, 16, 16), 903) * 0.7 + 0.5)
        c = rnd((2, 8, 16, 16), 904).abs().clamp(0, 1)
        with torch.no_grad():
            y.view(-1)[5] = bad
            y.view(-1)[-2] = bad             # inside the scalar tail handling too when n % 4 != 0 (not here) and in another block
        y.requires_grad_(True)
        loss = ops.l1_clamp_loss(y, c)
        loss.backward()
        yr = y.detach().double().cpu().requires_grad_(True)
        lr = O.l1_after_clamp(yr, c.double().cpu())
        lr.backward()
        assert bool(torch.isnan(loss.detach())) == loss_nan == bool(torch.isnan(lr.detach()))
        if not loss_nan:
            assert abs(float(loss.detach()) - float(lr.detach())) < 1e-6 * abs(float(lr.detach()))
        assert torch.isfinite(y.grad).all() and float(y.grad.view(-1)[5]) == 0.0
        close(y.grad, yr.grad, 1e-6, what="dy at non-finite outputs")


@guarded
def check_multi_copy(dev):
    """mphsir_multi_copy: many fp32 tensors -> their arena slots in one launch: lengths around the 4096-float block, a source that
    is not 16-byte aligned, repeated use of the table ring."""
    _use(dev)
    from mp_hsir_amd import ops
    d = torch.device(dev)
    lens = (5, 4096, 4097, 12, 100000, 3, 8192, 1)
    arena = alloc((sum((n + 3) // 4 * 4 for n in lens) + 8,))
    dsts, o = [], 0
    for n in lens:
        dsts.append(arena[o:o + n])
        o += (n + 3) // 4 * 4
    mc = ops.MultiCopy(d, 16, ring=2)
    for rep in range(5):
        srcs = [rnd((n,), 910 + rep * 16 + i) for i, n in enumerate(lens)]
        srcs[3] = rnd((16,), 990 + rep)[1:13]
        mc(dsts, srcs)
        for a, b in zip(dsts, srcs):
            assert torch.equal(a.cpu(), b.cpu())


class tn_form:
    """`with tn_form(f):` runs the 16-bit big-tile token-reduction GEMMs in form f (1 = transposed-read kernel, 2 = ring form)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        from mp_hsir_amd import ops
        self.prev, ops.TN_FORM = ops.TN_FORM, self.form

    def __exit__(self, *exc):
        from mp_hsir_amd import ops
        ops.TN_FORM = self.prev
        return False


@guarded
def check_gemm_tn(dev, dtype, M, N1, N2, nsplit, batch, tile128=None):
    _use(dev)
    from mp_hsir_amd import ops
    shape_a = (batch, M, N1) if batch else (M, N1)
    shape_b = (batch, M, N2) if batch else (M, N2)
    a, b = rnd(shape_a, 51, dtype), rnd(shape_b, 52, dtype)
    c, cs = ops.gemm_tn(a, b, nsplit=nsplit, colsum=True, tile128=tile128)
    ref = a.double().cpu().transpose(-1, -2) @ b.double().cpu()
    close(c, ref, 3e-6 if dtype == torch.float32 else 1e-2, what="c")          # 16-bit inputs are exact here: fp32 accumulation order only
    close(cs, a.double().cpu().sum(dim=-2), 3e-6 if dtype == torch.float32 else 1e-2, what="colsum")
    # strided views (column slices of a wider matrix), as the backward uses them
    wide = rnd((M, N1 + 24), 53, dtype)
    if not batch:
        c2 = ops.gemm_tn(wide[:, 8:8 + N1], b, nsplit=nsplit)
        close(c2, wide[:, 8:8 + N1].double().cpu().t() @ b.double().cpu(), 3e-6 if dtype == torch.float32 else 1e-2, what="c of a strided view")


@guarded
def check_conv3x3(dev, dtype, B, H, W, Cin, Cout):
    """implicit-GEMM dense conv: forward, input gradient (flipped/transposed weights) and weight gradient
    (im2col + token-reduction GEMM) vs torch autograd in fp64."""
    _use(dev)
    import torch.nn.functional as F
    from mp_hsir_amd import ops
    x, dy = rnd((B, H, W, Cin), 61, dtype), rnd((B, H, W, Cout), 62, dtype)
    w = rnd((Cout, Cin, 3, 3), 63, scale=(9 * Cin) ** -0.5)
    Cp, Np = ops.round_up(Cin, 32), ops.round_up(Cout, 16)
    xp = F.pad(x, (0, Cp - Cin)).contiguous()
    y = ops.conv3x3_tok(xp, ops.pack_conv3x3(w, dtype))[..., :Cout]
    Co32 = ops.round_up(Cout, 32)
    dyp = F.pad(dy, (0, Co32 - Cout)).contiguous()
    dx = ops.conv3x3_tok(dyp, ops.pack_conv3x3(w, dtype, flip_transpose=True))[..., :Cin]
    dw = ops.gemm_tn(dy.reshape(-1, Cout).contiguous() if Cout % 8 == 0 else F.pad(dy, (0, Np - Cout)).reshape(-1, Np).contiguous(),
                     ops.im2col3x3(xp))[:Cout].reshape(Cout, 9, Cp)[:, :, :Cin].permute(0, 2, 1).reshape(Cout, Cin, 3, 3)
    xr = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wr = w.to(dtype).double().cpu().requires_grad_(True)
    yr = F.conv2d(xr, wr, None, 1, 1)
    yr.backward(dy.double().cpu().permute(0, 3, 1, 2))
    close(y, yr.detach().permute(0, 2, 3, 1), TOL[dtype], geom=(B, H, W), what="y")
    close(dx, xr.grad.permute(0, 2, 3, 1), TOL[dtype], geom=(B, H, W), what="dx")
    close(dw, wr.grad, TOL[dtype], geom=(B, H, W), what="dw")
    if dtype != torch.float32:      # the same weight gradient with the gather inside the token-reduction GEMM (no im2col matrix)
        dw2 = ops.conv3x3_wgrad(dyp.reshape(-1, Co32), xp, nsplit=3)[:Cout].reshape(Cout, 9, Cp)[:, :, :Cin].permute(0, 2, 1).reshape(Cout, Cin, 3, 3)
        close(dw2, wr.grad, TOL[dtype], geom=(B, H, W), what="dw gathered")
        close(dw2, dw, 1e-5, geom=(B, H, W), what="dw gathered vs im2col")
        dw3 = ops.conv3x3_wgrad(dyp.reshape(-1, Co32), xp)[:Cout].reshape(Cout, 9, Cp)[:, :, :Cin].permute(0, 2, 1).reshape(Cout, Cin, 3, 3)
        close(dw3, dw, 1e-5, geom=(B, H, W), what="dw gathered, one split, vs im2col")
        # the nn.Conv2d layout straight out of the ordered partial reduction (padding dropped, taps transposed there), immediate and
        # deferred to the end of a reduce_scope: bitwise the slice / permute of the plain form
        dw4 = ops.conv3x3_wgrad(dyp.reshape(-1, Co32), xp, nsplit=3, cout=Cout, cin=Cin)
        with ops.reduce_scope():
            dw5 = ops.conv3x3_wgrad(dyp.reshape(-1, Co32), xp, nsplit=3, cout=Cout, cin=Cin)
        assert dw4.is_contiguous() and torch.equal(dw4.cpu(), dw2.cpu()) and torch.equal(dw5.cpu(), dw2.cpu())


@guarded
def check_reduce_parts(dev):
    """mphsir_reduce_parts: deferred scope (several segments, one launch), odd lengths (scalar path), batched layout,
    > 32 segments (two launches), and bitwise equality with an ordered fp32 sum."""
    _use(dev)
    from mp_hsir_amd import ops
    shapes = [((5, 7, 12), False), ((3, 225, 2), False), ((4, 6, 16, 8), True), ((1, 9, 4), False), ((17, 33), False),
              ((300, 18), False), ((130, 2, 32), False), ((2, 70, 5), True)]
    parts = [rnd(s, 70 + i) for i, (s, _) in enumerate(shapes)]
    with ops.reduce_scope():
        outs = [ops.reduce_parts(p, batched=b) for p, (_, b) in zip(parts, shapes)]
    for p, o, (_, b) in zip(parts, outs, shapes):
        ref = p.double().sum(1 if b else 0)
        assert rel_l2(o, ref) < 3e-7, (p.shape, rel_l2(o, ref))
    many = [rnd((3, 8 + i), 90 + i) for i in range(40)]
    with ops.reduce_scope():
        outs = [ops.reduce_parts(p) for p in many]
    for p, o in zip(many, outs):
        assert torch.equal(o.cpu(), ((p[0] + p[1]) + p[2]).cpu())
    assert torch.equal(ops.reduce_parts(many[0]).cpu(), outs[0].cpu())          # immediate mode outside a scope
    big = rnd((300, 18), 99)
    assert torch.equal(ops.reduce_parts(big).cpu(), ops.reduce_parts(big.clone()).cpu())   # fixed order: bitwise reproducible


@guarded
def check_pack_gather(dev, dtype):
    _use(dev)
    from mp_hsir_amd import ops
    arena = rnd((1000,), 95)
    g = torch.Generator().manual_seed(5)
    idx = inp(torch.randint(-1, 1000, (256,), generator=g, dtype=torch.int32))
    out = ops.pack_gather(arena, idx, dtype)
    ref = torch.where(idx >= 0, arena[idx.clamp(min=0).long()], torch.zeros(())).to(dtype)
    assert torch.equal(out.cpu(), ref.cpu())


@guarded
def check_reduce_block(dev):
    """2-D segments of mphsir_reduce_parts: sub-block extraction with un-padding, stacking two row ranges into one
    output, a transposed destination, a single-row block and an unaligned sub-block (scalar path)."""
    _use(dev)
    from mp_hsir_amd import ops
    part = rnd((5, 24, 40), 120)
    full = part.double().sum(0)
    with ops.reduce_scope():
        a = alloc((12, 40), fill=None)
        ops.reduce_block(part, 0, 6, 0, 40, a[:6])
        ops.reduce_block(part, 16, 6, 0, 40, a[6:])
        b = ops.reduce_block(part, 4, 8, 8, 16, alloc((8, 16), fill=None))
        c = ops.reduce_block(part, 0, 9, 0, 24, alloc((24, 9), fill=None), transpose=True)
        d = ops.reduce_block(part, 3, 1, 5, 7, alloc((1, 7), fill=None))
        e = ops.reduce_block(part, 2, 5, 3, 10, alloc((5, 10), fill=None))
        wide = alloc((8, 32))
        ops.reduce_block(part, 1, 8, 4, 12, wide[:, 8:20])
        one = rnd((1, 1, 8), 121)                                     # one partial, one row
        f = ops.reduce_block(one, 0, 1, 0, 8, alloc((1, 8), fill=None))
    assert torch.equal(f.cpu(), one[0].cpu())
    assert rel_l2(a, torch.cat([full[:6], full[16:22]])) < 3e-7
    assert rel_l2(b, full[4:12, 8:24]) < 3e-7 and rel_l2(c, full[:9, :24].t()) < 3e-7
    assert rel_l2(d, full[3:4, 5:12]) < 3e-7 and rel_l2(e, full[2:7, 3:13]) < 3e-7
    assert rel_l2(wide[:, 8:20], full[1:9, 4:16]) < 3e-7 and float(wide[:, :8].abs().sum()) == 0 and float(wide[:, 20:].abs().sum()) == 0


@guarded
def check_gemm_tn_grouped(dev, dt=torch.bfloat16):
    """16-bit token-reduction GEMMs deferred inside a reduce_scope are issued as ONE grouped launch: mixed widths (64- and
    128-wide tile classes in one group), column sums, un-padding blocks, > 8 problems (two launches) == separate calls."""
    _use(dev)
    from mp_hsir_amd import ops
    shapes = [(256, 64, 128), (192, 136, 48), (320, 40, 56), (256, 160, 136), (128, 64, 64), (256, 200, 72), (192, 96, 96),
              (256, 24, 264), (128, 72, 40), (320, 128, 128)]
    A = [rnd((m, n1), 150 + i, dt) for i, (m, n1, n2) in enumerate(shapes)]
    B = [rnd((m, n2), 170 + i, dt) for i, (m, n1, n2) in enumerate(shapes)]
    ref = [ops.gemm_tn(a, b, nsplit=2, colsum=True) for a, b in zip(A, B)]                      # immediate launches
    ops.ACCOUNT = {}
    with ops.reduce_scope():
        got = [ops.gemm_tn(a, b, nsplit=2, colsum=True) for a, b in zip(A, B)]
        blk = ops.gemm_tn_blocks(A[3], B[3], [(0, 40), (96, 40)], ncols=100, colsum=True)
    acct, ops.ACCOUNT = ops.ACCOUNT, None
    for (c0, s0), (c1, s1) in zip(ref, got):
        assert torch.equal(c0.cpu(), c1.cpu()) and torch.equal(s0.cpu(), s1.cpu())
    full = A[3].double().cpu().t() @ B[3].double().cpu()
    close(blk[0], torch.cat([full[:40, :100], full[96:136, :100]]), 1e-2, what="blocks")
    close(blk[1], torch.cat([A[3].double().cpu().sum(0)[:40], A[3].double().cpu().sum(0)[96:136]]), 1e-2, what="blocks colsum")


# ---- backward kernels at the benchmarked widths: fp64 autograd of the oracle on dtype-rounded weights ------------------
_ROUNDED = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight", "gobal_spectral_attn.qkv.weight")
GTOL = {torch.float32: 2e-5, torch.bfloat16: 6e-2, torch.float16: 2e-2}


@guarded
def check_pgsstb_backward_oracle(dev, dtype, name, B=2, hw=(16, 16), drop_path=True):
    """A whole PGSSTB block (win_attn_bwd + ln_bwd_win + combine_bwd + pg_gate_bwd + the channel-attention backward chain +
    gated_mlp_bwd + every token-reduction GEMM) at one shape class of BLOCK_CASES, batch 2, WITH DropPath factors, against
    fp64 autograd of the oracle run on the weights as the kernels see them (GEMM weights rounded to `dtype`).  Every
    gradient is compared as a full tensor."""
    _use(dev)
    from golden.cases import BLOCK_CASES
    from golden.detfill import det_value
    from mp_hsir_amd import autograd_ops as AG
    from mp_hsir_amd.net.MP_HSIR import PGSSTB
    c = BLOCK_CASES[name]
    C, heads, shift = c["C"], c["heads"], c["shift"]
    H, W = hw
    blk = PGSSTB(C, heads, [64, 64], 8, shift, 0.0, 2.66, c["cr"], 128).eval()
    with torch.no_grad():
        for k, p in blk.named_parameters():
            p.copy_(det_value(k, p.shape).float())
    blk = blk.to(dev)
    x = rnd((B, H, W, C), 301, dtype).requires_grad_(True)
    cot = rnd((B, H, W, C), 302, dtype)
    k1 = inp(torch.tensor([1.0 / 0.9, 0.0][:B] if drop_path else [1.0] * B))
    k2 = inp(torch.tensor([0.0, 1.0 / 0.95][:B] if drop_path else [1.0] * B))
    y = AG.pgsstb(blk, x, k1, k2)
    (y.float() * cot.float()).sum().backward()
    # oracle
    P = {}
    for k, p in blk.named_parameters():
        v = p.detach().cpu()
        if k in _ROUNDED:
            v = v.to(dtype)
        P[k] = v.double().requires_grad_(True)
    xd = x.detach().double().cpu().requires_grad_(True)
    yr = O.pgsstb(P, "", xd, heads, shifted=shift > 0, keep=(k1.double().cpu(), k2.double().cpu()))
    (yr * cot.double().cpu()).sum().backward()
    tol = GTOL[dtype]
    pairs = {"out": (y.detach().float(), yr.detach()), "dx": (x.grad.float(), xd.grad)}
    for k, p in blk.named_parameters():
        pairs[k] = (p.grad.float(), P[k].grad)
    errs = {k: rel_l2(g, r) for k, (g, r) in pairs.items()}          # whole-tensor values: returned and printed as before
    bad = {k: v for k, v in errs.items() if not v < (TOL[dtype] * 2 if k == "out" else tol)}
    assert not bad, (name, str(dtype), bad)
    for k, (g, r) in pairs.items():                                   # and per tensor: no slice of it (sample, image row, channel, ...) stands out
        close(g, r, TOL[dtype] * 2 if k == "out" else tol, geom=(B, H, W), what=k, whole=errs[k])
    return errs


@guarded
def check_win_attn_bwd_head_split(dev, dtype, C=128, heads=4, shape=(2, 16, 16)):
    """win_attn_bwd with the heads of a window dealt to several workgroups returns exactly what one workgroup per window does."""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    x, dsa = rnd((B, H, W, C), 71, dtype), rnd((B, H, W, C), 72, dtype)
    dmu = rnd((B * H * W // 64, C), 73)
    lnw, lnb = rnd((C,), 74, scale=0.1, shift=1), rnd((C,), 75, scale=0.1)
    wqkv, bqkv = rnd((3 * C, C), 76, dtype, scale=C ** -0.5), rnd((3 * C,), 77, scale=0.1)
    rpb = rnd((225, heads), 78, scale=0.2)
    wprojT = rnd((C, C), 79, dtype, scale=C ** -0.5)
    ref = ops.win_attn_bwd(x, dsa, dmu, lnw, lnb, wqkv, bqkv, rpb, wprojT, heads, 4, head_split=1)
    for hs in (2, heads):
        out = ops.win_attn_bwd(x, dsa, dmu, lnw, lnb, wqkv, bqkv, rpb, wprojT, heads, 4, head_split=hs)
        assert all(torch.equal(a, b) for a, b in zip(out, ref)), hs
    auto = ops.win_attn_bwd(x, dsa, dmu, lnw, lnb, wqkv, bqkv, rpb, wprojT, heads, 4)
    assert all(torch.equal(a, b) for a, b in zip(auto, ref))


@guarded
def check_combine_bwd(dev, dtype, C=128, shift=4, shape=(2, 16, 24)):
    """mphsir_combine_bwd against its definition (backward of gemm_tok epilogue 2)."""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    dy, sa = rnd((B, H, W, C), 311, dtype), rnd((B, H, W, C), 312, dtype)
    gate = rnd((B * (H // 8) * (W // 8), C), 313)
    keep = inp(torch.tensor([1.25, 0.5][:B]))
    d_out, d_sa, dgate = ops.combine_bwd(dy, sa, gate, keep, shift)
    dyd, sad = dy.double().cpu(), sa.double().cpu()
    do_ref = (keep.double().cpu().reshape(B, 1, 1, 1) * dyd).to(dtype).double()          # stored rounded
    gw = gate.double().cpu()[:, None, :].expand(-1, 64, -1)
    gimg = O.from_windows(gw, B, H, W)
    if shift:
        gimg = torch.roll(gimg, (shift, shift), (1, 2))
    close(d_out, do_ref, TOL[dtype], geom=(B, H, W), what="d_out")
    close(d_sa, do_ref * gimg, TOL[dtype], geom=(B, H, W), what="d_sa")
    prod = do_ref * sad
    if shift:
        prod = torch.roll(prod, (-shift, -shift), (1, 2))
    close(dgate, O.to_windows(prod).sum(1), TOL[dtype], geom=(B, H, W), what="dgate")          # window-major: one row per window
    # keep = None: d_out aliases dy
    d_out2, d_sa2, _ = ops.combine_bwd(dy, sa, gate, None, shift)
    assert d_out2.data_ptr() == dy.data_ptr()
    close(d_sa2, dyd * gimg, TOL[dtype], geom=(B, H, W), what="d_sa without keep")


@guarded
def check_pg_gate_bwd(dev, C, cr, nW=20, factor_dtype=torch.float32, inputs="unit"):
    """mphsir_pg_gate_bwd (+ the factor-product GEMM that yields its eight parameter gradients) against fp64 autograd
    of the oracle's pg_spectral_gate."""
    _use(dev)
    from golden.detfill import det_value
    from mp_hsir_amd import ops
    r = C // cr
    shapes = {"linear_down.weight": (r, C), "linear_up.weight": (C, r), "linear_prompt.weight": (128, C), "prompt_param": (1, 1, 128, r),
              "q.weight": (r, r), "kv.weight": (2 * r, r), "proj.weight": (r, r), "proj.bias": (r,)}
    P = {k: det_value("local_spectral_attn." + k, shp).float() for k, shp in shapes.items()}
    assert inputs in ("unit", "peaked")
    if inputs == "peaked":          # q and the k rows of kv x 4: the logits q k / sqrt(r) x 16
        P["q.weight"] = P["q.weight"] * 4.0
        P["kv.weight"] = torch.cat([P["kv.weight"][:r] * 4.0, P["kv.weight"][r:]], 0)
    pg = {k: inp(v.contiguous()) for k, v in P.items()}
    pg["prompt_param"] = pg["prompt_param"].reshape(128, r).contiguous()
    mu, dgate = rnd((nW, C), 321), rnd((nW, C), 322)
    with ops.reduce_scope():
        dmu, g = ops.pg_gate_bwd(mu, dgate, pg, factor_dtype=factor_dtype)
    Pd = {"pg." + k: v.double().requires_grad_(True) for k, v in P.items()}
    mud = mu.double().cpu().requires_grad_(True)
    gate = O.pg_spectral_gate(Pd, "pg.", mud[:, None, :].expand(-1, 64, -1))
    (gate * dgate.double().cpu()).sum().backward()
    tol = 2e-5 if factor_dtype == torch.float32 else 2e-2
    own = {}

    def in_dtype(what):
        def f(c):
            if not own:
                with torch.enable_grad():
                    Pc = {"pg." + k: c(v).requires_grad_(True) for k, v in P.items()}
                    muc = c(mu).requires_grad_(True)
                    (O.pg_spectral_gate(Pc, "pg.", muc[:, None, :].expand(-1, 64, -1)) * c(dgate)).sum().backward()
                own.update({k: Pc["pg." + k].grad for k in shapes}, dmu=muc.grad)
            return own[what]
        return f
    close(dmu, mud.grad, yard_bar(inputs, torch.float32, 2e-5, "dmu", mud.grad, in_dtype("dmu")), what="dmu")
    for k in shapes:
        close(g[k].reshape(shapes[k]), Pd["pg." + k].grad, yard_bar(inputs, torch.float32, tol, k, Pd["pg." + k].grad, in_dtype(k)), what=k)


@guarded
def check_pg_gate_fwd(dev, C, cr, nW=20, inputs="unit"):
    """mphsir_pg_gate_fwd on its own against the oracle's pg_spectral_gate (MP_HSIR.py:136-152) -- incl. widths the shipped
    nets do not have (C = 512 with r = 16: the register-resident Wup path must not take them)."""
    _use(dev)
    from golden.detfill import det_value
    from mp_hsir_amd import ops
    r = C // cr
    shapes = {"linear_down.weight": (r, C), "linear_up.weight": (C, r), "linear_prompt.weight": (128, C), "prompt_param": (1, 1, 128, r),
              "q.weight": (r, r), "kv.weight": (2 * r, r), "proj.weight": (r, r), "proj.bias": (r,)}
    P = {k: det_value("local_spectral_attn." + k, shp).float() for k, shp in shapes.items()}
    assert inputs in ("unit", "peaked")
    if inputs == "peaked":          # q and the k rows of kv x 4: the logits q k / sqrt(r) x 16
        P["q.weight"] = P["q.weight"] * 4.0
        P["kv.weight"] = torch.cat([P["kv.weight"][:r] * 4.0, P["kv.weight"][r:]], 0)
    pg = {k: inp(v.contiguous()) for k, v in P.items()}
    pg["prompt_param"] = pg["prompt_param"].reshape(128, r).contiguous()
    mu = rnd((nW, C), 323)
    gate = ops.pg_gate_fwd(mu, pg)
    Pd = {"pg." + k: v.double() for k, v in P.items()}
    want = O.pg_spectral_gate(Pd, "pg.", mu.double().cpu()[:, None, :].expand(-1, 64, -1))
    tol = yard_bar(inputs, torch.float32, 2e-5, "gate", want, lambda c: O.pg_spectral_gate({"pg." + k: c(v) for k, v in P.items()}, "pg.", c(mu)[:, None, :].expand(-1, 64, -1)))
    close(gate, want, tol, what="gate")


@guarded
def check_fold_bwd_split_dm(dev, dtype, C=64, heads=2, B=2, nsp=5):
    """mphsir_spectral_fold_bwd with dM handed over as the SPLIT PARTIALS of the token-reduction GEMM (B, splits, C, C): the kernel's
    in-order sum while staging against the ordered-sum launch (reduce_parts) followed by the plain call"""
    _use(dev)
    from mp_hsir_amd import ops
    hd = C // heads
    gp = rnd((B, 1, heads, hd, hd), 601)
    sp = rnd((B, 1, 2, C), 602).abs() + 0.5
    temp = (rnd((heads,), 603, scale=0.3, shift=1)).contiguous()
    wo = rnd((C, C), 604, scale=C ** -0.5)
    part = rnd((B, nsp, C, C), 605)
    dm = ops.reduce_parts(part, batched=True)
    a = ops.spectral_fold_bwd(gp, sp, temp, wo, dm, dtype, reduce=False)
    b = ops.spectral_fold_bwd(gp, sp, temp, wo, part, dtype, reduce=False)
    # (the same partials summed in a different fixed order -- reduce_parts deals the splits to lanes -- so fp32 reassociation, not bits)
    for what, x, y in zip(("W2", "dWo", "dtemp"), a, b):
        tol = 1e-6 if x.dtype == torch.float32 else 2e-3
        close(y, x.double().cpu(), tol, what=what)


@guarded
def check_ln_bwd_win_dxn(dev, dtype, C=64, shape=(2, 16, 16), shift=4, inputs="unit"):
    """mphsir_ln_bwd_win_dxn (d_xn = dQKV Wqkv formed inside the LayerNorm-backward launch) against gemm_tok + ln_bwd_win on the same
    operands, and both against an fp64 evaluation (the fused form keeps d_xn in fp32: it must be no further from fp64 than the pair)"""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    M = B * H * W
    assert ops.ln_bwd_win_dxn_fits(M, C, dtype)
    x, dres = rnd((B, H, W, C), 921, dtype, profile=row_profile(inputs)), rnd((B, H, W, C), 922, dtype)
    dqkv = rnd((M, 3 * C), 923, dtype)
    wT = rnd((C, 3 * C), 924, dtype, scale=(3 * C) ** -0.5)
    ln_w = (rnd((C,), 925, scale=0.2, shift=1)).contiguous()
    dx_a, part_a = ops.ln_bwd_win(x, ops.gemm_tok(dqkv, wT), dres, ln_w, shift)
    dx_b, part_b = ops.ln_bwd_win_dxn(x, dqkv, wT, dres, ln_w, shift)
    # fp64: d_xn in window order -> image order through the same index map the oracle's window partition uses
    x64, dr64 = x.double().cpu(), dres.double().cpu()
    dxn_w = (dqkv.double().cpu() @ wT.double().cpu().t()).reshape(B, H // 8, W // 8, 8, 8, C)          # (b, wy, wx, ty, tx, c) in the SHIFTED frame
    dxn_s = dxn_w.permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    dxn = torch.roll(dxn_s, shifts=(shift, shift), dims=(1, 2))                                            # back to the image frame
    xr = x64.clone().requires_grad_(True)
    lw = ln_w.double().cpu().clone().requires_grad_(True)
    lb = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.layer_norm(xr, (C,), lw, lb, 1e-5)
    (y * dxn).sum().backward()
    dx64 = xr.grad + dr64
    pa, pb = part_a.double().cpu().sum(0), part_b.double().cpu().sum(0)
    tol = TOL[dtype]
    own = {}

    def in_dtype(what):
        def f(c):
            if not own:
                with torch.enable_grad():
                    xc, lwc = c(x).requires_grad_(True), c(ln_w).requires_grad_(True)
                    lbc = torch.zeros(C, dtype=xc.dtype, requires_grad=True)
                    (O.layer_norm_c(xc, lwc, lbc) * c(dxn)).sum().backward()
                own.update(dx=xc.grad + c(dres), dgamma=lwc.grad, dbeta=lbc.grad)
            return own[what]
        return f
    res = dict(dx_pair=rel_l2(dx_a, dx64), dgamma_pair=rel_l2(pa[0], lw.grad), dbeta_pair=rel_l2(pa[1], lb.grad))
    res.update(dx=close(dx_b, dx64, yard_bar(inputs, dtype, tol, "dx", dx64, in_dtype("dx")), geom=(B, H, W), what="dx"),
               dgamma=close(pb[0], lw.grad, yard_bar(inputs, dtype, tol, "dgamma", lw.grad, in_dtype("dgamma")), geom=(B, H, W), what="dgamma"),
               dbeta=close(pb[1], lb.grad, yard_bar(inputs, dtype, tol, "dbeta", lb.grad, in_dtype("dbeta")), geom=(B, H, W), what="dbeta"))
    assert res["dx"] <= res["dx_pair"] * 1.05 + 1e-7 and res["dgamma"] <= res["dgamma_pair"] * 1.05 + 1e-6 and res["dbeta"] <= res["dbeta_pair"] * 1.05 + 1e-6, res
    # a second residual gradient (the BaseBlock skip's): the same launch adds it; the LayerNorm partials do not move
    dres2 = rnd((B, H, W, C), 926, dtype)
    dx_c, part_c = ops.ln_bwd_win_dxn(x, dqkv, wT, dres, ln_w, shift, dres2=dres2)
    assert torch.equal(part_c, part_b)
    res["dx_skip"] = close(dx_c, dx64 + dres2.double().cpu(), tol, geom=(B, H, W), what="dx with the skip gradient")
    return res


@guarded
def check_ln_bwd_tok_dxn(dev, dtype, C=64, K=384, M=256, inputs="unit"):
    """mphsir_ln_bwd_tok_dxn (token order, any K % 32 == 0, LN(x) as a second output) against gemm_tok + ln_bwd_tok on the same operands"""
    _use(dev)
    from mp_hsir_amd import ops
    assert ops.ln_bwd_win_dxn_fits(M, C, dtype)
    x, dres = rnd((M, C), 931, dtype, profile=row_profile(inputs)), rnd((M, C), 932, dtype)
    dy = rnd((M, K), 933, dtype)
    wT = rnd((C, K), 934, dtype, scale=K ** -0.5)
    ln_w, ln_b = (rnd((C,), 935, scale=0.2, shift=1)).contiguous(), (rnd((C,), 936, scale=0.1)).contiguous()
    with ops.reduce_scope():
        a = ops.ln_bwd_tok(x, ops.gemm_tok(dy, wT), dres, ln_w, ln_b)
        b = ops.ln_bwd_tok_dxn(x, dy, wT, dres, ln_w, ln_b)
    dxn = dy.double().cpu() @ wT.double().cpu().t()
    xr = x.double().cpu().clone().requires_grad_(True)
    lw, lb = ln_w.double().cpu().clone().requires_grad_(True), ln_b.double().cpu().clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (C,), lw, lb, 1e-5)
    (y * dxn).sum().backward()
    want = (xr.grad + dres.double().cpu(), lw.grad, lb.grad, y.detach())
    res, own = {}, {}

    def in_dtype(what):
        def f(c):
            if not own:
                with torch.enable_grad():
                    xc, lwc, lbc = c(x).requires_grad_(True), c(ln_w).requires_grad_(True), c(ln_b).requires_grad_(True)
                    yc = O.layer_norm_c(xc, lwc, lbc)
                    (yc * c(dxn)).sum().backward()
                own.update(dx=xc.grad + c(dres), dgamma=lwc.grad, dbeta=lbc.grad, xn=yc.detach())
            return own[what]
        return f
    for name, pa, pb, w in zip(("dx", "dgamma", "dbeta", "xn"), a, b, want):
        res[name] = (rel_l2(pa, w), close(pb, w, yard_bar(inputs, dtype, TOL[dtype], name, w, in_dtype(name)), what=name))
        assert res[name][1] <= res[name][0] * 1.05 + 1e-6, res
    close(b[3], a[3].double().cpu(), TOL[dtype] / 4, what="xn vs pair")      # LN(x): the same formula (the compiler contracts its fmas differently in the two kernels)
    # no residual path (TVSP's norm12 on the batch-invariant prompt map), LN(x) not wanted
    with ops.reduce_scope():
        c = ops.ln_bwd_tok_dxn(x, dy, wT, None, ln_w, ln_b, want_xn=False)
    assert c[3] is None and torch.equal(c[1], b[1]) and torch.equal(c[2], b[2])
    close(c[0], xr.grad, TOL[dtype], what="dx without residual")
    # fp32 rows of x with 16-bit dy / weights / d_res (TVSP's norm11 on the fp32 text map): against the fp32 LayerNorm backward on d_xn
    # formed in fp64 from the same 16-bit operands
    if C <= 192:
        assert ops.ln_bwd_tok_dxn_f32_fits(M, C, dtype)
        x32 = rnd((M, C), 937)
        with ops.reduce_scope():
            d = ops.ln_bwd_tok_dxn(x32, dy, wT, dres, ln_w, ln_b, want_xn=False)
        assert d[0].dtype == torch.float32
        xr2 = x32.double().cpu().clone().requires_grad_(True)
        lw2, lb2 = ln_w.double().cpu().clone().requires_grad_(True), ln_b.double().cpu().clone().requires_grad_(True)
        (torch.nn.functional.layer_norm(xr2, (C,), lw2, lb2, 1e-5) * dxn).sum().backward()
        # fp32 arithmetic on exactly representable operands: fp32 rounding only
        res["f32_rows"] = (close(d[0], xr2.grad + dres.double().cpu(), 2e-5, what="dx of fp32 rows"), close(d[1], lw2.grad, 2e-5, what="dgamma of fp32 rows"),
                           close(d[2], lb2.grad, 2e-5, what="dbeta of fp32 rows"))
    return res


@guarded
def check_fold_bwd_forms_dm(dev, dtype, C=64, heads=2, B=3, N=256):
    """mphsir_spectral_fold_bwd forming dM = d_out^T v itself (N > 0: the lower pyramid levels) against the token-reduction GEMM followed
    by the plain call, and dM against an fp64 product of the same operands"""
    _use(dev)
    from mp_hsir_amd import ops
    hd = C // heads
    assert ops.fold_bwd_forms_dm(N, C, heads, dtype)
    gp = rnd((B, 1, heads, hd, hd), 611)
    sp = rnd((B, 1, 2, C), 612).abs() + 0.5
    temp = (rnd((heads,), 613, scale=0.3, shift=1)).contiguous()
    wo = rnd((C, C), 614, scale=C ** -0.5)
    d_out, v = rnd((B * N, C), 615, dtype), rnd((B * N, C), 616, dtype)
    dm = ops.gemm_tn(d_out.reshape(B, N, C), v.reshape(B, N, C), reduce=False)
    a = ops.spectral_fold_bwd(gp, sp, temp, wo, dm, dtype, reduce=False)
    b = ops.spectral_fold_bwd(gp, sp, temp, wo, None, dtype, reduce=False, d_out=d_out, v=v)
    # fp64 reference of W2 / dWo / dtemp through the plain call on an fp64-accurate dM
    dm64 = inp(torch.einsum("bnc,bnd->bcd", d_out.double().cpu().reshape(B, N, C), v.double().cpu().reshape(B, N, C)).float())
    c = ops.spectral_fold_bwd(gp, sp, temp, wo, dm64.contiguous(), dtype, reduce=False)
    res = {}
    for name, x, y, z in zip(("W2", "dWo", "dtemp"), a, b, c):
        tol = 1e-5 if x.dtype == torch.float32 else 4e-3
        res[name] = (close(y, x.double().cpu(), tol, what=name + " vs gemm_tn"), close(y, z.double().cpu(), tol, what=name + " vs fp64 dM"))
    # w2_blocks: only each head's own column blocks of its q / k rows are written (what the fused backward reads) -- those entries are
    # BITWISE the dense call's, everything outside them is left alone (here: the NaN the buffer was filled with is not visible in W2's
    # blocks, and the dense W2 is zero outside them)
    for kw in (dict(dM=dm), dict(dM=None, d_out=d_out, v=v)):
        dM_ = kw.pop("dM")
        dense = ops.spectral_fold_bwd(gp, sp, temp, wo, dM_, dtype, reduce=False, **kw)
        blk = ops.spectral_fold_bwd(gp, sp, temp, wo, dM_, dtype, reduce=False, w2_blocks=True, **kw)
        mask = alloc((2 * C, 2 * C), torch.bool)
        for h in range(heads):
            for r0 in (h * hd, C + h * hd):
                mask[r0:r0 + hd, h * hd:(h + 1) * hd] = True
                mask[r0:r0 + hd, C + h * hd:C + (h + 1) * hd] = True
        assert torch.equal(blk[0][:, mask], dense[0][:, mask]) and float(dense[0][:, ~mask].float().abs().max()) == 0.0
        assert torch.equal(blk[1], dense[1]) and torch.equal(blk[2], dense[2])
    return res


@guarded
def check_spectral_dqkv_bwd(dev, dtype, C, heads, shape, nblk=None):
    """mphsir_spectral_dqkv_bwd (dv, [dq | dk], depthwise backward + tap gradients in one launch) against the three launches it replaces
    -- gemm_tok(d_out, M_b^T), gemm_tok([q | k], W2), dwconv3x3_bwd -- on the same operands:
      * round_dall=1: [dq | dk | dv] rounded to the storage type as the three-launch path stores it -> dt BITWISE equal (head widths whose
        K chunks align with the token GEMM's: 32 / 64), tap gradients within fp32 summation order;
      * the product form (fp32 [dq | dk | dv] in LDS): within the storage type's rounding of the three-launch path, and closer to an fp64
        evaluation of the same formula than it."""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    M, hd = B * H * W, C // heads
    assert ops.spectral_dqkv_bwd_fits(C, heads, H, W, dtype), (C, heads, shape)
    qk, d_out, t = rnd((M, 2 * C), 901, dtype), rnd((M, C), 902, dtype), rnd((M, 3 * C), 903, dtype)
    W2 = alloc((B, 2 * C, 2 * C), role="input")          # the block structure spectral_fold_bwd emits
    full = rnd((B, 2 * C, 2 * C), 904, scale=(2 * hd) ** -0.5)
    for h in range(heads):
        qs, ks = slice(h * hd, (h + 1) * hd), slice(C + h * hd, C + (h + 1) * hd)
        W2[:, qs, ks] = full[:, qs, ks]
        W2[:, ks, qs] = full[:, ks, qs]
    idx = inp(torch.arange(2 * C))
    W2[:, idx, idx] = full[:, idx, idx]
    W2 = W2.to(dtype).contiguous()
    MbT = rnd((B, C, C), 905, dtype, scale=C ** -0.5)
    w9 = rnd((9, 3 * C), 906, scale=1 / 3)
    # the three launches
    dall = alloc((M, 3 * C), dtype, fill=None)
    ops.gemm_tok(d_out, MbT, out=dall[:, 2 * C:])
    ops.gemm_tok(qk, W2, out=dall[:, :2 * C])
    with ops.reduce_scope():
        dt_ref, dw_ref = ops.dwconv3x3_bwd(t.reshape(B, H, W, 3 * C), dall.reshape(B, H, W, 3 * C), w9, col_ranges=[(0, 3 * C)])
    dt_ref = dt_ref.reshape(M, 3 * C)
    res = {}
    for nb in ([nblk] if nblk else [None, 1, 3]):
        with ops.reduce_scope():
            dt_r, dw_r = ops.spectral_dqkv_bwd(qk, d_out, t, W2, MbT, w9, B, H, W, C, heads, nblk=nb, round_dall=True)
        if hd in (32, 64):
            assert torch.equal(dt_r, dt_ref), ("dt not bitwise the three-launch path's", C, heads, shape, nb, rel_l2(dt_r, dt_ref))
        else:
            close(dt_r, dt_ref, 3e-3, geom=(B, H, W), what="dt rounded vs three launches")
        res["dw_round_%s" % nb] = close(dw_r, dw_ref, 1e-5 if hd in (32, 64) else 3e-3, geom=(B, H, W), what="dw rounded vs three launches")
    with ops.reduce_scope():
        dt_f, dw_f = ops.spectral_dqkv_bwd(qk, d_out, t, W2, MbT, w9, B, H, W, C, heads, nblk=nblk)
    # fp64 evaluation of the same formula on the same (rounded) operands
    qk64, do64, t64, w964 = qk.double().cpu(), d_out.double().cpu(), t.double().cpu(), w9.double().cpu()
    d64 = torch.empty((M, 3 * C), dtype=torch.float64)
    for b in range(B):
        rows = slice(b * H * W, (b + 1) * H * W)
        d64[rows, :2 * C] = qk64[rows] @ W2[b].double().cpu().t()
        d64[rows, 2 * C:] = do64[rows] @ MbT[b].double().cpu().t()
    dy = d64.reshape(B, H, W, 3 * C).permute(0, 3, 1, 2)
    wk = w964.t().reshape(3 * C, 1, 3, 3)
    tt = t64.reshape(B, H, W, 3 * C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wk = wk.clone().requires_grad_(True)
    (torch.nn.functional.conv2d(tt, wk, padding=1, groups=3 * C) * dy).sum().backward()
    dt64 = tt.grad.permute(0, 2, 3, 1).reshape(M, 3 * C)
    dw64 = wk.grad.reshape(3 * C, 9)
    tol = TOL[dtype]
    res.update(dt=close(dt_f, dt64, tol, geom=(B, H, W), what="dt"), dt_three=rel_l2(dt_ref, dt64),
               dw=close(dw_f, dw64, tol, geom=(B, H, W), what="dw"), dw_three=rel_l2(dw_ref, dw64))
    assert res["dt"] <= res["dt_three"] * 1.05 and res["dw"] <= res["dw_three"] * 1.05 + 1e-6, res
    return res


@guarded
def check_channel_attention_bwd(dev, dtype, C, heads, shape, cross=False, inputs="unit"):
    """The channel ("spectral") attention backward chain -- gemm_tn (dM), spectral_fold_bwd, the [dq|dk] / dv token GEMMs,
    depthwise backward + tap gradients -- as the prompt modules use it (self: TransformerBlock :289-322; cross:
    CrossTransformer :220-249), against fp64 autograd of the oracle."""
    _use(dev)
    from mp_hsir_amd import autograd_ops as AG
    from mp_hsir_amd import ops
    B, H, W = shape
    M = B * H * W
    pk = inputs == "peaked"          # temperature x 8, k channel 3 x 2^-10; no zero channel: below the clamp the derivative is 1e12 in the reference too
    assert inputs == "unit" or pk
    P = {"temperature": rnd((heads, 1, 1), 331, scale=0.3 * (8 if pk else 1), shift=8 if pk else 1), "project_out.weight": rnd((C, C, 1, 1), 332, scale=C ** -0.5)}
    if cross:
        P.update({"q.weight": rnd((C, C, 1, 1), 333, scale=C ** -0.5),
                  "kv.weight": rnd((2 * C, C, 1, 1), 334, scale=C ** -0.5, edit=peaked_qkv_edit(C, 2.0 ** -5, k_row0=0) if pk else None),
                  "q_dwconv.weight": rnd((C, 1, 3, 3), 335, scale=1 / 3),
                  "kv_dwconv.weight": rnd((2 * C, 1, 3, 3), 336, scale=1 / 3, edit=peaked_qkv_edit(C, 2.0 ** -5, k_row0=0) if pk else None)})
    else:
        P.update({"qkv.weight": rnd((3 * C, C, 1, 1), 333, scale=C ** -0.5, edit=peaked_qkv_edit(C, 2.0 ** -5) if pk else None),
                  "qkv_dwconv.weight": rnd((3 * C, 1, 3, 3), 335, scale=1 / 3, edit=peaked_qkv_edit(C, 2.0 ** -5) if pk else None)})
    xq, xkv = rnd((B, H, W, C), 337, dtype), rnd((B, H, W, C), 338, dtype)
    d_out = rnd((M, C), 339, dtype)
    temp = P["temperature"].reshape(heads).contiguous()
    wo = P["project_out.weight"].reshape(C, C).contiguous()
    if cross:
        tq = ops.gemm_tok(xq.reshape(M, C), P["q.weight"].reshape(C, C).to(dtype))
        tkv = ops.gemm_tok(xkv.reshape(M, C), P["kv.weight"].reshape(2 * C, C).to(dtype))
        w9 = torch.cat([ops.pack_dw(P["q_dwconv.weight"]), ops.pack_dw(P["kv_dwconv.weight"])], 1).contiguous()
        t_q, t_k, t_v = tq, tkv[:, :C], tkv[:, C:]
        v4 = lambda t, n: t.reshape(B, H, W, n)
        tq4, tkv4 = v4(tq, C), v4(tkv, 2 * C)
        views = (tq4, tkv4[..., :C], tkv4[..., C:])
    else:
        t = ops.gemm_tok(xq.reshape(M, C), P["qkv.weight"].reshape(3 * C, C).to(dtype))
        w9 = ops.pack_dw(P["qkv_dwconv.weight"])
        t_q, t_k, t_v = t[:, :C], t[:, C:2 * C], t[:, 2 * C:]
        t4 = t.reshape(B, H, W, 3 * C)
        views = (t4[..., :C], t4[..., C:2 * C], t4[..., 2 * C:])
    v, gp, sp, _ = ops.dwconv_gram(t_q, t_k, t_v, w9[:, :C], w9[:, C:2 * C], w9[:, 2 * C:], 3 * C, B, H, W, C, heads)
    Mb, MbT, gp, sp = ops.spectral_fold(gp, sp, temp, wo, dtype, transposed=True)
    out = ops.gemm_tok(v, Mb)
    with ops.reduce_scope():
        if cross:
            dtq, dkv, dw, dtemp, dwo = AG.channel_attention_bwd_cross(d_out, tq4, tkv4, w9, v, gp, sp, MbT, P["temperature"], P["project_out.weight"], heads)
            assert dtq.shape == (B, H, W, C) and dkv.shape == (M, 2 * C)
            dkv4 = dkv.reshape(B, H, W, 2 * C)
            dtk, dtv = dkv4[..., :C], dkv4[..., C:]
        else:
            dt_all, dw, dtemp, dwo = AG.channel_attention_bwd_self(d_out, t4, w9, v, gp, sp, MbT, P["temperature"], P["project_out.weight"], heads)
            assert dt_all.shape == (M, 3 * C)
            dt4 = dt_all.reshape(B, H, W, 3 * C)
            dtq, dtk, dtv = dt4[..., :C], dt4[..., C:2 * C], dt4[..., 2 * C:]
    assert dw.shape == (3 * C, 9) and dw.dtype == torch.float32
    dwq, dwk, dwv = dw[:C], dw[C:2 * C], dw[2 * C:]            # the per-tensor gradients: slices of the joined buffers the entry points return
    # oracle on the 1x1-conv outputs as the kernels saw them (dtype-rounded), fp64 from there on
    tqd = views[0].detach().double().cpu().requires_grad_(True)
    tkd = views[1].detach().double().cpu().requires_grad_(True)
    tvd = views[2].detach().double().cpu().requires_grad_(True)
    w9d = w9.double().cpu().requires_grad_(True)                                # [9][3C] tap-major
    wd = w9d.t().reshape(3 * C, 1, 3, 3)
    Td = {"temperature": P["temperature"].double().cpu().requires_grad_(True), "wo": P["project_out.weight"].double().cpu().requires_grad_(True)}
    q = O.depthwise3x3(tqd, wd[:C])
    k = O.depthwise3x3(tkd, wd[C:2 * C])
    vv = O.depthwise3x3(tvd, wd[2 * C:])
    ref = O._channel_attention_core(q, k, vv, Td["temperature"], Td["wo"], heads)
    own = {}

    def in_dtype(what):
        def f(c):
            if not own:
                with torch.enable_grad():
                    lv = [c(views[i].detach()).requires_grad_(True) for i in range(3)]
                    w9c = c(w9).requires_grad_(True)
                    wc = w9c.t().reshape(3 * C, 1, 3, 3)
                    tc, woc = c(P["temperature"]).requires_grad_(True), c(P["project_out.weight"]).requires_grad_(True)
                    oc = O._channel_attention_core(O.depthwise3x3(lv[0], wc[:C]), O.depthwise3x3(lv[1], wc[C:2 * C]), O.depthwise3x3(lv[2], wc[2 * C:]), tc, woc, heads)
                    (oc * c(d_out).reshape(B, H, W, C)).sum().backward()
                g9 = w9c.grad.t()
                own.update(out=oc.detach(), dtq=lv[0].grad, dtk=lv[1].grad, dtv=lv[2].grad, dtemp=tc.grad, dwo=woc.grad, dw_q=g9[:C], dw_k=g9[C:2 * C], dw_v=g9[2 * C:])
            return own[what]
        return f
    close(out.reshape(B, H, W, C), ref.detach(), yard_bar(inputs, dtype, TOL[dtype] * 2, "out", ref.detach(), in_dtype("out")), geom=(B, H, W), what="out")
    (ref * d_out.double().cpu().reshape(B, H, W, C)).sum().backward()
    tol = GTOL[dtype] / (2 if dtype == torch.bfloat16 else 1)
    got = {"dtq": dtq, "dtk": dtk, "dtv": dtv, "dtemp": dtemp.reshape(heads, 1, 1), "dwo": dwo.reshape(C, C, 1, 1),
           "dw_q": dwq, "dw_k": dwk, "dw_v": dwv}
    dw9 = w9d.grad.t()                                                          # (3C, 9)
    want = {"dtq": tqd.grad, "dtk": tkd.grad, "dtv": tvd.grad, "dtemp": Td["temperature"].grad, "dwo": Td["wo"].grad,
            "dw_q": dw9[:C], "dw_k": dw9[C:2 * C], "dw_v": dw9[2 * C:]}
    errs = {n: rel_l2(got[n], want[n]) for n in got}
    bars = {n: yard_bar(inputs, dtype, tol, n, want[n], in_dtype(n)) for n in got}
    bad = {n: e for n, e in errs.items() if not e < bars[n]}
    assert not bad, (C, heads, shape, str(dtype), bad)
    for n in got:
        close(got[n], want[n], bars[n], geom=(B, H, W), what=n, whole=errs[n])
    return errs


@guarded
def check_channel_attention_bwd_refuses_layouts(dev, dtype=torch.float32, C=64, heads=2, shape=(1, 16, 16)):
    """The self entry point declares its layouts -- t one contiguous (B,H,W,3C), w9 one contiguous fp32 (9,3C) -- and raises on anything
    else BEFORE any launch: there is no slower path to fall to."""
    _use(dev)
    from mp_hsir_amd import autograd_ops as AG
    from mp_hsir_amd import ops
    B, H, W = shape
    M, hd = B * H * W, C // heads
    d_out, v = rnd((M, C), 341, dtype), rnd((M, C), 342, dtype)
    gp, sp = rnd((B, 1, heads, hd, hd), 343), rnd((B, 1, 2, C), 344).abs() + 1
    MbT = rnd((B, C, C), 345, dtype, scale=C ** -0.5)
    temp, wo = rnd((heads, 1, 1), 346, scale=0.3, shift=1), rnd((C, C, 1, 1), 347, scale=C ** -0.5)
    t, w9 = rnd((B, H, W, 3 * C), 348, dtype), rnd((9, 3 * C), 349, scale=1 / 3)
    wide_t, wide_w9 = rnd((B, H, W, 4 * C), 350, dtype), rnd((9, 4 * C), 351, scale=1 / 3)
    bad = {"t: pitch 4C": (wide_t[..., :3 * C], w9),
           "t: (M,3C)": (t.reshape(M, 3 * C), w9),
           "w9: pitch 4C": (t, wide_w9[:, :3 * C]),
           "w9: (3C,9) transposed": (t, rnd((3 * C, 9), 352, scale=1 / 3).t()),
           "w9: not fp32": (t, w9.to(torch.float64))}
    for what, (t_, w9_) in bad.items():
        ops.ACCOUNT = {}
        try:
            try:
                AG.channel_attention_bwd_self(d_out, t_, w9_, v, gp, sp, MbT, temp, wo, heads)
            except AssertionError as e:
                assert "stride" in str(e) and str(tuple(t_.shape if what[0] == "t" else w9_.shape)) in str(e), (what, str(e))
            else:
                raise RuntimeError("channel_attention_bwd_self accepted " + what)
            assert not ops.ACCOUNT, (what, "launched before refusing", sorted(ops.ACCOUNT))
        finally:
            ops.ACCOUNT = None


@guarded
def check_join_gradients(dev, shape=(1, 8, 16), C=32):
    """The joins that complete a buffer whose right half its producer already wrote (conv1x1(out=) -> _JoinLeft, conv3x3(out=) ->
    shuffle_join) against the same producers followed by torch.cat / pixel_shuffle2, fp32: the output and the gradients of both halves'
    inputs and of the conv weight, bit for bit (the same kernels on the same values: only the row pitch they go through differs)."""
    _use(dev)
    from mp_hsir_amd import autograd_ops as AG
    B, H, W = shape
    cot = rnd((B, H, W, 2 * C), 366)

    def run(left, ksize, joined):
        conv = torch.nn.Conv2d(C, C, ksize, padding=ksize // 2, bias=False).to(dev)
        with torch.no_grad():
            conv.weight.copy_(rnd(conv.weight.shape, 361, scale=(C * ksize * ksize) ** -0.5))
        produce = AG.conv1x1 if ksize == 1 else AG.conv3x3
        lshape = (B, H, W, C) if left == "plain" else (B, H // 2, W // 2, 4 * C)
        x, yin = rnd(lshape, 362).requires_grad_(True), rnd((B, H, W, C), 363).requires_grad_(True)
        if joined:
            buf = alloc((B, H, W, 2 * C), fill=None)
            p = produce(yin, conv, out=buf[..., C:])
            j = AG._JoinLeft.apply(x, p, buf) if left == "plain" else AG.shuffle_join(x, p, buf)
        else:
            j = torch.cat([x if left == "plain" else AG.pixel_shuffle2(x), produce(yin, conv)], dim=-1)
        (j * cot).sum().backward()
        return j.detach(), x.grad, yin.grad, conv.weight.grad

    for left, ksize in (("plain", 1), ("shuffled", 3), ("shuffled", 1)):
        got, want = run(left, ksize, True), run(left, ksize, False)
        for name, g, w in zip(("out", "d left", "d producer input", "d conv weight"), got, want):
            assert g is not None and g.shape == w.shape and torch.equal(g, w), (left, ksize, name, rel_l2(g, w))


@guarded
def check_loss_scaler(dev):
    """mphsir_grad_check / flat_adamw_scaled / scaler_update against torch.optim.AdamW + the GradScaler rules: a finite step equals
    AdamW on the unscaled gradient, an overflowing step changes nothing but halves the scale and restarts the streak (and
    does not advance Adam's step count), `interval` good steps double the scale."""
    _use(dev)
    from mp_hsir_amd import ops
    n = 4096
    p0 = rnd((n,), 401)
    p, m, v = alloc((n,), fill=None).copy_(p0), alloc((n,)), alloc((n,))
    ref = torch.nn.Parameter(p0.detach().cpu().clone())
    opt = torch.optim.AdamW([ref], lr=1e-2)
    sc = ops.new_loss_scaler(dev, 1024.0)
    for step in range(5):
        g = rnd((n,), 410 + step)
        scaled = g * float(sc[0])
        if step == 2:
            scaled = scaled.clone()
            scaled[17] = float("inf")
        before = (p.clone(), m.clone(), v.clone(), sc.clone())
        ops.scaled_adamw_step(p, scaled, m, v, sc, 1e-2, interval=2)
        if step == 2:
            assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])
            assert float(sc[0]) == float(before[3][0]) * 0.5 and float(sc[1]) == 0.0 and float(sc[2]) == 0.0 and float(sc[3]) == float(before[3][3])
            continue
        ref.grad = g.detach().cpu().clone()
        opt.step()
        close(p, ref.detach(), 2e-6, what="p after step %d" % step)
    # steps 0,1 good -> x2 after the second; step 2 overflow -> /2; steps 3,4 good -> x2
    assert float(sc[0]) == 1024.0 * 2 * 0.5 * 2 and float(sc[3]) == 4.0


@guarded
def check_layernorm_tok(dev, dtype, M=200, C=64, inputs="unit"):
    """mphsir_layernorm_tok (TVSP's norm11, net/MP_HSIR.py:282: fp32 rows in, compute dtype out) against F.layer_norm in fp64; the optional
    cast copy of the input BITWISE against .to(dtype); the vector form (C % 16 == 0) and the element-wise form (C % 4 == 0)"""
    _use(dev)
    from mp_hsir_amd import ops
    lw, lb = (rnd((C,), 521, scale=0.2, shift=1)).contiguous(), (rnd((C,), 522, scale=0.1)).contiguous()
    for src in (torch.float32, dtype):
        x = rnd((M, C), 523, src, profile=row_profile(inputs))
        y, xc = ops.layernorm_tok(x, lw, lb, dtype, want_cast=True)
        want = torch.nn.functional.layer_norm(x.double().cpu(), (C,), lw.double().cpu(), lb.double().cpu(), 1e-5)
        assert y.dtype == dtype
        tol = yard_bar(inputs, dtype, TOL[dtype], "y", want, lambda c: O.layer_norm_c(c(x), c(lw), c(lb)))
        close(y, want, tol, what="y")
        assert torch.equal(xc, x.to(dtype))
        assert torch.equal(ops.layernorm_tok(x, lw, lb, dtype), y)


@guarded
def check_heads(dev, dtype, B=3, C=31, H=24, W=20, T=6, n=2):
    """heads.hip against the framework expressions they replace (net/MP_HSIR.py:519-527, :824, :842-843): the layout kernels BITWISE
    (one rounding each, the same one), the task-prompt algebra to fp32 rounding, forward and backward through the autograd wrappers."""
    _use(dev)
    import torch.nn.functional as F
    from mp_hsir_amd import ops
    from mp_hsir_amd import autograd_ops as AG
    inp = rnd((B, C, H, W), 511)
    cp = ops.round_up(C, 32)
    x = ops.nchw_to_cl(inp, dtype, cp)
    ref = F.pad(inp.to(dtype).permute(0, 2, 3, 1), (0, cp - C)).contiguous()
    assert x.shape == ref.shape and torch.equal(x, ref)
    y = rnd((B, H, W, cp), 512, dtype)
    o = ops.cl_to_nchw_add(y, C, inp)
    assert torch.equal(o, y[..., :C].permute(0, 3, 1, 2).to(torch.float32) + inp)
    assert torch.equal(ops.cl_to_nchw_add(y, C), y[..., :C].permute(0, 3, 1, 2).to(torch.float32).contiguous())
    # autograd: d(output head) = the layout kernel on the incoming gradient; the padded channels get zeros
    yg = y.clone().requires_grad_(True)
    g = rnd((B, C, H, W), 513)
    AG._OutputHead.apply(yg, inp).backward(g)
    assert torch.equal(yg.grad, F.pad(g.to(dtype).permute(0, 2, 3, 1), (0, cp - C)).contiguous())
    ig = inp.clone().requires_grad_(True)
    gx = rnd((B, H, W, cp), 514, dtype)
    AG._InputHead.apply(ig, dtype).backward(gx)
    assert torch.equal(ig.grad, gx[..., :C].permute(0, 3, 1, 2).to(torch.float32).contiguous())
    # task weights + weighted means
    ids = as_input(torch.randint(0, T, (B, n), generator=torch.Generator().manual_seed(515)))
    w = ops.task_weights(ids, T)
    wr = F.one_hot(ids, T).float().mean(dim=1)
    assert torch.equal(w, wr)
    table = rnd((1, T, 40, 1, 1), 516).requires_grad_(True)          # text_prompt_learnable's shape
    L = AG.mix_rows(w, table)
    tr = table.detach().clone().requires_grad_(True)
    Lr = (wr.unsqueeze(-1) * tr[0, :, :, 0, 0].unsqueeze(0)).mean(dim=1)
    close(L, Lr.detach(), 1e-6, geom=(B, H, W), what="L")              # (B, 40): not a token tensor, the view leaves it alone
    dL = rnd(L.shape, 517)
    L.backward(dL)
    Lr.backward(dL)
    assert table.grad.shape == table.shape
    close(table.grad, tr.grad, 1e-6, geom=(B, H, W), what="d table")


@guarded
def check_resamplers(dev, dtype, B=3, ps=16, D=32, H=40, W=24):
    """mphsir_tvsp_text_map (+bwd) against the reference's own expression (broadcast multiply + F.interpolate nearest,
    net/MP_HSIR.py:575-577) and mphsir_resize_bilinear (+bwd) against F.interpolate(bilinear) (:580), fp64 autograd."""
    _use(dev)
    import torch.nn.functional as F
    from mp_hsir_amd import ops
    L, clip = rnd((B, D), 501), rnd((B, 512), 502)
    text = ops.tvsp_text_map(L, clip, ps)
    Ld, cd = L.double().cpu().requires_grad_(True), clip.double().cpu()
    ref = F.interpolate(Ld.reshape(B, D, 1, 1) * cd.reshape(1, 1, B, 512).expand(B, 1, B, 512), (ps, ps), mode="nearest")   # (B,D,ps,ps)
    close(text, ref.detach().permute(0, 2, 3, 1), 2e-7, geom=(B, ps, ps), what="text map")
    dt = rnd((B, ps, ps, D), 503)
    ref.backward(dt.double().cpu().permute(0, 3, 1, 2))
    close(ops.tvsp_text_map_bwd(dt, clip), Ld.grad, 2e-6, geom=(B, ps, ps), what="dL")
    x = rnd((B, ps, ps, D), 504, dtype)
    y = ops.resize_bilinear(x, H, W)
    xd = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.interpolate(xd, (H, W), mode="bilinear", align_corners=False)
    close(y, yr.detach().permute(0, 2, 3, 1), TOL[dtype], geom=(B, H, W), what="y")
    dy = rnd((B, H, W, D), 505, dtype)
    yr.backward(dy.double().cpu().permute(0, 3, 1, 2))
    close(ops.resize_bilinear(dy, ps, ps, backward=True), xd.grad.permute(0, 2, 3, 1), TOL[dtype], geom=(B, ps, ps), what="dx")


# ---- edge shapes: for each entry point the smallest shape its MPHSIR_REQUIREs and *_fits predicates accept, so that an overrun of one
# tile falls into a guard band (tests/guard.py) rather than into the tensor, and one shape with a ragged tail where the kernel has one.
# (name, check, args after (dev, dtype), kwargs, dtypes: None = fp32 + bf16, "half" = bf16 + fp16, "none" = the check takes no dtype)
EDGE_CASES = [
    ("gemm_tok_min", "gemm_tok", (64, 16, 32, False, 0), {}, None),                    # M % 64, N % 16, K % 32: one tile of each
    ("gemm_tok_min_ln_res", "gemm_tok", (64, 16, 32, True, 1), {}, None),
    ("gemm_tok_ring_min", "gemm_tok_ring", (64, 16, 32, 0), {}, "half"),               # fewer tiles than workgroups
    ("gemm_tok_ring_res", "gemm_tok_ring", (256, 32, 32, 1), {}, "half"),
    ("gated_mlp_min", "gated_mlp", (32, 85), dict(M=64), None),
    ("gated_mlp_min_two_tiles", "gated_mlp", (32, 85), dict(M=64, tpw=2), None),
    ("gated_mlp_min_eight_waves", "gated_mlp", (32, 85), dict(M=64, tpw=3), "half"),
    ("gated_mlp_min_res", "gated_mlp", (32, 85), dict(M=64, res=True), None),
    ("gated_mlp_bwd_min", "gated_mlp_bwd", (32, 85), dict(M=64), None),                # one 64-row tile: dx / xn / h / dpre / dm end with it
    ("gated_mlp_bwd_min_variant1", "gated_mlp_bwd", (32, 85), dict(M=64, variant=1), None),
    ("gated_mlp_bwd_min_variant3", "gated_mlp_bwd", (32, 85), dict(M=64, variant=3), None),
    ("gated_mlp_bwd_min_variant4", "gated_mlp_bwd", (32, 85), dict(M=64, variant=4), None),
    ("gated_mlp_bwd_min_hsplit", "gated_mlp_bwd", (96, 255), dict(M=64, hsplit=2), "half"),   # the fp32 partials dxn_part (hsplit, M, C)
    ("dwconv_gram_one_row", "spectral_attention_chain", (32, 2, (1, 1, 64), 1), {}, None),      # H = 1: both halo rows outside the image
    ("dwconv_gram_one_row_split", "spectral_attention_chain", (32, 2, (1, 1, 128), 2), {}, None),
    ("dwconv_gram_8x8", "spectral_attention_chain", (32, 2, (1, 8, 8), 1), {}, None),
    ("layernorm_one_row", "layernorm_tok", (), dict(M=1, C=4), None),
    ("layernorm_63x20", "layernorm_tok", (), dict(M=63, C=20), None),
    ("layernorm_65x16", "layernorm_tok", (), dict(M=65, C=16), None),
    ("gemm_tn_one_row", "gemm_tn", (1, 8, 8, 1, 0), {}, None),
    ("gemm_tn_8_rows", "gemm_tn", (8, 8, 8, 1, 0), {}, None),
    ("gemm_tn_130_rows", "gemm_tn", (130, 8, 8, 2, 0), {}, None),
    ("dwconv_one_row", "dwconv_plain", ((1, 1, 8, 32),), {}, None),                     # both halo rows lie outside the image
    ("dwconv_8x8", "dwconv_plain", ((1, 8, 8, 32),), {}, None),
    ("dwconv_one_row_c8", "dwconv_plain", ((1, 1, 8, 8),), {}, None),
    ("conv3x3_64_tokens", "conv3x3", (1, 8, 8, 32, 16), {}, None),
    ("combine_bwd_one_window", "combine_bwd", (), dict(C=64, shift=0, shape=(1, 8, 8)), None),
    ("combine_bwd_one_window_shifted", "combine_bwd", (), dict(C=64, shift=4, shape=(1, 8, 8)), None),
    ("ln_bwd_win_dxn_one_window", "ln_bwd_win_dxn", (), dict(C=64, shape=(1, 8, 8), shift=0), "half"),
    ("ln_bwd_win_dxn_one_window_shifted", "ln_bwd_win_dxn", (), dict(C=64, shape=(1, 8, 8), shift=4), "half"),
    ("win_attn_bwd_one_window", "win_attn_bwd_head_split", (), dict(C=64, heads=2, shape=(1, 8, 8)), "half"),
    ("heads_one_channel", "heads", (), dict(B=1, C=1, H=8, W=8), None),
    ("heads_172_channels", "heads", (), dict(B=1, C=172, H=8, W=8, T=7, n=1), None),
    ("resamplers_min", "resamplers", (), dict(B=1, ps=2, D=8, H=4, W=4), None),           # D = 8: one 16-byte vector of a 16-bit row
    ("pg_gate_fwd_one_window", "pg_gate_fwd", (128, 8), dict(nW=1), "none"),
    ("pg_gate_fwd_17_windows", "pg_gate_fwd", (128, 8), dict(nW=17), "none"),
    ("pg_gate_bwd_one_window", "pg_gate_bwd", (128, 8), dict(nW=1), "none"),
    ("pg_gate_bwd_17_windows", "pg_gate_bwd", (128, 8), dict(nW=17), "none"),
    ("reduce_block_one_row", "reduce_block", (), {}, "none"),
]
WIN_EDGE_CASES = [("tiny", "encoder_level1.blocks.1.", 1, 0, (1, 8, 8, 32)), ("tiny", "encoder_level1.blocks.1.", 1, 4, (1, 8, 8, 32))]      # a single window


def edge_params():
    """(id, check name, args, kwargs, dtype or None) for pytest.mark.parametrize, the dtypes expanded"""
    out = []
    for name, fn, a, kw, dts in EDGE_CASES:
        for dt in {None: DTYPES, "half": [torch.bfloat16, torch.float16], "none": [None]}[dts]:
            out.append((name + ("" if dt is None else "-" + str(dt).replace("torch.", "")), fn, a, kw, dt))
    return out


def run_edge(dev, fn, a, kw, dt):
    check = globals()["check_" + fn]
    return check(dev, *a, **kw) if dt is None else check(dev, dt, *a, **kw)


# ---- the checks under input profiles (INPUT_PROFILES): each at the smallest shapes it has, because the host fp64 reference and the
# yardstick are what cost time.  (id, check, args after (dev, dtype), kwargs, profiles, GPU dtypes as in EDGE_CASES, emulator dtype:
# bf16 for the forms that exist in 16 bits only, fp32 otherwise).  The bar of every comparison is yard_bar's.
_F32, _BF = torch.float32, torch.bfloat16
PROFILE_CASES = [
    ("layernorm_200x64", "layernorm_tok", (), dict(M=200, C=64), ("offset", "flat", "outlier"), None, _F32),
    ("layernorm_63x20", "layernorm_tok", (), dict(M=63, C=20), ("offset", "flat", "outlier"), None, _F32),
    ("gemm_tok_ln_64", "gemm_tok", (64, 16, 32, True, 1), {}, ("offset", "flat"), None, _F32),
    ("gemm_tok_ln_128", "gemm_tok", (128, 96, 96, True, 0), {}, ("offset", "flat"), None, _F32),
    ("gated_mlp_32", "gated_mlp", (32, 85), dict(M=128), ("flat", "outlier", "gain"), None, _F32),
    ("gated_mlp_96", "gated_mlp", (96, 255), dict(M=128), ("flat", "outlier", "gain"), None, _F32),
    ("gated_mlp_32_eight_waves", "gated_mlp", (32, 85), dict(M=128, tpw=3), ("flat", "outlier", "gain"), "half", _BF),
    ("gated_mlp_96_eight_waves", "gated_mlp", (96, 255), dict(M=128, tpw=3), ("flat", "outlier", "gain"), "half", _BF),
    # the hidden split needs HP % (32 hsplit) == 0: (32, 85) has HP = 96, so its smallest shape is (96, 255), forward and backward
    ("gated_mlp_96_hsplit", "gated_mlp", (96, 255), dict(M=128, hsplit=2), ("flat", "outlier", "gain"), "half", _BF),
    ("gated_mlp_bwd", "gated_mlp_bwd", (32, 85), {}, ("flat", "gain"), None, _F32),
    ("gated_mlp_bwd_variant1", "gated_mlp_bwd", (32, 85), dict(variant=1), ("flat", "gain"), None, _F32),
    ("gated_mlp_bwd_variant3", "gated_mlp_bwd", (32, 85), dict(variant=3), ("flat", "gain"), None, _F32),
    ("gated_mlp_bwd_variant4", "gated_mlp_bwd", (32, 85), dict(variant=4), ("flat", "gain"), None, _F32),
    ("gated_mlp_bwd_hsplit", "gated_mlp_bwd", (96, 255), dict(hsplit=2), ("flat", "gain"), "half", _BF),
    ("gdfn_fused", "gdfn_fused", (64, 170, (1, 8, 16), None), {}, ("flat", "gain"), "half", _BF),
    ("fused_pass_a_ln", "fused_pass_a", (64, 4, (1, 16, 16), 1, True), {}, ("flat", "outlier"), None, _F32),
    ("fused_pass_a_rows_ln", "fused_pass_a", (64, 2, (1, 8, 32), None, True), dict(row_segments=1), ("flat", "outlier"), "half", _BF),
    ("ln_bwd_win_dxn_one_window", "ln_bwd_win_dxn", (), dict(C=64, shape=(1, 8, 8), shift=4), ("offset", "flat"), "half", _BF),
    ("ln_bwd_win_dxn_2x16x16", "ln_bwd_win_dxn", (), dict(C=64, shape=(2, 16, 16), shift=4), ("offset", "flat"), "half", _BF),
    ("ln_bwd_tok_dxn", "ln_bwd_tok_dxn", (), dict(C=64, K=384, M=256), ("offset", "flat"), "half", _BF),
    ("spectral_chain_32", "spectral_attention_chain", (32, 2, (1, 8, 16), 1), {}, ("peaked",), None, _F32),
    ("spectral_chain_64", "spectral_attention_chain", (64, 2, (1, 16, 16), 2), {}, ("peaked",), None, _F32),
    ("channel_attention_bwd", "channel_attention_bwd", (64, 2, (1, 16, 16), False), {}, ("peaked",), None, _F32),
    # 16-bit, N <= 1024, heads of 32 / 64: the fold backward forms dM = d_out^T v itself (ops.fold_bwd_forms_dm) -- the form
    # check_fold_bwd_forms_dm compares with its own plain call; here it stands against fp64 autograd with small k norms
    ("channel_attention_bwd_forms_dm", "channel_attention_bwd", (64, 2, (1, 16, 16), False), {}, ("peaked",), "half", _BF),
    ("channel_attention_bwd_cross", "channel_attention_bwd", (128, 2, (2, 8, 16), True), {}, ("peaked",), "half", _BF),
    ("pg_gate_fwd_one_window", "pg_gate_fwd", (128, 8), dict(nW=1), ("peaked",), "none", None),
    ("pg_gate_fwd_17_windows", "pg_gate_fwd", (128, 8), dict(nW=17), ("peaked",), "none", None),
    ("pg_gate_bwd_one_window", "pg_gate_bwd", (128, 8), dict(nW=1), ("peaked",), "none", None),
    ("pg_gate_bwd_17_windows", "pg_gate_bwd", (128, 8), dict(nW=17), ("peaked",), "none", None),
]
# window attention takes the manifest fixture: the single-window edge case with both shifts, and (1, 8, 16, 32)
WIN_PROFILE_CASES = WIN_EDGE_CASES + [("tiny", "encoder_level1.blocks.1.", 1, 4, (1, 8, 16, 32))]
WIN_PROFILES = ("flat", "peaked")
# `saturated` runs in bf16 only: logits of +-95 are ill-conditioned, torch's own evaluation is 0.9-1.2e-6 (fp32) and 4.8-5.6e-3 (fp16) from fp64,
# which leaves the fp32 case over its slice bound and the fp16 case over the YARD_CAP of its tolerance (2e-6 / 4e-3): not tests.  bf16 (tolerance
# 3e-2, yardstick 2.4-3.2e-2) has the room, and Math<bf16_t>::exp is the exp the training step runs.
WIN_SATURATED_DTYPES = [torch.bfloat16]


def profile_params(emulator):
    """(id, check name, args, kwargs, dtype or None, profile) for pytest.mark.parametrize: every dtype the check runs on the GPU, one on the emulator"""
    out = []
    for name, fn, a, kw, profiles, dts, emu_dt in PROFILE_CASES:
        for dt in ([emu_dt] if emulator else {None: DTYPES, "half": [torch.bfloat16, torch.float16], "none": [None]}[dts]):
            for prof in profiles:
                out.append(("%s-%s%s" % (name, prof, "" if dt is None else "-" + str(dt).replace("torch.", "")), fn, a, kw, dt, prof))
    return out


def run_profile(dev, fn, a, kw, dt, prof):
    check = globals()["check_" + fn]
    return check(dev, *a, inputs=prof, **kw) if dt is None else check(dev, dt, *a, inputs=prof, **kw)
