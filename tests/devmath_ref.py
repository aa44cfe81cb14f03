"""Grids, fp64 references and bars for the device math probes (tests/devprobe/probe.hip): shared by tests/test_devmath_emu.py (the
emulated build) and tests/test_devmath_gpu.py (the gfx950 build on an MI355X).

Every bar here is either the one csrc/mphsir_dev.h documents for its own polynomial, or follows from the number formats (derivation
beside it), or is a multiple of torch's own CPU evaluation in the same precision (the yardstick, computed in the test).  None is taken
from what the code under test returns; the measured values are recorded beside the bars for the reader.
"""
import ctypes
import math

import torch

WHAT = {"gelu": 0, "gelu_pair": 1, "exp": 2, "ln_rstd": 3, "cvt": 4, "rcp": 5, "cvt_store4": 6, "cvt_vec16": 7, "gelu_erf": 8}
POLICY = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
F16_POLICIES = [torch.bfloat16, torch.float16]


def load(path):
    lib = ctypes.CDLL(path)
    lib.mphsir_probe.restype = ctypes.c_int
    lib.mphsir_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                 ctypes.c_int32, ctypes.c_void_p]
    return lib


def run(lib, what, policy, x, dev="cpu", C=1):
    """x: fp32 values (any device) -> (out0 fp32, out1 fp32, out1's 4 bytes as int32), all on the CPU"""
    x = x.detach().to(torch.float32).to(dev).contiguous()
    n = x.numel()
    out0 = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    out1 = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream if torch.device(dev).type == "cuda" else 0
    rc = lib.mphsir_probe(WHAT[what], POLICY[policy], x.data_ptr(), out0.data_ptr(), out1.data_ptr(), n, C, stream)
    assert rc == 0, "mphsir_probe(%s, %s) returned %d" % (what, policy, rc)
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    out0, out1 = out0.cpu(), out1.cpu()
    return out0, out1, out1.view(torch.int32)


# ---- grids -----------------------------------------------------------------------------------------------------------------------
N_EMU, N_GPU = 2 ** 16 + 1, 2 ** 20 + 1
SMALLEST_NORMAL, A_SUBNORMAL = 2.0 ** -126, 1e-40


def _ulp_neighbours(v, kmax=8):
    out, up, dn = [v], torch.tensor(v, dtype=torch.float32), torch.tensor(v, dtype=torch.float32)
    for _ in range(kmax):
        up = torch.nextafter(up, torch.tensor(float("inf")))
        dn = torch.nextafter(dn, torch.tensor(float("-inf")))
        out += [float(up), float(dn)]
    return out


def specials():
    """+-4 +- k ulp (k <= 8), +-0, +-1e-30, the smallest normal and a subnormal, +-88, +-1e4, +-3e38, +-inf"""
    s = _ulp_neighbours(4.0) + _ulp_neighbours(-4.0)
    for v in (0.0, 1e-30, SMALLEST_NORMAL, A_SUBNORMAL, 88.0, 1e4, 3e38, float("inf")):
        s += [v, -v]
    return torch.tensor(s, dtype=torch.float64).to(torch.float32)


def gelu_grid(n):
    return torch.cat([torch.linspace(-12.0, 12.0, n, dtype=torch.float64).to(torch.float32), specials()])


def exp_grid(n):
    """[-104, 0]: all a max-subtracted softmax produces"""
    extra = torch.tensor([0.0, -0.0, -1e-30, -A_SUBNORMAL, -87.0, -87.3365, -88.0, -103.9], dtype=torch.float32)
    return torch.cat([torch.linspace(-104.0, 0.0, n, dtype=torch.float64).to(torch.float32), extra])


def var_grid():
    """v / C of the LayerNorm form: 0, and 1e-12 ... 1e8 (64 points per decade, fp32)"""
    return torch.cat([torch.zeros(1), torch.logspace(-12, 8, 20 * 64 + 1, dtype=torch.float64).to(torch.float32)])


# ---- GELU ------------------------------------------------------------------------------------------------------------------------
def phi64(x):
    return 0.5 * torch.special.erfc(-x.double() / math.sqrt(2.0))


def gelu64(x):
    """x Phi(x) in fp64; 0 at -inf (the limit), +inf at +inf"""
    x = x.double()
    return torch.where(torch.isinf(x), torch.where(x > 0, x, torch.zeros_like(x)), x * phi64(x))


def dgelu64(x):
    """Phi(x) + x phi(x) in fp64; the limits 0 / 1 at -inf / +inf"""
    x = x.double()
    xf = torch.where(torch.isinf(x), torch.zeros_like(x), x)
    d = phi64(xf) + xf * torch.exp(-0.5 * xf * xf) / math.sqrt(2.0 * math.pi)
    return torch.where(torch.isinf(x), (x > 0).double(), d)


# The documented bounds of Math<bf16_t>::gelu / gelu_pair (the header comment in csrc/mphsir_dev.h).  They are bounds of the POLYNOMIALS
# with the header's fp32 coefficients (poly_gelu64 below; test_reference_polynomial_holds_its_bounds pins that side in fp64); the fp32
# Horner evaluation of the device adds its own rounding, bounded point by point by eval_allowance() below.  Two findings of the probes:
#  * the header gave the bounds as those of the fp32 evaluation; they were two-digit roundings of its maxima (Phi: 5.507e-5 in fp32 at
#    x >= 4 against "5.5e-5", the tail -4 Phi(-4) = -2.203e-4 against "2.2e-4"), so the fp32 evaluation missed them by 0.1-0.2 %;
#  * GELU' inside the clamp was stated as 5.5e-5; the polynomial has an equal ripple of 5.52e-5 up to |x| = 2.7 that grows to 6.17e-5 at 3.77
#    and 6.95e-5 at |x| = 4: no evaluation of these coefficients holds 5.5e-5.
# In both the comment was wrong, not the code (the fp64 evaluation of the same coefficients decides it); the header now states these
# figures as bounds of the polynomial, 7.0e-5 for GELU', and the rounding of the fp32 evaluation beside them.
PHI_BOUND = 5.5e-5              # |Phi - exact| everywhere; |GELU - exact| <= PHI_BOUND |x| for x > -4
GELU_TAIL_BOUND = 2.2e-4        # |GELU - exact| for x <= -4 (the device value there is the constant -4 Phi_poly(-4))
DGELU_BOUND = 7.0e-5            # |GELU' - exact| inside the clamp
DGELU_TAIL_BOUND = 5.8e-4       # |GELU' - exact| below -4; GELU'(x) - 1/2 is odd (GELU'(-x) = 1 - GELU'(x)) and so is the polynomial, hence the
                                # same bound holds above +4
# the coefficients of the header restated, highest degree first (P: Phi = 1/2 + xc P(xc^2); Q: GELU' = 1/2 + xc Q(xc^2)), for the fp64
# evaluation that tells a wrong comment from wrong code when the device misses a bound
P_COEF = [-1.580785614e-09, 1.217110679e-07, -4.100865681e-06, 8.066738519e-05, -1.048204373e-03, 9.664873593e-03, -6.617537886e-02, 3.988475204e-01]
Q_COEF = [9.796149447e-10, -8.218865588e-08, 3.028365654e-06, -6.495783600e-05, 9.073287947e-04, -8.716330864e-03, 5.845612660e-02,
          -2.648265660e-01, 7.976095676e-01]
EPS32 = 2.0 ** -24


def _c32(coef):
    return [float(torch.tensor(c, dtype=torch.float32)) for c in coef]


def _horner64(coef, u):
    c = _c32(coef)
    acc = torch.full_like(u, c[0])
    for v in c[1:]:
        acc = acc * u + v
    return acc


def _horner_allowance(coef, u):
    """first-order bound of what an fp32 Horner evaluation (one fma = one rounding per step, at u = fl(xc^2)) can differ from the exact value
    of the polynomial: every step's rounding, 2^-24 |y_i|, carried to the end by the remaining powers of u (the running error bound), plus
    the rounding of u itself through the polynomial's own derivative"""
    c = _c32(coef)
    y, dy, run = torch.full_like(u, c[0]), torch.zeros_like(u), torch.zeros_like(u)
    for v in c[1:]:
        dy = dy * u + y
        y = y * u + v
        run = run * u + y.abs()
    return EPS32 * (run + dy.abs() * u)


def eval_allowance(x):
    """(Phi, GELU, GELU'): the rounding an fp32 evaluation of the header's forms may add to the polynomial's own error, per point: the Horner
    allowance times |xc|, one more rounding for the closing fma (|Phi| <= 1, |GELU'| <= 1.001) and one for the product with max(x, -4).
    At |x| >= 4: 2.4e-6, that times |max(x, -4)|, and 3.0e-5 (seen in the emulated fp32 evaluation: 6e-7 and 1.1e-5).
    Measured, 2^20 + 1 points, one MI355X, 2026-10-20, identical for bf16 and fp16: Phi 5.513e-5 (x >= 4), GELU tail 2.203e-4, GELU' 7.1e-5
    inside the clamp (at x = 3.778; the emulator's fmaf chain gives 8.0e-5 at 3.999999) and 5.751e-4 beyond; gelu_pair.g bitwise gelu."""
    x = x.double()
    xf = torch.where(torch.isinf(x), torch.zeros_like(x), x)
    xc = xf.clamp(-4.0, 4.0)
    u = xc * xc
    a_phi = xc.abs() * _horner_allowance(P_COEF, u) + EPS32
    a_g = xf.clamp_min(-4.0).abs() * (a_phi + EPS32)
    a_dg = xc.abs() * _horner_allowance(Q_COEF, u) + 1.001 * EPS32
    return a_phi, a_g, a_dg


def poly_gelu64(x):
    """the header's polynomial GELU and GELU' with its fp32 coefficients, evaluated in fp64"""
    x = x.double()
    xc = x.clamp(-4.0, 4.0)
    u = xc * xc
    return x.clamp_min(-4.0) * (xc * _horner64(P_COEF, u) + 0.5), xc * _horner64(Q_COEF, u) + 0.5


def gelu16_violations(x, g, dg=None, fp32_eval=True):
    """the documented bounds on a 16-bit-policy result (fp32_eval: plus the rounding allowance of an fp32 evaluation; False for the fp64
    evaluation of the polynomial itself); returns a list of messages (empty: all hold) and the worst error / bar of each bound"""
    x64, g64 = x.double(), g.double()
    fin = torch.isfinite(x64)
    msgs, worst = [], {}
    a_phi, a_g, a_dg = eval_allowance(x) if fp32_eval else (torch.zeros_like(x64),) * 3

    def bound(name, err, bar, mask, val):
        e = torch.where(mask, err / bar, torch.zeros_like(err))
        e = torch.where(torch.isnan(e) & mask, torch.full_like(e, float("inf")), e)
        i = int(e.argmax())
        worst[name] = "%.4g (%.4g x the bar) at x = %.7g" % (float(err[i]), float(e[i]), float(x[i]))
        if float(e[i]) > 1.0:
            msgs.append("%s: error %.4g = %.4g x the bar %.4g at x = %r (got %r)" % (name, float(err[i]), float(e[i]), float(bar[i]), float(x[i]), float(val[i])))

    up = fin & (x64 > -4.0)
    err = (g64 - gelu64(x)).abs()
    bound("GELU, x > -4", err, PHI_BOUND * x64.abs() + a_g, up & (x64 != 0), g)
    bound("GELU, x <= -4", err, GELU_TAIL_BOUND + a_g, fin & (x64 <= -4.0), g)
    big = fin & (x64.abs() >= 2.0 ** -10)
    phi_dev = g64 / x64.clamp_min(-4.0)          # the rounding of g = max(x, -4) Phi is part of a_g: 2 * 2^-24 here
    bound("Phi", (phi_dev - phi64(x)).abs(), PHI_BOUND + a_phi + 2 * EPS32, big, g)
    z = fin & (x64 == 0)
    if bool(z.any()) and float(g64[z].abs().max()) != 0.0:
        msgs.append("GELU(+-0) is not 0")
    if dg is not None:
        derr = (dg.double() - dgelu64(x)).abs()
        bound("GELU', |x| <= 4", derr, DGELU_BOUND + a_dg, fin & (x64.abs() <= 4.0), dg)
        bound("GELU', |x| > 4", derr, DGELU_TAIL_BOUND + a_dg, x64.abs() > 4.0, dg)          # the infinities included: the limits 0 and 1
    pinf, ninf = x64 == float("inf"), x64 == float("-inf")
    tail = GELU_TAIL_BOUND + (4.0 * 2.5e-6 if fp32_eval else 0.0)          # the allowance at xc = -4 (2.4e-6) times |max(x, -4)|
    if bool(pinf.any()) and not bool((g64[pinf] == float("inf")).all()):
        msgs.append("GELU(+inf) is %r, not +inf" % g[pinf].tolist())
    if bool(ninf.any()) and not bool((torch.isfinite(g64[ninf]) & (g64[ninf].abs() <= tail)).all()):
        msgs.append("GELU(-inf) is %r: not finite within %g" % (g[ninf].tolist(), tail))
    return msgs, worst


# fp32 policy (erff / expf): error in units of 2^-24 max(|x|, 1); bar = 3 x torch's own CPU fp32 F.gelu on the same grid, at most 16 units.
# Measured, 2^20 + 1 points, one MI355X, 2026-10-20: gelu / gelu_erf / gelu_pair.g 1.88 units (at x = 1.21), torch's CPU F.gelu 6.38 (its
# tail near -4) -> bar 16 (the cap); gelu_pair.dg 2.19 units against torch's 2.25 -> bar 6.76.  Emulator (libm erff), 2^16 + 1 points: 1.66 / 2.13.
GELU32_FACTOR, GELU32_CAP = 3.0, 16.0


def units32(x, got, exact):
    x64 = x.double()
    fin = torch.isfinite(x64) & torch.isfinite(exact)          # +-3e38 included; the infinities: devmath_checks.check_gelu32
    u = (got.double() - exact).abs() / (2.0 ** -24 * x64.abs().clamp_min(1.0))
    u = torch.where(fin, u, torch.zeros_like(u))
    u = torch.where(torch.isnan(u), torch.full_like(u, float("inf")), u)
    i = int(u.argmax())
    return float(u[i]), float(x[i])


def gelu32_bar(x):
    """(bar, yardstick): the yardstick is torch's CPU fp32 F.gelu against fp64 on the same grid"""
    y, _ = units32(x, torch.nn.functional.gelu(x.float()), gelu64(x))
    return min(GELU32_FACTOR * y, GELU32_CAP), y


def dgelu32_bar(x):
    """the same for GELU' = Phi + x phi: torch's CPU fp32 evaluation of that expression"""
    xf = x.float()
    t = 0.5 * (1.0 + torch.erf(xf * 0.7071067811865476)) + xf * 0.3989422804014327 * torch.exp(-0.5 * xf * xf)
    y, _ = units32(x, t, dgelu64(x))
    return min(GELU32_FACTOR * y, GELU32_CAP), y


# ---- exp of the 16-bit policy (__expf: v_exp_f32 of x log2 e) --------------------------------------------------------------------------
# relative error <= 2^-22 + |x| 2^-23 where the exact result is above 2^-126: one rounding of x log2 e followed by an exp2 within one ulp
# (2^-23, doubled for the rounding of the result's neighbours) -- the first term -- and the rounding of the argument, 2^-24 |x log2 e|, carried
# through the exponential: ln 2 * 2^-24 |x| log2 e = 2^-24 |x|, allowed twice -- the second.  Below 2^-126 the hardware may flush: absolute
# error <= 2^-126.  EXP_CAP: if a device misses the derived bar the finding is the measurement, the bar becomes 1.5 x measured, and beyond
# 2^-18 relative it is a defect.
# Measured, 2^20 + 1 points on [-104, 0], one MI355X, 2026-10-20: __expf worst relative error 3.83e-6 at x = -44.4 = 0.59 x the derived bar
# there (the derived bar holds; no fallback to 1.5 x measured needed); results below 2^-126 are flushed to 0 (worst absolute error 2^-126
# exactly, at the boundary).  expf of the fp32 policy: 8.1e-8.  Emulator (libm expf for both): 5.9e-8.
EXP_FLOOR = 2.0 ** -126
EXP_CAP = 2.0 ** -18


def exp_bar(x):
    return 2.0 ** -22 + x.double().abs() * 2.0 ** -23


def exp_violations(x, got):
    x64 = x.double()
    exact = torch.exp(x64)
    err = (got.double() - exact).abs()
    normal = exact > EXP_FLOOR
    rel = torch.where(normal, err / exact / exp_bar(x), torch.zeros_like(err))
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
    i = int(rel.argmax())
    relraw = torch.where(normal, err / exact, torch.zeros_like(err))
    msgs = []
    if float(rel[i]) > 1.0:
        msgs.append("exp: %.4g x the bar (relative error %.4g) at x = %r" % (float(rel[i]), float(err[i] / exact[i]), float(x[i])))
    sub = torch.where(~normal, err, torch.zeros_like(err))
    sub = torch.where(torch.isnan(sub), torch.full_like(sub, float("inf")), sub)
    j = int(sub.argmax())
    if float(sub[j]) > EXP_FLOOR:
        msgs.append("exp: absolute error %.4g below 2^-126 at x = %r" % (float(sub[j]), float(x[j])))
    return msgs, {"worst rel / bar": float(rel[i]), "at": float(x[i]), "worst rel": float(relraw.max()), "worst abs below 2^-126": float(sub[j])}


# ---- the LayerNorm rstd form: rsqrtf(d2 / C + 1e-5f) ---------------------------------------------------------------------------------
# relative error <= 4 * 2^-24 against fp64 1 / sqrt(d2 / C + 1e-5): the quotient and the sum round once each (2^-24 each, halved by the
# root: 2^-24 together), the hardware rsq is within one ulp (2^-23 = 2 * 2^-24): 3 * 2^-24, one more for the fp32 form of 1e-5.
# Measured, one MI355X, 2026-10-20: 1.42 x 2^-24 (C = 64) and 1.55 x 2^-24 (C = 20); emulator (1 / sqrtf): 1.65 x 2^-24.
LN_EPS = 1e-5
RSTD_BAR = 4.0 * 2.0 ** -24
RSTD_WIDTHS = (64, 20)


def rstd_case(C):
    """(d2 fp32 as the kernel holds it, fp64 reference of the form on exactly that d2)"""
    d2 = (var_grid().double() * C).to(torch.float32)
    return d2, 1.0 / torch.sqrt(d2.double() / C + LN_EPS)


# ---- 1.0f / x ------------------------------------------------------------------------------------------------------------------------
# IEEE division is within 2^-24; a compiler may legitimately lower it to the hardware reciprocal with one Newton step or to v_rcp_f32
# alone, documented at one ulp: 2^-23.  On |x| in [1e-30, 1e30] neither the operand nor the result is subnormal.
# Measured, one MI355X, 2026-10-20: 0.99 x 2^-24 (the compiler emits the correctly rounded division), the same on the emulator.
RCP_BAR = 2.0 ** -23


def rcp_grid():
    m = torch.logspace(-30, 30, 60 * 128 + 1, dtype=torch.float64).to(torch.float32)
    return torch.cat([m, -m, torch.tensor([1.0, 3.0, 7.0, 10.0, 0.1])])


# ---- conversions ---------------------------------------------------------------------------------------------------------------------
def _from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def cvt_table(dtype):
    """fp32 inputs for from_f32<T>: every tie pattern of a few exponents with its two fp32 neighbours (the all-ones mantissa rounds up into
    the next binade), the largest finite value / the last fp32 below the overflow tie / the tie itself (the first value that becomes inf) /
    far beyond, fp16 subnormals with their ties and values at and below half the smallest one, +-0, +-inf -- each with both signs"""
    drop = 16 if dtype == torch.bfloat16 else 13          # fp32 mantissa bits that the format drops
    kept = 23 - drop
    bits = []
    exps = (127, 126, 130, 120, 1) if dtype == torch.bfloat16 else (127, 126, 130, 120, 113, 142)      # fp16: 113 = 2^-14 (smallest normal), 142 = 2^15 (top binade)
    for e in exps:
        for m in range(1 << kept):
            tie = (e << 23) | (m << drop) | (1 << (drop - 1))
            bits += [tie - 1, tie, tie + 1, (e << 23) | (m << drop)]
    if dtype == torch.bfloat16:
        bits += [0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF]          # max, just below the tie, the tie (-> inf), above
        bits += [0x00000001, 0x00008000, 0x00010000, 0x00018000, 0x007F8000, 0x007FFFFF, 0x00800000]      # fp32 subnormals = bf16 subnormals
    else:
        bits += [0x477FE000, 0x477FEFFF, 0x477FF000, 0x477FF001, 0x47800000, 0x7F7FFFFF]          # 65504, < 65520, 65520 (-> inf), 65536, fp32 max
        vals = []
        for k in list(range(0, 40)) + list(range(1000, 1026)):          # k 2^-24: the subnormals (k < 1024) and the first normals
            vals += [k * 2.0 ** -24, (k + 0.5) * 2.0 ** -24]
        sub = torch.tensor(vals, dtype=torch.float64).to(torch.float32)
        nb = torch.cat([sub, torch.nextafter(sub, torch.tensor(float("inf"))), torch.nextafter(sub, torch.tensor(0.0))])
        small = torch.tensor([2.0 ** -25, 2.0 ** -26, 1e-30, A_SUBNORMAL], dtype=torch.float64).to(torch.float32)
        small = torch.cat([small, torch.nextafter(small[:1], torch.tensor(float("inf"))), torch.nextafter(small[:1], torch.tensor(0.0))])
        bits += [int(b) & 0xFFFFFFFF for b in torch.cat([nb, small]).view(torch.int32).tolist()]
    x = _from_bits(bits)
    x = torch.cat([x, torch.tensor([0.0, float("inf")])])
    return torch.cat([x, -x])


def cvt_expected(x, dtype):
    """(bit pattern as int32 in 0 ... 65535, the value widened to fp32) of torch's CPU conversion"""
    t = x.to(dtype)
    return t.view(torch.int16).to(torch.int32) & 0xFFFF, t.float()
