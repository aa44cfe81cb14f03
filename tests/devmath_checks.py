"""The bodies of the device math probe tests, shared by tests/test_devmath_emu.py and tests/test_devmath_gpu.py: each takes the loaded
probe library, the device its buffers live on and the size of the equally spaced grid.  Grids, references and bars: tests/devmath_ref.py."""
import torch

import devmath_ref as R


def _name(policy):
    return str(policy).replace("torch.", "")


def check_gelu16(lib, dev, n, policy):
    """the documented bounds of the polynomial GELU / GELU' of the 16-bit policies, gelu(+-inf), and gelu_pair.g bitwise gelu"""
    x = R.gelu_grid(n)
    g, _, _ = R.run(lib, "gelu", policy, x, dev)
    gp, dgp, _ = R.run(lib, "gelu_pair", policy, x, dev)
    m1, w1 = R.gelu16_violations(x, g)
    m2, w2 = R.gelu16_violations(x, gp, dgp)
    print("devmath %s gelu: %s" % (_name(policy), "; ".join("%s: %s" % kv for kv in w1.items())))
    print("devmath %s gelu_pair: %s" % (_name(policy), "; ".join("%s: %s" % kv for kv in w2.items())))
    if m1 or m2:
        # which is wrong, the comment or the code?  the same coefficients in fp64:
        g64, dg64 = R.poly_gelu64(x)
        m3, _ = R.gelu16_violations(x, g64, dg64, fp32_eval=False)
        raise AssertionError("; ".join(m1 + m2) + " -- the fp64 evaluation of the header's coefficients " +
                             ("misses the bounds too (%s): the comment or the coefficients are wrong" % "; ".join(m3) if m3 else
                              "holds every bound: the device's evaluation differs from the polynomial"))
    diff = g.view(torch.int32) != gp.view(torch.int32)
    assert not bool(diff.any()), "gelu_pair(x).g differs from gelu(x) in %d of %d points, first at x = %r: %r vs %r" % (
        int(diff.sum()), x.numel(), float(x[diff][0]), float(gp[diff][0]), float(g[diff][0]))


def check_gelu32(lib, dev, n):
    """Math<float>::gelu, gelu_pair and gelu_erf in units of 2^-24 max(|x|, 1) against 3 x torch's own CPU fp32 error (at most 16)"""
    x = R.gelu_grid(n)
    bar, yard = R.gelu32_bar(x)
    dbar, dyard = R.dgelu32_bar(x)
    exact, dexact = R.gelu64(x), R.dgelu64(x)
    got = {"gelu": R.run(lib, "gelu", torch.float32, x, dev)[0], "gelu_erf": R.run(lib, "gelu_erf", torch.float32, x, dev)[0]}
    got["gelu_pair.g"], dg, _ = R.run(lib, "gelu_pair", torch.float32, x, dev)
    bad = []
    for name, v in got.items():
        u, at = R.units32(x, v, exact)
        print("devmath float32 %s: %.3f units at x = %r (yardstick %.3f, bar %.3f)" % (name, u, at, yard, bar))
        if not u <= bar:
            bad.append("%s: %.3f units of 2^-24 max(|x|, 1) at x = %r, bar %.3f (torch CPU fp32: %.3f)" % (name, u, at, bar, yard))
    u, at = R.units32(x, dg, dexact)
    print("devmath float32 gelu_pair.dg: %.3f units at x = %r (yardstick %.3f, bar %.3f)" % (u, at, dyard, dbar))
    if not u <= dbar:
        bad.append("gelu_pair.dg: %.3f units at x = %r, bar %.3f (torch CPU fp32: %.3f)" % (u, at, dbar, dyard))
    # the infinities of the grid.  +inf -> +inf.  -inf: 0.5 x (1 + erf) is -inf * 0 = NaN in fp32 arithmetic, and torch's own CPU fp32 F.gelu -- the
    # yardstick of this policy -- returns NaN there too: the result must be 0, -0, or NaN where the yardstick is NaN as well
    pinf, ninf = x == float("inf"), x == float("-inf")
    yard_ninf = torch.nn.functional.gelu(x[ninf].float())
    for name, v in got.items():
        print("devmath float32 %s: +inf -> %r, -inf -> %r (torch CPU fp32 F.gelu: %r, %r)" % (
            name, v[pinf].tolist(), v[ninf].tolist(), torch.nn.functional.gelu(x[pinf].float()).tolist(), yard_ninf.tolist()))
        if not bool((v[pinf] == float("inf")).all()):
            bad.append("%s(+inf) is %r, not +inf" % (name, v[pinf].tolist()))
        if not bool(((v[ninf] == 0) | (torch.isnan(v[ninf]) & torch.isnan(yard_ninf))).all()):
            bad.append("%s(-inf) is %r: neither 0 nor a NaN the yardstick shares (%r)" % (name, v[ninf].tolist(), yard_ninf.tolist()))
    assert not bad, "; ".join(bad)


def check_exp16(lib, dev, n):
    x = R.exp_grid(n)
    for policy in R.F16_POLICIES:
        got, _, _ = R.run(lib, "exp", policy, x, dev)
        msgs, worst = R.exp_violations(x, got)
        print("devmath %s exp: %s" % (_name(policy), ", ".join("%s %.4g" % kv for kv in worst.items())))
        assert not msgs, "; ".join(msgs)


def check_exp32(lib, dev, n):
    """Math<float>::exp (expf) on the same range under the same bar: the library routine is within it by a wide margin"""
    x = R.exp_grid(n)
    got, _, _ = R.run(lib, "exp", torch.float32, x, dev)
    msgs, worst = R.exp_violations(x, got)
    print("devmath float32 exp: %s" % ", ".join("%s %.4g" % kv for kv in worst.items()))
    assert not msgs, "; ".join(msgs)


def check_rstd(lib, dev):
    """rsqrtf(d2 / C + 1e-5f): the value of epsilon and its place inside the root, from variance 0 to 1e8"""
    for C in R.RSTD_WIDTHS:
        d2, ref = R.rstd_case(C)
        got, _, _ = R.run(lib, "ln_rstd", torch.float32, d2, dev, C=C)
        rel = (got.double() - ref).abs() / ref
        rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
        i = int(rel.argmax())
        print("devmath ln_rstd C = %d: worst relative error %.3g = %.2f x 2^-24 at v / C = %.3g (bar 4 x 2^-24)" % (C, float(rel[i]), float(rel[i]) * 2 ** 24, float(d2[i]) / C))
        assert float(rel[i]) <= R.RSTD_BAR, "rsqrtf(d2 / %d + 1e-5f): relative error %.3g at v / C = %.3g: got %r, fp64 %r (bar %.3g)" % (
            C, float(rel[i]), float(d2[i]) / C, float(got[i]), float(ref[i]), R.RSTD_BAR)


def check_rcp(lib, dev):
    x = R.rcp_grid()
    got, _, _ = R.run(lib, "rcp", torch.float32, x, dev)
    rel = ((got.double() - 1.0 / x.double()) * x.double()).abs()
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
    i = int(rel.argmax())
    print("devmath rcp: worst relative error %.3g = %.2f x 2^-24 at x = %r" % (float(rel[i]), float(rel[i]) * 2 ** 24, float(x[i])))
    assert float(rel[i]) <= R.RCP_BAR, "1.0f / x: relative error %.3g at x = %r (bar %.3g)" % (float(rel[i]), float(x[i]), R.RCP_BAR)


def check_conversions(lib, dev, dtype):
    """from_f32<T>, store4<T> and Vec16<T>::set bitwise against torch's CPU conversion"""
    x = R.cvt_table(dtype)
    want_bits, want_val = R.cvt_expected(x, dtype)
    for what in ("cvt", "cvt_store4", "cvt_vec16"):
        val, _, bits = R.run(lib, what, dtype, x, dev)
        bad = bits != want_bits
        assert not bool(bad.any()), "%s %s: %d of %d patterns differ from torch, first: fp32 0x%08x (%r) -> 0x%04x, torch 0x%04x" % (
            what, _name(dtype), int(bad.sum()), x.numel(), int(x.view(torch.int32)[bad][0]) & 0xFFFFFFFF, float(x[bad][0]), int(bits[bad][0]), int(want_bits[bad][0]))
        assert torch.equal(val.view(torch.int32), want_val.view(torch.int32)), "%s %s: to_f32 of the stored value differs" % (what, _name(dtype))
    print("devmath conversions %s: %d patterns bitwise equal to torch for from_f32, store4 and Vec16::set" % (_name(dtype), x.numel()))
    xf = R.cvt_table(torch.bfloat16)
    val, _, bits = R.run(lib, "cvt", torch.float32, xf, dev)
    assert torch.equal(bits, xf.view(torch.int32)) and torch.equal(val.view(torch.int32), xf.view(torch.int32)), "from_f32<float> is not the identity"


def report_nan(lib, dev):
    """what one NaN becomes in gelu / gelu_pair: printed, nothing asserted (fmaxf and fmed3 drop NaNs, so the 16-bit forward may return a
    finite number; changing that is not part of these tests)"""
    x = torch.tensor([float("nan")])
    lines = []
    for policy in (torch.float32, torch.bfloat16, torch.float16):
        g, _, _ = R.run(lib, "gelu", policy, x, dev)
        gp, dgp, _ = R.run(lib, "gelu_pair", policy, x, dev)
        lines.append("devmath NaN %s: gelu -> %r, gelu_pair -> (%r, %r)" % (_name(policy), float(g[0]), float(gp[0]), float(dgp[0])))
    print("\n".join(lines))
    return lines
