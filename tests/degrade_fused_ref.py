"""TEST INFRASTRUCTURE for the fused degradation launch (mphsir_degrade_batch, mp-hsir_amd/csrc/degrade.hip): a numpy restatement of
Philox4x32-10 and of the three draw formulas of include/mphsir.h in float64, a per-kind reference composed from oracle/degrade_oracle.py
and its `augment`, and the checks that tests/test_degrade_fused_emu.py (CPU emulator) and tests/test_degrade_fused_gpu.py (MI355X) share:
each takes the device the bound library runs on."""
import os

import numpy as np
import torch

from oracle import degrade_oracle as DO

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "degrade.npz"))
KIND = {"none": 0, "gaussianN": 1, "complexN": 2, "blur": 3, "sr": 4, "inpaint": 5, "bandmiss": 6, "haze": 7}
M32 = np.uint64(0xFFFFFFFF)

# Tolerances.  Exact kinds (products with 0 / 1, selections, copies) are compared bitwise.  3e-7, 5e-6 and 3e-6 are the bars
# tests/test_degrade.py holds the tensor path to (noise sums; stencils and bicubic; haze).  Z_TOL bounds |z - float64 helper| of the
# generated normal draw: measured 1.39e-6 on the emulator (glibc logf / cosf) and 1.39e-6 on the MI355X (ocml) over 31 x 64 x 64 draws
# (seed 77, ordinal 3), times 4.  The two agree because the error is not libm's: 2 pi b is rounded to fp32 in front of the cosine, up to
# 3.7e-7 in the argument times a radius of up to 5.8.  Anything above 1e-5 is a wrong sampler whatever the margin says.
TOL_SUM, TOL_TAPS, TOL_HAZE, Z_TOL = 3e-7, 5e-6, 3e-6, 4 * 1.39e-6
assert Z_TOL <= 1e-5


# ---- Philox4x32-10 and the draws -----------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words and key words as uint64 arrays (or scalars) holding 32-bit values -> four uint64 arrays of 32-bit values"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def draws(seed, ordinal, shape):
    """-> (z float64, u0 float32, u1 float32) of every element of the un-augmented (B,C,N,N) cube, as include/mphsir.h defines them"""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r0, r1, r2, r3 = philox4x32_10(idx & M32, idx >> np.uint64(32), 0, int(ordinal) & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)
    a = ((r0 >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    b = (r1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    z = np.sqrt(-2.0 * np.log(a)) * np.cos(2.0 * np.pi * b)
    u0 = ((r2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    u1 = ((r3 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return z.reshape(shape), u0.reshape(shape), u1.reshape(shape)


# ---- plans -----------------------------------------------------------------------------------------------------------------------------
def stencil_table(kernels):
    st = torch.zeros((len(kernels), 21, 21), dtype=torch.float32)
    for i, k in enumerate(kernels):
        k = torch.as_tensor(np.asarray(k), dtype=torch.float32)
        st[i, :k.shape[0], :k.shape[1]] = k
    return st, [int(np.asarray(k).shape[0]) for k in kernels]


def make_plan(dev, B, C, N, menu, task=None, aug=None, param=None, sub=None, kernels=(), sr_factor=(), **tabs):
    """a DegradePlan with every table present (zeros unless given); menu: kind names; tables as numpy / lists / tensors"""
    from mp_hsir_amd import ops

    def t(v, dt, shape):
        if v is None:
            return torch.zeros(shape, dtype=dt, device=dev)
        v = torch.as_tensor(np.asarray(v.cpu() if torch.is_tensor(v) else v)).to(dt).reshape(shape)
        return v.contiguous().to(dev)
    st, ks = stencil_table(kernels) if len(kernels) else (None, [])
    return ops.DegradePlan([KIND[m] if isinstance(m, str) else m for m in menu], ks, sr_factor,
                           task=t(task, torch.int32, (B,)), aug=t(aug, torch.int32, (B,)), param=t(param, torch.float32, (B,)),
                           sub=t(sub, torch.int32, (B,)), band_sigma=t(tabs.get("band_sigma"), torch.float32, (B, C)),
                           band_flag=t(tabs.get("band_flag"), torch.uint8, (B, C)), col_dead=t(tabs.get("col_dead"), torch.uint8, (B, C, N)),
                           col_off=t(tabs.get("col_off"), torch.float32, (B, C, N)), stencils=None if st is None else st.to(dev),
                           cirrus=t(tabs.get("cirrus"), torch.float32, (B, N, N)), atm=t(tabs.get("atm"), torch.float32, (B, C)),
                           haze_ratio=t(tabs.get("haze_ratio"), torch.float32, (C,)))


def run(dev, clean, plan, draws3=None, seed=0, ordinal=0):
    """-> (degraded, clean_aug) as numpy"""
    from mp_hsir_amd import ops
    x = torch.as_tensor(clean).to(dev).contiguous()
    dr = None if draws3 is None else tuple(None if d is None else torch.as_tensor(np.asarray(d, dtype=np.float32)).to(dev).contiguous() for d in draws3)
    deg, cl = ops.degrade_batch(x, plan, seed=seed, ordinal=ordinal, draws=dr)
    return deg.cpu().numpy(), cl.cpu().numpy()


def one_kind(dev, clean, kind, aug=0, draws3=None, seed=0, ordinal=0, **kw):
    """the whole batch as ONE kind under one mode (aug: an int or a list per sample)"""
    B, C, N, _ = clean.shape
    aug = [aug] * B if np.isscalar(aug) else aug
    plan = make_plan(dev, B, C, N, [kind], aug=aug, **kw)
    return run(dev, clean, plan, draws3, seed, ordinal)


def aug_batch(y, modes):
    return np.stack([DO.augment(y[b], int(m)) for b, m in enumerate(modes)])


def fixture_clean():
    return np.random.RandomState(1).rand(9, 32, 32).astype(np.float32)


# ---- the fixture cases: name -> (kwargs of one_kind, draws, expected aug-0 output, tolerance or None for bitwise) -----------------------
def fixture_cases():
    G, x = GOLD, fixture_clean()
    C, N = 9, 32
    shape = (1, C, N, N)
    z0 = np.zeros(shape, np.float32)
    cases = {}
    cases["gauss"] = (dict(kind="gaussianN", param=[float(G["gauss/sigma"])]), (G["gauss/noise"][None], z0, z0), G["gauss/out"], TOL_SUM)
    cases["noniid"] = (dict(kind="complexN", band_sigma=G["noniid/band_sigma"][None]), (G["noniid/noise"][None], z0, z0), G["noniid/out"], TOL_SUM)
    off = np.zeros((1, C, N), np.float32)
    for i, b in enumerate(G["stripe/bands"]):
        off[0, int(b), G["stripe/loc%d" % i].astype(int)] = G["stripe/val%d" % i]
    cases["stripe"] = (dict(kind="complexN", sub=[2], col_off=off), (z0, z0, z0), G["stripe/out"], TOL_SUM)
    dead = np.zeros((1, C, N), np.uint8)
    for i, b in enumerate(G["deadline/bands"]):
        dead[0, int(b), G["deadline/loc%d" % i].astype(int)] = 1
    cases["deadline"] = (dict(kind="complexN", sub=[0], col_dead=dead), (z0, z0, z0), G["deadline/out"], None)
    # impulse: the fixture stores the flipped / salted sets; as draws, u0 = 0 where flipped (< amount 0.5) else 0.75, u1 = 0.25 / 0.75
    flag = np.zeros((1, C), np.uint8)
    u0, u1 = np.full(shape, 0.75, np.float32), np.full(shape, 0.75, np.float32)
    for i, b in enumerate(G["impulse/bands"]):
        flag[0, int(b)] = 1
        u0[0, int(b)][G["impulse/flipped"][i].astype(bool)] = 0.0
        u1[0, int(b)][G["impulse/salted"][i].astype(bool)] = 0.25
    u0[0, flag[0] == 0] = 0.0                                                    # bands that were not chosen must not flip whatever u0 says
    cases["impulse"] = (dict(kind="complexN", sub=[1], param=[0.5], band_flag=flag), (z0, u0, u1), G["impulse/out"], None)
    cases["mask"] = (dict(kind="inpaint", param=[0.8]), (z0, G["mask/u"][None].astype(np.float32), z0), G["mask/out"], None)
    lost = np.zeros((1, C), np.uint8)
    lost[0, G["bandloss/lost"].astype(int)] = 1
    cases["bandloss"] = (dict(kind="bandmiss", band_flag=lost), None, G["bandloss/out"], None)
    for k in (7, 9, 15):
        cases["gblur%d" % k] = (dict(kind="blur", kernels=[DO.gaussian_kernel2d(k)]), None, G["gblur%d/out" % k], TOL_TAPS)
    cases["cblur9"] = (dict(kind="blur", kernels=[DO.circle_kernel2d(9)]), None, G["cblur9/out"], TOL_TAPS)
    cases["sblur5"] = (dict(kind="blur", kernels=[np.full((5, 5), 1 / 25, dtype=np.float32)]), None, G["sblur5/out"], TOL_TAPS)
    for f in (2, 4, 8):
        cases["sr%d" % f] = (dict(kind="sr", sr_factor=[f]), None, G["sr%d/out" % f], TOL_TAPS)
    return x[None], cases


def check_fixtures(dev, names=None, modes=range(8)):
    x, cases = fixture_cases()
    for name, (kw, dr, want, tol) in cases.items():
        if names is not None and name not in names:
            continue
        got0, cl0 = one_kind(dev, x, aug=0, draws3=dr, **kw)
        err = np.abs(got0[0].astype(np.float64) - want).max()
        print("fixture %-9s aug 0: max abs error %.3g (bar %s)" % (name, err, "bitwise" if tol is None else "%.1g" % tol))
        if tol is None:
            assert np.array_equal(got0[0], want), name
        else:
            assert err <= tol, (name, err)
        assert np.array_equal(cl0, x), name
        for m in modes:
            got, cl = one_kind(dev, x, aug=m, draws3=dr, **kw)
            assert np.array_equal(got[0], DO.augment(got0[0], m)), (name, m)
            assert np.array_equal(cl[0], GOLD["aug%d/out" % m]), (name, m)


# ---- one mixed batch against the tensor path ---------------------------------------------------------------------------------------------
MIXED = ["gaussianN", "complexN:0", "complexN:1", "complexN:2", "blur:0", "blur:1", "blur:2", "blur:3", "sr:0", "sr:1", "sr:2", "inpaint", "bandmiss",
         "haze", "none", "gaussianN"]


def check_mixed_batch(dev):
    """B = 16, C = 5, N = 32: every kind (all three complexN subtypes, four stencils, three sr factors), all eight modes, explicit draws
    shared by the launch and the tensor functions of mp-hsir_amd/degrade.py"""
    from mp_hsir_amd import degrade as D
    B, C, N = 16, 5, 32
    rs = np.random.RandomState(11)
    x = rs.rand(B, C, N, N).astype(np.float32)
    z, u0, u1 = rs.randn(B, C, N, N).astype(np.float32), rs.rand(B, C, N, N).astype(np.float32), rs.rand(B, C, N, N).astype(np.float32)
    kernels = [D.gaussian_kernel2d(9), D.motion_kernel2d(15, 45), D.circle_kernel2d(9), D.gaussian_kernel2d(21)]
    factors = [2, 4, 8]
    menu = ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss", "haze", "none"]
    task = [menu.index(s.split(":")[0]) for s in MIXED]
    sub = [int(s.split(":")[1]) if ":" in s else 0 for s in MIXED]
    aug = [(3 * b + 1) % 8 for b in range(B)]
    assert sorted(set(aug)) == list(range(8))
    param = rs.choice([0.1, 0.3, 0.5, 0.7], B).astype(np.float32)
    param[MIXED.index("haze")] = 0.9
    band_sigma = rs.choice([10, 30, 50, 70], (B, C)).astype(np.float32) / 255
    bands = rs.rand(B, C) < 0.5
    bands[:, 0] = True
    is_cx = np.array([s.startswith("complexN") for s in MIXED])
    dead = (rs.rand(B, C, N) < 0.1) & bands[:, :, None] & (np.array(sub) == 0)[:, None, None] & is_cx[:, None, None]
    off = ((rs.rand(B, C, N) * 0.5 - 0.25) * (rs.rand(B, C, N) < 0.1) * bands[:, :, None] * ((np.array(sub) == 2) & is_cx)[:, None, None]).astype(np.float32)
    lost = rs.rand(B, C) < 0.4
    flag = np.where(np.array([s == "bandmiss" for s in MIXED])[:, None], lost, bands)
    cirrus = rs.rand(B, N, N).astype(np.float32) * 1.3                    # some 1 - omega * cirrus <= 0
    tt = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a)).to(dt).to(dev)      # noqa: E731
    xt, zt, u0t, u1t = tt(x), tt(z), tt(u0), tt(u1)
    atm = xt.reshape(B, C, -1).topk(1, dim=-1).values.mean(-1)
    lam = torch.linspace(400, 1000, 100, dtype=torch.float64)[:C]
    plan = make_plan(dev, B, C, N, menu, task=task, aug=aug, param=param, sub=sub, kernels=kernels, sr_factor=factors, band_sigma=band_sigma,
                     band_flag=flag, col_dead=dead, col_off=off, cirrus=cirrus, atm=atm, haze_ratio=(lam[0] / lam).float())
    got, cl = run(dev, x, plan, (z, u0, u1))
    assert np.array_equal(cl, aug_batch(x, aug)), "clean_aug must be a bitwise copy under the mode"
    assert (1 - 0.9 * cirrus[MIXED.index("haze")] <= 0).any()
    for b, spec in enumerate(MIXED):
        name, xs, s = spec.split(":")[0], xt[b:b + 1], slice(b, b + 1)
        if name == "gaussianN":
            want, tol = D.gaussian_noise(xs, tt(param[s]), zt[s]), TOL_SUM
        elif name == "complexN":
            y = D.gaussian_noise_non_iid(xs, tt(band_sigma[s]), zt[s])
            y = D.deadline_noise(y, tt(dead[s], torch.bool))
            flipped = (u0t[s] < float(param[b])) & tt(bands[s], torch.bool)[:, :, None, None] & bool(sub[b] == 1)
            y = D.impulse_noise(y, flipped, u1t[s] < 0.5)
            want, tol = D.stripe_noise(y, tt(bands[s], torch.bool), tt(off[s])), TOL_SUM
        elif name == "blur":
            want, tol = D.blur(xs, kernels[sub[b]]), TOL_TAPS
        elif name == "sr":
            want, tol = D.super_resolution_input(xs, factors[sub[b]]), TOL_TAPS
        elif name == "inpaint":
            want, tol = D.random_mask(xs, u0t[s], tt(param[s])), None
        elif name == "bandmiss":
            want, tol = D.band_loss(xs, tt(lost[s], torch.bool)), None
        elif name == "haze":
            want, tol = D.haze(xs, tt(cirrus[s]), tt(param[s])), TOL_HAZE
        else:
            want, tol = xs, None
        want = D.augment(want, torch.tensor([aug[b]], device=want.device))[0].cpu().numpy()
        err = np.abs(got[b].astype(np.float64) - want).max()
        print("mixed batch sample %2d %-11s mode %d: max abs difference %.3g (bar %s)" % (b, spec, aug[b], err, "bitwise" if tol is None else "%.1g" % tol))
        if tol is None:
            assert np.array_equal(got[b], want), spec
        else:
            assert err <= tol, (spec, err)


# ---- float64 oracle for one kind (C,H,W) ---------------------------------------------------------------------------------------------------
def oracle_blur(x, ker):
    C, H, W = x.shape
    k = ker.shape[0]
    p = k // 2
    xp = np.zeros((C, H + 2 * p, W + 2 * p), dtype=np.float64)
    xp[:, p:p + H, p:p + W] = x
    out = np.zeros((C, H, W), dtype=np.float64)
    for dy in range(k):
        for dx in range(k):
            out += float(ker[dy, dx]) * xp[:, dy:dy + H, dx:dx + W]
    return out


def sr_footprint(N, f, y, x):
    """low-resolution pixels (ly, lx) whose clamped 4 x 4 bicubic taps include the source pixel (y, x)"""
    n = N // f

    def hits(v):
        out = []
        for o in range(n):
            i0 = int(np.floor(np.float32(N - 1) / np.float32(n - 1) * np.float32(o)))
            if v in [min(max(i0 + j, 0), N - 1) for j in range(-1, 3)]:
                out.append(o)
        return out
    return [(ly, lx) for ly in hits(y) for lx in hits(x)]


def check_small_planes(dev, shapes=((1, 1, 16), (2, 3, 20), (1, 31, 16))):
    """index math at the smallest planes: a 21 x 21 stencil on N = 16 (halo larger than half the plane), sr f = 8 on N = 16 (a 2 x 2
    low-resolution image), N = 20 (no power of two; quarter turns), C = 1 / 31, B = 1 -- each against the float64 oracle, all eight modes"""
    rs = np.random.RandomState(12)
    for B, C, N in shapes:
        x = rs.rand(B, C, N, N).astype(np.float32)
        ker = rs.rand(21, 21).astype(np.float32)
        ker /= ker.sum()
        for m in range(8):
            got, cl = one_kind(dev, x, "blur", aug=m, kernels=[ker])
            want = aug_batch(np.stack([oracle_blur(x[b], ker) for b in range(B)]), [m] * B)
            err = np.abs(got - want).max()
            assert err <= 441 * 2.0 ** -24, ("blur21", (B, C, N), m, err)
            assert np.array_equal(cl, aug_batch(x, [m] * B))
            fs = [f for f in (2, 4, 5, 8, 10) if N % f == 0 and N // f >= 2]
            for i, f in enumerate(fs):
                got, _ = one_kind(dev, x, "sr", aug=m, sr_factor=fs, sub=[i] * B)
                want = aug_batch(np.stack([DO.resize_nearest(DO.bicubic_downsample(x[b], f), f) for b in range(B)]), [m] * B)
                err = np.abs(got.astype(np.float64) - want).max()
                assert err <= TOL_TAPS, ("sr", f, (B, C, N), m, err)
        print("small planes %s: blur 21 x 21 and sr %s under all modes within bounds" % ((B, C, N), fs))


def check_blur21_at_64(dev):
    """N = 64, k = 21 against the float64 oracle: k^2 2^-24 = 2.6e-5, the sequential fp32 summation bound for weights that sum to 1 over
    data in [0, 1]"""
    rs = np.random.RandomState(13)
    x = rs.rand(1, 2, 64, 64).astype(np.float32)
    ker = DO.gaussian_kernel2d(21)
    got, _ = one_kind(dev, x, "blur", aug=3, kernels=[ker])
    err = np.abs(got[0] - DO.augment(oracle_blur(x[0], ker), 3)).max()
    print("blur k = 21 at N = 64: max abs error %.3g (bound %.3g)" % (err, 441 * 2.0 ** -24))
    assert err <= 441 * 2.0 ** -24


def check_largest_plane(dev):
    """N = 128, the largest plane, with the 21 x 21 halo and the 64 x 64 image of sr f = 2 in one launch: 102 KiB of dynamic LDS, above the
    64 KiB a kernel gets without asking; one blur and one sr sample, under a quarter turn and a flip.  Blur against the float64 oracle.
    sr against the tensor function, which is its definition (bicubic "as F.interpolate"): F.interpolate forms the source coordinate
    scale * o in fp32, whose ulp at 64..127 is 7.6e-6, so at this size it is itself about 1e-5 away from a float64 restatement (printed,
    not asserted) -- the 5e-6 bar is for two fp32 evaluations of the same formula"""
    from mp_hsir_amd import degrade as D
    rs = np.random.RandomState(16)
    x = rs.rand(2, 2, 128, 128).astype(np.float32)
    ker = DO.gaussian_kernel2d(21)
    plan = make_plan(dev, 2, 2, 128, ["blur", "sr"], task=[0, 1], aug=[2, 5], kernels=[ker], sr_factor=[2])
    got, cl = run(dev, x, plan)
    assert np.array_equal(cl, aug_batch(x, [2, 5]))
    e_blur = np.abs(got[0] - DO.augment(oracle_blur(x[0], ker), 2)).max()
    tens = D.super_resolution_input(torch.as_tensor(x[1:2]).to(dev), 2)[0].cpu().numpy()
    f64 = DO.resize_nearest(DO.bicubic_downsample(x[1], 2), 2)
    e_sr = np.abs(got[1].astype(np.float64) - DO.augment(tens, 5)).max()
    print("N = 128: blur 21 x 21 max abs error %.3g (bound %.3g); sr f = 2 against the tensor function %.3g (bar %.1g); against float64: kernel %.3g, "
          "tensor function %.3g" % (e_blur, 441 * 2.0 ** -24, e_sr, TOL_TAPS, np.abs(got[1] - DO.augment(f64, 5)).max(), np.abs(tens - f64).max()))
    assert e_blur <= 441 * 2.0 ** -24 and e_sr <= TOL_TAPS


def check_kernel_philox_known_answer(dev):
    """the kernel's own Philox against Random123's known answer: element 0 of the cube under seed 0, ordinal 0 is counter 0^4, key 0^2,
    whose third word 0xbc57ac4c gives u0 = 0xbc57ac * 2^-24; inpainting keeps the element for a ratio one step below u0 and drops it at u0"""
    u0 = np.float32(0xbc57ac * 2.0 ** -24)
    ones = np.ones((2, 1, 16, 16), np.float32)
    got, _ = one_kind(dev, ones, "inpaint", param=[np.nextafter(u0, np.float32(0)), u0], seed=0, ordinal=0)
    assert got[0, 0, 0, 0] == 1.0, "u0 > ratio for the ratio just below the known answer"
    want = draws(0, 0, ones.shape)[1]
    assert want[0, 0, 0, 0] == u0 and np.array_equal(got[1], (want[1] > u0).astype(np.float32))


# ---- generated draws ------------------------------------------------------------------------------------------------------------------------
def check_generated_uniforms(dev, seed=0x1234567887654321, ordinal=5):
    """u0 through inpaint at several ratios and through complexN / impulse at several amounts (u1: salt or pepper): the kept / flipped /
    salted sets are bitwise those of the helper"""
    B, C, N = 4, 3, 20
    _, u0, u1 = draws(seed, ordinal, (B, C, N, N))
    ones = np.ones((B, C, N, N), np.float32)
    ratios = np.array([0.1, 0.5, 0.8, 0.97], np.float32)
    for m in (0, 6):
        got, _ = one_kind(dev, ones, "inpaint", aug=m, param=ratios, seed=seed, ordinal=ordinal)
        want = aug_batch((u0 > ratios[:, None, None, None]).astype(np.float32), [m] * B)
        assert np.array_equal(got, want), "inpaint kept set (mode %d)" % m
        half = ones * 0.5
        got, _ = one_kind(dev, half, "complexN", aug=m, param=ratios, sub=[1] * B, band_flag=np.ones((B, C), np.uint8), seed=seed, ordinal=ordinal)
        flipped = u0 < ratios[:, None, None, None]
        want = aug_batch(np.where(flipped, np.where(u1 < 0.5, 1.0, 0.0), 0.5).astype(np.float32), [m] * B)
        assert np.array_equal(got, want), "impulse flipped / salted sets (mode %d)" % m
    assert 0.3 < (u0 < 0.5).mean() < 0.7


def check_generated_normal(dev, seed=77, ordinal=3, shape=(1, 31, 64, 64)):
    """z through gaussianN on a zero cube with sigma = 1 against the float64 helper; moments over 31 x 64 x 64 draws"""
    z, _, _ = draws(seed, ordinal, shape)
    got, _ = one_kind(dev, np.zeros(shape, np.float32), "gaussianN", param=[1.0] * shape[0], seed=seed, ordinal=ordinal)
    dev_max = np.abs(got.astype(np.float64) - z).max()
    n = z.size
    mean, var = got.astype(np.float64).mean(), got.astype(np.float64).var()
    print("generated z: max |kernel - float64 helper| %.3g over %d draws (tolerance %.3g); mean %.3g (5 sigma %.3g), var - 1 %.3g (5 sigma %.3g)"
          % (dev_max, n, Z_TOL, mean, 5 / np.sqrt(n), var - 1, 5 * np.sqrt(2.0 / n)))
    assert dev_max <= Z_TOL
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2.0 / n)
    return dev_max


def check_generated_properties(dev):
    B, C, N = 3, 4, 20
    x = np.random.RandomState(14).rand(B, C, N, N).astype(np.float32)
    kw = dict(kind="complexN", param=[0.3] * B, sub=[1] * B, band_flag=np.ones((B, C), np.uint8), band_sigma=np.full((B, C), 0.1, np.float32))
    a, _ = one_kind(dev, x, seed=9, ordinal=2, **kw)
    b, _ = one_kind(dev, x, seed=9, ordinal=2, **kw)
    assert np.array_equal(a, b), "same (seed, ordinal): bitwise equal"
    assert not np.array_equal(a, one_kind(dev, x, seed=9, ordinal=3, **kw)[0]) and not np.array_equal(a, one_kind(dev, x, seed=10, ordinal=2, **kw)[0])
    assert not np.array_equal(a, one_kind(dev, x, seed=9 + (1 << 32), ordinal=2, **kw)[0]), "the high word of the seed is part of the key"
    for m in range(1, 8):
        got, _ = one_kind(dev, x, aug=m, seed=9, ordinal=2, **kw)
        assert np.array_equal(got, aug_batch(a, [m] * B)), "mode %d: the draws follow the source element" % m
    # a device ordinal gives what the same host ordinal gives
    plan = make_plan(dev, B, C, N, ["complexN"], **{k: v for k, v in kw.items() if k != "kind"})
    from mp_hsir_amd import ops
    c, _ = ops.degrade_batch(torch.as_tensor(x).to(dev), plan, seed=9, ordinal=torch.tensor([2], dtype=torch.int64, device=dev))
    assert np.array_equal(c.cpu().numpy(), a)


def check_nan_poisons_its_dependents(dev):
    """one NaN at (b 0, c 1, y 5, x 17) of a (1,3,32,32) cube: the set of NaN outputs per kind, under a transposing mode"""
    N, m, pos = 32, 3, (5, 17)
    x = np.random.RandomState(15).rand(1, 3, N, N).astype(np.float32)
    x[0, 1, pos[0], pos[1]] = np.nan

    def expect(mask2d):
        full = np.zeros((1, 3, N, N), bool)
        full[0, 1] = mask2d
        return aug_batch(full, [m])
    own = np.zeros((N, N), bool)
    own[pos] = True
    kern = np.full((7, 7), 1 / 49, np.float32)
    nb = np.zeros((N, N), bool)
    nb[max(pos[0] - 3, 0):pos[0] + 4, max(pos[1] - 3, 0):pos[1] + 4] = True
    srm = np.zeros((N, N), bool)
    for ly, lx in sr_footprint(N, 4, *pos):
        srm[4 * ly:4 * ly + 4, 4 * lx:4 * lx + 4] = True
    assert 16 <= srm.sum() <= 16 * 16
    ones = np.ones((1, 3), np.uint8)
    for name, kw, mask in (("gaussianN", dict(param=[0.1]), own), ("blur", dict(kernels=[kern]), nb), ("sr", dict(sr_factor=[4]), srm),
                           ("inpaint", dict(param=[0.9]), own), ("bandmiss", dict(band_flag=ones), own), ("none", {}, own),
                           ("haze", dict(param=[0.5], cirrus=np.full((1, N, N), 0.5), atm=np.ones((1, 3)), haze_ratio=np.ones(3)), own)):
        got, cl = one_kind(dev, x, name, aug=m, seed=1, ordinal=1, **kw)
        assert np.array_equal(np.isnan(got), expect(mask)), name
        assert np.array_equal(np.isnan(cl), expect(own)), name
    # an impulse replaces the element: with amount 1 every element of a chosen band flips, and the NaN is gone
    got, _ = one_kind(dev, x, "complexN", aug=m, param=[1.0], sub=[1], band_flag=ones, seed=1, ordinal=1)
    assert not np.isnan(got).any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    import pytest
    from mp_hsir_amd import degrade as D
    from mp_hsir_amd import ops
    x = torch.zeros((1, 2, 16, 16), device=dev)

    def call(clean=x, N=16, draws3=None, **kw):
        B, C = clean.shape[:2]
        return ops.degrade_batch(clean, make_plan(dev, B, C, N, **kw), seed=0, ordinal=0, draws=draws3)
    with pytest.raises(RuntimeError, match="must be square"):
        ops.degrade_batch(torch.zeros((1, 2, 16, 20), device=dev), ops.DegradePlan([0], task=torch.zeros(1, dtype=torch.int32, device=dev),
                                                                                   aug=torch.zeros(1, dtype=torch.int32, device=dev)), seed=0, ordinal=0)
    with pytest.raises(RuntimeError, match="does not fit in LDS"):
        call(torch.zeros((1, 1, 132, 132), device=dev), N=132, menu=["none"])
    with pytest.raises(RuntimeError, match="must be odd and <= 21"):
        call(menu=["blur"], kernels=[np.ones((8, 8))])
    with pytest.raises(RuntimeError, match="must be odd and <= 21"):
        p = make_plan(dev, 1, 2, 16, ["blur"], kernels=[np.ones((21, 21))])
        p.ksize = [23]
        ops.degrade_batch(x, p, seed=0, ordinal=0)
    with pytest.raises(RuntimeError, match="must divide N = 16"):
        call(menu=["sr"], sr_factor=[3])
    with pytest.raises(RuntimeError, match="leave N / f >= 2"):
        call(menu=["sr"], sr_factor=[16])
    with pytest.raises(RuntimeError, match="unknown kind 8"):
        call(menu=["none", 8])
    z = torch.zeros_like(x)
    for dr in ((z, None, None), (z, z, None), (None, z, z)):
        with pytest.raises(RuntimeError, match="all three or none"):
            call(menu=["gaussianN"], draws3=dr)
    call(menu=["gaussianN"], draws3=(z, z, z))
    with pytest.raises(ValueError, match="poissonN"):
        D.DegradationSynthesizer("remote_sensing", ["gaussianN", "poissonN"], dev, fused=True)
    D.DegradationSynthesizer("remote_sensing", ["gaussianN", "poissonN"], dev)                    # the tensor path keeps it


# ---- the synthesiser ---------------------------------------------------------------------------------------------------------------------
def check_synthesizer_fused(dev, B=48):
    """everything tests/test_degrade.py::check_synthesizer asserts of the tensor path, then per kind by the returned task ids"""
    import pytest
    from mp_hsir_amd import degrade as D
    types = ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"]
    syn = D.DegradationSynthesizer("natural_scene", types, dev, seed=7, fused=True)
    C, N = 31, 64
    clean_b = torch.rand((B, C, N, N), generator=torch.Generator().manual_seed(3)).to(dev)
    deg, cl, prompt = syn(clean_b)
    assert deg.shape == cl.shape == clean_b.shape and prompt.shape == (B, 1) and prompt.dtype == torch.int64
    assert int(prompt.min()) >= 0 and int(prompt.max()) <= 5 and len(prompt.unique()) >= 4
    assert torch.isfinite(deg).all()
    assert torch.equal(cl.flatten(1).sort(dim=1).values, clean_b.flatten(1).sort(dim=1).values)
    assert not torch.equal(cl, clean_b), "modes are drawn from 1..7"
    deg, cl, ids = deg.cpu().double(), cl.cpu().double(), prompt[:, 0].cpu().tolist()
    n = C * N * N
    seen = set()
    for b, t in enumerate(ids):
        y, x, name = deg[b], cl[b], types[t]
        r = y - x
        seen.add(name)
        if name == "gaussianN":
            s = float(r.std()) * 255
            tol = 5.0 / np.sqrt(2.0 * n)                               # relative standard error of a standard deviation over n samples
            assert 30 * (1 - tol) <= s <= 70 * (1 + tol), (b, s)
        elif name == "inpaint":
            kept = float((y != 0).double().mean())
            assert any(abs(kept - (1 - q)) <= 5 * np.sqrt(q * (1 - q) / n) for q in (0.7, 0.8, 0.9)), (b, kept)
            assert torch.equal(y[y != 0], x[y != 0])
        elif name == "bandmiss":
            lost = int((y.flatten(1).abs().sum(1) == 0).sum())
            assert lost in (int(np.float32(0.1) * C), int(np.float32(0.2) * C), int(np.float32(0.3) * C)) and lost in (3, 6, 9), (b, lost)
            keep = y.flatten(1).abs().sum(1) != 0
            assert torch.equal(y[keep], x[keep])
        elif name == "sr":
            fs = [f for f in (2, 4, 8) if all(torch.equal(y[:, i::f, j::f], y[:, 0::f, 0::f]) for i in range(f) for j in range(f))]
            assert fs, "sample %d is not constant on f x f blocks for any f of the menu" % b
        elif name == "blur":
            assert float(r.abs().max()) > 0.05 and float(y.min()) >= 0 and float(y.max()) <= 1
        elif name == "complexN":
            # in the source frame stripes and dead lines run along columns; under a transposing mode along rows: look along both axes
            found = []
            for axis in (1, 2):
                dead_cols = (y == 0).all(dim=axis)                                   # (C, 64)
                nb = int((dead_cols.sum(1) > 0).sum())
                if nb:
                    cnt = dead_cols.sum(1)
                    assert nb == C // 3 and int(cnt[cnt > 0].min()) >= 4 and int(cnt.max()) <= 9, (b, nb, cnt)
                    found.append("deadline")
            ones = (y == 1).flatten(1).sum(1)
            if int(ones.sum()):
                assert int((ones > 0).sum()) == C // 3, (b, ones)
                found.append("impulse")
            if not found:
                hit = False
                for axis in (1, 2):
                    mu = r.mean(dim=axis)                                            # (C, 64) line means of the residual
                    sd = r.flatten(1).std(dim=1, keepdim=True) / np.sqrt(N)
                    lines = (mu.abs() > 6 * sd).sum(1)
                    if int(lines.sum()):
                        assert int((lines > 0).sum()) <= C // 3 and int(lines.max()) <= 8, (b, lines)
                        hit = True
                assert hit, "complexN sample %d shows no subtype" % b
                found.append("stripe")
            assert len(found) == 1, (b, found)
            seen.add("complexN/" + found[0])
    print("synthesiser fused=True: kinds seen %s" % sorted(seen))
    assert {"gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"} <= seen
    # the batch ordinal counts calls: the same clean batch again gives another batch; the remote-sensing menu (haze, circle blur) runs
    d2 = syn(clean_b)[0]
    assert not torch.equal(d2.cpu().double(), deg)
    syn2 = D.DegradationSynthesizer("remote_sensing", ["gaussianN", "complexN", "blur", "sr", "inpaint", "haze", "bandmiss", "circle_blur"], dev, seed=9,
                                    fused=True)
    d3, c3, p3 = syn2(torch.rand((14, 100, 64, 64), generator=torch.Generator().manual_seed(4)).to(dev))
    assert torch.isfinite(d3).all() and int(p3.max()) <= 7 and d3.shape == (14, 100, 64, 64)
    with pytest.raises(ValueError):
        D.DegradationSynthesizer("natural_scene", ["haze"], dev, fused=True)
