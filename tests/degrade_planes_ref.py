"""TEST INFRASTRUCTURE for the tiled degradation launch (mphsir_degrade_planes, mp-hsir_amd/csrc/degrade.hip): the checks that
tests/test_degrade_planes_emu.py (CPU emulator) and tests/test_degrade_planes_gpu.py (MI355X) share, each taking the device the bound
library runs on.  Built on tests/degrade_fused_ref.py: its plan builder, its numpy Philox draws and its tolerances -- the bars the plane
form is held to; no tolerance is introduced here."""
import ctypes
import types

import numpy as np
import pytest
import torch

import degrade_fused_ref as R
from degrade_fused_ref import TOL_HAZE, TOL_SUM, TOL_TAPS, Z_TOL

MENU = ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss", "haze"]
# every kind with every subtype / stencil / factor of the one plan: (kind, sub)
VARIANTS = [("gaussianN", 0), ("complexN", 0), ("complexN", 1), ("complexN", 2), ("blur", 0), ("blur", 1), ("blur", 2), ("blur", 3), ("sr", 0),
            ("sr", 1), ("sr", 2), ("inpaint", 0), ("bandmiss", 0), ("haze", 0)]
FACTORS = [2, 4, 8]


def kernels():
    from mp_hsir_amd import degrade as D
    return [D.gaussian_kernel2d(7), D.gaussian_kernel2d(15), D.gaussian_kernel2d(21), D.motion_kernel2d(15, 45)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_dev(dev, a, dt=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dt).contiguous().to(dev)


def tables(rs, B, C, H, W):
    """random tables of every kind for a (B,C,H,W) cube; some 1 - omega * cirrus <= 0"""
    lam = torch.linspace(400, 1000, 100, dtype=torch.float64)[:C]
    flag = rs.rand(B, C) < 0.5
    flag[:, 0] = True
    return dict(band_sigma=rs.choice([10, 30, 50, 70], (B, C)).astype(np.float32) / 255, band_flag=flag, col_dead=rs.rand(B, C, W) < 0.1,
                col_off=((rs.rand(B, C, W) * 0.5 - 0.25) * (rs.rand(B, C, W) < 0.1)).astype(np.float32), cirrus=rs.rand(B, H, W).astype(np.float32) * 1.3,
                atm=rs.rand(B, C).astype(np.float32), haze_ratio=(lam[0] / lam).float().numpy())


def make_plan(dev, B, C, H, W, variants, modes, tabs, param, with_sr=True):
    """the one plan (every kind in the menu, four stencils, three factors) with sample b as variants[b] under modes[b] (None: aug NULL).
    degrade_fused_ref.make_plan shapes its tables by one N: the column tables and the cirrus map are set here, by (H, W).  with_sr=False:
    no sr in the menu and no factor table (extents that 2, 4 and 8 do not divide)"""
    menu = [k for k in MENU if with_sr or k != "sr"]
    task = [menu.index(k) for k, _ in variants]
    plan = R.make_plan(dev, B, C, W, menu, task=task, aug=modes if modes is not None else [0] * B, param=param, sub=[s for _, s in variants], kernels=kernels(),
                       sr_factor=FACTORS if with_sr else [], **{k: v for k, v in tabs.items() if k != "cirrus"})
    plan.cirrus = to_dev(dev, tabs["cirrus"]).reshape(B, H, W).contiguous()
    if modes is None:
        plan.aug = None
    return plan


def run_planes(dev, x, plan, draws3=None, seed=0, ordinal=0, want_clean=True, out=None):
    from mp_hsir_amd import ops
    dr = None if draws3 is None else tuple(to_dev(dev, d) for d in draws3)
    deg, cl = ops.degrade_planes(to_dev(dev, x), plan, seed=seed, ordinal=ordinal, draws=dr, out=out, want_clean=want_clean)
    return deg.cpu().numpy(), None if cl is None else cl.cpu().numpy()


# ---- 1. bitwise against the plane form ------------------------------------------------------------------------------------------------------
def check_bitwise_against_the_plane_form(dev, N, explicit, pairs=None):
    """B = 2, C = 3: every (variant, mode) pair of `pairs` (default: all 14 x 8), two per launch, through both entry points with one
    plan, seed 77, ordinal 3 (or explicit draws); a NaN at (63, 64) of band 1 of every blur and sr sample"""
    from mp_hsir_amd import ops
    B, C = 2, 3
    rs = np.random.RandomState(21 + N)
    pairs = list(pairs) if pairs is not None else [(v, m) for m in range(8) for v in range(len(VARIANTS))]
    assert len(pairs) % 2 == 0
    tabs = tables(rs, B, C, N, N)
    dr = None
    if explicit:
        dr = tuple(to_dev(dev, a) for a in (rs.randn(B, C, N, N), rs.rand(B, C, N, N), rs.rand(B, C, N, N)))
    seen = set()
    for i in range(0, len(pairs), 2):
        vs, ms = [VARIANTS[pairs[i + j][0]] for j in range(2)], [pairs[i + j][1] for j in range(2)]
        x = rs.rand(B, C, N, N).astype(np.float32)
        for b, (kind, _) in enumerate(vs):
            if kind in ("blur", "sr"):
                x[b, 1, 63, 64] = np.nan
        plan = make_plan(dev, B, C, N, N, vs, ms, tabs, rs.choice([0.1, 0.3, 0.5, 0.9], B).astype(np.float32))
        xt = to_dev(dev, x)
        want = ops.degrade_batch(xt, plan, seed=77, ordinal=3, draws=dr)
        got = ops.degrade_planes(xt, plan, seed=77, ordinal=3, draws=dr)
        for name, g, w in zip(("degraded", "clean_aug"), got, want):
            g, w = g.cpu().numpy(), w.cpu().numpy()
            for b in range(B):
                assert np.array_equal(bits(g[b]), bits(w[b])), "%s of %s under mode %d at N = %d differs from the plane form in %d elements" % (
                    name, vs[b], ms[b], N, int((bits(g[b]) != bits(w[b])).sum()))
        for b, (kind, sub) in enumerate(vs):
            if kind in ("blur", "sr"):
                # the NaN reaches the outputs that depend on it (for sr: when a low-resolution pixel has it among its taps) and no other band
                hit = kind == "blur" or bool(R.sr_footprint(N, FACTORS[sub], 63, 64))
                assert np.isnan(got[0][b, 1].cpu().numpy()).any() == hit and not np.isnan(got[0][b, 0].cpu().numpy()).any()
            seen.add((vs[b], ms[b]))
    print("N = %d, %s draws: %d (kind, mode) pairs bitwise equal to the plane form" % (N, "explicit" if explicit else "generated", len(seen)))
    return seen


# ---- 2. beyond the plane form, against the tensor functions ---------------------------------------------------------------------------------
def tensor_reference(dev, variant, xt, tabs, param, zt, u0t, u1t):
    """-> (the tensor function of mp-hsir_amd/degrade.py for one variant on the (1,C,H,W) cube, tolerance or None for bitwise)"""
    from mp_hsir_amd import degrade as D
    kind, sub = variant
    tb = lambda k, dt=torch.float32: to_dev(dev, tabs[k], dt)      # noqa: E731
    par = to_dev(dev, param)
    if kind == "gaussianN":
        return D.gaussian_noise(xt, par, zt), TOL_SUM
    if kind == "complexN":
        y = D.gaussian_noise_non_iid(xt, tb("band_sigma"), zt)
        y = D.deadline_noise(y, tb("col_dead", torch.bool))
        flipped = (u0t < float(param[0])) & tb("band_flag", torch.bool)[:, :, None, None] & bool(sub == 1)
        y = D.impulse_noise(y, flipped, u1t < 0.5)
        return D.stripe_noise(y, torch.ones_like(tb("band_flag", torch.bool)), tb("col_off")), TOL_SUM
    if kind == "blur":
        return D.blur(xt, kernels()[sub].to(dev)), TOL_TAPS
    if kind == "sr":
        return D.super_resolution_input(xt, FACTORS[sub]), TOL_TAPS
    if kind == "inpaint":
        return D.random_mask(xt, u0t, par), None
    if kind == "bandmiss":
        return D.band_loss(xt, tb("band_flag", torch.bool)), None
    if kind == "haze":
        # D.haze with the plan's own atmospheric light (the function takes it from the cube: the top pixel here)
        return D.haze(xt, tb("cirrus"), par), TOL_HAZE
    raise AssertionError(kind)


def check_against_the_tensor_functions(dev, shape, with_sr):
    """mode 0 (aug NULL), explicit draws, one variant per launch on a plane no plane form accepts"""
    B, C, H, W = shape
    assert B == 1
    rs = np.random.RandomState(31 + W)
    x = rs.rand(*shape).astype(np.float32)
    z, u0, u1 = rs.randn(*shape).astype(np.float32), rs.rand(*shape).astype(np.float32), rs.rand(*shape).astype(np.float32)
    xt, zt, u0t, u1t = (to_dev(dev, a) for a in (x, z, u0, u1))
    tabs = tables(rs, B, C, H, W)
    tabs["atm"] = x.reshape(B, C, -1).max(-1)                             # top_k = 1 at these sizes: D.haze takes the top pixel
    assert max(int(H * W * 0.01 / 100), 1) == 1
    for variant in VARIANTS:
        if variant[0] == "sr" and not with_sr:
            continue
        param = np.array([0.9 if variant[0] == "haze" else 0.3], np.float32)
        plan = make_plan(dev, B, C, H, W, [variant], None, tabs, param, with_sr)
        got, cl = run_planes(dev, x, plan, (z, u0, u1))
        assert np.array_equal(bits(cl), bits(x)), "clean_aug under mode 0 is a bitwise copy"
        want, tol = tensor_reference(dev, variant, xt, tabs, param, zt, u0t, u1t)
        want = want.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want).max()
        print("%s %-14s max abs difference %.3g (bar %s)" % (shape, variant, err, "bitwise" if tol is None else "%.1g" % tol))
        if tol is None:
            assert np.array_equal(got, want), variant
        else:
            assert err <= tol, (variant, err)
    assert (1 - 0.9 * tabs["cirrus"] <= 0).any()


# ---- 3. generated draws on a non-square plane -------------------------------------------------------------------------------------------------
def check_generated_draws(dev, shape=(1, 2, 72, 136), seed=77, ordinal=3):
    B, C, H, W = shape
    z, u0, _ = R.draws(seed, ordinal, shape)
    rs = np.random.RandomState(5)
    tabs = tables(rs, B, C, H, W)
    sigma = 0.25
    x = rs.rand(*shape).astype(np.float32)
    plan = make_plan(dev, B, C, H, W, [("gaussianN", 0)], None, tabs, np.array([sigma], np.float32))
    got, _ = run_planes(dev, x, plan, seed=seed, ordinal=ordinal)
    err = np.abs(got.astype(np.float64) - (x.astype(np.float64) + z * np.float64(np.float32(sigma)))).max()
    print("generated z on %s: max |kernel - float64 helper| %.3g (bar %.3g sigma + %.1g)" % (shape, err, Z_TOL, TOL_SUM))
    assert err <= Z_TOL * sigma + TOL_SUM
    other, _ = run_planes(dev, x, plan, seed=seed, ordinal=ordinal + 1)
    assert not np.array_equal(got, other), "another ordinal is another cube"
    plan = make_plan(dev, B, C, H, W, [("inpaint", 0)], None, tabs, np.array([0.6], np.float32))
    got, _ = run_planes(dev, x, plan, seed=seed, ordinal=ordinal)
    assert np.array_equal(got, x * (u0 > np.float32(0.6))), "the kept set is bitwise the helper's"
    assert not np.array_equal(got, run_planes(dev, x, plan, seed=seed, ordinal=ordinal + 1)[0])


# ---- 4. clean_aug = NULL, aug = NULL -----------------------------------------------------------------------------------------------------------
def check_optional_pointers(dev):
    """every variant at (2,3,72,72) (square, so that aug may be given) and one at (1,3,67,131): `degraded` with clean_aug = NULL and
    aug = NULL is the run that passes a clean_aug and an aug of zeros; the cube behind `degraded` in one allocation -- where a copy would
    have gone -- keeps its sentinel"""
    for shape, variants in (((2, 3, 72, 72), VARIANTS), ((1, 3, 67, 131), [("blur", 2), ("gaussianN", 0)])):
        B, C, H, W = shape
        rs = np.random.RandomState(41)
        x = rs.rand(*shape).astype(np.float32)
        tabs = tables(rs, B, C, H, W)
        for i in range(0, len(variants), B):
            vs = [variants[(i + b) % len(variants)] for b in range(B)]
            param = rs.choice([0.1, 0.5, 0.9], B).astype(np.float32)
            full, cl = run_planes(dev, x, make_plan(dev, B, C, H, W, vs, [0] * B if H == W else None, tabs, param, H % 8 == 0), seed=3, ordinal=1)
            assert np.array_equal(bits(cl), bits(x))
            buf = torch.full((2,) + shape, -7.0, dtype=torch.float32).to(dev)
            got, none = run_planes(dev, x, make_plan(dev, B, C, H, W, vs, None, tabs, param, H % 8 == 0), seed=3, ordinal=1, out=(buf[0], None))
            assert none is None and np.array_equal(bits(got), bits(full)), vs
            assert bool((buf[1] == -7.0).all()) and np.array_equal(bits(buf[0].cpu().numpy()), bits(full)), "nothing is written beside `degraded`"


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------
def check_refusals(dev):
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    rs = np.random.RandomState(0)
    B, C, H, W = 1, 2, 16, 24
    x = torch.zeros((B, C, H, W)).to(dev)
    tabs = tables(rs, B, C, H, W)
    par = np.zeros(B, np.float32)

    def plan(variants=(("gaussianN", 0),), modes=None):
        return make_plan(dev, B, C, H, W, list(variants), modes, tabs, par)
    ops.degrade_planes(x, plan(), seed=0, ordinal=0)
    with pytest.raises(RuntimeError, match="not square: aug must be NULL"):
        ops.degrade_planes(x, plan(modes=[0]), seed=0, ordinal=0)
    p = plan()
    p.sr_factor = [2, 5]
    with pytest.raises(RuntimeError, match="sr factor 5 must divide H = 16 and W = 24"):
        ops.degrade_planes(x, p, seed=0, ordinal=0)
    p.sr_factor = [8]
    ops.degrade_planes(x, p, seed=0, ordinal=0)
    x2 = torch.zeros((B, C, 32, 16)).to(dev)
    t2 = tables(rs, B, C, 32, 16)
    p2 = make_plan(dev, B, C, 32, 16, [("sr", 0)], None, t2, par)
    p2.sr_factor = [16]
    with pytest.raises(RuntimeError, match="leave H / f >= 2 and W / f >= 2"):
        ops.degrade_planes(x2, p2, seed=0, ordinal=0)
    z = torch.zeros_like(x)
    for dr in ((z, z, None), (z, None, z), (None, z, z)):
        with pytest.raises(RuntimeError, match="all three or none"):
            ops.degrade_planes(x, plan(), seed=0, ordinal=0, draws=dr)
    ops.degrade_planes(x, plan(), seed=0, ordinal=0, draws=(z, z, z))
    p = plan()
    p.menu = p.menu + [8]
    with pytest.raises(RuntimeError, match="unknown kind 8"):
        ops.degrade_planes(x, p, seed=0, ordinal=0)
    p = plan()
    p.ksize = [7, 15, 23, 15]
    with pytest.raises(RuntimeError, match="must be odd and <= 21"):
        ops.degrade_planes(x, p, seed=0, ordinal=0)
    lib = L.load()
    a = L.DegradeArgs()
    a.struct_size -= 4
    assert lib.mphsir_degrade_planes(ctypes.byref(a), None) == -1 and b"struct_size" in lib.mphsir_last_error()
    assert lib.mphsir_degrade_planes(None, None) == -1 and b"null pointer" in lib.mphsir_last_error()


# ---- 6. SceneDegrader ---------------------------------------------------------------------------------------------------------------------------
def scene_opts(**kw):
    o = dict(gaussian_noise_sigma=70, gaussian_noise_sigmas=[10, 30, 50, 70], stripe_nosie_ratio=[0.05, 0.15], deadline_nosie_ratio=[0.05, 0.15],
             impulse_nosie_ratio=[0.1, 0.3, 0.5, 0.7], gaussian_blur_radius=15, motion_blur_radius=(15, 45), downsample_factor=8, mask_ratio=0.9,
             haze_omega=1, bandmis_ratio=0.3)
    o.update(kw)
    return types.SimpleNamespace(**o)


def check_scene_degrader(dev, shape=(1, 9, 72, 136), seed=2025):
    """modes 0-10: the launch against the tensor function of the mode, fed the plan's own tables and the numpy Philox draws of
    (seed, cube ordinal); the tables themselves: the counts of test.py::degrade_for_mode"""
    from mp_hsir_amd import degrade as D
    from mp_hsir_amd import ops
    B, C, H, W = shape
    o = scene_opts()
    x = np.random.RandomState(61).rand(*shape).astype(np.float32)
    xt = to_dev(dev, x)
    sd, twin = D.SceneDegrader("natural_scene", dev, seed), D.SceneDegrader("natural_scene", dev, seed)
    for mode in range(11):
        plan = sd.plan(xt, mode, o)
        got, pid = twin(xt, mode, o)
        ordinal = twin.ordinal
        assert ordinal == mode and pid == {0: 0, 1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 0, 7: 3, 8: 4, 9: 5, 10: 5}[mode]
        sd.ordinal += 1
        again, _ = ops.degrade_planes(xt, plan, seed=seed, ordinal=ordinal, want_clean=False)
        assert torch.equal(got, again), "two degraders with one seed give the same plan and the same cube (mode %d)" % mode
        z, u0, u1 = R.draws(seed, ordinal, shape)
        zt, u0t, u1t = to_dev(dev, z), to_dev(dev, u0), to_dev(dev, u1)
        par = plan.param
        tol_z = 0.0
        if mode == 0:
            assert abs(float(par[0]) - 70 / 255.0) < 1e-7
            want, tol, tol_z = D.gaussian_noise(xt, par, zt), TOL_SUM, Z_TOL * 70 / 255.0
        elif mode <= 4:
            nb = C // 3
            flag, dead, off = plan.band_flag.bool(), plan.col_dead.bool(), plan.col_off
            y = D.gaussian_noise_non_iid(xt, plan.band_sigma, zt)
            y = D.deadline_noise(y, dead)
            y = D.impulse_noise(y, (u0t < par.reshape(B, 1, 1, 1)) & flag[:, :, None, None] & (mode == 4), u1t < 0.5)
            want, tol, tol_z = D.stripe_noise(y, torch.ones_like(flag), off), TOL_SUM, Z_TOL * 70 / 255.0
            sig = set(np.round(plan.band_sigma.cpu().numpy().ravel() * 255).astype(int).tolist())
            assert sig <= {10, 30, 50, 70} and int(plan.sub[0]) == {1: 0, 2: 2, 3: 0, 4: 1}[mode]
            nd, ns = dead.sum(-1)[0].cpu().numpy(), (off != 0).sum(-1)[0].cpu().numpy()
            if mode == 1:
                assert not flag.any() and not dead.any() and not (off != 0).any()
            if mode == 2:           # int(0.05 W) .. int(0.15 W) - 1 columns in floor(C / 3) bands
                assert (ns > 0).sum() <= nb and ns.max() <= int(0.15 * W) - 1 and ns[ns > 0].min() >= int(0.05 * W) and not dead.any()
                assert float(off.abs().max()) <= 0.25
            if mode == 3:           # ceil(0.05 W) .. ceil(0.15 W) - 1 columns in floor(C / 3) bands
                assert (nd > 0).sum() == nb and int(np.ceil(0.05 * W)) <= nd[nd > 0].min() and nd.max() <= int(np.ceil(0.15 * W)) - 1
            if mode == 4:
                assert int(flag.sum()) == nb and round(float(par[0]), 4) in (0.1, 0.3, 0.5, 0.7)
        elif mode in (5, 6):
            ker = D.gaussian_kernel2d(15) if mode == 5 else D.motion_kernel2d(15, 45)
            assert plan.ksize == [15] and torch.equal(plan.stencils[0, :15, :15].cpu(), ker)
            want, tol = D.blur(xt, ker.to(dev)), TOL_TAPS
        elif mode == 7:
            want, tol = D.super_resolution_input(xt, 8), TOL_TAPS
        elif mode == 8:
            want, tol = D.random_mask(xt, u0t, par), None
        elif mode == 9:
            assert float(plan.cirrus.min()) >= 0 and float(plan.cirrus.max()) <= 1 and torch.equal(plan.atm, xt.reshape(B, C, -1).amax(-1))
            want, tol = D.haze(xt, plan.cirrus, par), TOL_HAZE
        else:
            assert int(plan.band_flag.sum()) == int(0.3 * C)
            want, tol = D.band_loss(xt, plan.band_flag.bool()), None
        err = float((got.double() - want.double()).abs().max())
        print("SceneDegrader mode %2d: max abs difference %.3g (bar %s)" % (mode, err, "bitwise" if tol is None else "%.3g" % (tol + tol_z)))
        if tol is None:
            assert torch.equal(got, want.to(got.dtype)), mode
        else:
            assert err <= tol + tol_z, (mode, err)
    # the cube ordinal counts calls: the same cube again is another cube
    a = D.SceneDegrader("natural_scene", dev, seed)
    first, second = a(xt, 0, o)[0], a(xt, 0, o)[0]
    assert a.ordinal == 1 and not torch.equal(first, second)
    assert D.SceneDegrader("remote_sensing", dev, seed).prompt_id(10) == 6
    with pytest.raises(ValueError, match="Poisson"):
        a.plan(xt, 11, o)


# ---- 7. the synthesiser beyond 128 x 128 --------------------------------------------------------------------------------------------------------
def check_synthesizer(dev, B=4, C=5, N=192, calls=6):
    """DegradationSynthesizer(fused=True) at N = 192, both default menus: what degrade_fused_ref.check_synthesizer_fused asserts per kind,
    with the counts of this width.  Several calls, so that most kinds of a menu turn up"""
    from mp_hsir_amd import degrade as D
    from mp_hsir_amd import ops
    menus = {"natural_scene": ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"],
             "remote_sensing": ["gaussianN", "complexN", "blur", "sr", "inpaint", "haze", "bandmiss"]}
    used = []
    real = ops.degrade_planes
    for data_type, menu in menus.items():
        syn = D.DegradationSynthesizer(data_type, menu, dev, seed=7, fused=True)
        clean_b = torch.rand((B, C, N, N), generator=torch.Generator().manual_seed(3)).to(dev)
        seen = set()
        n = C * N * N
        for _ in range(calls):
            ops.degrade_planes = lambda *a, **k: (used.append(1), real(*a, **k))[1]
            try:
                deg, cl, prompt = syn(clean_b)
            finally:
                ops.degrade_planes = real
            assert deg.shape == cl.shape == clean_b.shape and prompt.shape == (B, 1) and prompt.dtype == torch.int64
            assert torch.isfinite(deg).all() and int(prompt.min()) >= 0 and int(prompt.max()) < len(menu)
            assert torch.equal(cl.flatten(1).sort(dim=1).values, clean_b.flatten(1).sort(dim=1).values)
            assert not torch.equal(cl, clean_b), "modes are drawn from 1..7"
            deg_c, cl_c = deg.cpu().double(), cl.cpu().double()
            for b, t in enumerate(prompt[:, 0].cpu().tolist()):
                y, x, name = deg_c[b], cl_c[b], menu[t]
                r = y - x
                seen.add(name)
                if name == "gaussianN":
                    s, tol = float(r.std()) * 255, 5.0 / np.sqrt(2.0 * n)
                    assert 30 * (1 - tol) <= s <= 70 * (1 + tol), (b, s)
                elif name == "inpaint":
                    kept = float((y != 0).double().mean())
                    assert any(abs(kept - (1 - q)) <= 5 * np.sqrt(q * (1 - q) / n) for q in (0.7, 0.8, 0.9)), (b, kept)
                    assert torch.equal(y[y != 0], x[y != 0])
                elif name == "bandmiss":
                    lost = int((y.flatten(1).abs().sum(1) == 0).sum())
                    assert lost in (int(np.float32(0.1) * C), int(np.float32(0.2) * C), int(np.float32(0.3) * C)), (b, lost)
                    keep = y.flatten(1).abs().sum(1) != 0
                    assert torch.equal(y[keep], x[keep])
                elif name == "sr":
                    assert [f for f in (2, 4, 8) if all(torch.equal(y[:, i::f, j::f], y[:, 0::f, 0::f]) for i in range(f) for j in range(f))], b
                elif name == "blur":
                    assert float(r.abs().max()) > 0.05 and float(y.min()) >= 0 and float(y.max()) <= 1
                elif name == "haze":
                    assert float(r.abs().max()) > 0.01 and float(y.min()) >= 0 and float(y.max()) <= 1 + 1e-6
                elif name == "complexN":
                    # in the source frame stripes and dead lines run along columns; under a transposing mode along rows: look along both axes
                    found = []
                    for axis in (1, 2):
                        dead_cols = (y == 0).all(dim=axis)
                        nbd = int((dead_cols.sum(1) > 0).sum())
                        if nbd:
                            cnt = dead_cols.sum(1)
                            assert nbd == C // 3 and int(cnt[cnt > 0].min()) >= int(np.ceil(0.05 * N)) and int(cnt.max()) <= int(np.ceil(0.15 * N)) - 1, (b, cnt)
                            found.append("deadline")
                    ones = (y == 1).flatten(1).sum(1)
                    if int(ones.sum()):
                        assert int((ones > 0).sum()) == C // 3, (b, ones)
                        found.append("impulse")
                    if not found:
                        hit = False
                        for axis in (1, 2):
                            mu = r.mean(dim=axis)
                            sd = r.flatten(1).std(dim=1, keepdim=True) / np.sqrt(N)
                            lines = (mu.abs() > 6 * sd).sum(1)
                            if int(lines.sum()):
                                assert int((lines > 0).sum()) <= C // 3 and int(lines.max()) <= int(0.15 * N) - 1, (b, lines)
                                hit = True
                        assert hit, "complexN sample %d shows no subtype" % b
                        found.append("stripe")
                    assert len(found) == 1, (b, found)
        print("synthesiser fused=True at N = %d, %s: kinds seen %s" % (N, data_type, sorted(seen)))
        assert len(seen) >= len(menu) - 2
    assert len(used) == 2 * calls, "every call beyond 128 x 128 goes through degrade_planes"
    # a plane that fits keeps the plane form's launch
    syn = D.DegradationSynthesizer("natural_scene", menus["natural_scene"], dev, seed=7, fused=True)
    ops.degrade_planes = lambda *a, **k: (_ for _ in ()).throw(AssertionError("degrade_planes at N = 64"))
    try:
        syn(torch.rand((2, C, 64, 64)).to(dev))
    finally:
        ops.degrade_planes = real
