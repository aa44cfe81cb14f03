"""Checks of mphsir_cassi (mp-hsir_amd/csrc/cassi.hip), degrade.cassi_measure / CassiMask and the cassi branches of the synthesiser and of
test.py, written once and run on the CPU emulator (tests/test_cassi_emu.py) and on the GPU (tests/test_cassi_gpu.py): `device` is "cpu"
or "cuda".

Two references.  `numpy_cassi` restates the reference's Degradation._sd_cassi (utils/degradation_utils.py:202-225) in numpy on the fp32
cube and mask; tests/golden/cassi.npz holds what the reference's function itself returned for three cases
(tests/golden/make_cassi_golden.py).  degrade.cassi_measure is the tensor form.  All three and the kernel must give the same FLOATS:
equal where finite or infinite (==, so a zero of either sign is a zero), NaN where the reference has NaN.  No tolerance anywhere."""
import ctypes
import os

import numpy as np
import torch

from util import same_floats  # noqa: F401  (the tests reach it through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cassi.npz")


def numpy_cassi(x, mask, origin, step=2):
    """x (C,H,W) float32, mask (MH,MW), origin (my, mx) -> (C,H,W) float32"""
    C, H, W = x.shape
    my, mx = int(origin[0]), int(origin[1])
    mod = x * mask[my:my + H, mx:mx + W].astype(np.float32)
    meas = np.zeros((H, W + (C - 1) * step), dtype=np.float32)
    for c in range(C):
        meas[:, step * c:step * c + W] += mod[c]
    out = np.stack([meas[:, step * c:step * c + W] for c in range(C)])
    with np.errstate(all="ignore"):
        return ((out - meas.min()) / (meas.max() - meas.min())).astype(np.float32)


def numpy_batch(x, mask, origins, step=2):
    return np.stack([numpy_cassi(x[b], mask, origins[b], step) for b in range(x.shape[0])])


def golden_cases():
    """[(name, clean (C,H,W), mask, origin (2,), out (C,H,W))] of the fixture; the clean cubes are re-created from their seeds"""
    d = np.load(GOLDEN)
    out = []
    for name in ("c9", "c5", "c31"):
        seed, C, H, W = (int(v) for v in d[name + "/seed_shape"])
        out.append((name, np.random.RandomState(seed).rand(C, H, W).astype(np.float32), d[name + "/mask"], d[name + "/origin"], d[name + "/out"]))
    return out


def _dev(a, device, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(device)


def run(device, x, mask, origins=None, step=2, aug=None, task=None, task_id=0, want_clean_aug=False, out=None):
    """numpy in, numpy out through ops.cassi"""
    from mp_hsir_amd import ops
    t = lambda v: None if v is None else _dev(v, device, torch.int32)                   # noqa: E731
    deg, ca = ops.cassi(_dev(x, device), _dev(mask, device), t(origins), step, aug=t(aug), task=t(task), task_id=task_id,
                        want_clean_aug=want_clean_aug, out=out)
    return deg.cpu().numpy(), None if ca is None else ca.cpu().numpy()


def tensor_form(device, x, mask, origins, step, aug=None):
    """degrade.cassi_measure (+ degrade.augment) evaluated on `device`"""
    from mp_hsir_amd import degrade as D
    y = D.cassi_measure(_dev(x, device), _dev(mask, device), None if origins is None else _dev(origins, device), step)
    if aug is not None:
        y = D.augment(y, _dev(aug, device))
    return y.cpu().numpy()


def check_one(device, x, mask, origins, step, aug, want_clean_aug, label):
    from mp_hsir_amd import degrade as D
    got, ca = run(device, x, mask, origins, step, aug, want_clean_aug=want_clean_aug)
    want = numpy_batch(x, mask, origins, step)
    if aug is not None:
        want = D.augment(torch.from_numpy(want), torch.as_tensor(aug)).numpy()
    assert same_floats(got, want), "%s: the kernel differs from numpy at %d of %d elements" % (label, int((got != want).sum()), want.size)
    assert same_floats(got, tensor_form(device, x, mask, origins, step, aug)), "%s: the kernel differs from the tensor form" % label
    assert (ca is not None) == want_clean_aug
    if want_clean_aug:
        ref = x if aug is None else D.augment(torch.from_numpy(x), torch.as_tensor(aug)).numpy()
        assert ca.tobytes() == ref.tobytes(), "%s: clean_aug is not a bitwise copy of augment(clean)" % label
    return got


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
def check_square_all_modes(device, step):
    """B = 3, C = 9, 32 x 32 (one emit block per plane, 8 measure blocks), mask 48 x 40, distinct origins, the 16-byte path; every mode
    0..7 over three calls, with and without clean_aug"""
    rs = np.random.RandomState(100 + step)
    x = rs.rand(3, 9, 32, 32).astype(np.float32)
    mask = (rs.rand(48, 40) < 0.5).astype(np.float32)
    origins = [(0, 0), (16, 8), (7, 3)]
    for aug in ([0, 1, 2], [3, 4, 5], [6, 7, 1]):
        for want in (True, False):
            check_one(device, x, mask, origins, step, aug, want, "step %d, modes %s, clean_aug %s" % (step, aug, want))


def check_non_square(device):
    """(2,5,16,24) with aug=None and a real-valued mask of the plane's size; then 40 rows: two emit blocks, the second partial"""
    rs = np.random.RandomState(5)
    check_one(device, rs.rand(2, 5, 16, 24).astype(np.float32), rs.rand(16, 24).astype(np.float32), [(0, 0), (0, 0)], 2, None, True, "16 x 24")
    check_one(device, rs.rand(1, 3, 40, 8).astype(np.float32), rs.rand(41, 9).astype(np.float32), [(1, 1)], 2, None, True, "40 x 8")


def check_scalar_path(device):
    """(1,7,19,35): W % 4 != 0 and Wm = 35 + 6 * 3 = 53 is odd: element-wise stores, a partial last measure block (19 = 4 * 4 + 3)"""
    rs = np.random.RandomState(7)
    x, mask = rs.rand(1, 7, 19, 35).astype(np.float32), rs.rand(30, 50).astype(np.float32)
    for want in (True, False):
        check_one(device, x, mask, [(11, 15)], 3, None, want, "19 x 35")
    # a square plane of odd width under every mode: the element-wise stores with flips and transposes
    x, mask = rs.rand(2, 3, 9, 9).astype(np.float32), rs.rand(12, 10).astype(np.float32)
    for aug in ([0, 1], [2, 3], [4, 5], [6, 7]):
        check_one(device, x, mask, [(3, 1), (0, 0)], 2, aug, True, "9 x 9, modes %s" % aug)


def check_golden(device):
    """every case of the fixture: the reference's own output, one sample each"""
    for name, x, mask, origin, out in golden_cases():
        got, _ = run(device, x[None], mask, [origin], 2)
        assert same_floats(got[0], out), "%s: the kernel differs from the reference's _sd_cassi" % name


def check_task_filter(device):
    """B = 4, task = [0,1,0,1], task_id = 1, outputs pre-filled: samples 0 and 2 keep the fill bitwise in both outputs, 1 and 3 equal
    the unfiltered call"""
    rs = np.random.RandomState(9)
    x, mask = rs.rand(4, 5, 16, 16).astype(np.float32), rs.rand(20, 20).astype(np.float32)
    origins, aug = [(0, 0), (4, 4), (1, 2), (3, 0)], [1, 2, 3, 4]
    full, full_c = run(device, x, mask, origins, 2, aug, want_clean_aug=True)
    out = (torch.full((4, 5, 16, 16), -7.0, device=device), torch.full((4, 5, 16, 16), -7.0, device=device))
    got, got_c = run(device, x, mask, origins, 2, aug, task=[0, 1, 0, 1], task_id=1, out=out)
    fill = np.full((5, 16, 16), -7.0, dtype=np.float32)
    for b in (0, 2):
        assert got[b].tobytes() == fill.tobytes() and got_c[b].tobytes() == fill.tobytes(), "sample %d was touched" % b
    for b in (1, 3):
        assert got[b].tobytes() == full[b].tobytes() and got_c[b].tobytes() == full_c[b].tobytes(), "sample %d differs from the unfiltered call" % b
    # a task id nobody has: nothing is written
    out[0].fill_(-7.0)
    got, _ = run(device, x, mask, origins, 2, aug, task=[0, 1, 0, 1], task_id=5, out=(out[0], None))
    assert float(got.min()) == -7.0 == float(got.max())


def check_origins(device):
    """origins (-5, 10**6) give the result of the clamped origin (0, MW - W); origin=None is (0, 0)"""
    rs = np.random.RandomState(11)
    x, mask = rs.rand(2, 5, 16, 16).astype(np.float32), rs.rand(24, 40).astype(np.float32)
    got, _ = run(device, x, mask, [(-5, 10 ** 6), (10 ** 6, -1)], 2)
    assert same_floats(got, numpy_batch(x, mask, [(0, 24), (8, 0)], 2))
    assert same_floats(tensor_form(device, x, mask, [(-5, 10 ** 6), (10 ** 6, -1)], 2), got), "the tensor form clamps alike"
    got, _ = run(device, x, mask, None, 2)
    assert same_floats(got, numpy_batch(x, mask, [(0, 0), (0, 0)], 2))


def check_nan_and_zero(device):
    """one NaN element makes exactly that sample all NaN, an all-zero sample (a constant measurement) is all NaN, the other samples of
    the batch are unaffected; +-inf follow IEEE arithmetic as numpy's"""
    rs = np.random.RandomState(13)
    base, mask = rs.rand(3, 5, 16, 16).astype(np.float32), np.ones((16, 16), dtype=np.float32)
    org = [(0, 0)] * 3
    clean = check_one(device, base, mask, org, 2, [1, 2, 3], False, "clean")
    for where in ((1, 0, 0, 0), (1, 4, 15, 15), (1, 2, 7, 9)):
        x = base.copy()
        x[where] = np.nan
        got = check_one(device, x, mask, org, 2, [1, 2, 3], False, "NaN at %s" % (where,))
        assert np.isnan(got[1]).all(), "a NaN anywhere in the measurement makes the whole sample NaN"
        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2]), "and only that sample"
    x = base.copy()
    x[2] = 0.0
    got = check_one(device, x, mask, org, 2, [1, 2, 3], False, "all-zero sample")
    assert np.isnan(got[2]).all() and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    for v in (np.inf, -np.inf):
        x = base.copy()
        x[0, 1, 3, 3] = v
        got = check_one(device, x, mask, org, 2, None, False, "%s in sample 0" % v)
        assert np.isnan(got[0]).any() and np.isfinite(got[1]).all()


def check_reproducible(device):
    rs = np.random.RandomState(15)
    x, mask = rs.rand(2, 9, 32, 32).astype(np.float32), rs.rand(32, 32).astype(np.float32)
    one, two = run(device, x, mask, None, 2, [5, 6], want_clean_aug=True), run(device, x, mask, None, 2, [5, 6], want_clean_aug=True)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()


def check_refusals(device):
    """every MPHSIR_EINVAL case: nothing is launched (outputs and workspace keep their fill); negative size queries"""
    import mp_hsir_amd._lib as L
    lib = L.load()
    B, C, H, W, MH, MW = 2, 3, 8, 8, 12, 10
    q = lib.mphsir_cassi_workspace_bytes
    need = q(B, C, H, W, 2)
    assert need == 4 * (B * H * (W + (C - 1) * 2) + 2 * B * 2)
    assert q(1, 7, 19, 35, 3) == 4 * ((19 * 53 + 3) // 4 * 4 + 2 * 5)
    for bad in ((0, C, H, W, 2), (B, 0, H, W, 2), (65536, C, H, W, 2), (B, 65536, H, W, 2), (B, C, 0, W, 2), (B, C, H, W, 0), (B, C, H, W, 9),
                (1, 1, 65536, 32768, 1), (1, 65535, 40000, 30000, 8)):
        assert q(*bad) < 0, bad
    x = torch.rand(B, C, H, W).to(device)
    mask = torch.rand(MH, MW).to(device)
    aug = torch.zeros(B, dtype=torch.int32, device=device)
    deg, ca = torch.full((B, C, H, W), -7.0, device=device), torch.full((B, C, H, W), -7.0, device=device)
    ws = torch.full((need // 4 + 4,), -7.0, device=device)
    assert ws.data_ptr() % 16 == 0

    def args(**kw):
        a = L.CassiArgs(clean=x.data_ptr(), mask=mask.data_ptr(), origin=None, task=None, aug=None, degraded=deg.data_ptr(), clean_aug=ca.data_ptr(),
                        workspace=ws.data_ptr(), workspace_bytes=need, B=B, C=C, H=H, W=W, MH=MH, MW=MW, step=2, task_id=0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.mphsir_cassi(ctypes.byref(a), None) == -1
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()
        if device == "cuda":
            torch.cuda.synchronize()
        for t in (deg, ca, ws):
            assert float(t.min()) == -7.0 == float(t.max()), "something was launched"

    refused(args(struct_size=ctypes.sizeof(L.CassiArgs) - 8), "struct_size")
    refused(args(MH=H - 1), "does not hold")
    refused(args(MW=W - 1), "does not hold")
    refused(args(step=0), "step")
    refused(args(step=9), "step")
    refused(args(H=6, MH=12, aug=aug.data_ptr()), "not square")
    refused(args(workspace_bytes=need - 1), "workspace")
    refused(args(workspace=ws.data_ptr() + 4), "workspace")
    refused(args(degraded=x.data_ptr()), "distinct")
    refused(args(clean_aug=x.data_ptr()), "distinct")
    refused(args(B=65536), "bad sizes")
    refused(args(C=65536), "bad sizes")
    refused(args(B=0), "bad sizes")
    refused(args(mask=None), "null pointer")
    refused(args(degraded=None), "null pointer")
    assert lib.mphsir_cassi(ctypes.byref(args()), None) == 0
    if device == "cuda":
        torch.cuda.synchronize()
    assert same_floats(deg.cpu().numpy(), numpy_batch(x.cpu().numpy(), mask.cpu().numpy(), [(0, 0)] * B, 2)) and torch.equal(ca, x)
    assert lib.mphsir_kernel_name(37) == b"cassi_measure" and lib.mphsir_kernel_name(38) == b"cassi_emit"


# ---- the synthesiser, the source, test.py ------------------------------------------------------------------------------------------------
def check_synthesizer(device, menu, N, B=8, C=5):
    """DegradationSynthesizer(fused=True) on a menu with cassi: the cassi samples equal augment(cassi_measure(clean[b], ...), mode[b])
    rebuilt from the plan's own tables, the others are bitwise what the degradation launch alone gives with that plan; clean_aug is
    augment(clean); the prompt is the task id.  Two synthesisers of one seed draw the same plan: one shows it, the other is called."""
    from mp_hsir_amd import degrade as D, ops
    ci = menu.index("cassi")
    for seed in range(5, 10):
        shown, used = (D.DegradationSynthesizer("natural_scene", menu, device, seed=seed, fused=True) for _ in range(2))
        clean = torch.rand((B, C, N, N), generator=torch.Generator().manual_seed(seed)).to(device)
        plan, de_id = shown.fused_plan(clean)
        mine = (de_id == ci).cpu()
        if bool(mine.any()) and (len(menu) == 1 or not bool(mine.all())):
            break
    else:
        raise AssertionError("no seed in 5..9 gives a batch with cassi samples beside others")
    degraded, clean_aug, prompt = used(clean)
    assert torch.equal(prompt, de_id.reshape(B, 1)) and prompt.dtype == torch.int64
    mode = plan.aug.long()
    assert torch.equal(clean_aug, D.augment(clean, mode))
    assert plan.cassi_origin.shape == (B, 2) and plan.cassi_origin.dtype == torch.int32
    want = D.augment(D.cassi_measure(clean, used.cassi_mask.mask, plan.cassi_origin, 2), mode)
    want_np = numpy_batch(clean.cpu().numpy(), used.cassi_mask.mask.cpu().numpy(), plan.cassi_origin.cpu().numpy(), 2)
    want_np = D.augment(torch.from_numpy(want_np), mode.cpu()).numpy()
    assert used.cassi_mask.shape == (256, 256) and set(np.unique(used.cassi_mask.mask.cpu().numpy())) == {0.0, 1.0}
    if len(menu) > 1:
        fn = ops.degrade_batch if N * N <= 128 * 128 else ops.degrade_planes
        others, _ = fn(clean, plan, seed=shown.seed, ordinal=0)
    for b in range(B):
        if bool(mine[b]):
            assert same_floats(degraded[b].cpu().numpy(), want[b].cpu().numpy()), "cassi sample %d differs from the tensor form" % b
            assert same_floats(degraded[b].cpu().numpy(), want_np[b]), "cassi sample %d differs from numpy" % b
        else:
            assert degraded[b].cpu().numpy().tobytes() == others[b].cpu().numpy().tobytes(), "sample %d (task %d) was changed" % (b, int(de_id[b]))
    # the tensor path of the synthesiser accepts the menu too
    y, c, p = D.DegradationSynthesizer("natural_scene", menu, device, seed=3)(clean)
    assert y.shape == c.shape == clean.shape and bool(torch.isfinite(y).all()) and int(p.max()) < len(menu)


def check_source(device):
    from mp_hsir_amd.data import SyntheticPatchSource
    src = SyntheticPatchSource(5, 64, 4, 1, device, de_types=["cassi"], fused_degrade=True)
    for _ in range(2):
        (names, ids), degraded, clean, prompt = src.next()
        assert degraded.shape == clean.shape == (4, 5, 64, 64) and prompt.shape == (4, 1)
        assert int(prompt.abs().max()) == 0 and bool(torch.isfinite(degraded).all()) and bool(torch.isfinite(clean).all())
        assert float(degraded.min()) == 0.0 and float(degraded.max()) == 1.0


def test_py_options(argv=()):
    import importlib
    T = importlib.import_module("mp_hsir_amd.test")
    return T, T.build_parser().parse_args(list(argv))


def check_test_py_mode_13(device):
    """test.py's mode 13 on a 1 x 7 x 72 x 136 cube: the tensor form (--fused_degrade 0, degrade_for_mode) and the launch pair
    (--fused_degrade 1, SceneDegrader) give equal outputs and prompt id 0; the default mask covers the cube; a small mask file ends the run"""
    from mp_hsir_amd import degrade as D
    T, o = test_py_options(["--mode", "13", "--seed", "77"])
    clean = torch.rand((1, 7, 72, 136), generator=torch.Generator().manual_seed(1)).to(device)
    a, pa = T.degrade_for_mode(o, clean, D.Draws(device, o.seed + 1), o.model)
    b, pb = D.SceneDegrader(o.model, device, o.seed + 1)(clean, 13, o)
    assert pa == pb == 0 and a.shape == b.shape == clean.shape
    assert same_floats(b.cpu().numpy(), a.cpu().numpy())
    assert float(a.min()) == 0.0 and float(a.max()) == 1.0
    assert D.scene_cassi_mask(o, torch.device(device), 72, 136).shape == (256, 256)
    assert D.scene_cassi_mask(o, torch.device(device), 300, 136).shape == (300, 256)
    return T, o


def check_launch_list(device):
    """ops.ACCOUNT of one fused synthesiser call: a menu without cassi issues the degradation launch alone (what it issued before the
    cassi task existed), a mixed menu that launch and the cassi pair, the fine-tune menu the pair alone"""
    from mp_hsir_amd import degrade as D, ops
    clean = torch.rand((4, 5, 32, 32), generator=torch.Generator().manual_seed(1)).to(device)
    want = {("gaussianN", "inpaint", "bandmiss"): {"degrade": 1}, ("gaussianN", "cassi"): {"degrade": 1, "cassi": 1}, ("cassi",): {"cassi": 1}}
    for menu, launches in want.items():
        syn = D.DegradationSynthesizer("natural_scene", list(menu), device, seed=3, fused=True)
        assert (syn.cassi_mask is None) == ("cassi" not in menu)
        ops.ACCOUNT = {}
        try:
            syn(clean)
            got = {k: v[0] for k, v in ops.ACCOUNT.items()}
        finally:
            ops.ACCOUNT = None
        assert got == launches, (menu, got)
