"""Checks of the window-attention backward that forms the total d_sa itself (ops.win_attn_bwd branch=..., attribute
ops.BRANCH_BWD_FUSED), shared by the CPU-emulator tests (tests/test_branch_bwd_emu.py) and the MI355X tests
(tests/test_branch_bwd_gpu.py).  Each kernel check is one tiny launch; the whole-block runs are computed once per
(case, shift, switch) and shared by the accuracy and the determinism tests."""
import torch

import kernel_checks as K
from guard import guarded
from kernel_checks import GTOL, TOL, _ROUNDED, _use, close, inp, rel_l2, rnd
from oracle import mp_hsir_oracle as O

PROLOGUE_CASES = [(64, 2), (128, 4), (128, 2), (256, 8)]
BLOCK_NAMES = ["nat_enc1", "nat_enc2", "nat_latent"]
# gradients that lie behind the changed launches: the guard against a gross error hiding under the wide 16-bit bar
GUARDED = ("dx", "norm1.", "attn.qkv.", "attn.proj.", "local_spectral_attn.")


class branch_bwd_fused:
    """`with branch_bwd_fused(on):` runs the attention backward with the attribute ops.BRANCH_BWD_FUSED at `on`.  The capability
    predicate (ops.win_attn_bwd_dsa_fits) is the production one; the tuning rule (ops.win_attn_bwd_dsa_pays: only where one workgroup
    owns a window, i.e. from 512 windows on) is told to take the path at the 8 windows of the whole-block shape too."""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        from mp_hsir_amd import ops
        self.prev = (ops.BRANCH_BWD_FUSED, ops.BRANCH_BWD_SPLIT_HEADS_TOO)
        ops.BRANCH_BWD_FUSED, ops.BRANCH_BWD_SPLIT_HEADS_TOO = self.on, True

    def __exit__(self, *exc):
        from mp_hsir_amd import ops
        ops.BRANCH_BWD_FUSED, ops.BRANCH_BWD_SPLIT_HEADS_TOO = self.prev
        return False


def _to_window_rows(img, shift):
    """(B,H,W,C) image order -> (M,C) in the window-token order of win_attn_bwd's outputs"""
    if shift:
        img = torch.roll(img, (-shift, -shift), (1, 2))
    return O.to_windows(img).reshape(-1, img.shape[-1])


def _from_window_rows(rows, B, H, W, shift):
    img = O.from_windows(rows.reshape(-1, 64, rows.shape[-1]), B, H, W)
    return torch.roll(img, (shift, shift), (1, 2)) if shift else img


def _prologue_inputs(dtype, C, heads, shape):
    B, H, W = shape
    M = B * H * W
    t = dict(x=rnd((B, H, W, C), 71, dtype), dmu=rnd((M // 64, C), 73),
             lnw=rnd((C,), 74, scale=0.1, shift=1), lnb=rnd((C,), 75, scale=0.1),
             wqkv=rnd((3 * C, C), 76, dtype, scale=C ** -0.5), bqkv=rnd((3 * C,), 77, scale=0.1),
             rpb=rnd((225, heads), 78, scale=0.2), wprojT=rnd((C, C), 79, dtype, scale=C ** -0.5),
             dt3=rnd((M, 3 * C), 81, dtype), wsT=rnd((C, 3 * C), 82, dtype, scale=(3 * C) ** -0.5),
             d_out=rnd((B, H, W, C), 83, dtype), sa=rnd((B, H, W, C), 84, dtype), gate=rnd((M // 64, C), 85))
    return t


@guarded
def check_dsa_prologue(dev, dtype, C, heads, shift, shape=(2, 16, 16)):
    """win_attn_bwd with dT3 / WsT / dOut / gate: dSAt against the fp64 definition
        total = dT3[pix] WsT^T + d_out[pix] * gate[win] + dmu[win] / 64
    within TOL[dtype] and not above the error of the three launches it replaces (combine_bwd -> gemm_tok epi 1 -> the plain
    prologue: three roundings where this has one); the other outputs are exactly what the plain kernel returns for the
    same (rounded) total d_sa -- nothing behind the prologue changed; head_split leaves every output bitwise unchanged."""
    _use(dev)
    from mp_hsir_amd import ops
    B, H, W = shape
    M = B * H * W
    t = _prologue_inputs(dtype, C, heads, shape)
    assert ops.win_attn_bwd_dsa_fits(C, heads, dtype)
    tail = (t["lnw"], t["lnb"], t["wqkv"], t["bqkv"], t["rpb"], t["wprojT"], heads, shift)
    branch = dict(dt3=t["dt3"], wsT=t["wsT"], d_out=t["d_out"].reshape(M, C), gate=t["gate"])
    dqkv, xnw, dsat, drpb = ops.win_attn_bwd(t["x"], None, t["dmu"], *tail, branch=branch)
    # fp64 definition, window-token order
    gimg = _from_window_rows(t["gate"].double().cpu()[:, None, :].expand(-1, 64, -1).reshape(M, C), B, H, W, shift)
    img = (t["dt3"].double().cpu() @ t["wsT"].double().cpu().t()).reshape(B, H, W, C) + t["d_out"].double().cpu() * gimg
    want = _to_window_rows(img, shift) + (t["dmu"].double().cpu() / 64.0)[:, None, :].expand(-1, 64, -1).reshape(M, C)
    # (both sides back in image order: the same permutation of the rows, so the whole-tensor value is what it was, and the slices are
    # image rows, image columns and samples)
    e_fused = close(_from_window_rows(dsat.reshape(M, C).double().cpu(), B, H, W, shift), _from_window_rows(want, B, H, W, shift), TOL[dtype],
                    geom=(B, H, W), what="dSAt")
    # the three launches it replaces (keep = None: combine_bwd's d_out is its dy, the same d_out as above)
    _, d_sa, _ = ops.combine_bwd(t["d_out"], t["sa"], t["gate"], None, shift)
    d_sa = ops.gemm_tok(t["dt3"], t["wsT"], epi=1, res=d_sa.reshape(M, C)).reshape(B, H, W, C)
    _, _, dsat3, _ = ops.win_attn_bwd(t["x"], d_sa, t["dmu"], *tail)
    e_three = rel_l2(_from_window_rows(dsat3.reshape(M, C).double().cpu(), B, H, W, shift), _from_window_rows(want, B, H, W, shift))
    print("dSAt rel-L2 vs fp64: fused %.3e, three launches %.3e (C=%d heads=%d shift=%d %s)" % (e_fused, e_three, C, heads, shift, dtype))
    assert e_fused <= e_three, (e_fused, e_three)
    # everything behind the prologue: the plain kernel fed the same rounded total (dmu = 0 adds nothing) returns the same bits
    same = inp(_from_window_rows(dsat.reshape(M, C).cpu(), B, H, W, shift).contiguous())
    ref = ops.win_attn_bwd(t["x"], same, K.alloc(t["dmu"].shape, role="input"), *tail)
    for name, a, b in zip(("dqkv", "XNw", "dSAt", "drpb"), (dqkv, xnw, dsat, drpb), ref):
        assert torch.equal(a.cpu(), b.cpu()), (name, rel_l2(a.float(), b.double().cpu()))
    if heads == 8:
        one = ops.win_attn_bwd(t["x"], None, t["dmu"], *tail, head_split=1, branch=branch)
        for hs in (2, 8):
            out = ops.win_attn_bwd(t["x"], None, t["dmu"], *tail, head_split=hs, branch=branch)
            assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(out, one)), hs
        assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip((dqkv, xnw, dsat, drpb), one))


@guarded
def check_dsa_fits(dev):
    """the predicate: natural widths in the 16-bit types with the switch on; everything else keeps the launches"""
    _use(dev)
    from mp_hsir_amd import ops
    for dt in (torch.bfloat16, torch.float16):
        assert all(ops.win_attn_bwd_dsa_fits(C, h, dt) for C, h in PROLOGUE_CASES)
        assert not any(ops.win_attn_bwd_dsa_fits(C, h, dt) for C, h in ((96, 2), (192, 4), (384, 8), (32, 1)))
    assert not ops.win_attn_bwd_dsa_fits(128, 4, torch.float32)
    # the host takes the path where one workgroup owns a window: the benchmark's level 2 (512 windows) does, its latent level (128
    # windows, heads dealt to four workgroups) keeps its launches
    assert ops.win_attn_bwd_dsa_pays(32, 32, 32, 4) and not ops.win_attn_bwd_dsa_pays(32, 16, 16, 8)
    assert ops.win_attn_bwd_dsa_pays(2, 16, 16, 1)       # a single head is never dealt out
    with branch_bwd_fused(False):
        assert not ops.win_attn_bwd_dsa_fits(128, 4, torch.bfloat16)


# ---- whole block: the procedure of kernel_checks.check_pgsstb_backward_oracle, with the switch either way ---------------------
_RUNS = {}
_ORACLE = {}
_YARD = {}
# the block backward under input profiles (kernel_checks.INPUT_PROFILES): win_attn_bwd has its own copy of the LayerNorm epsilon and
# recomputes the softmax, and stands against fp64 autograd only inside the whole block.  `flat` acts on the x draw, `peaked` on the q and k
# rows of attn.qkv.weight (x 4: logits x 16), `saturated` x 8 (logits past the 88.7 where exp overflows fp32: see kernel_checks).
# (block, B, (H, W)): one window, and run_block's own shape
PROFILE_SHAPES = [(1, (8, 8)), (2, (16, 16))]
PROFILES = ("flat", "peaked", "saturated")
# (`saturated` at one window: torch's own bf16 autograd is 0.081 from fp64 for d attn.qkv.weight, the cap allows 0.080: not a test; at (2, 16, 16): 0.069)
PROFILE_CASES = [(B, hw, p) for B, hw in PROFILE_SHAPES for p in PROFILES if not (p == "saturated" and B == 1)]
_QK_FACTOR = {"peaked": 4.0, "saturated": 8.0}
# what win_attn_bwd itself produces or feeds directly: these must stay under the yardstick cap in every profile case, or the case fails
# (`saturated`: torch's own bf16 autograd misses the bias-table gradient by 0.10-0.13 at logits of +-95, over the cap: not required there)
_REQ = ("out", "dx", "attn.qkv.weight", "attn.qkv.bias")
PROFILE_REQUIRED = {"unit": (), "flat": _REQ + ("attn.relative_position_bias_table",), "peaked": _REQ + ("attn.relative_position_bias_table",), "saturated": _REQ}


def _block(dev, name, shift, inputs="unit"):
    from golden.cases import BLOCK_CASES
    from golden.detfill import det_value
    from mp_hsir_amd.net.MP_HSIR import PGSSTB
    c = BLOCK_CASES[name]
    blk = PGSSTB(c["C"], c["heads"], [64, 64], 8, shift, 0.0, 2.66, c["cr"], 128).eval()
    with torch.no_grad():
        for k, p in blk.named_parameters():
            p.copy_(det_value(k, p.shape).float())
            if k == "attn.qkv.weight" and inputs in _QK_FACTOR:
                p[:2 * c["C"]] *= _QK_FACTOR[inputs]
    return blk.to(dev), c


@guarded
def run_block(dev, dtype, name, shift, fused, B=2, hw=(16, 16), inputs="unit"):
    """one forward + backward of the block on `dev`: {"out", "dx", parameter name: gradient} (CPU tensors) and the launch counts"""
    _use(dev)
    from mp_hsir_amd import autograd_ops as AG
    from mp_hsir_amd import ops
    H, W = hw
    blk, c = _block(dev, name, shift, inputs)
    x = rnd((B, H, W, c["C"]), 301, dtype, profile=K.row_profile(inputs)).requires_grad_(True)
    cot = rnd((B, H, W, c["C"]), 302, dtype)
    k1 = inp(torch.tensor([1.0 / 0.9, 0.0][:B]))
    k2 = inp(torch.tensor([0.0, 1.0 / 0.95][:B]))
    ops.ACCOUNT = {}
    with branch_bwd_fused(fused):
        y = AG.pgsstb(blk, x, k1, k2)
        (y.float() * cot.float()).sum().backward()
    acct, ops.ACCOUNT = ops.ACCOUNT, None
    got = {"out": y.detach().float().cpu(), "dx": x.grad.float().cpu()}
    for k, p in blk.named_parameters():
        got[k] = p.grad.float().cpu()
    return got, {k: v[0] for k, v in acct.items()}


def block_run_cached(dev, dtype, name, shift, fused, B=2, hw=(16, 16), inputs="unit"):
    key = (dev, dtype, name, shift, bool(fused), B, hw, inputs)
    if key not in _RUNS:
        _RUNS[key] = run_block(dev, dtype, name, shift, fused, B=B, hw=hw, inputs=inputs)
    return _RUNS[key]


def block_oracle(dtype, name, shift, B=2, hw=(16, 16), inputs="unit"):
    """fp64 autograd of the oracle on the weights as the kernels see them (GEMM weights rounded to dtype), DropPath factors on.  Under an
    input profile also the yardstick (_YARD): autograd of the same oracle with every operand and op result in the compute dtype"""
    key = (dtype, name, shift, B, hw, inputs)
    if key in _ORACLE:
        return _ORACLE[key]
    prev = K._DEV[0]
    _use("cpu")
    H, W = hw
    blk, c = _block("cpu", name, shift, inputs)
    P = {}
    for k, p in blk.named_parameters():
        v = p.detach()
        if k in _ROUNDED:
            v = v.to(dtype)
        P[k] = v.double().requires_grad_(True)
    x0 = rnd((B, H, W, c["C"]), 301, dtype, profile=K.row_profile(inputs))
    xd = x0.double().requires_grad_(True)
    cot = rnd((B, H, W, c["C"]), 302, dtype).double()
    _use(prev)
    k1 = torch.tensor([1.0 / 0.9, 0.0][:B]).double()
    k2 = torch.tensor([0.0, 1.0 / 0.95][:B]).double()
    yr = O.pgsstb(P, "", xd, c["heads"], shifted=shift > 0, keep=(k1, k2))
    (yr * cot).sum().backward()
    want = {"out": yr.detach(), "dx": xd.grad}
    for k in P:
        want[k] = P[k].grad
    _ORACLE[key] = want
    if inputs != "unit":
        Pc = {k: v.detach().to(dtype).requires_grad_(True) for k, v in P.items()}
        xc = x0.detach().clone().requires_grad_(True)
        yc = O.pgsstb(Pc, "", xc, c["heads"], shifted=shift > 0, keep=(k1.to(dtype), k2.to(dtype)))
        (yc * cot.to(dtype)).sum().backward()
        _YARD[key] = dict({k: Pc[k].grad for k in Pc}, out=yc.detach(), dx=xc.grad)
    return want


@guarded
def check_block(dev, dtype, name, shift, B=2, hw=(16, 16), inputs="unit"):
    """every gradient of the block within GTOL of fp64 autograd with the switch on and off; behind the changed launches the fused
    error is at most the unfused error + 0.1 GTOL; the fused run launches no gemm_tok for the spectral qkv data gradient.  Under an input
    profile the bar of every tensor is kernel_checks.yard_bar's: max(that tolerance, 3 x the oracle's own error in the compute dtype)"""
    want = block_oracle(dtype, name, shift, B, hw, inputs)
    own = _YARD.get((dtype, name, shift, B, hw, inputs))
    errs = {}
    for fused in (True, False):
        got, acct = block_run_cached(dev, dtype, name, shift, fused, B, hw, inputs)
        errs[fused] = {k: rel_l2(got[k], want[k]) for k in want}
        for k in want:          # per tensor: no sample, image row, image column or channel of it stands out
            bar = K.yard_bar(inputs, dtype, TOL[dtype] * 2 if k == "out" else GTOL[dtype], k, want[k], lambda cast, k=k: own[k], required=k in PROFILE_REQUIRED[inputs])
            if bar is None:          # a small gradient that torch's own 16-bit autograd misses by more than the cap (printed): not a test of the kernel
                continue
            assert errs[fused][k] < bar, (name, shift, "fused" if fused else "unfused", k, errs[fused][k], bar)
            close(got[k], want[k], bar, geom=(B,) + tuple(hw), what=k, whole=errs[fused][k])
        errs[fused]["_acct"] = acct
    a1, a0 = errs[True].pop("_acct"), errs[False].pop("_acct")
    assert a1.get("gemm_tok", 0) == a0.get("gemm_tok", 0) - 1, (a1.get("gemm_tok"), a0.get("gemm_tok"))
    assert a1["win_attn_bwd"] == a0["win_attn_bwd"] == 1
    for k in want:
        if k == "dx" or any(k.startswith(g) for g in GUARDED):
            print("%s shift=%d %-44s fused %.3e  unfused %.3e" % (name, shift, k, errs[True][k], errs[False][k]))
            assert errs[True][k] <= errs[False][k] + 0.1 * GTOL[dtype], (name, shift, k, errs[True][k], errs[False][k])
    return errs


@guarded
def check_block_deterministic(dev, dtype, name, shift):
    """two runs with the switch on return the same bits"""
    first, _ = block_run_cached(dev, dtype, name, shift, True)
    again, _ = run_block(dev, dtype, name, shift, True)
    for k in first:
        assert torch.equal(first[k], again[k]), (name, shift, k)
