"""Adversarial wave schedules on the CPU emulator (tests/hipemu/include/hip/hip_runtime.h, hipemu_set_schedule).

The library has no atomics and no summation order that depends on scheduling, so a kernel that orders its LDS traffic with barriers
gives the same BITS under every legal schedule; a missing or misplaced barrier, a ring slot reused too early, a read of LDS nobody
wrote, or a dependence on an earlier block of the same launch gives different bits under some schedule.  Every case runs a parity
check once under the default schedule with the recorder of tests/guard.py on, then again under each adversarial schedule, and every
recorded tensor (what the check compared, and every buffer ops.py allocated for a kernel to write) must hold the same bits.  The
check's own assertions run every time.  tests/hipemu/selftest.hip holds kernels with planted faults: proof that each schedule finds
the fault it is there for, and that the correct twins pass all of them."""
import collections
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import guard
import kernel_checks as K
from emu import bind_emulator

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mp-hsir_amd", "csrc")
DESC = 0x100                    # HIPEMU_SCHED_DESC_BLOCKS
BF, F32 = torch.bfloat16, torch.float32
SEEDS = (0x5EED, 0xC0FFEE)      # the two random schedules of every case
SEED_DESC = 0xB10C              # the random schedule that also walks the blocks backwards
MODE_NAMES = {0: "default", 1: "reversed threads", 2: "reversed waves", 3: "random", 4: "laggard wave", 5: "sprinter wave"}


def _handle(path):
    lib = ctypes.CDLL(path)
    lib.hipemu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_uint64]
    lib.hipemu_set_schedule.restype = None
    lib.hipemu_get_schedule.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
    lib.hipemu_max_waves.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def emu():
    import build_emu
    bind_emulator()
    lib = _handle(build_emu.OUT)
    yield lib
    lib.hipemu_set_schedule(0, 0)


def describe(mode, seed):
    return "%s%s (mode %d%s, seed %d)" % (MODE_NAMES[mode & 0xff], ", descending blocks" if mode & DESC else "", mode & 0xff,
                                          " | 0x100" if mode & DESC else "", seed)


def schedules(waves):
    """modes 1, 2 and 3 with two seeds, modes 4 and 5 once per wave of the widest workgroup, descending blocks with mode 3.  Cut for
    time: a workgroup of more than eight waves (the 1024-thread spectral kernels) gets the laggard and the sprinter at its
    first two waves, its middle wave and its last wave only -- the waves that can have a role of their own (a loader, a reducer)"""
    special = range(waves) if waves <= 8 else (0, 1, waves // 2, waves - 1)
    out = [(1, 0), (2, 0)] + [(3, s) for s in SEEDS]
    out += [(4, w) for w in special] + [(5, w) for w in special]
    return out + [(3 | DESC, SEED_DESC)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# (id, family, accounts, run): `accounts` are the ops.ACCOUNT names the run must reach (what ties a case to a source file below); ()
# where the check keeps the account itself
def _manifest():
    with open(os.path.join(HERE, "golden", "state_dict_manifest.json")) as f:
        return json.load(f)


def _k(name, *a, **kw):
    return lambda: getattr(K, name)("cpu", *a, **kw)


def _tn(form, name, *a, **kw):
    def run():
        with K.tn_form(form):
            getattr(K, name)("cpu", *a, **kw)
    return run


def _win(i):
    return lambda: K.check_win_attn("cpu", BF, *K.WIN_CASES[i], _manifest())


def _win32(i):
    return lambda: K.check_win_attn("cpu", F32, *K.WIN_CASES[i], _manifest())


def _block(fused):
    def run():          # run_block itself: check_block keeps the runs of a process in a cache, so a second call would launch nothing
        import branch_bwd_checks as BB
        got, launches = BB.run_block("cpu", BF, BB.BLOCK_NAMES[0], 4, fused, B=1, hw=(8, 16))
        assert launches["win_attn_bwd"] == 1 and launches["gated_mlp_bwd"] == 1, launches
        for k in sorted(got):
            assert torch.isfinite(got[k]).all(), k
            guard.record(got[k], "block " + k)
    return run


def _prologue():
    import branch_bwd_checks as BB
    BB.check_dsa_prologue("cpu", BF, 64, 2, 4, shape=(1, 8, 16))


_RING = [(256, 64, 64, 0, 0, None, None), (512, 96, 96, 1, 0, 128, 104), (1024, 208, 160, 0, 4, None, 256)]      # test_emu_kernels.test_gemm_tok_ring
_MLP = K.MLP_CASES[0]

KERNEL_CASES = [
    ("gemm_tok-bf16", "gemm_tok", ("gemm_tok",), _k("check_gemm_tok", BF, *K.GEMM_CASES[0])),
    ("gemm_tok-fp32", "gemm_tok", ("gemm_tok",), _k("check_gemm_tok", F32, *K.GEMM_CASES[0])),
    ("gemm_tok-ln-epi1", "gemm_tok", ("gemm_tok",), _k("check_gemm_tok", BF, *K.GEMM_CASES[3])),
    ("gemm_tok_ring-0", "gemm_tok", ("gemm_tok",), _k("check_gemm_tok_ring", BF, *_RING[0])),
    ("gemm_tok_ring-1", "gemm_tok", ("gemm_tok",), _k("check_gemm_tok_ring", BF, *_RING[1])),
    ("gemm_tok_ring-2", "gemm_tok", ("gemm_tok",), _k("check_gemm_tok_ring", BF, *_RING[2])),
    ("gated_mlp-tpw0", "gated_mlp", ("gated_mlp",), _k("check_gated_mlp", BF, *_MLP)),
    ("gated_mlp-tpw2", "gated_mlp", ("gated_mlp",), _k("check_gated_mlp", BF, *_MLP, tpw=2, M=256)),
    ("gated_mlp-tpw3", "gated_mlp", ("gated_mlp",), _k("check_gated_mlp", BF, *_MLP, tpw=3, M=256)),
    ("gated_mlp-hsplit2", "gated_mlp", ("gated_mlp",), _k("check_gated_mlp", BF, 96, 255, M=256, hsplit=2)),
    ("gated_mlp-fp32", "gated_mlp", ("gated_mlp",), _k("check_gated_mlp", F32, *_MLP)),
    ("win_attn-shifted", "win_attn", ("win_attn",), _win(0)),
    ("win_attn-unshifted", "win_attn", ("win_attn",), _win(2)),
    ("win_attn-fp32", "win_attn", ("win_attn",), _win32(0)),
    ("spectral_chain", "spectral", ("dwconv_gram", "spectral_fold"), _k("check_spectral_attention_chain", BF, *K.SPEC_CASES[0])),
    ("spectral_chain-fp32", "spectral", ("dwconv_gram", "spectral_fold"), _k("check_spectral_attention_chain", F32, *K.SPEC_CASES[0])),
    ("fused_pass_a", "spectral_fused", ("qkv_dwconv_gram",), _k("check_fused_pass_a", BF, *K.FUSED_CASES[0])),
    ("fused_pass_a-head_groups", "spectral_fused", ("qkv_dwconv_gram",), _k("check_fused_pass_a", BF, *K.FUSED_HG_CASES[0][:5], hgroups=K.FUSED_HG_CASES[0][5])),
    ("fused_pass_a-rows", "spectral_rows", ("qkv_dwconv_gram",), _k("check_fused_pass_a", BF, *K.ROWS_CASES[0][:3], None, K.ROWS_CASES[0][4], row_segments=K.ROWS_CASES[0][3])),
    ("gdfn_fused", "gdfn_fused", ("gdfn_fused",), _k("check_gdfn_fused", BF, *K.GDFN_FUSED_CASES[0])),
    ("dwconv_plain-lds_tile", "dwconv", ("dwconv3x3",), _k("check_dwconv_plain", BF, (1, 8, 16, 32))),
    ("dwconv_bwd", "dwconv", ("dwconv3x3_bwd",), _k("check_dwconv_bwd", BF, K.DW_BWD_CASES[0])),
    ("dwconv_gate_bwd", "spectral", ("gdfn_gate_bwd",), _k("check_dwconv_gate_bwd", BF, shape=(1, 8, 16), hid=85)),
    ("gdfn_chain", "spectral", ("dwconv_gate",), _k("check_gdfn_chain", BF)),
    ("gemm_tn-form1", "gemm_tn", ("gemm_tn",), _tn(1, "check_gemm_tn", BF, 256, 64, 64, 2, 0)),
    ("gemm_tn-form2", "gemm_tn", ("gemm_tn",), _tn(2, "check_gemm_tn", BF, 256, 64, 64, 2, 0)),
    ("gemm_tn-fp32", "gemm_tn", ("gemm_tn",), _k("check_gemm_tn", F32, 128, 32, 32, 1, 2)),
    ("gemm_tn_grouped-form1", "gemm_tn", (), _tn(1, "check_gemm_tn_grouped")),
    ("gemm_tn_grouped-form2", "gemm_tn", (), _tn(2, "check_gemm_tn_grouped")),
    ("conv3x3-form1", "conv3x3", ("conv3x3_tok",), _tn(1, "check_conv3x3", BF, 1, 8, 8, 31, 32)),
    ("conv3x3-form2", "conv3x3", ("conv3x3_tok",), _tn(2, "check_conv3x3", BF, 1, 8, 8, 31, 32)),
    ("conv3x3-fp32", "conv3x3", ("conv3x3_tok",), _tn(2, "check_conv3x3", F32, 1, 8, 8, 31, 32)),
    ("gated_mlp_bwd-v0", "gated_mlp_bwd", ("gated_mlp_bwd",), _k("check_gated_mlp_bwd", BF, *_MLP)),
    ("gated_mlp_bwd-v1", "gated_mlp_bwd", ("gated_mlp_bwd",), _k("check_gated_mlp_bwd", BF, *_MLP, variant=1)),
    ("gated_mlp_bwd-v2", "gated_mlp_bwd", ("gated_mlp_bwd",), _k("check_gated_mlp_bwd", BF, *_MLP, variant=2)),
    ("gated_mlp_bwd-v3", "gated_mlp_bwd", ("gated_mlp_bwd",), _k("check_gated_mlp_bwd", BF, *_MLP, variant=3)),
    ("gated_mlp_bwd-v4", "gated_mlp_bwd", ("gated_mlp_bwd",), _k("check_gated_mlp_bwd", BF, *_MLP, variant=4)),
    ("gated_mlp_bwd-fp32", "gated_mlp_bwd", ("gated_mlp_bwd",), _k("check_gated_mlp_bwd", F32, *_MLP)),
    ("gated_mlp_wgrad", "gated_mlp_wgrad", ("gated_mlp_wgrad",), _k("check_gated_mlp_wgrad", BF, *_MLP, M=256, nch=1, ranges=8, keep=True)),
    ("pg_gate_fwd", "pg_gate", ("pg_gate",), _k("check_pg_gate_fwd", 128, 8, nW=5)),
    ("pg_gate_bwd", "pg_gate", ("pg_gate_bwd",), _k("check_pg_gate_bwd", 128, 8, nW=5)),
    ("ln_bwd_win_dxn", "ln_bwd_dxn", ("ln_bwd_win",), _k("check_ln_bwd_win_dxn", BF, 64, (1, 8, 16), 4)),
    ("ln_bwd_tok_dxn", "ln_bwd_dxn", (), _k("check_ln_bwd_tok_dxn", BF, 64, 384, 128)),
    ("fold_bwd-split_dm", "small_bwd", ("spectral_fold_bwd",), _k("check_fold_bwd_split_dm", BF, 64, 2, nsp=5)),
    ("fold_bwd-forms_dm", "small_bwd", ("spectral_fold_bwd",), _k("check_fold_bwd_forms_dm", BF, 64, 2, B=2, N=256)),
    ("spectral_dqkv_bwd", "spectral_bwd", ("spectral_dqkv_bwd",), _k("check_spectral_dqkv_bwd", BF, 32, 1, (2, 8, 16))),
    ("combine_bwd", "block_bwd", ("combine_bwd",), _k("check_combine_bwd", BF, 32, 4, (1, 8, 16))),
    ("win_attn_bwd-dsa_prologue", "block_bwd", ("win_attn_bwd",), _prologue),
    ("block_backward-fused", "block_bwd", (), _block(True)),
    ("block_backward-unfused", "block_bwd", (), _block(False)),
    ("reduce_parts", "arena", ("reduce_parts",), _k("check_reduce_parts")),
    ("reduce_block", "arena", ("reduce_parts",), _k("check_reduce_block")),
    ("l1_clamp_loss", "arena", ("l1_clamp_loss",), _k("check_l1_clamp_loss")),
    ("heads", "heads", ("layout",), _k("check_heads", BF, B=1, C=40, H=9, W=7, T=7, n=1)),
]


# ---- the data-side kernels: their checks call ops.* and compare in numpy; the outputs are recorded where ops hands them back -----
DATA_OPS = ("quality_bands", "quality_meter", "scene_blend_tiles", "scene_gather_tiles", "scene_gather_d4", "scene_fold_d4", "cassi",
            "spectral_loss", "spectral_loss_grad", "grad_norm", "flat_adamw_ex", "patch_sample", "degrade_batch", "degrade_planes")


def _tensors(x, out):
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif isinstance(x, (tuple, list)):
        for v in x:
            _tensors(v, out)
    elif isinstance(x, dict):
        for v in x.values():
            _tensors(v, out)
    return out


class recorded_ops:
    """while active, every call of the ops functions in DATA_OPS records its tensor arguments (the in-place outputs among them) and
    results after the call"""

    def __enter__(self):
        from mp_hsir_amd import ops
        self.ops, self.saved = ops, {n: getattr(ops, n) for n in DATA_OPS}
        for name, fn in self.saved.items():
            def wrapped(*a, _fn=fn, _name=name, **kw):
                res = _fn(*a, **kw)
                for t in _tensors([a, kw, res], []):
                    guard.record(t, "ops." + _name)
                return res
            setattr(ops, name, wrapped)

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)
        return False


def _quality():
    import quality_ref as Q
    from mp_hsir_amd import ops
    r, c = Q.smooth_pair(2, 5, 33, 45, seed=2)                      # H, W no multiples of the 32 x 32 block: four blocks a band
    p, s, a, n = ops.quality_bands(torch.from_numpy(r), torch.from_numpy(c))
    mse, psnr, ssim = Q.bands(r, c)
    assert np.abs(s.numpy() - ssim).max() <= Q.tol(33, 45)


def _scene_blend():
    import scene_ref as R
    from mp_hsir_amd import ops
    H, W, T, ov = R.SMALL_SHAPES[0]
    th, tw, oy, ox = R.plan_tiles(H, W, T, ov)
    tiles = torch.from_numpy(np.random.default_rng(2).random((len(oy) * len(ox), 5, th, tw), dtype=np.float32))
    got = ops.scene_blend_tiles(tiles, torch.tensor(oy, dtype=torch.int32), torch.tensor(ox, dtype=torch.int32), ov, H, W)
    want, _ = R.blend(tiles.numpy(), oy, ox, ov, H, W)
    assert np.abs(got.numpy().astype(np.float64) - want).max() <= R.BLEND_TOL


def _d4_fold():
    import ensemble_ref as E
    from mp_hsir_amd import ops
    n, C, th = 2, 5, 36
    G = len(E.MODES8)
    y = torch.from_numpy(np.random.default_rng(3).random((G * n, C, th, th), dtype=np.float32))
    store = torch.full((n, C, th, th), float("nan"))
    for j0 in range(0, G * n, 3):                                   # batches of three: a tile's passes arrive in several calls
        cnt = min(3, G * n - j0)
        ops.scene_fold_d4(y[j0:j0 + cnt].contiguous(), store, j0, cnt, E.MODES8)
    assert torch.isfinite(store).all()


def _ref(module, name, *a, **kw):
    def run():
        getattr(__import__(module), name)("cpu", *a, **kw)
    return run


DATA_CASES = [
    ("quality", "quality", ("quality",), _quality),
    ("quality_meter", "quality_meter", ("quality_meter",), _ref("quality_meter_ref", "check_values", 5, 31, "random")),
    ("scene_blend", "scene", ("scene",), _scene_blend),
    ("scene_d4_fold", "scene_d4", ("scene",), _d4_fold),
    ("cassi", "cassi", ("cassi",), _ref("cassi_ref", "check_non_square")),
    ("spectral_loss", "spectral_loss", ("spectral_loss",), _ref("spectral_loss_ref", "check_values", (3, 8, 5, 7))),
    ("optim_grad_norm", "optim", ("grad_norm",), _ref("optim_ex_ref", "check_norm", 1028)),
    ("patch_minmax", "patch_sample", ("patch_sample",), _ref("patch_sample_ref", "check_alignment")),
    ("degrade_batch", "degrade", ("degrade",), _ref("degrade_fused_ref", "check_small_planes", shapes=((2, 3, 20),))),
    ("degrade_planes", "degrade", ("degrade",), _ref("degrade_planes_ref", "check_against_the_tensor_functions", (1, 3, 67, 131), False)),
]

CASES = KERNEL_CASES + DATA_CASES

# source file -> the ops.ACCOUNT names of its entry points of which at least one case must reach each, and (for the files whose
# kernels hide behind another file's entry point) the case that selects them.  test_every_lds_source_file_has_a_case keeps it whole.
FILES = {
    "arena.hip": (("reduce_parts", "l1_clamp_loss"), ()),
    "block_bwd.hip": (("combine_bwd", "win_attn_bwd", "ln_bwd_win"), ()),
    "cassi.hip": (("cassi",), ()),
    "conv3x3.hip": (("conv3x3_tok",), ()),
    "degrade.hip": (("degrade",), ("degrade_batch", "degrade_planes")),
    "dwconv.hip": (("dwconv3x3", "dwconv3x3_bwd"), ()),
    "gated_mlp.hip": (("gated_mlp",), ()),
    "gated_mlp_bwd.hip": (("gated_mlp_bwd",), ()),
    "gated_mlp_wgrad.hip": (("gated_mlp_wgrad",), ()),
    "gdfn_fused.hip": (("gdfn_fused",), ()),
    "gemm_tn.hip": (("gemm_tn",), ("gemm_tn-form1", "gemm_tn-form2", "gemm_tn_grouped-form2")),
    "gemm_tok.hip": (("gemm_tok",), ("gemm_tok_ring-0",)),
    "heads.hip": (("layout",), ()),
    "ln_bwd_dxn.hip": (("ln_bwd_win",), ("ln_bwd_win_dxn", "ln_bwd_tok_dxn")),
    "optim.hip": (("grad_norm",), ()),
    "patch_sample.hip": (("patch_sample",), ()),
    "pg_gate.hip": (("pg_gate", "pg_gate_bwd"), ()),
    "quality.hip": (("quality",), ()),
    "quality_meter.hip": (("quality_meter",), ()),
    "scene_d4.hip": (("scene",), ("scene_d4_fold",)),
    "small_bwd.hip": (("spectral_fold_bwd",), ()),
    "spectral.hip": (("dwconv_gram", "spectral_fold", "dwconv_gate"), ("dwconv_gate_bwd",)),
    "spectral_bwd.hip": (("spectral_dqkv_bwd",), ()),
    "spectral_fused.hip": (("qkv_dwconv_gram",), ("fused_pass_a",)),
    "spectral_loss.hip": (("spectral_loss",), ()),
    "spectral_rows.hip": (("qkv_dwconv_gram",), ("fused_pass_a-rows",)),
    "win_attn.hip": (("win_attn",), ()),
}
LDS_USE = re.compile(r"__syncthreads\s*\(|__builtin_amdgcn_s_barrier|__shared__|HIP_DYNAMIC_SHARED")

STATS = collections.OrderedDict()      # family -> [cases, tensors compared per schedule, schedules run, seconds]


def _run(lib, case, mode, seed):
    from mp_hsir_amd import ops
    cid, family, accounts, fn = case
    lib.hipemu_set_schedule(mode, seed)
    ops.ACCOUNT = {}
    try:
        with guard.recording() as rec, recorded_ops():
            fn()
        seen, waves = set(ops.ACCOUNT or ()), lib.hipemu_max_waves()
    finally:
        ops.ACCOUNT = None
        lib.hipemu_set_schedule(0, 0)
    return list(rec), seen, waves


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bits_do_not_depend_on_the_schedule(case, emu):
    cid, family, accounts, _ = case
    t0 = time.time()
    base, seen, waves = _run(emu, case, 0, 0)
    t_base = time.time() - t0
    assert base, "%s: the check recorded nothing" % cid
    assert set(accounts) <= seen, "%s reached %s, not %s" % (cid, sorted(seen), sorted(set(accounts) - seen))
    assert waves > 1, "%s: no workgroup of this case has more than one wave" % cid
    plan = schedules(waves)
    for k, (mode, seed) in enumerate(plan):
        got, seen_s, waves_s = _run(emu, case, mode, seed)
        if k == 0 and len(got) != len(base):            # the first run of a check may allocate what later runs find cached (a workspace)
            base, _, _ = _run(emu, case, 0, 0)
        assert (waves_s, seen_s) == (waves, seen), "%s under %s launched other kernels than under the default schedule (a cached result?): widest " \
            "workgroup %d waves against %d, %s against %s" % (cid, describe(mode, seed), waves_s, waves, sorted(seen_s), sorted(seen))
        assert len(got) == len(base), "%s under %s: %d tensors recorded, %d under the default schedule" % (cid, describe(mode, seed), len(got), len(base))
        for i, ((what, a), (_, b)) in enumerate(zip(base, got)):
            diff = guard.first_difference(a, b)
            assert diff is None, "%s under %s: recorded tensor %d of %d (%s) is not bitwise the default schedule's: %s (default against this schedule)" \
                % (cid, describe(mode, seed), i, len(base), what, diff)
    st = STATS.setdefault(family, [0, 0, 0, 0.0])
    st[0] += 1
    st[1] += len(base)
    st[2] += len(plan)
    st[3] += time.time() - t0
    print("%s: %d tensors x %d schedules (widest workgroup %d waves), default run %.2f s, all %.2f s" % (cid, len(base), len(plan), waves, t_base, time.time() - t0))


def test_report():
    """per kernel family: cases, tensors compared, schedules (printed with -s; the figures of DESIGN.md)"""
    for family, (cases, tensors, scheds, secs) in STATS.items():
        print("schedules: %-16s %2d cases, %4d tensors per schedule, %3d schedule runs, %6.1f s" % (family, cases, tensors, scheds, secs))


# ---- meta: no LDS-using source file without a case --------------------------------------------------------------------------------
def test_every_lds_source_file_has_a_case():
    using = set()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".hip"):
            with open(os.path.join(CSRC, name)) as f:
                if LDS_USE.search(f.read()):
                    using.add(name)
    assert using == set(FILES), "LDS / barrier-using sources without a schedule case: %s; listed but gone: %s" % (sorted(using - set(FILES)), sorted(set(FILES) - using))
    reached = set()
    for _, _, accounts, _ in CASES:
        reached |= set(accounts)
    ids = {c[0] for c in CASES}
    for name, (accounts, cases) in FILES.items():
        assert accounts and set(accounts) <= reached, "%s: no case reaches %s" % (name, sorted(set(accounts) - reached))
        assert set(cases) <= ids, "%s names cases that do not exist: %s" % (name, sorted(set(cases) - ids))
    assert len(ids) == len(CASES)
    assert LDS_USE.search("    __shared__ float red[4];") and LDS_USE.search("__syncthreads();") and LDS_USE.search("__builtin_amdgcn_s_barrier();")


# ---- the detector detects: tests/hipemu/selftest.hip ------------------------------------------------------------------------------
ALL_SCHEDULES = [(0, 0)] + schedules(4) + [(0 | DESC, 0), (2 | DESC, 0), (5 | DESC, 3)]


@pytest.fixture(scope="module")
def st():
    import build_emu
    lib = _handle(build_emu.build_selftest())
    yield lib
    lib.hipemu_set_schedule(0, 0)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _cross_wave(lib, fixed, blocks=2):
    x = np.random.default_rng(1).random(blocks * 64, dtype=np.float32)
    out = np.full(blocks * 64, -1.0, dtype=np.float32)
    lib.hipemu_selftest_cross_wave(_p(x), _p(out), blocks, fixed)
    return out, (2.0 * x).reshape(blocks, 64)[:, ::-1].reshape(-1) + 1.0


def _ring(lib, fixed, blocks=2, tiles=5):
    x = np.random.default_rng(2).random(blocks * tiles * 64, dtype=np.float32)
    out = np.full(blocks * 3 * 64, -1.0, dtype=np.float32)
    lib.hipemu_selftest_ring(_p(x), _p(out), blocks, tiles, fixed)
    want = np.zeros((blocks, 3, 64), dtype=np.float32)
    xs = x.reshape(blocks, tiles, 64)
    for w in range(3):
        for t in range(tiles):
            want[:, w] = want[:, w] * np.float32(0.5) + np.roll(xs[:, t], -w, axis=1) * np.float32(w + 1)
    return out, want.reshape(-1)


def _static_acc(lib, fixed, blocks=3):
    x = np.random.default_rng(3).random(blocks * 4 * 64, dtype=np.float32)
    out = np.full(blocks * 64, -1.0, dtype=np.float32)
    seen = np.zeros(blocks * 64, dtype=np.uint32)
    lib.hipemu_selftest_static_acc(_p(x), _p(out), _p(seen), blocks, fixed)
    want = np.zeros((blocks, 64), dtype=np.float32)
    for w in range(4):
        want += x.reshape(blocks, 4, 64)[:, w]
    return out, want.reshape(-1), seen


def _cross_block(lib, fixed, blocks=3):
    x = np.random.default_rng(4).random(64, dtype=np.float32)
    mid = np.zeros(64, dtype=np.float32)
    out = np.full(blocks * 64, -1.0, dtype=np.float32)
    lib.hipemu_selftest_cross_block(_p(x), _p(mid), _p(out), blocks, fixed)
    return out, (np.float32(3.0) * x)[None, :].repeat(blocks, 0).reshape(-1) + np.repeat(np.arange(blocks, dtype=np.float32), 64)


def _under(lib, mode, seed, fn, *a):
    lib.hipemu_set_schedule(mode, seed)
    try:
        return fn(lib, *a)
    finally:
        lib.hipemu_set_schedule(0, 0)


def test_set_schedule_round_trip(st):
    seed = ctypes.c_uint64(0)
    assert st.hipemu_get_schedule(ctypes.byref(seed)) == 0 and seed.value == 0          # mode 0 is the default
    st.hipemu_set_schedule(3 | DESC, 77)
    assert st.hipemu_get_schedule(ctypes.byref(seed)) == 3 | DESC and seed.value == 77
    st.hipemu_set_schedule(0, 0)


@pytest.mark.parametrize("kernel", [_cross_wave, _ring, _static_acc, _cross_block], ids=["a-cross_wave", "b-ring", "c-static_acc", "d-cross_block"])
def test_correct_twins_give_the_same_bits_under_every_schedule(st, kernel):
    base = _under(st, 0, 0, kernel, 1)
    assert base[0].tobytes() == base[1].tobytes(), "the twin is wrong under the default schedule"
    for mode, seed in ALL_SCHEDULES:
        got = _under(st, mode, seed, kernel, 1)
        assert got[0].tobytes() == base[0].tobytes(), describe(mode, seed)


def test_a_missing_barrier_between_two_waves_is_found(st):
    out, want = _under(st, 0, 0, _cross_wave, 0)
    assert out.tobytes() == want.tobytes(), "the planted fault must pass under the default schedule (wave 0 runs first)"
    for mode, seed in ((2, 0), (4, 0)):                     # descending waves; wave 0 as the laggard
        out, _ = _under(st, mode, seed, _cross_wave, 0)
        assert out.tobytes() != want.tobytes(), describe(mode, seed)
        assert out.view(np.uint32)[0] != 0xBF800000, "wave 3 must have run (and read the poison), not been skipped"
    assert _under(st, 4, 1, _cross_wave, 0)[0].tobytes() == want.tobytes()       # another laggard: wave 0 still runs before wave 3


def test_a_ring_slot_refilled_too_early_is_found(st):
    out, want = _under(st, 0, 0, _ring, 0)
    assert out.tobytes() == want.tobytes(), "the planted fault must pass under the default schedule (the producer is the last wave)"
    out, _ = _under(st, 5, 3, _ring, 0)                     # the producer sprints: it refills a slot before the consumers have read it
    assert out.tobytes() != want.tobytes()
    assert _under(st, 5, 0, _ring, 0)[0].tobytes() == want.tobytes()             # a consumer as the sprinter waits at the barrier instead


def test_static_lds_is_poisoned_before_every_block(st):
    out, want, seen = _under(st, 0, 0, _static_acc, 0)
    assert (seen == 0xCDCDCDCD).all(), "every block, the second and third included, must find the poison in a static __shared__ array"
    assert out.tobytes() != want.tobytes() and (np.abs(out) > 1e8).all()
    out, want, seen = _under(st, 0, 0, _static_acc, 1)
    assert out.tobytes() == want.tobytes() and (seen == 0xCDCDCDCD).all()


def test_a_dependence_on_an_earlier_block_is_found(st):
    out, want = _under(st, 0, 0, _cross_block, 0)
    assert out.tobytes() == want.tobytes(), "the planted fault must pass with ascending blocks"
    out, _ = _under(st, 0 | DESC, 0, _cross_block, 0)
    assert out.tobytes() != want.tobytes() and out[:64].tobytes() == want[:64].tobytes()      # block 0 itself is right; the others read zeros


def test_a_barrier_not_every_thread_reaches_is_reported_not_spun_on():
    """in a child process: the emulator must print the deadlock report and abort inside a second (it used to spin for ever)"""
    import build_emu
    code = ("import ctypes, sys, time\n"
            "lib = ctypes.CDLL(%r)\n"
            "out = (ctypes.c_float * 128)()\n"
            "print(repr(time.time()), flush=True)\n"
            "lib.hipemu_selftest_divergent_barrier(out)\n"
            "print('returned', flush=True)\n" % build_emu.build_selftest())
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    took = time.time() - float(r.stdout.split()[0])         # from the launch to the end of the child
    assert r.returncode == -6 and "returned" not in r.stdout, (r.returncode, r.stdout, r.stderr[-500:])
    assert "hipemu: deadlock in block (0,0,0) of grid (1,1,1), 128 threads: 64 wait at the block barrier, 0 at a wave rendezvous, 64 have finished" in r.stderr, r.stderr[-500:]
    assert took < 1.0, "the launch took %.2f s to end" % took
