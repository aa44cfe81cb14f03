"""What the host decides for the shapes that ship: which kernel form runs and with what launch shape, tabulated for the PGSSTB stages of
the two shipped configurations and pinned against a literal.  Nothing is launched: the `*_fits` entry points of the library are host
arithmetic (the CPU-emulated build of the same sources answers them), the rest are pure functions of sizes and dtype in ops.py.
A change of a threshold has to edit EXPECTED on purpose."""
import pytest
import torch

from emu import bind_emulator

# (C, heads, side) of the PGSSTB stages: encoder 1 / encoder 2 / latent / decoder 1 + refinement
STAGES = {"nat": [(64, 2, 64), (128, 4, 32), (256, 8, 16), (128, 2, 64)],
          "rs": [(96, 2, 64), (192, 4, 32), (384, 8, 16), (192, 2, 64)]}
BANDS = {"nat": (31, 64), "rs": (100, 96)}          # (in = out channels, dim) of the two head convs
# (configuration, dtype, batch, side multiplier): the two training steps, the fp32 parity path, the 512x512 batch-1 forward
RUNS = [("nat", torch.bfloat16, 32, 1), ("rs", torch.float16, 16, 1), ("nat", torch.float32, 2, 1), ("rs", torch.float32, 2, 1),
        ("nat", torch.bfloat16, 1, 8), ("rs", torch.float16, 1, 8)]
_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


def tabulate(ops):
    """run key -> {stage or conv key -> decisions}"""
    table = {}
    for cfg, dt, B, mult in RUNS:
        rows = table["%s/%s/b%d/x%d" % (cfg, _NAME[dt], B, mult)] = {}
        for C, heads, side in STAGES[cfg]:
            S = side * mult
            M, HW, HP = B * S * S, S * S, ops.round_up(int(C * 2.66), 32)
            nsf = ops.choose_nsplit_fused(B, S, S, C)
            rows["C%d/h%d/s%d" % (C, heads, S)] = dict(
                mlp_fuses=ops.gated_mlp_fuses(M, C, HW, dt), mlp_hsplit=ops.mlp_hsplit(M, C, HP),
                wgrad_fits=ops.gated_mlp_wgrad_fits(M, C, HP, dt), wgrad_plan=tuple(ops.mlp_wgrad_plan(M, C, HP, dt)),
                gram_fits=ops.qkv_dwconv_gram_fits(C, heads, S, S, dt), rows_fits=ops.qkv_dwconv_gram_rows_fits(C, heads, S, S, dt),
                row_segments=ops.choose_row_segments(B, S, S, C, heads), nsplit_fused=nsf, head_groups=ops.choose_head_groups(B, nsf, heads, C),
                spectral_bwd_fits=ops.spectral_dqkv_bwd_fits(C, heads, S, S, dt),
                dsa_fits=ops.win_attn_bwd_dsa_fits(C, heads, dt), dsa_pays=bool(ops.win_attn_bwd_dsa_pays(B, S, S, heads)),
                ln_win_dxn_fits=ops.ln_bwd_win_dxn_fits(M, C, dt), ln_tok_dxn_f32_fits=ops.ln_bwd_tok_dxn_f32_fits(M, C, dt),
                fold_forms_dm=ops.fold_bwd_forms_dm(HW, C, heads, dt),
                # (form, tile128, nsplit) of the weight-gradient GEMMs of a block: window-attention qkv and proj, the spectral qkv conv,
                # and the batched dM = d_out^T v in front of the fold backward
                tn_qkv=tuple(ops.tn_split(M, 3 * C, C, dt)), tn_proj=tuple(ops.tn_split(M, C, C, dt)),
                tn_spectral_qkv=tuple(ops.tn_split(M, 3 * C, C, dt)), tn_dm=tuple(ops.tn_split(HW, C, C, dt, Bt=B, batched=True)))
        bands, dim = BANDS[cfg]
        M = B * (64 * mult) ** 2
        for name, cin, cout in (("embed", bands, dim), ("output", 2 * dim, bands)):
            cp, co = ops.round_up(cin, 32), ops.round_up(cout, 32)
            # 16-bit: the im2col gather inside conv3x3_wgrad; fp32: im2col3x3 + gemm_tn
            rows["conv3x3/" + name] = (ops.conv3x3_wgrad_split(M, co, cp) if dt != torch.float32 else tuple(ops.tn_split(M, co, 9 * cp, dt)))
    return table


COLUMNS = ("mlp_fuses", "mlp_hsplit", "wgrad_fits", "wgrad_plan", "gram_fits", "rows_fits", "row_segments", "nsplit_fused", "head_groups",
           "spectral_bwd_fits", "dsa_fits", "dsa_pays", "ln_win_dxn_fits", "ln_tok_dxn_f32_fits", "fold_forms_dm", "tn_qkv", "tn_proj",
           "tn_spectral_qkv", "tn_dm")
# Taken at commit 894b026 ("Tests: device math probes and parity checks off the unit Gaussian"), the parent of the change that retired the
# environment switches: the same calls against that commit's ops.py with no variable set, the two split formulas copied by hand out of
# its gemm_tn and conv3x3_wgrad.  Stage rows in COLUMNS order; conv rows: the split of conv3x3_wgrad (16-bit) or (form, tile128, nsplit)
# of the im2col GEMM (fp32).
EXPECTED = {
    "nat/bf16/b32/x1": {
        "C64/h2/s64": (True, 1, True, (1, 80), True, True, 4, 16, 1, True, True, True, True, True, False, (1, True, 128), (2, True, 128), (1, True, 128), (1, True, 16)),
        "C128/h4/s32": (True, 1, True, (1, 40), True, True, 4, 8, 2, True, True, True, True, True, True, (1, True, 68), (1, True, 102), (1, True, 68), (1, True, 3)),
        "C256/h8/s16": (False, 2, False, (1, 8), True, False, 4, 2, 4, True, True, False, True, False, True, (1, True, 8), (1, True, 12), (1, True, 8), (1, True, 1)),
        "C128/h2/s64": (True, 1, True, (1, 40), True, True, 2, 16, 1, True, True, True, True, True, False, (1, True, 128), (2, True, 128), (1, True, 128), (1, True, 12)),
        "conv3x3/embed": 128,
        "conv3x3/output": 56,
    },
    "rs/fp16/b16/x1": {
        "C96/h2/s64": (True, 1, True, (1, 64), True, True, 4, 32, 1, True, False, True, True, True, False, (1, True, 128), (2, True, 128), (1, True, 128), (1, True, 16)),
        "C192/h4/s32": (False, 1, False, (1, 32), True, True, 4, 8, 4, True, False, False, True, True, True, (1, True, 22), (1, True, 34), (1, True, 22), (1, True, 2)),
        "C384/h8/s16": (False, 4, False, (1, 8), True, False, 4, 2, 8, True, False, False, False, False, True, (1, True, 2), (1, True, 4), (1, True, 2), (1, True, 1)),
        "C192/h2/s64": (False, 1, False, (1, 32), True, False, 4, 32, 1, True, False, True, True, True, False, (1, True, 51), (1, True, 128), (1, True, 51), (1, True, 8)),
        "conv3x3/embed": 56,
        "conv3x3/output": 36,
    },
    "nat/fp32/b2/x1": {
        "C64/h2/s64": (False, 1, False, (1, 56), True, False, 16, 32, 2, False, False, False, False, False, False, (1, False, 16), (1, False, 16), (1, False, 16), (1, False, 8)),
        "C128/h4/s32": (False, 1, False, (1, 8), False, False, 8, 8, 4, False, False, False, False, False, False, (1, False, 4), (1, False, 4), (1, False, 4), (1, False, 2)),
        "C256/h8/s16": (False, 2, False, (1, 8), False, False, 4, 2, 8, False, False, False, False, False, False, (1, False, 1), (1, False, 1), (1, False, 1), (1, False, 1)),
        "C128/h2/s64": (False, 1, False, (1, 24), False, False, 16, 32, 2, False, False, False, False, False, False, (1, False, 16), (1, False, 16), (1, False, 16), (1, False, 8)),
        "conv3x3/embed": (1, False, 16),
        "conv3x3/output": (1, False, 16),
    },
    "rs/fp32/b2/x1": {
        "C96/h2/s64": (False, 1, False, (1, 40), False, False, 16, 32, 2, False, False, False, False, False, False, (1, False, 16), (1, False, 16), (1, False, 16), (1, False, 8)),
        "C192/h4/s32": (False, 8, False, (1, 8), False, False, 8, 8, 4, False, False, False, False, False, False, (1, False, 4), (1, False, 4), (1, False, 4), (1, False, 2)),
        "C384/h8/s16": (False, 32, False, (1, 8), False, False, 4, 2, 8, False, False, False, False, False, False, (1, False, 1), (1, False, 1), (1, False, 1), (1, False, 1)),
        "C192/h2/s64": (False, 2, False, (1, 16), False, False, 16, 32, 2, False, False, False, False, False, False, (1, False, 16), (1, False, 16), (1, False, 16), (1, False, 8)),
        "conv3x3/embed": (1, False, 16),
        "conv3x3/output": (1, False, 14),
    },
    "nat/bf16/b1/x8": {
        "C64/h2/s512": (True, 1, True, (1, 80), True, True, 16, 512, 1, True, True, True, True, True, False, (1, True, 128), (2, True, 128), (1, True, 128), (1, True, 128)),
        "C128/h4/s256": (True, 1, True, (1, 40), True, True, 16, 512, 1, True, True, True, True, True, False, (1, True, 128), (2, True, 128), (1, True, 128), (1, True, 128)),
        "C256/h8/s128": (False, 1, False, (1, 16), True, True, 16, 128, 2, True, True, False, True, False, False, (1, True, 17), (1, True, 25), (1, True, 17), (1, True, 25)),
        "C128/h2/s512": (True, 1, True, (1, 40), True, True, 8, 512, 1, True, True, True, True, True, False, (1, True, 128), (2, True, 128), (1, True, 128), (1, True, 128)),
        "conv3x3/embed": 128,
        "conv3x3/output": 56,
    },
    "rs/fp16/b1/x8": {
        "C96/h2/s512": (True, 1, True, (1, 64), True, True, 8, 512, 1, True, False, True, True, True, False, (1, True, 128), (2, True, 128), (1, True, 128), (1, True, 128)),
        "C192/h4/s256": (False, 1, False, (1, 32), True, True, 8, 512, 1, True, False, True, True, True, False, (1, True, 51), (1, True, 128), (1, True, 51), (1, True, 128)),
        "C384/h8/s128": (False, 1, False, (1, 16), True, False, 8, 128, 2, True, False, False, False, False, False, (1, True, 11), (1, True, 17), (1, True, 11), (1, True, 17)),
        "C192/h2/s512": (False, 1, False, (1, 32), True, False, 8, 512, 1, True, False, True, True, True, False, (1, True, 64), (1, True, 128), (1, True, 64), (1, True, 128)),
        "conv3x3/embed": 56,
        "conv3x3/output": 36,
    },
}


def test_host_dispatch_of_the_shipped_shapes_is_the_pinned_table():
    from mp_hsir_amd import ops
    got = tabulate(ops)
    assert got.keys() == EXPECTED.keys()
    for run in EXPECTED:
        assert got[run].keys() == EXPECTED[run].keys(), run
        for key, want in EXPECTED[run].items():
            if key.startswith("conv3x3/"):
                assert got[run][key] == want, (run, key, got[run][key], want)
                continue
            assert got[run][key].keys() == set(COLUMNS)
            bad = {c: (got[run][key][c], w) for c, w in zip(COLUMNS, want) if got[run][key][c] != w}
            assert not bad, (run, key, bad)      # column -> (decided now, pinned)

