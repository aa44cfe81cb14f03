"""The C-ABI shared library loads and exports every symbol include/mphsir.h declares (no compute)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mp-hsir_amd", "libmphsir.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        sys.path.insert(0, os.path.join(ROOT, "mp-hsir_amd"))
        import build
        build.build(verbose=False)
    return ctypes.CDLL(LIB)


def declared_symbols():
    """every `mphsir_name (` outside a comment: deliberately not the parser of mp_hsir_amd._lib, so that a prototype it skips is caught"""
    text = open(os.path.join(ROOT, "include", "mphsir.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mphsir_\w+)\s*\(", text)))


def test_every_declared_symbol_is_exported(lib):
    import mp_hsir_amd._lib as L
    names = L.symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), "libmphsir.so does not export %s" % n


def test_python_binding_covers_the_header():
    import mp_hsir_amd._lib as L
    assert L.symbols() == declared_symbols() and len(L.symbols()) == 92


def test_version_and_error_text(lib):
    lib.mphsir_version.restype = ctypes.c_char_p
    lib.mphsir_last_error.restype = ctypes.c_char_p
    assert lib.mphsir_version().decode().endswith("gfx950")
    assert lib.mphsir_gemm_tok(None, 0, None) == -1            # EINVAL, nothing launched
    assert b"null pointer" in lib.mphsir_last_error()


def test_library_contains_gfx950_code_objects():
    blob = open(LIB, "rb").read()
    assert b"gfx950" in blob and b"gfx90a" not in blob and b"gfx942" not in blob


def test_ops_refuse_cpu_tensors_without_fallback(lib):
    """Product path must fail loudly: no CPU fallback, no silent oracle routing."""
    import torch
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    saved = (L._lib, L._is_emu)
    try:
        L._lib, L._is_emu = None, False
        L.load()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.gemm_tok(torch.zeros(64, 32), torch.zeros(16, 32))
        with pytest.raises(RuntimeError, match="not found"):
            L.load("/nonexistent/libmphsir.so")
    finally:
        L._lib, L._is_emu = saved


def test_workspace_size_queries_match_the_python_allocations(lib):
    """mphsir_*_workspace_bytes (the caller owns every buffer and asks the library for its size) agree with what
    mp-hsir_amd/ops.py allocates for the same shapes (pure host arithmetic: no GPU needed)."""
    for f in ("mphsir_gemm_tn_workspace_bytes", "mphsir_dwconv_gram_workspace_bytes", "mphsir_pg_gate_bwd_workspace_bytes",
              "mphsir_win_attn_bwd_workspace_bytes"):
        getattr(lib, f).restype = ctypes.c_int64
    assert lib.mphsir_gemm_tn_workspace_bytes(704, 128, 42, 1, 1) == 42 * (704 * 128 + 704) * 4
    assert lib.mphsir_dwconv_gram_workspace_bytes(32, 16, 128, 2) == 32 * 16 * (2 * 64 * 64 + 256) * 4
    kl, kr = ctypes.c_int32(0), ctypes.c_int32(0)
    n = lib.mphsir_pg_gate_bwd_workspace_bytes(2048, 128, 16, 1, ctypes.byref(kl), ctypes.byref(kr))
    assert (kl.value, kr.value) == (464, 216) and n == 2048 * (464 + 216) * 2          # ops.pg_gate_bwd: round_up(C+5r+256, 8), round_up(5r+1+C, 8)
    M = 32 * 64 * 64
    assert lib.mphsir_win_attn_bwd_workspace_bytes(32, 64, 64, 128, 2, 1) == M * 5 * 128 * 2 + (M // 64) * 225 * 2 * 4
    assert lib.mphsir_gemm_tn_workspace_bytes(0, 1, 1, 1, 0) < 0


# ---- the args structs: mp_hsir_amd._lib builds them from include/mphsir.h, so what is pinned here is the header itself --------------------
def test_every_args_struct_starts_with_its_size():
    import mp_hsir_amd._lib as L
    args = {n: c for n, c in L.STRUCTS.items() if n.endswith("_args")}
    assert len(L.STRUCTS) == 30 and len(args) == 28 and sorted(set(L.STRUCTS) - set(args)) == ["mphsir_gemm_tn_problem", "mphsir_reduce_seg"]
    for name, cls in L.STRUCTS.items():
        assert getattr(L, cls.__name__) is cls and issubclass(cls, L._Args) == (name in args), name
    for name, cls in args.items():
        assert cls._fields_[0] == ("struct_size", ctypes.c_uint32), "%s must start with struct_size" % name
        assert cls().struct_size == ctypes.sizeof(cls)


def test_the_float_bearing_args_structs_are_frozen():
    """the ABI freeze of the optimizer and loss structs: member lists, float members, entry points, their place in INTEGRATION.md"""
    import mp_hsir_amd._lib as L

    def members(cls, ty=None):
        return [n for n, t in cls._fields_[1:] if ty is None or t is ty]

    assert members(L.SpectralLossArgs) == ["y", "clean", "grad", "out", "workspace", "workspace_bytes", "B", "C", "H", "W", "w_sam", "w_sdiff"]
    assert members(L.SsimLossArgs) == ["y", "clean", "grad", "base_loss", "out", "workspace", "workspace_bytes", "B", "C", "H", "W", "w_ssim", "accumulate"]
    assert members(L.SpectralLossArgs, ctypes.c_float) == ["w_sam", "w_sdiff"] and members(L.SsimLossArgs, ctypes.c_float) == ["w_ssim"]
    assert members(L.GradNormArgs, ctypes.c_float) == ["grad_scale", "max_norm"]
    assert members(L.FlatAdamwExArgs, ctypes.c_float) == ["lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale", "ema_decay"]
    assert {"mphsir_grad_norm", "mphsir_grad_norm_workspace_bytes", "mphsir_flat_adamw_ex", "mphsir_spectral_loss", "mphsir_spectral_loss_workspace_bytes",
            "mphsir_ssim_loss", "mphsir_ssim_loss_workspace_bytes"} <= set(L.symbols())
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mphsir_grad_norm_args", "mphsir_flat_adamw_ex_args", "mphsir_spectral_loss_args", "mphsir_ssim_loss_args"):
        assert name in md, name
    assert L.CONSTANTS["MPHSIR_K_COUNT"] == 41, "the SSIM pair launches under the ids of the spectral-loss pair"


def test_integration_md_structs_match_the_header():
    """The binding INTEGRATION.md shows a maintainer is executable ctypes code: its Structure classes must be the header's structs
    (round 5 shipped a doc whose MlpArgs ended 13 fields early)."""
    import mp_hsir_amd._lib as L
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    found = 0
    for cls, comment, body in re.findall(r"class (\w+)\(ctypes\.Structure\):\s*#\s*struct (mphsir_\w+)[^\n]*\n(\s+_fields_ = \[.*?\])[ \t]*(?:#[^\n]*)?\n", md, flags=re.S):
        ns = {"ctypes": ctypes}
        exec("class %s(ctypes.Structure):\n%s" % (cls, body), ns)
        got = ns[cls]._fields_
        want = L.STRUCTS[comment]._fields_
        assert [n for n, _ in got] == [n for n, _ in want], "INTEGRATION.md %s != %s" % (cls, comment)
        assert all(ctypes.sizeof(a[1]) == ctypes.sizeof(b[1]) for a, b in zip(got, want))
        found += 1
    assert found >= 1


def test_a_short_args_struct_is_refused(lib):
    """struct_size: a caller compiled against an older, shorter struct gets EINVAL and a message, nothing is read past its end"""
    import mp_hsir_amd._lib as L
    lib.mphsir_last_error.restype = ctypes.c_char_p
    a = L.MlpArgs()
    assert a.struct_size == ctypes.sizeof(L.MlpArgs)
    a.struct_size -= 8
    assert lib.mphsir_gated_mlp_fwd(ctypes.byref(a), 1, None) == -1
    assert b"struct_size" in lib.mphsir_last_error()
    g = L.GemmArgs()
    g.struct_size = 0
    assert lib.mphsir_gemm_tok(ctypes.byref(g), 1, None) == -1 and b"struct_size" in lib.mphsir_last_error()


# ---- the header parser of mp_hsir_amd._lib on synthetic headers (no library) -------------------------------------------------------------
GOOD_HEADER = """
#define MPHSIR_EBAD (-3)   /* a comment */
#define MPHSIR_TINY 1e-6
#define MPHSIR_MASK 0x10
typedef struct mphsir_toy_args {
    uint32_t struct_size;   /* = sizeof */
    const float* w9; float scale, bias;
    int64_t n; int32_t B, H;
} mphsir_toy_args;
typedef struct mphsir_toy_seg { const void* src; int32_t n; } mphsir_toy_seg;
const char* mphsir_toy_name(int kid);
int mphsir_toy(const mphsir_toy_args* a, int dtype, void* stream);
int64_t mphsir_toy_bytes(int32_t B, int32_t form /* 1 | 2 */,
                         int32_t* KL, const mphsir_toy_seg* segs,
                         float scale);
int mphsir_toy_none(void);
"""


def test_parser_accepts_the_constructs_of_the_header():
    import mp_hsir_amd._lib as L
    structs, protos, consts = L.parse_header(GOOD_HEADER)
    assert consts == {"MPHSIR_EBAD": -3, "MPHSIR_TINY": 1e-6, "MPHSIR_MASK": 16} and isinstance(consts["MPHSIR_TINY"], float)
    toy, seg = structs["mphsir_toy_args"], structs["mphsir_toy_seg"]
    assert list(structs) == ["mphsir_toy_args", "mphsir_toy_seg"] and (toy.__name__, seg.__name__) == ("ToyArgs", "ToySeg")
    assert toy._fields_ == [("struct_size", ctypes.c_uint32), ("w9", ctypes.c_void_p), ("scale", ctypes.c_float), ("bias", ctypes.c_float),
                            ("n", ctypes.c_int64), ("B", ctypes.c_int32), ("H", ctypes.c_int32)]
    assert issubclass(toy, L._Args) and toy(n=3).struct_size == ctypes.sizeof(toy) == 40
    assert not issubclass(seg, L._Args) and seg._fields_ == [("src", ctypes.c_void_p), ("n", ctypes.c_int32)]
    assert protos == {"mphsir_toy_name": (ctypes.c_char_p, [ctypes.c_int]),
                      "mphsir_toy": (ctypes.c_int, [ctypes.POINTER(toy), ctypes.c_int, ctypes.c_void_p]),
                      "mphsir_toy_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(seg), ctypes.c_float]),
                      "mphsir_toy_none": (ctypes.c_int, [])}


@pytest.mark.parametrize("name,text", [
    ("mphsir_a_args", "typedef struct mphsir_a_args { uint32_t struct_size; float taps[9]; } mphsir_a_args;"),                          # array member
    ("mphsir_b_args", "typedef struct mphsir_b_args { uint32_t struct_size; struct { int32_t x; } in; } mphsir_b_args;"),              # nested struct
    ("mphsir_c_args", "typedef struct mphsir_c_args { uint32_t struct_size; union { int32_t i; float f; } u; } mphsir_c_args;"),       # nested union
    ("mphsir_d_args", "typedef struct mphsir_d_args { uint32_t struct_size; int (*done)(int); } mphsir_d_args;"),                      # function pointer member
    ("mphsir_e_args", "typedef struct mphsir_e_args { uint32_t struct_size; int32_t on : 1; } mphsir_e_args;"),                        # bit-field
    ("mphsir_f_args", "typedef struct mphsir_f_args { uint32_t struct_size; size_t n; } mphsir_f_args;"),                              # unknown type name
    ("mphsir_g_args", "typedef struct mphsir_g_args { uint32_t struct_size; float** rows; } mphsir_g_args;"),                          # pointer to pointer
    ("mphsir_h_args", "struct mphsir_h_args { uint32_t struct_size; };"),                                                              # a struct without its typedef
    ("mphsir_fn_a", "int mphsir_fn_a(int (*done)(int), void* stream);"),                                                               # function pointer argument
    ("mphsir_fn_b", "int mphsir_fn_b(unsigned n, void* stream);"),                                                                     # unknown type name
    ("mphsir_fn_c", "int mphsir_fn_c(float** rows, void* stream);"),                                                                   # pointer to pointer
    ("mphsir_fn_d", "int mphsir_fn_d(const mphsir_nowhere_args* a, void* stream);"),                                                   # unknown struct
    ("mphsir_fn_e", "double mphsir_fn_e(int kid);"),                                                                                   # unknown return type
    ("mphsir_fn_f", "int mphsir_fn_f(float taps[9]);"),                                                                                # array argument
])
def test_parser_refuses_what_it_does_not_model(name, text):
    import mp_hsir_amd._lib as L
    with pytest.raises(RuntimeError, match=r"mphsir\.h: %s: cannot bind" % name):
        L.parse_header(GOOD_HEADER + text)


def test_the_header_is_read_once_per_process(lib, monkeypatch):
    import mp_hsir_amd._lib as L
    monkeypatch.setattr(L, "_HEADER", "/nonexistent/mphsir.h")
    with pytest.raises(RuntimeError, match="not found"):
        L._read_header()
    saved = (L._lib, L._is_emu)
    try:
        assert L.load(LIB) is not None and L.symbols()            # a second load() binds from the parse of the import, not from the file
    finally:
        L._lib, L._is_emu = saved
