"""The guard harness (tests/guard.py) against fake "kernels" written as torch index operations inside the guarded buffers: every way
a kernel can be wrong while returning the right tensor is detected through the mechanism meant for it, and a correct kernel
yields an empty report.  CPU, plain torch: no emulator, no GPU; every stray access stays inside memory the test owns."""
import pytest
import torch

import guard
from guard import Guard, guarded, guarded_ops
from util import rel_l2

M, C = 64, 20
FLOATS = [torch.float32, torch.bfloat16, torch.float16]


def _master(dtype, seed=7):
    return torch.randn((M, C), generator=torch.Generator().manual_seed(seed)).to(dtype)


def _copy_kernel(G, x, y, rows=M, first_row=0):
    """y[first_row : first_row + rows] = x[...] through the whole buffers: rows past M run into the bands, as a kernel's would"""
    xw, x0 = G.whole(x)
    yw, y0 = G.whole(y)
    lo, hi = first_row * C, (first_row + rows) * C
    yw[y0 + lo:y0 + hi] = xw[x0 + lo:x0 + hi]


@pytest.mark.parametrize("dtype", FLOATS)
def test_correct_kernel_gives_an_empty_report(dtype):
    G = Guard("cpu")
    x = G.input(_master(dtype), seed=7)
    y = G.alloc((M, C), dtype, "cpu", "output")
    z = G.alloc((M, C), dtype, "cpu", "output", fill=0)
    assert float(z.float().abs().max()) == 0.0 and torch.isnan(y.float()).all()
    _copy_kernel(G, x, y)
    assert G.verify() == []
    assert torch.equal(y, _master(dtype))


@pytest.mark.parametrize("dtype", FLOATS + [torch.int32, torch.int64, torch.uint8])
def test_store_one_element_after_the_end(dtype):
    G = Guard("cpu")
    y = G.alloc((M, C), dtype, "cpu", "output", fill=0)
    w, o = G.whole(y)
    w[o + M * C] = 1
    rep = G.verify()
    assert len(rep) == 1 and rep[0].startswith("BAND test_guard_host.py")
    assert "test_store_one_element_after_the_end -> y " in rep[0]
    assert "1 elements damaged AFTER the tensor, first at element 0 past its end" in rep[0]


@pytest.mark.parametrize("dtype", FLOATS + [torch.int32])
def test_store_one_element_before_the_start(dtype):
    G = Guard("cpu")
    y = G.alloc((M, C), dtype, "cpu", "output", fill=0)
    w, o = G.whole(y)
    w[o - 1] = 1
    rep = G.verify()
    assert len(rep) == 1 and "test_store_one_element_before_the_start -> y " in rep[0]
    assert "1 elements damaged BEFORE the tensor, first at element -1 (1 before its start)" in rep[0]


@pytest.mark.parametrize("dtype", FLOATS)
def test_row_copied_from_an_input_band_into_an_output_band(dtype):
    """a row bound off by one (`t0 <= M`): the kernel reads one row past X and writes it one row past Y.  The copied row is X's band:
    with one pattern for both roles the overrun would rewrite Y's sentinel bit for bit (a cast copy moves bits; x86 keeps NaN
    payloads).  The patterns differ by role, so it is damage; the input band itself is intact (it was only read)."""
    G = Guard("cpu")
    x = G.input(_master(dtype), seed=7)
    y = G.alloc((M, C), dtype, "cpu", "output")
    _copy_kernel(G, x, y, rows=M + 1)
    assert torch.equal(y, _master(dtype))                      # what a parity check sees is right
    rep = G.verify()
    assert len(rep) == 1, rep
    assert "-> y " in rep[0] and "[output]" in rep[0]
    assert "%d elements damaged AFTER the tensor, first at element 0 past its end" % C in rep[0]
    assert "holds 0x%x" % (guard.input_pattern(dtype) & ((1 << 8 * dtype.itemsize) - 1)) in rep[0]


@pytest.mark.parametrize("dtype", FLOATS)
def test_patterns_differ_between_roles(dtype):
    pats = {guard.input_pattern(dtype), guard.prefill_pattern(dtype)}
    assert len(pats) == 2
    outs = {guard.output_pattern(dtype, c, s) for c in range(300) for s in (0, 1)}
    assert not (outs & pats)
    assert guard.output_pattern(dtype, 3, 0) != guard.output_pattern(dtype, 3, 1) != guard.output_pattern(dtype, 4, 0)
    ints = guard._INT[dtype.itemsize]
    for p in (guard.input_pattern(dtype), guard.prefill_pattern(dtype)):           # NaN in this format
        assert torch.isnan(torch.tensor([p], dtype=ints).view(dtype)).all()
    assert torch.isfinite(torch.tensor([guard.output_pattern(dtype, 5, 1)], dtype=ints).view(dtype)).all()


@pytest.mark.parametrize("dtype", FLOATS)
def test_output_with_one_16_row_tile_left_unwritten(dtype):
    G = Guard("cpu")
    x = G.input(_master(dtype), seed=7)
    y = G.alloc((M, C), dtype, "cpu", "output")
    _copy_kernel(G, x, y, rows=M - 16)
    rep = G.verify()
    assert len(rep) == 1 and rep[0].startswith("PREFILL") and "-> y " in rep[0]
    assert "%d of %d elements never written, first at flat element %d = index (%d, 0)" % (16 * C, M * C, (M - 16) * C, M - 16) in rep[0]
    # a `zeros` interior makes no such claim: its value is the contract
    G = Guard("cpu")
    z = G.alloc((M, C), dtype, "cpu", "output", fill=0)
    assert G.verify() == [] and float(z.float().abs().max()) == 0.0


def test_partial_ok_needs_its_condition():
    """an entry of PARTIAL_OK holds for its (function, name) only, and only while the local it names is true"""
    def spectral_fold_bwd(G, w2_blocks):
        W2 = G.alloc((4, 8), torch.float32, "cpu", "output")
        W2[:, :4] = 0
        return W2

    def unlisted(G, w2_blocks):
        W2 = G.alloc((4, 8), torch.float32, "cpu", "output")
        W2[:, :4] = 0
        return W2

    key = ("spectral_fold_bwd", "W2")
    assert key in guard.PARTIAL_OK and guard.PARTIAL_OK[key][0] == "w2_blocks"
    try:
        guard._SRC = guard._SRC + ("test_guard_host.py",)
        for fn, flag, clean in ((spectral_fold_bwd, True, True), (spectral_fold_bwd, False, False), (unlisted, True, False)):
            G = Guard("cpu")
            fn(G, flag)
            assert (G.verify() == []) == clean, (fn.__name__, flag)
    finally:
        guard._SRC = guard._SRC[:-1]
    for (fn, name), (cond, reason) in guard.PARTIAL_OK.items():
        assert "*" not in fn and "*" not in name and len(reason) > 40


def test_input_modified_in_place():
    G = Guard("cpu")
    x = G.input(_master(torch.bfloat16), seed=11)
    y = G.alloc((M, C), torch.bfloat16, "cpu", "output")
    _copy_kernel(G, x, y)
    x[3, 5] += 1
    rep = G.verify()
    assert len(rep) == 1 and rep[0].startswith("INPUT") and "(seed 11)" in rep[0]
    assert "1 elements changed, first at flat element %d = index (3, 5)" % (3 * C + 5) in rep[0]


@guarded
def _fake_check_reads_past_the_end(dev, dtype):
    """y[i] = x[i] + x[i + 1]: the last row reads one row past X"""
    G = guard.active()
    m = _master(dtype)
    x = G.input(m, seed=7)
    y = G.alloc((M, C), dtype, dev, "output")
    w, o = G.whole(x)
    y.copy_((w[o:o + M * C].float() + w[o + C:o + (M + 1) * C].float()).reshape(M, C))
    ref = m.double()
    ref[:-1] += m.double()[1:]
    assert rel_l2(y[:-1].double(), ref[:-1]) < 1e-2                  # every row but the last is right
    err = rel_l2(y.double(), ref)
    assert err < 1e-2, err


@pytest.mark.parametrize("dtype", FLOATS)
def test_result_computed_from_an_input_band_element_is_nan(dtype):
    """an out-of-range read leaves no trace in any band; the input band is a NaN, so the result fails the check's own bound"""
    with pytest.raises(AssertionError) as e:
        _fake_check_reads_past_the_end("cpu", dtype)
    assert not isinstance(e.value, guard.Report) and "nan" in str(e.value)
    assert guard.active() is None


@pytest.mark.parametrize("dtype", FLOATS + [torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool])
@pytest.mark.parametrize("shape", [(1,), (3, 5), (70, 20), (7, 1, 3), (2, 225, 2), (1, 8, 8, 172), (300, 4099)])
def test_interiors_are_16_byte_aligned_and_bands_are_sized_by_the_rule(dtype, shape):
    G = Guard("cpu")
    t = G.alloc(shape, dtype, "cpu", "output")
    assert t.data_ptr() % 16 == 0 and tuple(t.shape) == shape and t.is_contiguous() and t.dtype == dtype
    b = G.bufs[-1]
    pitch = shape[-1] * dtype.itemsize
    assert b.band % 256 == 0 and b.band >= min(max(4096, 128 * pitch), 1 << 20) and b.band <= (1 << 20)
    assert b.raw.numel() == 2 * b.band + t.numel() * dtype.itemsize
    assert G.verify()[0].startswith("PREFILL") and len(G.verify()) == 1


def test_proxy_wraps_the_four_functions_and_forwards_the_rest():
    from mp_hsir_amd import autograd_ops, ops
    with guarded_ops("cpu") as G:
        assert ops.torch is not torch and autograd_ops.torch is ops.torch
        assert ops.torch.float32 is torch.float32 and ops.torch.nn is torch.nn and ops.torch.cat is torch.cat
        a = ops.torch.empty((5, 7), dtype=torch.bfloat16, device="cpu")
        b = ops.torch.zeros(12, dtype=torch.float32)
        src = torch.randn(2, 3, 4, 5).permute(0, 2, 3, 1)               # dense, permuted
        c = ops.torch.empty_like(src)
        d = ops.torch.zeros_like(src, dtype=torch.float16)
        e = ops.torch.empty_like(src[..., :3])                            # not dense: the real call makes it contiguous
        assert len(G.bufs) == 5
        assert c.stride() == torch.empty_like(src).stride() == src.stride() and c.shape == src.shape
        assert d.stride() == src.stride() and d.dtype == torch.float16 and float(d.abs().max()) == 0.0
        assert e.stride() == torch.empty_like(src[..., :3]).stride()
        assert torch.isnan(a.float()).all() and float(b.abs().max()) == 0.0 and b.shape == (12,)
        assert all(t.data_ptr() % 16 == 0 for t in (a, b, c, d, e))
        # what the guard does not own passes through: another device type, empty tensors, pinned host tables
        assert ops.torch.empty((0, 4)).numel() == 0 and ops.torch.empty((2,), device="meta").device.type == "meta"
        assert ops.torch.empty((3,), pin_memory=False).shape == (3,)
        assert len(G.bufs) == 5
        assert G.skipped == {"no elements": 1, "a meta tensor under a cpu guard": 1, "keyword pin_memory": 1}, G.skipped
        c.fill_(1.0)
        e.fill_(1.0)
        a.fill_(2.0)
        assert G.verify() == []
    assert ops.torch is torch and autograd_ops.torch is torch and guard.active() is None


def test_proxy_is_restored_after_an_exception_and_the_decorator_is_reentrant():
    from mp_hsir_amd import autograd_ops, ops

    @guarded
    def inner(dev, fail):
        assert guard.active() is not None and ops.torch is not torch
        ops.torch.empty((4, 4), dtype=torch.float32, device=dev).fill_(0.0)
        if fail:
            raise RuntimeError("boom")
        return "inner"

    @guarded
    def outer(dev, fail):
        g = guard.active()
        r = inner(dev, fail)
        assert guard.active() is g and len(g.bufs) == 1               # the inner check joined this guard and left it active
        return r + "+outer"

    assert outer("cpu", False) == "inner+outer"
    assert ops.torch is torch and guard.active() is None
    with pytest.raises(RuntimeError, match="boom"):
        outer("cpu", True)
    assert ops.torch is torch and autograd_ops.torch is torch and guard.active() is None
    with pytest.raises(ZeroDivisionError):
        with guarded_ops("cpu"):
            1 / 0
    assert ops.torch is torch and autograd_ops.torch is torch and guard.active() is None


def test_decorator_fails_the_check_with_the_report_and_counts_allocations():
    @guarded
    def check_overrun(dev):
        G = guard.active()
        y = G.alloc((M, C), torch.float32, dev, "output", fill=0)
        w, o = G.whole(y)
        w[o + M * C + 2] = 3.0
        return "parity ok"

    before = list(guard.STATS.get(__name__, [0, 0, {}]))
    with pytest.raises(guard.Report) as e:
        check_overrun("cpu")
    assert "check_overrun" in str(e.value) and "first at element 2 past its end" in str(e.value)
    after = guard.STATS[__name__]
    assert after[0] == before[0] + 1 and after[1] == before[1] + 1
