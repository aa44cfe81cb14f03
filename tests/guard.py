"""TEST INFRASTRUCTURE: guard bands and poisoned outputs around the kernel parity checks.

A parity check compares what a kernel returns with a reference.  Two things it cannot see: a store or a load outside the tensors
(the caching allocator's slack swallows it) and an element the kernel never writes (the recycled block still holds the previous
call's correct answer).  While a `Guard` is active

  * every tensor `mp_hsir_amd.ops` / `autograd_ops` allocate (torch.empty / zeros / empty_like / zeros_like) and every input the
    checks draw (kernel_checks.rnd, kernel_checks.alloc) is a view in the middle of a larger buffer, with a sentinel band on both
    sides;
  * the interior of an `empty` is prefilled with a NaN pattern ("never written");
  * each input keeps the CPU master it was generated from (and a twin of it on the device, so that the comparison after the check
    joins the one batched reduction).

`verify()` synchronizes once and reports damaged bands (site, side, first damaged element, count), `empty` interiors that still hold
prefill (unless listed in PARTIAL_OK), inputs that changed (unless listed in INPLACE_OK) and -- through the checks' own rel-L2
assertions -- NaN that an out-of-range read pulled into a result.

The product code is not touched: the module global `torch` of ops / autograd_ops is swapped for a proxy for the duration of one check.
The guard adds fills, compares and one synchronize; it launches nothing from the library."""
import atexit
import functools
import linecache
import os
import re
import sys

import torch as _torch

BAND_MIN = 4096             # bytes
BAND_ROWS = 128             # the largest token tile in csrc/ : a whole tile past the end still lands in the band
BAND_MAX = 1 << 20
ALIGN = 256                 # keeps the interior 16-byte aligned (every entry point MPHSIR_REQUIREs that) for any band size
INPUT_CHECK_MAX = 64 << 20  # inputs up to this many bytes are compared bitwise with their CPU master

# the allocation functions the proxy wraps; tests/test_guard_meta.py checks that ops.py / autograd_ops.py use no other
WRAPPED = ("empty", "zeros", "empty_like", "zeros_like")
# every torch function that hands out fresh memory a kernel could be pointed at
ALLOCATORS = WRAPPED + ("ones", "full", "ones_like", "full_like", "empty_strided", "rand", "randn", "rand_like", "randn_like",
                        "empty_permuted", "zeros_strided")

# ---- patterns: written and compared through an integer view of the element width ------------------------------------------------
# floats: input bands and the prefill are NaNs in every format of that width (16 bit: bf16 AND fp16); the three roles never share a
# pattern, so a row copied from an input band into an output band (NaN payloads propagate; a cast copy moves bits) is damage.
_INT = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}
_IN_NAN = {2: 0x7FC5, 4: 0x7FC01A2B, 8: 0x7FF800001A2B3C4D}
_PREFILL_NAN = {2: 0xFFD3, 4: 0xFFC5D3E7, 8: 0xFFF80000D3E70001}
_IN_BYTE, _PREFILL_BYTE = 0x7A, 0xD3


def _signed(v, size):
    bits = 8 * size
    v &= (1 << bits) - 1
    return v - (1 << bits) if size > 1 and v >= 1 << (bits - 1) else v


def _rep(byte, size):
    return int.from_bytes(bytes([byte]) * size, "little")


def input_pattern(dtype):
    size = dtype.itemsize
    return _signed(_IN_NAN[size] if dtype.is_floating_point and size in _IN_NAN else _rep(_IN_BYTE, size), size)


def prefill_pattern(dtype):
    size = dtype.itemsize
    return _signed(_PREFILL_NAN[size] if dtype.is_floating_point and size in _PREFILL_NAN else _rep(_PREFILL_BYTE, size), size)


def output_pattern(dtype, counter, side):
    """top nibble 0xB (no input band or prefill pattern has it), the rest a per-allocation, per-side counter: a copy from one band to
    another cannot reproduce a sentinel.  Floats of every width read it as a finite negative number."""
    size = dtype.itemsize
    n = 2 * counter + side
    if size == 1:
        return 0xB0 | (n % 15)
    bits = 8 * size
    body = (n * 0x9E3779B1 + 0x5D) % (1 << (bits - 4))
    return _signed((0xB << (bits - 4)) | body, size)


def band_bytes(shape, dtype):
    pitch = (shape[-1] if len(shape) else 1) * dtype.itemsize
    b = min(max(BAND_MIN, BAND_ROWS * pitch), BAND_MAX)
    return (b + ALIGN - 1) // ALIGN * ALIGN


# ---- what may stay unwritten, what may change ---------------------------------------------------------------------------------
# (ops function, assigned name) -> who never reads the unwritten elements.  No wildcards: a new partly written buffer is a report
# until somebody has looked at its readers.
PARTIAL_OK = {
    # (ops function, name): (local of that function that must be true for the entry to hold, or None; who never reads the rest)
    ("MultiCopy.__init__", "self.host"): (None, "pointer-table ring of `capacity` rows: a call fills rows [0, n) and mphsir_multi_copy(table, n, ...) "
                                                "reads those n (include/mphsir.h, mphsir_multi_copy)"),
    ("MultiCopy.__init__", "self.dev"): (None, "the device copy of the same table: dv[:n].copy_(h[:n]), the launch reads n rows"),
    ("MultiCopy.__init__", "self.for_capture"): (None, "table pairs set aside for calls under graph capture; eager calls never touch them"),
    ("spectral_fold_bwd", "W2"): ("w2_blocks", "mphsir_fold_bwd_args.w2_blocks (include/mphsir.h): only the entries mphsir_spectral_dqkv_bwd reads are written, "
                                               "per head the columns [h hd, (h+1) hd) and [C + h hd, C + (h+1) hd) of its q and k rows; the only consumer of "
                                               "that W2 is that launch (autograd_ops.channel_attention_bwd_self / _cross), and under the guard the rest is "
                                               "NaN, so a read of it would fail the parity assertions.  With w2_blocks = 0 the whole matrix must be written"),
}

# (check function, rnd seed) -> the line of include/mphsir.h that lets the kernel change that input.  None today: every check hands
# the in-place entry points (the AdamW steps, multi_copy's destinations) clones or buffers of its own.
INPLACE_OK = {}

# on by default; MPHSIR_TEST_GUARD=0 runs the checks bare (to see what the parity assertions notice on their own)
ENABLED = os.environ.get("MPHSIR_TEST_GUARD", "1") != "0"
_SRC = ("ops.py", "autograd_ops.py")
_ACTIVE = [None]
STATS = {}                  # check module -> [guarded checks, guarded allocations, {reason: allocations passed through unguarded}]
BARE = {}                   # check module -> checks that ran without the guard (MPHSIR_TEST_GUARD=0)


def active():
    return _ACTIVE[0]


# ---- recorder (tests/test_emu_schedules.py) -------------------------------------------------------------------------------------
# Inactive by default.  While `recording()` is active, every tensor a check compares -- kernel_checks.close's `got`, both sides of a
# torch.equal -- and, when a guarded check ends, every non-input buffer the guard handed out (what ops.py allocated for a kernel to
# write: results, workspaces, partials) is appended to a list as a CPU clone.  Nothing is asserted here and no comparison changes: two
# runs of the same check under two schedules of the emulator are compared record by record, bit by bit, by the caller.
_RECORD = [None]


def record(tensor, what=""):
    if _RECORD[0] is not None and isinstance(tensor, _torch.Tensor):
        _RECORD[0].append((what, tensor.detach().cpu().contiguous().clone()))


class recording:
    def __enter__(self):
        assert _RECORD[0] is None, "recording() does not nest"
        self.saved_equal = _torch.equal
        real = self.saved_equal

        def equal(a, b):
            record(a, "equal lhs")
            record(b, "equal rhs")
            return real(a, b)
        _torch.equal = equal
        _RECORD[0] = []
        return _RECORD[0]

    def __exit__(self, *exc):
        _torch.equal = self.saved_equal
        _RECORD[0] = None
        return False


def first_difference(a, b):
    """None when two recorded tensors hold the same bits (a NaN equals itself), else a description of the first differing element"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape / dtype %s %s against %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    if a.numel() == 0:
        return None
    ia, ib = a.reshape(-1).view(_torch.uint8), b.reshape(-1).view(_torch.uint8)
    if _torch.equal(ia, ib):
        return None
    flat = int((ia != ib).nonzero()[0]) // a.element_size()
    idx, rest = [], flat
    for n in reversed(a.shape):
        idx.append(rest % n)
        rest //= n
    n_diff = int((ia != ib).reshape(-1, a.element_size()).any(1).sum())
    return "%d of %d elements differ, first at index %s (flat %d): %r against %r" % (
        n_diff, a.numel(), tuple(reversed(idx)), flat, a.reshape(-1)[flat].item(), b.reshape(-1)[flat].item())


class Report(AssertionError):
    pass


class _Buf:
    __slots__ = ("raw", "view", "dtype", "role", "site", "band", "nbytes", "pat", "prefill", "master", "seed", "counter", "partial_ok", "twin")


def _site():
    """(function, assigned name, line, file) of the allocation: the innermost frame in ops.py / autograd_ops.py that is not a
    comprehension; outside them (a check's own buffer) the innermost frame of the check module"""
    frames = []
    f = sys._getframe(1)
    while f is not None:
        frames.append(f)
        f = f.f_back
    pick = None
    for f in frames:
        base = f.f_code.co_filename.rsplit("/", 1)[-1]
        if base in _SRC and not f.f_code.co_name.startswith("<"):
            pick = f
            break
    if pick is None:
        for f in frames:
            base = f.f_code.co_filename.rsplit("/", 1)[-1]
            if (base.endswith("_checks.py") or base.startswith("test_")) and f.f_code.co_name not in ("alloc", "rnd"):
                pick = f
                break
    if pick is None:
        return ("?", "?", 0, "?", None)
    key = (pick.f_code, pick.f_lineno)
    hit = _SITES.get(key)
    if hit is None:
        name = pick.f_code.co_name
        if "self" in pick.f_code.co_varnames[:1]:          # tracebacks of this Python carry no qualified names
            name = type(pick.f_locals["self"]).__name__ + "." + name
        line = linecache.getline(pick.f_code.co_filename, pick.f_lineno)
        m = re.match(r"\s*([\w\.\[\]:, ]+?)\s*=[^=]", line)
        lhs = m.group(1) if m else "<expr>"
        hit = _SITES[key] = (name, lhs, pick.f_lineno, pick.f_code.co_filename.rsplit("/", 1)[-1])
    return hit + (pick,)


_SITES = {}


class Guard:
    def __init__(self, device, check_name="?", module="?"):
        self.device = _torch.device(device)
        self.check_name, self.module = check_name, module
        self.bufs = []
        self.counter = 0
        self._last = None
        self.skipped = {}           # reason -> allocations that went to the real allocator, without bands

    def skip(self, reason):
        """an allocation the guard hands to the real allocator: counted, and printed with the module's line at exit"""
        self.skipped[reason] = self.skipped.get(reason, 0) + 1
        return None

    # -- allocation -------------------------------------------------------------------------------------------------------------
    def alloc(self, shape, dtype, device, role, fill=None, strides=None, master=None, seed=None):
        """a view of `shape` in the middle of a larger buffer from the real torch.empty.  role: "input" | "output" | "workspace";
        fill: None = prefill ("never written"), a number = that value (zeros / ones / full), "keep" = the caller writes it (inputs)"""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        size = dtype.itemsize
        if strides is None:
            span = n
        else:
            span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if n else 0
        if n == 0 or size not in _INT:
            self.skip("no elements" if n == 0 else "element size %d" % size)
            return _torch.empty(shape, dtype=dtype, device=device)
        b = _Buf()
        b.band, b.nbytes, b.dtype, b.role, b.counter = band_bytes(shape, dtype), span * size, dtype, role, self.counter
        self.counter += 1
        b.raw = _torch.empty((2 * b.band + b.nbytes,), dtype=_torch.uint8, device=device)
        assert b.raw.data_ptr() % 16 == 0
        ints = _INT[size]
        if role == "input":
            b.pat = (input_pattern(dtype), input_pattern(dtype))
        else:
            b.pat = (output_pattern(dtype, b.counter, 0), output_pattern(dtype, b.counter, 1))
        b.raw[:b.band].view(ints).fill_(b.pat[0])
        b.raw[b.band + b.nbytes:].view(ints).fill_(b.pat[1])
        flat = b.raw[b.band:b.band + b.nbytes].view(dtype)
        b.prefill = None
        if fill is None:
            b.prefill = prefill_pattern(dtype)
            b.raw[b.band:b.band + b.nbytes].view(ints).fill_(b.prefill)
        elif fill != "keep":
            flat.fill_(fill)
        b.view = flat.view(shape) if strides is None else flat.as_strided(shape, tuple(strides))
        b.master, b.seed, b.twin = master, seed, None
        name, lhs, line, fname, frame = _site()
        names = [s.strip() for s in lhs.split(",")]
        idx = 0
        if len(names) > 1:      # `u, dt_ = torch.empty_like(du), torch.empty_like(t)`: the k-th allocation of one execution of that line
            if self._last is not None and self._last[:3] == (name, line, fname) and self._last[3] + 1 < len(names):
                idx = self._last[3] + 1
            lhs = names[idx]
        self._last = (name, line, fname, idx)
        b.site = (name, lhs, line, fname)
        ok = PARTIAL_OK.get((name, lhs))
        b.partial_ok = ok is not None and (ok[0] is None or bool(frame.f_locals.get(ok[0])))
        self.bufs.append(b)
        return b.view

    def whole(self, view):
        """(the whole buffer of a guarded tensor -- band, interior, band -- as a flat tensor of its dtype, element offset of the interior):
        for tests of the harness itself, whose fake kernels stray on purpose and must stay inside memory the test owns"""
        for b in self.bufs:
            if b.view is view:
                return b.raw.view(b.dtype), b.band // b.dtype.itemsize
        raise KeyError("not a tensor of this guard")

    def input(self, master, seed=None):
        """a guarded copy of the CPU tensor `master` on the guard's device; the master is kept for the bitwise comparison"""
        master = master.contiguous()
        v = self.alloc(master.shape, master.dtype, self.device, "input", fill="keep", master=master, seed=seed)
        v.copy_(master)
        b = self.bufs[-1]
        # a twin of the master on the device (a plain allocation of its own, nowhere near the guarded tensor): the comparison after
        # the check joins the one batched reduction instead of one device-to-host copy per input; the CPU master stays the reference
        # of the detailed report
        b.twin = v.detach().clone() if b.nbytes <= INPUT_CHECK_MAX else None
        return v

    # -- verification -----------------------------------------------------------------------------------------------------------
    def verify(self):
        """[] or a list of findings (strings).  One synchronize; the per-buffer counts are reduced on the device and fetched at once,
        details only for what is damaged."""
        if self.device.type == "cuda":
            _torch.cuda.synchronize(self.device)
        if not self.bufs:
            return []
        counts = []
        zero = _torch.zeros((), dtype=_torch.int64, device=self.bufs[0].raw.device)
        for b in self.bufs:
            ints = _INT[b.dtype.itemsize]
            counts.append((b.raw[:b.band].view(ints) != b.pat[0]).sum())
            counts.append((b.raw[b.band + b.nbytes:].view(ints) != b.pat[1]).sum())
            if b.prefill is not None:
                counts.append((b.raw[b.band:b.band + b.nbytes].view(ints) == b.prefill).sum())
            else:
                counts.append(zero)
            if b.twin is not None and (self.check_name, b.seed) not in INPLACE_OK:
                counts.append((b.view.detach().view(ints) != b.twin.view(ints)).sum())
            else:
                counts.append(zero)
        counts = _torch.stack(counts).cpu().tolist()
        out = []
        for i, b in enumerate(self.bufs):
            before, after, stale, changed = counts[4 * i:4 * i + 4]
            size = b.dtype.itemsize
            ints = _INT[size]
            where = "%s:%d %s -> %s %s%s" % (b.site[3], b.site[2], b.site[0], b.site[1], str(b.dtype).replace("torch.", ""), list(b.view.shape))
            if before:
                band = b.raw[:b.band].view(ints)
                first = int((band != b.pat[0]).nonzero()[0])
                out.append("BAND %s [%s]: %d elements damaged BEFORE the tensor, first at element %d (%d before its start), holds 0x%x"
                           % (where, b.role, before, first - band.numel(), band.numel() - first, int(band[first]) & ((1 << 8 * size) - 1)))
            if after:
                band = b.raw[b.band + b.nbytes:].view(ints)
                first = int((band != b.pat[1]).nonzero()[0])
                out.append("BAND %s [%s]: %d elements damaged AFTER the tensor, first at element %d past its end, holds 0x%x"
                           % (where, b.role, after, first, int(band[first]) & ((1 << 8 * size) - 1)))
            if stale and not b.partial_ok:
                inner = b.raw[b.band:b.band + b.nbytes].view(ints)
                first = int((inner == b.prefill).nonzero()[0])
                out.append("PREFILL %s: %d of %d elements never written, first at flat element %d%s"
                           % (where, stale, inner.numel(), first, _unravel(first, b.view)))
            if changed:
                now = b.view.detach().cpu().contiguous().view(ints).reshape(-1)
                was = b.master.view(ints).reshape(-1)
                diff = now != was
                nd = int(diff.sum())
                if nd:
                    first = int(diff.nonzero()[0])
                    out.append("INPUT %s (seed %s): %d elements changed, first at flat element %d%s"
                               % (where, b.seed, nd, first, _unravel(first, b.view)))
                else:
                    out.append("INPUT %s (seed %s): equals its CPU master, but its device twin differs in %d elements (a stray store hit the twin)"
                               % (where, b.seed, changed))
        return out

    def release(self):
        self.bufs = []


def _unravel(flat, view):
    if not view.is_contiguous() or view.dim() < 2:
        return ""
    idx = []
    for s in reversed(view.shape):
        idx.append(flat % s)
        flat //= s
    return " = index %s" % (tuple(reversed(idx)),)


# ---- the proxy ----------------------------------------------------------------------------------------------------------------
class TorchProxy:
    """forwards every attribute to torch except the allocation functions ops.py / autograd_ops.py use"""

    def __init__(self, guard):
        object.__setattr__(self, "_g", guard)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    def _new(self, size, kw, fill):
        if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
            size = tuple(size[0])
        dtype = kw.pop("dtype", None) or _torch.get_default_dtype()
        device = _torch.device(kw.pop("device", None) or "cpu")
        if device.type != self._g.device.type:
            return self._g.skip("a %s tensor under a %s guard" % (device.type, self._g.device.type))
        if kw:              # pin_memory, requires_grad, memory_format, ...: the real call knows what they mean, the guard does not
            return self._g.skip("keyword " + " ".join(sorted(kw)))
        return self._g.alloc(size, dtype, device, "output", fill=fill)

    def empty(self, *size, **kw):
        t = self._new(size, dict(kw), None)
        return t if t is not None else _torch.empty(*size, **kw)

    def zeros(self, *size, **kw):
        t = self._new(size, dict(kw), 0)
        return t if t is not None else _torch.zeros(*size, **kw)

    def _like(self, x, kw, fill):
        kw = dict(kw)
        dtype = kw.pop("dtype", None) or x.dtype
        device = _torch.device(kw.pop("device", None) or x.device)
        if device.type != self._g.device.type:
            return self._g.skip("a %s tensor under a %s guard" % (device.type, self._g.device.type))
        if x.layout != _torch.strided:
            return self._g.skip("layout %s" % x.layout)
        if x.numel() == 0:
            return self._g.skip("no elements")
        # the strides the real call gives (a dense permuted tensor keeps its permutation), asked of the meta device
        meta = _torch.empty_like(_torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device="meta"), dtype=dtype, **kw)
        return self._g.alloc(x.shape, dtype, device, "output", fill=fill, strides=None if meta.is_contiguous() else meta.stride())

    def empty_like(self, x, **kw):
        t = self._like(x, kw, None)
        return t if t is not None else _torch.empty_like(x, **kw)

    def zeros_like(self, x, **kw):
        t = self._like(x, kw, 0)
        return t if t is not None else _torch.zeros_like(x, **kw)


class guarded_ops:
    """context manager: a Guard on `device`, the proxy installed as the module global `torch` of ops and autograd_ops; restored on
    exit, also on exception.  Nested use (a check that calls another check) joins the active guard."""

    def __init__(self, device, check_name="?", module="?"):
        self.args = (device, check_name, module)
        self.guard = None
        self.outer = False

    def __enter__(self):
        if _ACTIVE[0] is not None:
            self.outer, self.guard = True, _ACTIVE[0]
            return self.guard
        dev = _torch.device(self.args[0])
        if dev.type == "cuda":
            assert not _torch.cuda.is_current_stream_capturing(), "the guard does not run under graph capture"
        from mp_hsir_amd import autograd_ops, ops
        self.guard = Guard(*self.args)
        self.mods = (ops, autograd_ops)
        self.saved = [m.torch for m in self.mods]
        proxy = TorchProxy(self.guard)
        for m in self.mods:
            m.torch = proxy
        _ACTIVE[0] = self.guard
        return self.guard

    def __exit__(self, *exc):
        if self.outer:
            return False
        _ACTIVE[0] = None
        for m, t in zip(self.mods, self.saved):
            m.torch = t
        return False


def guarded(fn):
    """decorator of a check(dev, ...): activates the guard, runs the check, verifies, fails the check with the report; return values
    pass through; re-entrant"""
    @functools.wraps(fn)
    def run(dev, *a, **kw):
        if _ACTIVE[0] is not None:
            return fn(dev, *a, **kw)
        if not ENABLED:
            BARE[fn.__module__] = BARE.get(fn.__module__, 0) + 1
            return fn(dev, *a, **kw)
        with guarded_ops(dev, fn.__name__, fn.__module__) as g:
            try:
                res = fn(dev, *a, **kw)
                report = g.verify()
                if _RECORD[0] is not None:
                    for b in g.bufs:
                        if b.role != "input":
                            record(b.view, "%s:%d %s -> %s" % (b.site[3], b.site[2], b.site[0], b.site[1]))
            finally:
                st = STATS.setdefault(fn.__module__, [0, 0, {}])
                st[0] += 1
                st[1] += len(g.bufs)
                for why, k in g.skipped.items():
                    st[2][why] = st[2].get(why, 0) + k
                g.release()
        if report:
            more = ["... and %d more" % (len(report) - 12)] if len(report) > 12 else []
            raise Report("%s: the guard found %d problem(s) the parity assertions did not:\n  %s" % (fn.__name__, len(report), "\n  ".join(report[:12] + more)))
        return res
    run.__guarded__ = True
    return run


@atexit.register
def _say():
    """one line per check module at the end of the run: "the guard was active" is visible in the log, not assumed"""
    for mod, (checks, allocs, skipped) in sorted(STATS.items()):
        rest = ", ".join("%d x %s" % (k, why) for why, k in sorted(skipped.items())) or "none"
        sys.__stderr__.write("guard: %s: %d guarded checks, %d guarded allocations; passed through without bands: %s\n" % (mod, checks, allocs, rest))
    for mod, n in sorted(BARE.items()):
        sys.__stderr__.write("guard: DISABLED (MPHSIR_TEST_GUARD=0): %d checks of %s ran bare\n" % (n, mod))
