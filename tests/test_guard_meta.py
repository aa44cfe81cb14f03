"""The guard covers what it claims to cover: every check of the two check modules runs under it, and every allocation function
that occurs in ops.py / autograd_ops.py is one the proxy wraps -- a future torch.full or new_empty must not slip past unguarded."""
import os
import re

import branch_bwd_checks as BB
import guard
import kernel_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "mp-hsir_amd", f) for f in ("ops.py", "autograd_ops.py")]


def test_every_check_is_wrapped():
    seen = 0
    for mod in (K, BB):
        for name, fn in vars(mod).items():
            if callable(fn) and (name.startswith("check_") or name == "run_block"):
                assert getattr(fn, "__guarded__", False), "%s.%s runs without the guard" % (mod.__name__, name)
                seen += 1
    assert seen >= 48 and BB.run_block.__guarded__ and BB.check_dsa_prologue.__guarded__


def test_inputs_and_buffers_of_the_checks_go_through_the_guard():
    """a tensor reaches the device in the check modules only through rnd / inp / alloc: no allocation with `device=`, no `.to(dev)`,
    `.to(x.device)` or `.cuda()` outside those three helpers -- such a tensor would be handed to a kernel with nothing around it.
    The one exception is an nn.Module moved as a whole (the whole-block checks' parameters), which DESIGN.md names as outside the guard"""
    onto_device = re.compile(r"device\s*=|\.cuda\(|\.to\(\s*(dev\b|_DEV|[\w\.\[\]\"']+\.device)")
    module_move = re.compile(r"\bblk\.to\(dev\)|torch\.nn\.\w+\(.*\)\.to\(dev\)")
    for mod in (K, BB):
        with open(mod.__file__) as f:
            src = f.read()
        if mod is K:
            src = src[:src.index("def rnd(")] + src[src.index("class tok_form"):]
        hits = [ln.strip() for ln in src.splitlines() if onto_device.search(ln) and not module_move.search(ln)]
        assert not hits, hits
    for bad in ("k = torch.tensor([1.0]).to(dev)", "z = torch.zeros(n).to(_DEV[0])", "i = torch.arange(4, device=dev)", "t = x.cpu().to(y.device)",
                "w = torch.randint(0, 4, (8,)).cuda()"):
        assert onto_device.search(bad) and not module_move.search(bad), bad


def test_the_proxy_wraps_every_allocation_function_the_wrappers_use():
    used = {}
    for path in SOURCES:
        with open(path) as f:
            src = f.read()
        for m in re.finditer(r"\btorch\.(\w+)\(", src):
            if m.group(1) in guard.ALLOCATORS:
                used.setdefault(m.group(1), 0)
                used[m.group(1)] += 1
        # the method forms allocate as well and cannot be intercepted through the module global: none may occur
        assert not re.findall(r"\.new_(?:empty|zeros|ones|full|tensor|empty_strided)\(", src), path
    assert used and set(used) <= set(guard.WRAPPED), "allocation functions the guard does not wrap: %s" % sorted(set(used) - set(guard.WRAPPED))
    assert used["empty"] >= 50                   # the search itself still finds them
    for name in guard.WRAPPED:
        assert name in vars(guard.TorchProxy), name


def test_tables_are_explicit():
    for key, val in list(guard.PARTIAL_OK.items()) + list(guard.INPLACE_OK.items()):
        assert isinstance(key, tuple) and len(key) == 2 and all("*" not in str(k) and "?" not in str(k) for k in key)
    for cond, reason in guard.PARTIAL_OK.values():
        assert cond is None or cond.isidentifier()
        assert len(reason) > 40
