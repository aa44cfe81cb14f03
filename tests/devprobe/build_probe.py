"""TEST INFRASTRUCTURE: builds tests/devprobe/probe.hip (element-wise probes of the device math of csrc/mphsir_dev.h) two ways.

    python tests/devprobe/build_probe.py        # -> tests/devprobe/libmphsir_probe.so  and  tests/hipemu/_build/libmphsir_probe_emu.so

build_device(): hipcc for gfx950 with the flags of mp-hsir_amd/build.py (cross-compiles without a GPU; the library is git-ignored and
travels to the GPU box with the tree; __graft_entry__.build() calls it after the product library).  build_emulated(): the same source
against tests/hipemu, the way build_emu.build_selftest() builds selftest.hip.  Neither is ever linked into the product.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mp-hsir_amd", "csrc")
SRC = os.path.join(HERE, "probe.hip")
OUT = os.path.join(HERE, "libmphsir_probe.so")
RECIPE = "python tests/devprobe/build_probe.py"


def _product_build():
    sys.path.insert(0, os.path.join(ROOT, "mp-hsir_amd"))
    try:
        import build as product_build
    finally:
        sys.path.pop(0)
    return product_build


def _emu_build():
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    try:
        import build_emu
    finally:
        sys.path.pop(0)
    return build_emu


def _headers():
    """every header of csrc/ and the C ABI header: whatever mphsir_dev.h includes or comes to include"""
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(ROOT, "include", "mphsir.h")]


def _stale(out, deps):
    return not os.path.exists(out) or os.path.getmtime(out) <= max(os.path.getmtime(d) for d in deps)


def build_device():
    b = _product_build()
    if not _stale(OUT, [SRC, os.path.abspath(__file__), os.path.abspath(b.__file__)] + _headers()):
        return OUT
    cmd = [b.HIPCC] + b.FLAGS + ["-I", CSRC, "-shared", SRC, "-o", OUT]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (SRC, r.stderr[-8000:]))
    return OUT


def build_emulated():
    e = _emu_build()
    out = os.path.join(e.BUILD, "libmphsir_probe_emu.so")
    os.makedirs(e.BUILD, exist_ok=True)
    if not _stale(out, [SRC, os.path.abspath(__file__), os.path.abspath(e.__file__), os.path.join(e.HERE, "include", "hip", "hip_runtime.h")] + _headers()):
        return out
    flags = [f for f in e.FLAGS if "sanitize" not in f and f != "-shared-libasan"]
    r = subprocess.run([e.CXX] + flags + ["-DHIPEMU_IMPLEMENTATION", "-I", CSRC, "-shared", SRC, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipemu probe build failed:\n%s" % r.stderr[-8000:])
    return out


if __name__ == "__main__":
    print(build_device())
    print(build_emulated())
