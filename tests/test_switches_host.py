"""The environment variables the product reads are the six measurement / diagnosis switches of the table in tools/README.md, nothing
else: which kernel path runs follows from dtype and sizes, not from the environment.  Host only, nothing is launched."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mp-hsir_amd")
SWITCHES = {"MPHSIR_SIDE_BRANCH", "MPHSIR_PROMPT_SIDE", "MPHSIR_DW_SIDE", "MPHSIR_LOG_SEGS", "MPHSIR_LIB_AB", "MPHSIR_DIAG_SKIP"}
_READ = re.compile(r"""(?:os\.environ(?:\.get\s*\(|\s*\[)|os\.getenv\s*\(|\bgetenv\s*\()\s*["'](MPHSIR_\w+)["']""")


def _environment_reads():
    files = [p for p in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)]
    files += [p for p in glob.glob(os.path.join(PKG, "csrc", "**", "*"), recursive=True) if os.path.isfile(p)]
    found = {}
    for path in files:
        with open(path, errors="replace") as f:
            for name in _READ.findall(f.read()):
                found.setdefault(name, []).append(os.path.relpath(path, ROOT))
    return found


def test_the_product_reads_exactly_the_documented_switches():
    found = _environment_reads()
    assert set(found) == SWITCHES, {n: found[n] for n in set(found) ^ SWITCHES if n in found} or SWITCHES - set(found)
    with open(os.path.join(ROOT, "tools", "README.md")) as f:
        rows = [line for line in f if line.startswith("| `MPHSIR_")]
    documented = {re.match(r"\| `(MPHSIR_\w+)`", line).group(1) for line in rows}
    assert documented == SWITCHES, documented ^ SWITCHES


def _import_ops(value):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MPHSIR_")}
    env["MPHSIR_DW_SIDE"] = value
    code = "import sys; sys.path.insert(0, %r); from mp_hsir_amd import ops; print('DW_SIDE', ops.DW_SIDE)" % ROOT
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)


def test_dw_side_takes_0_and_2_only():
    r = _import_ops("1")
    assert r.returncode != 0 and "MPHSIR_DW_SIDE must be 0" in r.stderr and "or 2" in r.stderr, r.stderr[-2000:]
    r = _import_ops("0")
    assert r.returncode == 0 and r.stdout.split() == ["DW_SIDE", "0"], (r.stdout, r.stderr[-2000:])
