"""Device math probes on a real MI355X: tests/devprobe/libmphsir_probe.so (probe.hip built for gfx950 with the product's flags) against
the fp64 references and bars of tests/devmath_ref.py -- the device's own __expf, rsqrtf, fmed3, erff and conversion instructions, which the
emulator replaces and the operation-level tolerances cannot see."""
import os
import sys

import pytest
import torch

import devmath_checks as D
import devmath_ref as R

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "devprobe"))


@pytest.fixture(scope="module")
def lib():
    import build_probe
    # built by __graft_entry__.build() (build_probe.build_device()); never compiled here on GPU time, and never skipped
    assert os.path.exists(build_probe.OUT), "%s is missing: build it with `%s` (or __graft_entry__.build())" % (
        os.path.relpath(build_probe.OUT, build_probe.ROOT), build_probe.RECIPE)
    return R.load(build_probe.OUT)


@pytest.mark.parametrize("policy", R.F16_POLICIES)
def test_gelu16(lib, policy):
    D.check_gelu16(lib, "cuda", R.N_GPU, policy)


def test_gelu32(lib):
    D.check_gelu32(lib, "cuda", R.N_GPU)


def test_exp16(lib):
    D.check_exp16(lib, "cuda", R.N_GPU)


def test_exp32(lib):
    D.check_exp32(lib, "cuda", R.N_GPU)


def test_ln_rstd(lib):
    D.check_rstd(lib, "cuda")


def test_rcp(lib):
    D.check_rcp(lib, "cuda")


@pytest.mark.parametrize("dtype", R.F16_POLICIES)
def test_conversions(lib, dtype):
    D.check_conversions(lib, "cuda", dtype)


def test_nan_report(lib):
    D.report_nan(lib, "cuda")
