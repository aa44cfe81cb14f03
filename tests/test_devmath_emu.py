"""Device math probes on the CPU: tests/devprobe/probe.hip compiled against tests/hipemu.  The emulator replaces __expf, rsqrtf and fmed3
with libm expressions, so what these cases pin on the CPU is the polynomial, the clamp, the epsilon form and the conversions as the
header spells them; the device's own fast forms are pinned by tests/test_devmath_gpu.py with the same bodies and bars."""
import os
import sys

import pytest
import torch

import devmath_checks as D
import devmath_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "devprobe"))


@pytest.fixture(scope="module")
def lib():
    import build_probe
    return R.load(build_probe.build_emulated())


def test_reference_polynomial_holds_its_bounds():
    """the header's coefficients evaluated in fp64 hold every documented bound: the yardstick the device result is judged against when it
    misses one (a wrong comment and wrong code fail differently)"""
    x = R.gelu_grid(R.N_EMU)
    g, dg = R.poly_gelu64(x)
    msgs, worst = R.gelu16_violations(x, g, dg, fp32_eval=False)
    print("devmath fp64 polynomial: %s" % "; ".join("%s: %s" % kv for kv in worst.items()))
    assert not msgs, "; ".join(msgs)


@pytest.mark.parametrize("policy", R.F16_POLICIES)
def test_gelu16(lib, policy):
    D.check_gelu16(lib, "cpu", R.N_EMU, policy)


def test_gelu32(lib):
    D.check_gelu32(lib, "cpu", R.N_EMU)


def test_exp16(lib):
    D.check_exp16(lib, "cpu", R.N_EMU)


def test_exp32(lib):
    D.check_exp32(lib, "cpu", R.N_EMU)


def test_ln_rstd(lib):
    D.check_rstd(lib, "cpu")


def test_rcp(lib):
    D.check_rcp(lib, "cpu")


@pytest.mark.parametrize("dtype", R.F16_POLICIES)
def test_conversions(lib, dtype):
    D.check_conversions(lib, "cpu", dtype)


def test_nan_report(lib):
    D.report_nan(lib, "cpu")


def test_probe_refuses_bad_arguments(lib):
    x = torch.zeros(4)
    assert lib.mphsir_probe(99, 0, x.data_ptr(), x.data_ptr(), None, 4, 1, None) == -1
    assert lib.mphsir_probe(0, 7, x.data_ptr(), x.data_ptr(), None, 4, 1, None) == -2
    assert lib.mphsir_probe(0, 0, None, x.data_ptr(), None, 4, 1, None) == -2
    assert lib.mphsir_probe(0, 0, x.data_ptr(), x.data_ptr(), None, 0, 1, None) == -2
