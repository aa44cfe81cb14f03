"""The tiled degradation launch on a real MI355X: the checks of tests/degrade_planes_ref.py through libmphsir.so, the synthesiser beyond
128 x 128 without a host synchronisation, the launch inside a captured graph, and test.py --fused_degrade 1."""
import numpy as np
import pytest
import torch

import degrade_planes_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


@pytest.mark.parametrize("N", [128, 96])
@pytest.mark.parametrize("explicit", [False, True], ids=["generated", "explicit"])
def test_bitwise_equal_to_the_plane_form(N, explicit):
    assert len(P.check_bitwise_against_the_plane_form("cuda", N, explicit)) == len(P.VARIANTS) * 8


@pytest.mark.parametrize("shape,with_sr", [((1, 5, 72, 136), True), ((1, 3, 67, 131), False)], ids=["72x136", "67x131"])
def test_against_the_tensor_functions_beyond_the_plane_form(shape, with_sr):
    P.check_against_the_tensor_functions("cuda", shape, with_sr)


def test_generated_draws_on_a_non_square_plane():
    P.check_generated_draws("cuda")


def test_clean_aug_and_aug_may_be_null():
    P.check_optional_pointers("cuda")


def test_refusals():
    P.check_refusals("cuda")


def test_scene_degrader_modes_0_to_10():
    P.check_scene_degrader("cuda")


def test_blur_modes_dispatch_no_library_convolution():
    """modes 5 and 6 through SceneDegrader: no aten::convolution in a profiler trace (the tensor path's F.conv2d, profiled the same way,
    shows one)"""
    from torch.profiler import ProfilerActivity, profile
    from mp_hsir_amd import degrade as D
    o = P.scene_opts()
    x = torch.rand((1, 9, 72, 136), device="cuda")
    sd = D.SceneDegrader("natural_scene", "cuda", 3)
    for mode in (5, 6):
        sd(x, mode, o)
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        for mode in (5, 6):
            sd(x, mode, o)
    assert not [e.name for e in prof.events() if "convolution" in e.name or "conv2d" in e.name]
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        D.blur(x, D.gaussian_kernel2d(15))
    assert [e.name for e in prof.events() if "convolution" in e.name]


def test_synthesizer_fused_at_192_and_no_host_synchronisation():
    """the per-kind properties, then one warmed-up call under torch.cuda.set_sync_debug_mode("error") per default menu (the mode trips on
    this build: tests/test_degrade_fused_gpu.py shows the tensor path raising under it)"""
    from mp_hsir_amd import degrade as D
    P.check_synthesizer("cuda")
    for data_type, types, C in (("natural_scene", ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"], 31),
                                ("remote_sensing", ["gaussianN", "complexN", "blur", "sr", "inpaint", "haze", "bandmiss"], 100)):
        syn = D.DegradationSynthesizer(data_type, types, "cuda", seed=5, fused=True)
        clean = torch.rand((4, C, 192, 192), device="cuda")
        for _ in range(2):
            syn(clean)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            deg, cl, prompt = syn(clean)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.isfinite(deg).all() and deg.shape == cl.shape == clean.shape and prompt.shape == (4, 1)


def test_launch_inside_a_captured_graph():
    """degrade_planes with a device ordinal captured once and replayed twice: two different cubes, each bitwise the eager launch at its
    ordinal"""
    from mp_hsir_amd import ops
    B, C, H, W = 1, 3, 72, 136
    rs = np.random.RandomState(8)
    x = torch.as_tensor(rs.rand(B, C, H, W).astype(np.float32)).cuda()
    plan = P.make_plan("cuda", B, C, H, W, [("complexN", 1)], None, P.tables(rs, B, C, H, W), np.array([0.3], np.float32))
    ordinal = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = (torch.empty_like(x), torch.empty_like(x))
    ops.degrade_planes(x, plan, seed=5, ordinal=ordinal, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ordinal += 1
        ops.degrade_planes(x, plan, seed=5, ordinal=ordinal, out=out)
    got = []
    for _ in range(2):
        g.replay()
        got.append((int(ordinal), out[0].clone(), out[1].clone()))
    assert [o for o, _, _ in got] == [1, 2] and not torch.equal(got[0][1], got[1][1])
    for o, deg, cl in got:
        want, _ = ops.degrade_planes(x, plan, seed=5, ordinal=o)
        assert torch.equal(deg, want) and torch.equal(cl, x)


def test_test_py_with_fused_degrade():
    """evaluate_quality under --fused_degrade 1 on the tiny net: modes 0-10 score finite, mode 0 twice prints the same scores, mode 11
    ends the run, and a tiled run on a cube that is no multiple of 64 goes through"""
    import importlib
    import model_checks as M
    from golden.cases import TINY_CFG
    T = importlib.import_module("mp_hsir_amd.test")
    net = M.build_net(TINY_CFG, "cuda", torch.float32)
    base = ["--fused_degrade", "1", "--size", "128", "--cubes", "1", "--precision", "f32", "--allow_surrogate_clip", "1"]
    dev = torch.device("cuda")
    scores = {}
    for mode in range(11):
        o = T.build_parser().parse_args(base + ["--mode", str(mode)])
        p, s, sam, n = T.evaluate_quality(o, net, dev)
        assert n >= 1 and np.isfinite(p) and np.isfinite(s) and -1.0 <= s <= 1.0, (mode, p, s, n)
        scores[mode] = (p, s)
    o = T.build_parser().parse_args(base + ["--mode", "0"])
    assert T.evaluate_quality(o, net, dev)[:2] == scores[0], "the same seed and cube ordinal: the same cube, the same scores"
    with pytest.raises(SystemExit, match="Poisson"):
        T.evaluate_quality(T.build_parser().parse_args(base + ["--mode", "11"]), net, dev)
    o = T.build_parser().parse_args(["--fused_degrade", "1", "--size", "136", "--cubes", "1", "--tile", "64", "--tile_overlap", "16", "--mode", "5"])
    p, s, sam, n = T.evaluate_quality(o, net, dev)
    assert n >= 1 and np.isfinite(p) and np.isfinite(s)
