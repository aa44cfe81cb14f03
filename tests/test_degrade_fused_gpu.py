"""The fused degradation launch on a real MI355X: the checks of tests/degrade_fused_ref.py through libmphsir.so (a sample of the emulator
file's parametrisation), DegradationSynthesizer(fused=True) without a host synchronisation, and plan + launch inside a captured graph."""
import pytest
import torch

import degrade_fused_ref as R

pytestmark = pytest.mark.gpu
NATURAL = ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss", "motion_blur"]
REMOTE = ["gaussianN", "complexN", "blur", "sr", "inpaint", "haze", "bandmiss", "circle_blur"]


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


def test_reference_fixtures_with_explicit_draws():
    """every kind of the fixture at aug 0 against the reference's output; the modes: the two flips, a quarter turn and its flip"""
    R.check_fixtures("cuda", modes=(1, 2, 4, 7))


def test_fused_equals_the_tensor_path_on_one_mixed_batch():
    R.check_mixed_batch("cuda")


def test_smallest_planes_and_the_largest_stencil():
    R.check_small_planes("cuda", shapes=((2, 3, 20), (1, 31, 16)))
    R.check_blur21_at_64("cuda")
    R.check_largest_plane("cuda")


def test_generated_draws():
    R.check_kernel_philox_known_answer("cuda")
    R.check_generated_uniforms("cuda")
    R.check_generated_normal("cuda")


def test_generated_mode_properties_and_nan():
    R.check_generated_properties("cuda")
    R.check_nan_poisons_its_dependents("cuda")


def test_refusals():
    R.check_refusals("cuda")


def test_synthesizer_fused():
    R.check_synthesizer_fused("cuda")


def _sync_debug_mode_trips():
    """does torch.cuda.set_sync_debug_mode("error") raise on a blocking read-back on this build?"""
    x = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("data_type,types,C", [("natural_scene", NATURAL, 31), ("remote_sensing", REMOTE, 100)])
def test_fused_call_makes_no_host_synchronisation(data_type, types, C):
    """a warmed-up DegradationSynthesizer(fused=True) call under torch.cuda.set_sync_debug_mode("error"), both default menus (plus the
    menus' other blur).  The mode trips on this ROCm build (torch 2.10: .item() raises); the tensor path, run the same way, raises -- it
    is what the mode is there to catch.  Were the mode inert, the profiler leg below decides instead."""
    from mp_hsir_amd import degrade as D
    syn = D.DegradationSynthesizer(data_type, types, "cuda", seed=5, fused=True)
    clean = torch.rand((8, C, 64, 64), device="cuda")
    for _ in range(2):
        syn(clean)
    torch.cuda.synchronize()
    if _sync_debug_mode_trips():
        torch.cuda.set_sync_debug_mode("error")
        try:
            deg, cl, prompt = syn(clean)
            with pytest.raises(RuntimeError):
                D.DegradationSynthesizer(data_type, types, "cuda", seed=5)(clean)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            deg, cl, prompt = syn(clean)
        names = [e.name for e in prof.events()]
        bad = [n for n in names if "StreamSynchronize" in n or "DeviceSynchronize" in n or n.startswith("hipMemcpy") and "Async" not in n]
        assert not bad, bad
    assert torch.isfinite(deg).all() and deg.shape == cl.shape == clean.shape and prompt.shape == (8, 1)


def test_plan_and_launch_inside_a_captured_graph():
    """plan + launch captured once and replayed twice: the batch ordinal is a device scalar that the captured increment advances and the
    launch reads, so the two replays give two different, finite batches"""
    from mp_hsir_amd import degrade as D
    syn = D.DegradationSynthesizer("natural_scene", NATURAL, "cuda", seed=11, fused=True)
    clean = torch.rand((8, 31, 64, 64), device="cuda")
    for _ in range(2):
        syn(clean)
    torch.cuda.synchronize()
    before = int(syn._ordinal)
    g = torch.cuda.CUDAGraph()
    g.register_generator_state(syn.d.gen)
    with torch.cuda.graph(g):
        deg, cl, prompt = syn(clean)
    outs = []
    for _ in range(2):
        g.replay()
        outs.append((deg.clone(), cl.clone(), prompt.clone(), int(syn._ordinal)))
    assert [o[3] for o in outs] == [before + 1, before + 2], "every replay advances the ordinal by one"
    assert all(torch.isfinite(o[0]).all() for o in outs) and not torch.equal(outs[0][0], outs[1][0])
    for d_, c_, p_, _ in outs:
        assert torch.equal(c_.flatten(1).sort(dim=1).values, clean.flatten(1).sort(dim=1).values) and int(p_.max()) < len(NATURAL)
