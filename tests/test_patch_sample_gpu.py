"""mphsir_patch_sample, scene_store.SceneStore and data.SceneStoreSource on a real MI355X: the checks of tests/patch_sample_ref.py on the
GPU, plus what only the GPU can show -- a level past element 2^31 of the arena, a captured launch pair, a next() without a blocking host
synchronisation, and train.py --scene_dir end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import patch_sample_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib = None
    L._is_emu = False
    L.load()
    assert not L.is_emulated()


@pytest.mark.parametrize("C", [1, 3, 5])
def test_matches_numpy_over_two_pyramids(C):
    R.check_shapes("cuda", C)


def test_aligned_and_elementwise_rows():
    R.check_alignment("cuda")


def test_extremes_in_different_bands_first_and_last_element():
    R.check_extremes("cuda")


def test_nan_constant_and_infinite_windows():
    R.check_nan_and_inf("cuda")


def test_two_calls_are_bitwise_equal():
    R.check_reproducible("cuda")


def test_refusals_launch_nothing():
    R.check_refusals("cuda")


def test_device_side_values_are_clamped_into_the_tables():
    R.check_device_values_are_clamped("cuda")


def test_training_shape_matches_numpy():
    """the shape the source runs at: P = 64, C = 31, B = 32, grid origins of a 256-cropped level and jittered ones"""
    rs = np.random.RandomState(3)
    t = R.Tables([rs.rand(31, 256, 256).astype(np.float32), rs.rand(31, 192, 192).astype(np.float32)], "cuda")
    recs = [(int(l), int(y), int(x)) for l, y, x in zip(rs.randint(0, 2, 32), rs.randint(0, 2, 32) * 64, rs.randint(0, 2, 32) * 64)]
    t.check(recs, 64, label="grid origins")
    t.check([(l, y + 1 + i % 3, x + 1 + i % 5) for i, (l, y, x) in enumerate(recs)], 64, label="jittered origins")


def test_a_captured_pair_follows_the_index_array():
    """the launch pair captured in a graph reads index from device memory: replayed after the array was overwritten it follows the new indices"""
    from mp_hsir_amd import ops
    rs = np.random.RandomState(5)
    levels = R.pyramid([rs.rand(3, 64, 96)], scales=(1, .5))
    t = R.Tables(levels, "cuda")
    recs = R.grid(levels, 16, 16)
    rec = torch.tensor(recs, dtype=torch.int32, device="cuda")
    first, second = [0, 5, 9, 9, len(recs) - 1], [7, 1, len(recs) - 2, 3, 3]
    idx = torch.tensor(first, dtype=torch.int64, device="cuda")
    out = torch.empty((5, 3, 16, 16), device="cuda")
    ws = torch.empty((2 * 5 * 3,), device="cuda")
    ops.patch_sample(t.arena, t.levels, t.levels_host, rec, idx, 3, 16, out=out, workspace=ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.patch_sample(t.arena, t.levels, t.levels_host, rec, idx, 3, 16, out=out, workspace=ws)
    for order in (first, second, first):
        idx.copy_(torch.tensor(order, dtype=torch.int64, device="cuda"))
        out.fill_(-3.0)
        g.replay()
        torch.cuda.synchronize()
        assert R.same_floats(out.cpu().numpy(), R.numpy_patches(t.host, t.level_list, [recs[i] for i in order], 3, 16)), order


def test_a_level_past_two_to_the_31_elements():
    """an arena of 2^31 + 2^16 floats (8.6 GB, allocated, never filled) with one 3 x 32 x 32 level past element 2^31: the offset does not fit
    32 bits, the element arithmetic must be 64-bit"""
    from mp_hsir_amd import ops
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 1024 ** 3:
        pytest.skip("needs 12 GB of free device memory, %.1f GB are free" % (free / 1024 ** 3))
    n = 2 ** 31 + 2 ** 16
    off = 2 ** 31 + 1024
    arena = torch.empty((n,), dtype=torch.float32, device="cuda")
    rs = np.random.RandomState(31)
    lv = rs.rand(3, 32, 32).astype(np.float32)
    arena[off:off + lv.size] = torch.from_numpy(lv.reshape(-1)).cuda()
    levels_host = torch.tensor([[off, 32, 32]], dtype=torch.int64)
    recs = [(0, 0, 0), (0, 16, 16), (0, 5, 3)]
    rec = torch.tensor(recs, dtype=torch.int32, device="cuda")
    got = ops.patch_sample(arena, levels_host.cuda(), levels_host, rec, None, 3, 16).cpu().numpy()
    del arena
    want = R.numpy_patches(lv.reshape(-1), [(0, 32, 32)], recs, 3, 16)
    assert R.same_floats(got, want) and np.isfinite(got).all()


def test_store_records_against_numpy():
    R.check_store_against_numpy("cuda")


def test_source_equals_patch_db_source(tmp_path):
    R.check_source_equals_patch_db_source("cuda", tmp_path)


def test_jittered_windows_stay_inside_and_off_the_mask():
    R.check_jitter("cuda")


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


@pytest.mark.parametrize("jitter", [False, True])
def test_next_makes_no_host_synchronisation(jitter):
    """warmed-up SceneStoreSource.next() calls with fused_degrade=True under torch.cuda.set_sync_debug_mode("error"), across an epoch
    boundary (the permutation upload is a pinned, non-blocking copy).  Were the mode inert on this build, the profiler leg decides."""
    from mp_hsir_amd.data import SceneStoreSource
    st = R.small_store("cuda", patch=16)                    # sr's factor 8 needs N >= 16; the quarter-scale levels (8 x 12, 8 x 8) hold no window
    assert st.levels_host.shape[0] == 4
    src = SceneStoreSource(st, 8, ["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"], "natural_scene", "cuda", seed=5,
                           fused_degrade=True, jitter=jitter)
    for _ in range(2):
        src.next()
    torch.cuda.synchronize()
    steps = src.steps_per_epoch() + 2

    def run():
        for _ in range(steps):
            out = src.next()
        return out
    if _sync_debug_mode_trips():
        torch.cuda.set_sync_debug_mode("error")
        try:
            _, deg, clean, prompt = run()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            _, deg, clean, prompt = run()
        names = [e.name for e in prof.events()]
        bad = [n for n in names if "StreamSynchronize" in n or "DeviceSynchronize" in n or n.startswith("hipMemcpy") and "Async" not in n]
        assert not bad, bad
    assert torch.isfinite(deg).all() and deg.shape == clean.shape == (8, 31, 16, 16) and prompt.shape == (8, 1)


def _train(args):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "mp-hsir_amd", "train.py")] + args
    return subprocess.run(cmd, capture_output=True, text=True)


def test_train_py_trains_from_a_scene_directory(tmp_path):
    """train.py --synthetic 0 --scene_dir on two small .npy scenes (31 x 256 x 256: one crop multiple), patch 32, batch 16, one epoch: the
    logged loss is finite; --db_path beside --scene_dir is refused before anything is built"""
    scenes = tmp_path / "scenes"
    scenes.mkdir()
    rs = np.random.RandomState(1)
    for i in range(2):
        np.save(str(scenes / ("ICVL_%d.npy" % i)), rs.rand(31, 256, 256).astype(np.float32))
    common = ["--synthetic", "0", "--scene_dir", str(scenes), "--epochs", "1", "--allow_surrogate_clip", "1", "--data_type", "natural_scene",
              "--patch_size", "32", "--batch_size", "16", "--log_every", "5"]
    bad = _train(common + ["--db_path", str(tmp_path)])
    assert bad.returncode != 0 and "--db_path and --scene_dir" in bad.stderr + bad.stdout
    r = _train(common + ["--crop_jitter", "1", "--fused_degrade", "1"])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "scene store: 244 records" in r.stdout, r.stdout[-2000:]
    losses = [float(ln.split("train_loss")[1]) for ln in r.stdout.splitlines() if "train_loss" in ln]
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses), r.stdout[-2000:]
