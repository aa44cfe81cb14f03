"""The host logic of mp-hsir_amd/scene_store.py on the CPU: the zoom-level matrices and mask levels against scipy.ndimage.zoom, the band
adaptation against scipy.interpolate.interp1d, the end-to-end fixture tests/golden/scene_store.npz (written by the reference's own
Data2Volume: tests/golden/make_scene_store_golden.py), file loading, and the flags.  Patches go through the emulated kernels.

Bounds.  Matrices, float64 before the fp32 cast: 1e-10 absolute on data in [0, 1] (measured: 1.9e-15 on the shapes below).  Fixture: the
level is cast to fp32 (half an ulp of a value below 1: 3e-8, on p, min and max) and the patch takes two fp32 subtractions and one division
(half an ulp of the result each) -- a few 1e-7; measured maximum on the CPU 1.79e-7, the bar is 4 x that = 7.16e-7 (cap 2e-6)."""
import os

import numpy as np
import pytest
import torch
from scipy.interpolate import interp1d
from scipy.ndimage import zoom

from emu import bind_emulator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_store.npz")
MATRIX_BAR = 1e-10
FIXTURE_MEASURED = 1.79e-7
FIXTURE_BAR = 4 * FIXTURE_MEASURED
assert FIXTURE_BAR <= 2e-6


@pytest.fixture(scope="module", autouse=True)
def _emu():
    bind_emulator()


@pytest.mark.parametrize("shape", [(3, 256, 384), (2, 128, 130)])
@pytest.mark.parametrize("s", [0.5, 0.25])
def test_level_matrices_match_scipy_zoom(shape, s):
    from mp_hsir_amd import scene_store as S
    x = np.random.RandomState(shape[1]).rand(*shape)
    want = zoom(x, (1, s, s))
    got = S.zoom_level(torch.from_numpy(x), s).numpy()
    err = np.abs(got - want).max()
    print("zoom %s at %s: max |d| %.3g (bar %.1g)" % (shape, s, err, MATRIX_BAR))
    assert got.shape == want.shape and got.dtype == np.float64 and err <= MATRIX_BAR


@pytest.mark.parametrize("shape", [(256, 384), (128, 130), (77, 53)])
@pytest.mark.parametrize("s", [0.5, 0.25])
def test_mask_levels_equal_scipy_zoom_order_0(shape, s):
    from mp_hsir_amd import scene_store as S
    m = np.random.RandomState(shape[0]).rand(*shape) > 0.7
    assert np.array_equal(S.zoom_mask(m, s), zoom(m, (s, s), order=0))


def test_the_last_sample_of_width_384_is_zero_as_in_scipy():
    """(m - 1) * ((n - 1) / (m - 1)) rounds to just above n - 1 at n = 384, s = 0.5; scipy's mode 'constant' then returns 0 for the last
    column, and so must the level (the reference's patches hold that column)"""
    from mp_hsir_amd import scene_store as S
    x = np.random.RandomState(0).rand(1, 256, 384) + 1.0
    want = zoom(x, (1, .5, .5))
    assert np.all(want[:, :, -1] == 0.0) and np.all(want[:, :, -2] > 0.5)
    got = S.zoom_level(torch.from_numpy(x), .5).numpy()
    assert np.all(got[:, :, -1] == 0.0) and np.abs(got - want).max() <= MATRIX_BAR


@pytest.mark.parametrize("name", ["PaviaC", "WDC", "Houston"])
def test_band_matrix_matches_interp1d(name):
    """PaviaC (430-860) extrapolates at both ends, Houston (364-1046) at neither, WDC (400-2400) uses a fraction of its bands"""
    from mp_hsir_amd import scene_store as S
    lo, hi, n = S.REMOTE_SENSING_BANDS[name]
    d = np.random.RandomState(n).rand(n, 6, 7)
    want = interp1d(np.linspace(lo, hi, n), d, axis=0, kind="linear", fill_value="extrapolate")(np.linspace(400, 1000, 100))
    M = S.band_matrix(lo, hi, n)
    assert M.shape == (100, n) and (np.count_nonzero(M, axis=1) <= 2).all() and np.allclose(M.sum(axis=1), 1.0, atol=1e-12)
    if name == "PaviaC":
        assert M[0].min() < 0 and M[-1].min() < 0, "both ends extrapolate"
    err = np.abs(np.einsum("tn,nhw->thw", M, d) - want).max()
    print("%s: max |d| %.3g" % (name, err))
    assert err <= MATRIX_BAR


def test_remote_sensing_store_adapts_bands_by_source_name():
    from mp_hsir_amd import scene_store as S
    rs = np.random.RandomState(4)
    cube = rs.rand(102, 16, 16)
    st = S.SceneStore([cube], "remote_sensing", "cpu", patch=8, scales=(1,), strides=(8,), crop_multiple=16, sources=["PaviaC_3.mat"])
    assert st.C == 100 and len(st) == 4 and st.names == ["PaviaC_3.mat"] * 4
    want = np.einsum("tn,nhw->thw", S.band_matrix(430, 860, 102), cube).astype(np.float32)
    assert np.abs(st.arena.numpy().reshape(100, 16, 16) - want).max() <= 1e-6
    with pytest.raises(ValueError, match="none of"):
        S.SceneStore([cube], "remote_sensing", "cpu", patch=8, scales=(1,), strides=(8,), crop_multiple=16, sources=["Nowhere_1.mat"])
    with pytest.raises(ValueError, match="102"):
        S.SceneStore([rs.rand(103, 16, 16)], "remote_sensing", "cpu", patch=8, scales=(1,), strides=(8,), crop_multiple=16, sources=["PaviaC_1.mat"])


def test_natural_scene_store_interpolates_to_31_bands():
    from mp_hsir_amd import degrade, scene_store as S
    cube = np.random.RandomState(5).rand(9, 16, 16)
    st = S.SceneStore([cube], "natural_scene", "cpu", patch=8, scales=(1,), strides=(8,), crop_multiple=16)
    want = degrade.interpolate_bands(torch.from_numpy(cube)[None], 31)[0].to(torch.float32)
    assert st.C == 31 and torch.equal(st.arena.reshape(31, 16, 16), want)


def test_fixture_of_the_reference_preprocessing():
    """the reference's crop -> zoom -> Data2Volume on one 4 x 256 x 300 cube with a mask, ksize 16, strides (64, 32, 16): the store gives the
    same ordered origins, and every patch within the bar of the module docstring"""
    from mp_hsir_amd.scene_store import SceneStore
    g = np.load(GOLDEN)
    cube = g["cube_u8"].astype(np.float64) / 255.0
    st = SceneStore([(cube, g["mask"])], "natural_scene", "cpu", patch=int(g["ksize"]), scales=tuple(float(s) for s in g["scales"]),
                    strides=tuple(int(s) for s in g["strides"]), adapt_bands=False)
    assert st.levels_host[:, 1:].tolist() == [[256, 256], [128, 128], [64, 64]], "cropped to a multiple of 256, then 0.5 and 0.25"
    assert np.array_equal(st.records_host, g["origins"]), "same records in the same order: scene, scale, y, x"
    assert len(set(g["origins"][:, 0].tolist())) == 3 and st.degenerate == 0
    got = torch.cat(list(st.patches(batch=16))).numpy()
    want = g["patches"]
    assert not np.isnan(want).any() and got.shape == want.shape              # every record of the fixture is compared
    err = np.abs(got - want).max()
    print("fixture: %d patches, max |d| %.3g (measured on the CPU %.3g, bar %.3g)" % (want.shape[0], err, FIXTURE_MEASURED, FIXTURE_BAR))
    assert err <= FIXTURE_BAR


def test_degenerate_records_are_counted_and_can_be_dropped():
    from mp_hsir_amd.scene_store import SceneStore
    cube = np.random.RandomState(6).rand(31, 16, 32)
    cube[:, :8, 8:16] = 0.5                                     # one constant window of the full-scale grid
    kw = dict(patch=8, scales=(1,), strides=(8,), crop_multiple=16)
    st = SceneStore([cube], "natural_scene", "cpu", **kw)
    assert len(st) == 8 and st.degenerate == 1
    assert bool(torch.isnan(st.sample(torch.tensor([1]))).all()) and bool(torch.isfinite(st.sample(torch.tensor([0]))).all())
    dropped = SceneStore([cube], "natural_scene", "cpu", drop_degenerate=True, **kw)
    assert len(dropped) == 7 and dropped.degenerate == 1 and [tuple(r) for r in dropped.records_host[:2]] == [(0, 0, 0), (0, 0, 16)]


def test_files_mat_npy_and_the_v73_refusal(tmp_path):
    import scipy.io
    from mp_hsir_amd import scene_store as S
    rs = np.random.RandomState(8)
    cube = rs.rand(31, 16, 24)
    mask = np.zeros((16, 24), dtype=np.uint8)
    mask[0:3, 0:3] = 1
    scipy.io.savemat(str(tmp_path / "ICVL_a.mat"), {"data": cube.transpose(1, 2, 0), "mask": mask})
    np.save(str(tmp_path / "ICVL_b.npy"), cube.astype(np.float32))
    files = S.scene_files(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["ICVL_a.mat", "ICVL_b.npy"]
    st = S.SceneStore(files, "natural_scene", "cpu", patch=8, scales=(1,), strides=(8,), crop_multiple=8)
    assert len(st) == 5 + 6 and st.names[0] == "ICVL_a.mat" and st.names[-1] == "ICVL_b.npy"
    assert tuple(st.records_host[0]) == (0, 0, 8), "the window at (0, 0) touches the mask"
    assert torch.equal(st.arena[:31 * 16 * 24], torch.from_numpy(cube.astype(np.float32)).reshape(-1))
    with open(str(tmp_path / "new.mat"), "wb") as f:
        f.write(b"MATLAB 7.3 MAT-file, Platform: GLNXA64" + b" " * 200)
    with pytest.raises(RuntimeError, match="h5py"):
        S.load_scene(str(tmp_path / "new.mat"))
    with pytest.raises(ValueError, match="holds no"):
        S.SceneStore([cube], "natural_scene", "cpu")              # 16 x 24 cropped to multiples of 256 is empty


def test_flags():
    from mp_hsir_amd.options import build_parser
    o = build_parser().parse_args([])
    assert o.scene_dir == "" and o.crop_jitter == 0
    o = build_parser().parse_args(["--scene_dir", "/data/cubes", "--crop_jitter", "1", "--synthetic", "0"])
    assert o.scene_dir == "/data/cubes" and o.crop_jitter == 1 and o.db_path == ""


def test_a_level_smaller_than_the_patch_is_left_out():
    from mp_hsir_amd.scene_store import SceneStore
    cube = np.random.RandomState(10).rand(31, 32, 48)
    st = SceneStore([cube], "natural_scene", "cpu", patch=16, strides=(16, 8, 8), crop_multiple=16)
    assert st.levels_host[:, 1:].tolist() == [[32, 48], [16, 24]] and len(st) == 6 + 2           # the 8 x 12 level holds no 16 x 16 window
    assert bool(torch.isfinite(st.sample(torch.arange(len(st)))).all())
