"""The cassi task on the host (CPU, no kernel): the numpy restatement and degrade.cassi_measure against what the reference's _sd_cassi
returned (tests/golden/cassi.npz), the menu entry, the flags of options.py / test.py, the one-task net's sentence, the mask holder."""
import importlib

import numpy as np
import pytest
import torch

import cassi_ref as R


def test_numpy_restatement_and_tensor_form_reproduce_the_reference():
    from mp_hsir_amd import degrade as D
    cases = R.golden_cases()
    assert [c[1].shape for c in cases] == [(9, 32, 32), (5, 16, 24), (31, 20, 12)]
    for name, x, mask, origin, out in cases:
        assert out.dtype == np.float32 and out.min() == 0.0 and out.max() == 1.0
        assert np.array_equal(R.numpy_cassi(x, mask, origin), out), name
        got = D.cassi_measure(torch.from_numpy(x)[None], torch.from_numpy(mask), torch.tensor([origin.tolist()]))[0].numpy()
        assert np.array_equal(got, out), name
    # a batch with one origin per sample, a list of pairs, and a mask given in float64 (cast once)
    name, x, mask, origin, out = cases[0]
    xb = torch.from_numpy(np.stack([x, x[:, ::-1].copy()]))
    got = D.cassi_measure(xb, torch.from_numpy(mask.astype(np.float64)), [origin.tolist(), (0, 1)]).numpy()
    assert np.array_equal(got[0], out) and np.array_equal(got[1], R.numpy_cassi(xb[1].numpy(), mask, (0, 1)))
    with pytest.raises(ValueError, match="does not hold"):
        D.cassi_measure(xb, torch.from_numpy(mask[:31]))


def test_menu_entry_and_degrade_as():
    from mp_hsir_amd import degrade as D
    assert D.DE_DICT["natural_scene"]["cassi"] == [(0,)] and "cassi" not in D.DE_DICT["remote_sensing"]
    syn = D.DegradationSynthesizer("natural_scene", ["cassi"], "cpu", seed=3)
    x = torch.rand(3, 5, 16, 16)
    y = syn.degrade_as(x, "cassi")
    assert y.shape == x.shape and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    assert all(float(y[b].min()) == 0.0 and float(y[b].max()) == 1.0 for b in range(3))
    deg, clean, prompt = syn(x)
    assert deg.shape == clean.shape == x.shape and int(prompt.abs().max()) == 0
    with pytest.raises(ValueError, match="not defined"):
        D.DegradationSynthesizer("remote_sensing", ["cassi"], "cpu")
    assert D.DegradationSynthesizer("natural_scene", ["gaussianN"], "cpu").cassi_mask is None


def test_flags_of_options_and_test_py():
    O = importlib.import_module("mp_hsir_amd.options")
    o = O.build_parser().parse_args([])
    assert (o.task_classes, o.cassi_mask, o.cassi_step) == (0, "", 2)
    o = O.build_parser().parse_args(["--task_classes", "1", "--cassi_step", "3", "--cassi_mask", "m.npy", "--natural_scene_single_de_type", "cassi"])
    assert (o.task_classes, o.cassi_mask, o.cassi_step, o.natural_scene_single_de_type) == (1, "m.npy", 3, ["cassi"])
    T, t = R.test_py_options([])
    assert (t.task_classes, t.cassi_mask, t.cassi_step) == (0, "", 2)
    T, t = R.test_py_options(["--mode", "13", "--task_classes", "1", "--cassi_step", "1"])
    assert (t.mode, t.task_classes, t.cassi_step) == (13, 1, 1) and T.mode_dir(t) == "CASSI_step=1"
    assert "13" in T.__doc__ and "--cassi_mask" in T.__doc__
    from mp_hsir_amd import degrade as D
    assert D.SceneDegrader("natural_scene", "cpu", 1).prompt_id(13) == 0


def test_mode_13_on_the_host_and_a_small_mask_file_ends_the_run(tmp_path):
    from mp_hsir_amd import degrade as D
    T, o = R.test_py_options(["--mode", "13", "--seed", "5"])
    clean = torch.rand(1, 7, 72, 136)
    y, pid = T.degrade_for_mode(o, clean, D.Draws("cpu", o.seed + 1), o.model)
    assert pid == 0 and y.shape == clean.shape and float(y.min()) == 0.0 and float(y.max()) == 1.0
    mask = D.scene_cassi_mask(o, clean.device, 72, 136)
    origin = mask.origins(D.Draws("cpu", o.seed + 1), 1, 72, 136)
    assert np.array_equal(y[0].numpy(), R.numpy_cassi(clean[0].numpy(), mask.mask.numpy(), origin[0].tolist()))
    path = str(tmp_path / "small.npy")
    np.save(path, np.ones((72, 100), dtype=np.float64))
    o.cassi_mask = path
    with pytest.raises(SystemExit, match="smaller than the 72 x 136"):
        T.degrade_for_mode(o, clean, D.Draws("cpu", 1), o.model)
    # modes 0-12 are untouched: 14 still is no mode
    o.mode = 14
    with pytest.raises(SystemExit, match="unknown mode 14"):
        T.degrade_for_mode(o, clean, D.Draws("cpu", 1), o.model)


def test_one_task_net_carries_the_cassi_sentence():
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net, _TASK_PROMPTS, surrogate_clip_prompt
    net = MP_HSIR_Net(in_channel=8, out_channel=8, dim=32, num_blocks=[2, 2, 2], num_refinement_blocks=2, heads=[1, 2, 4], task_classes=1,
                      clip_prompt=surrogate_clip_prompt(1))
    assert net.text_prompt.task_text_prompts == [_TASK_PROMPTS["cassi"]]
    assert "coded aperture" in _TASK_PROMPTS["cassi"] and tuple(net.clip_prompts.shape) == (1, 512)


def test_cassi_mask_holder(tmp_path):
    import scipy.io as sio
    from mp_hsir_amd import degrade as D
    m = D.CassiMask("cpu", seed=4)
    assert m.shape == (256, 256) and m.mask.dtype == torch.float32 and set(m.mask.unique().tolist()) == {0.0, 1.0}
    assert 0.45 < float(m.mask.mean()) < 0.55 and torch.equal(m.mask, D.CassiMask("cpu", seed=4).mask)
    assert not torch.equal(m.mask, D.CassiMask("cpu", seed=5).mask)
    with pytest.raises(ValueError, match="smaller than the 257 x 64"):
        m.check(257, 64)
    with pytest.raises(ValueError, match="smaller than"):
        m.origins(D.Draws("cpu", 1), 2, 64, 300)
    org = m.origins(D.Draws("cpu", 1), 500, 64, 250)
    assert org.shape == (500, 2) and org.dtype == torch.int32
    assert int(org[:, 0].min()) == 0 and int(org[:, 0].max()) == 192 and int(org[:, 1].min()) == 0 and int(org[:, 1].max()) == 6
    assert torch.equal(D.CassiMask("cpu", shape=(64, 64)).origins(D.Draws("cpu", 1), 3, 64, 64), torch.zeros((3, 2), dtype=torch.int32))
    vals = np.random.RandomState(0).rand(40, 48)
    sio.savemat(str(tmp_path / "m.mat"), {"mask": vals})
    np.save(str(tmp_path / "m.npy"), vals)
    for fn in ("m.mat", "m.npy"):
        got = D.CassiMask("cpu", str(tmp_path / fn))
        assert got.shape == (40, 48) and np.array_equal(got.mask.numpy(), vals.astype(np.float32))
    np.save(str(tmp_path / "bad.npy"), np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="2-D"):
        D.CassiMask("cpu", str(tmp_path / "bad.npy"))


def test_ops_cassi_refuses_cpu_tensors():
    """the product library bound (not the emulator): a CPU tensor is an error, there is no fallback"""
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    saved = (L._lib, L._is_emu)
    try:
        L._lib, L._is_emu = None, False
        L.load()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.cassi(torch.zeros(1, 3, 8, 8), torch.ones(8, 8))
    finally:
        L._lib, L._is_emu = saved
