"""The SSIM loss term without a GPU: the data-parallel engine at world_size 2 over gloo with SpectralLoss(ssim=) (the kernels through the
CPU-emulated build) against a single-process float64 restatement of the loss on the full batch with torch.optim.AdamW, the flag,
SpectralLoss's constructor and weights(), the checkpoint helpers of train.py, and the built kernels (meta)."""
import importlib
import os
import subprocess
import sys

import pytest
import torch

import meta
import ssim_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
from emu import bind_emulator
bind_emulator()
from mp_hsir_amd.engine import DataParallelEngine, SpectralLoss
import ssim_loss_ref as R
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.manual_seed(100 + rank)           # different init per rank: the engine must broadcast rank 0's
net = R.ConvNet()
eng = DataParallelEngine(net, lr=1e-2, bucket_mb=0.0005, loss_fn=SpectralLoss(**%(kw)r))
g = torch.Generator().manual_seed(7)
xs = torch.rand(3, 4, 3, 8, 8, generator=g); cs = torch.rand(3, 4, 3, 8, 8, generator=g)
half = slice(rank * 2, rank * 2 + 2)
losses = []
for i in range(3):
    losses.append(float(eng.train_step(xs[i][half], cs[i][half], None)))
torch.save({"state": {k: v.detach().clone() for k, v in net.state_dict().items()}, "losses": losses, "parts": eng.loss_components()}, %(out)r + str(rank))
dist.destroy_process_group()
'''


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kw,port", [(dict(ssim=0.2), "29551"), (dict(sam=0.1, sdiff=0.1, ssim=0.2), "29552")], ids=["ssim", "sam+sdiff+ssim"])
def test_world2_gloo_matches_the_float64_loss_and_adamw(tmp_path, kw, port):
    script = tmp_path / "worker.py"
    out = str(tmp_path / "res")
    script.write_text(WORKER % dict(root=ROOT, out=out, kw=kw))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, WORLD_SIZE="2", OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=280) == 0
    r0, r1 = torch.load(out + "0"), torch.load(out + "1")
    for k in r0["state"]:
        assert torch.equal(r0["state"][k], r1["state"][k]), k
    # single process, full batch: every term is a mean over equally sized halves (SSIM: over the windows of every plane), so the mean of the
    # two half-batch losses is the full-batch loss; its gradient through float64 autograd of the avg_pool2d composite
    torch.manual_seed(100)
    net = R.ConvNet()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2)
    g = torch.Generator().manual_seed(7)
    xs = torch.rand(3, 4, 3, 8, 8, generator=g); cs = torch.rand(3, 4, 3, 8, 8, generator=g)
    full = dict(sam=0.0, sdiff=0.0)
    full.update(kw)
    for i in range(3):
        opt.zero_grad(set_to_none=True)
        loss = R.torch_loss(net(xs[i], None).double(), cs[i].double(), full["sam"], full["sdiff"], full["ssim"])
        loss.backward()
        opt.step()
        both = 0.5 * (r0["losses"][i] + r1["losses"][i])
        assert abs(both - float(loss.detach())) <= 2e-5 * float(loss.detach()), (i, both, float(loss.detach()))
    for k, v in net.state_dict().items():
        assert torch.allclose(r0["state"][k], v, rtol=2e-5, atol=2e-6), k
    assert r0["parts"]["loss"] == r0["losses"][-1] and -1.0 < r0["parts"]["ssim"] < 1.0


def test_flag_defaults_to_off():
    from mp_hsir_amd import options
    o = options.build_parser().parse_args([])
    assert o.loss_ssim == 0.0 and o.loss_sam == 0.0 and o.loss_sdiff == 0.0
    assert options.build_parser().parse_args(["--loss_ssim", "0.2"]).loss_ssim == 0.2
    assert "--loss_ssim" in options.__doc__
    T = importlib.import_module("mp_hsir_amd.train")
    assert "--loss_ssim" in T.__doc__


def test_constructor_and_weights():
    from mp_hsir_amd.engine import DataParallelEngine, SpectralLoss
    for kw in (dict(), dict(ssim=0.0), dict(sam=0.0, sdiff=0.0, ssim=0.0), dict(ssim=-0.1), dict(ssim=float("nan")), dict(ssim=float("inf")),
               dict(sam=-0.1, ssim=0.2)):
        with pytest.raises(AssertionError):
            SpectralLoss(**kw)
    assert SpectralLoss(sam=0.1).weights() == {"sam": 0.1, "sdiff": 0.0} and SpectralLoss(0.1, 0.3, 0.0).weights() == {"sam": 0.1, "sdiff": 0.3}
    assert SpectralLoss(ssim=0.2).weights() == {"sam": 0.0, "sdiff": 0.0, "ssim": 0.2}
    assert SpectralLoss(0.1, 0.1, 0.2).weights() == {"sam": 0.1, "sdiff": 0.1, "ssim": 0.2}
    assert not SpectralLoss(ssim=0.2).spectral and SpectralLoss(sdiff=0.1, ssim=0.2).spectral
    on = DataParallelEngine(R.ConvNet(), lr=1e-3, loss_fn=SpectralLoss(ssim=0.2))
    assert on._eager_hyper and on.loss_components() is None


def test_checkpoints_carry_the_ssim_weight_and_resume_names_it_only_when_a_side_has_one(tmp_path, capsys):
    from mp_hsir_amd.engine import DataParallelEngine, SpectralLoss
    T = importlib.import_module("mp_hsir_amd.train")

    class Net(R.ConvNet):
        def __init__(self):
            super().__init__()
            self.clip_prompts = torch.zeros(2, 4)
            self.text_prompt = type("TP", (), {"clip_source": "surrogate"})()

    def eng(**kw):
        return DataParallelEngine(Net(), lr=1e-3, **(dict(loss_fn=SpectralLoss(**kw)) if kw else {}))

    net = Net()
    e = DataParallelEngine(net, lr=1e-3, loss_fn=SpectralLoss(0.1, 0.05, 0.2))
    assert T.loss_weights(e) == {"sam": 0.1, "sdiff": 0.05, "ssim": 0.2} and T.loss_weights(eng()) == {"sam": 0.0, "sdiff": 0.0}
    path = str(tmp_path / "epoch=3.ckpt")
    T.save_checkpoint(path, net, e, epoch=3)
    assert torch.load(path)["mphsir_loss"] == {"sam": 0.1, "sdiff": 0.05, "ssim": 0.2}
    _, start = T.load_warm_start(Net(), path, torch.device("cpu"), eng(sam=0.1, sdiff=0.05, ssim=0.2), resume=True)
    assert start == 4 and "loss weights" not in capsys.readouterr().out
    T.load_warm_start(Net(), path, torch.device("cpu"), eng(sam=0.1, sdiff=0.05), resume=True)
    assert "trained with loss weights sam 0.1 sdiff 0.05 ssim 0.2, this run continues with sam 0.1 sdiff 0.05 ssim 0" in capsys.readouterr().out
    T.load_warm_start(Net(), path, torch.device("cpu"), eng(), resume=True)
    assert "trained with loss weights sam 0.1 sdiff 0.05 ssim 0.2, this run continues with sam 0 sdiff 0 ssim 0" in capsys.readouterr().out
    ckpt = torch.load(path)
    ckpt["mphsir_loss"] = {"sam": 0.1, "sdiff": 0.05}             # a checkpoint from before the flag existed
    T.load_warm_start(Net(), ckpt, torch.device("cpu"), eng(ssim=0.3), resume=True)
    assert "trained with loss weights sam 0.1 sdiff 0.05 ssim 0, this run continues with sam 0 sdiff 0 ssim 0.3" in capsys.readouterr().out
    T.load_warm_start(Net(), ckpt, torch.device("cpu"), eng(), resume=True)
    assert "trained with loss weights sam 0.1 sdiff 0.05, this run continues with sam 0 sdiff 0\n" in capsys.readouterr().out


# ---- meta: the built kernels (the args struct: tests/test_cabi.py) ----------------------------------------------------------------------
def test_kernels_exist_and_do_not_spill():
    ks = meta.kernels_by_name("arena")
    for name in ("mphsir::ssim_loss_kernel", "mphsir::ssim_loss_finish_kernel"):
        assert name in ks and len(ks[name]) == 1, sorted(ks)
        k = ks[name][0]
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k["max_flat_workgroup_size"] == 256
    # two workgroups per CU: at most 80 KB of the 160 KB of LDS each (and under the 64 KB of static LDS), which is two waves per SIMD: up
    # to 256 registers per lane do not lower that
    k = ks["mphsir::ssim_loss_kernel"][0]
    assert k.get("group_segment_fixed_size", 0) <= 64 * 1024 and k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 256, k

