"""End-to-end parity on the MI355X: the whole network through libmphsir vs the reference's golden
outputs (tests/golden/*.npz) -- fp32 path within the north star's 1e-3 relative / 0.01 dB PSNR (in
practice ~1e-6), bf16 path within the reference's own bf16-autocast deviation (1e-2)."""
import pytest
import torch

import model_checks as M
from golden.cases import TINY_CASES, FULL_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _real_library():
    import mp_hsir_amd._lib as L
    L._lib, L._is_emu = None, False
    L.load()


@pytest.mark.parametrize("name", list(TINY_CASES))
def test_tiny_forward_fp32(name):
    assert M.check_tiny_forward("cuda", name) < 2e-5


@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_width_forward_fp32(name):
    err, dpsnr = M.check_full_forward("cuda", name, torch.float32, tol=1e-3, dpsnr=0.01)
    assert err < 5e-5 and dpsnr < 1e-3, (err, dpsnr)     # far inside the north-star bar


@pytest.mark.parametrize("name", list(FULL_CASES))
def test_full_width_forward_bf16(name):
    err, dpsnr = M.check_full_forward("cuda", name, torch.bfloat16, tol=4e-2, dpsnr=0.25)
    print(name, "bf16 rel-L2", err, "dPSNR", dpsnr)


def test_run_to_run_determinism():
    """split-K Gram partials are reduced in a fixed order: two launches give identical bits."""
    c, clean, degraded = M.full_case_inputs("natural_mode0")
    net = M.build_net(c["cfg"], "cuda", torch.bfloat16)
    x, t = degraded.cuda(), torch.tensor(c["task"]).cuda()
    with torch.no_grad():
        net(x, t)                      # warm-up (packed-weight caches are built on first use)
        a, b = net(x, t), net(x, t)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_block_kernels_are_bitwise_reproducible(dtype):
    """one PGSSTB block (six HIP launches, no library ops) twice on the same input: identical bits."""
    from mp_hsir_amd.net.MP_HSIR import PGSSTB
    torch.manual_seed(0)
    blk = PGSSTB(128, 2, [64, 64], 8, 4, 0.0, 2.66, 8, 128).cuda().eval()
    x = torch.randn(4, 64, 64, 128, device="cuda").to(dtype)
    with torch.no_grad():
        a, b, c = blk(x), blk(x), blk(x)
    assert torch.equal(a, b) and torch.equal(b, c)


def test_batch_coupling_and_large_cube():
    """B=16 natural-scene forward (BASELINE config 2 shape) and one 256x256 cube run and stay finite;
    sample 0 of a B=16 batch differs from its B=1 result (TVSP batch coupling)."""
    c, clean, degraded = M.full_case_inputs("natural_mode0")
    net = M.build_net(c["cfg"], "cuda", torch.bfloat16)
    x1 = degraded.cuda()
    x16 = x1.repeat(16, 1, 1, 1)
    with torch.no_grad():
        y1 = net(x1, torch.zeros(1, dtype=torch.long, device="cuda"))
        y16 = net(x16, torch.arange(16, device="cuda") % 6)
        big = net(torch.rand(1, 31, 256, 256, device="cuda"), torch.zeros(1, dtype=torch.long, device="cuda"))
    assert torch.isfinite(y16).all() and torch.isfinite(big).all() and big.shape == (1, 31, 256, 256)
    assert not torch.allclose(y1[0], y16[0])


from golden.cases import BLOCK_CASES, CUBE_CASES


@pytest.mark.timeout(1800)
def test_b16_forward_vs_oracle_at_real_width():
    """BASELINE configs[1] (natural net, batch 16, bf16 forward) against the oracle on this host as full tensors, fp32 and bf16 --
    until round 6 that configuration was only property-checked at real width (finite, batch-coupled)."""
    print(M.check_b16_forward("cuda"))


@pytest.mark.timeout(2400)
@pytest.mark.parametrize("name", list(CUBE_CASES))
def test_full_size_cube_vs_reference_and_oracle(name):
    """missing-item 1 of the round-3 review: one whole 512x512x31 natural cube (test.py:150-188) and one 256x256 cube of the
    172-band remote-sensing width (test.py:440-469, BASELINE configs[3]) -- fp32 and bf16 HIP forward against the reference's
    statistics at that size and against the fp32 oracle run on this host, full tensors (see check_full_size_cube)."""
    res = M.check_full_size_cube("cuda", name)
    print(name, res)



@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["nat_enc1", "nat_enc2", "nat_refine", "rs_enc1"])
def test_fused_block_equals_unfused(name, dtype):
    """the whole-block Function (branch sum inside the gated-MLP launch: C <= 128, 16-bit) == attention Function + MLP Function,
    bit for bit: output (training and no-grad), dX, every parameter gradient"""
    M.check_fused_block_equals_unfused("cuda", name, dtype)


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("dtype,fuse", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True)])
def test_base_block_skip_gradient_on_equals_off(depth, dtype, fuse):
    """the BaseBlock skip gradient through autograd_ops.SkipGrad against autograd's own sum: every parameter gradient bit for bit, dx
    within the block-gradient bars, the holder empty after each backward"""
    M.check_base_skip_bwd("cuda", depth, dtype, fuse)


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_block_gradients_fp32(name):
    """every shape class of both shipped configurations (C 64..384, head_dim 32..96) + TVSP + PromptFusion: output, dX and
    every parameter gradient of the HIP path vs the reference's (2e-5 rel-L2; 1e-3 is the north-star bar)."""
    assert M.check_block_gradients("cuda", name, torch.float32, tol=2e-5) < 2e-5


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_block_gradients_bf16(name):
    """same at the benchmark's compute dtype: bf16 storage, fp32 accumulation.  Bars tensor by tensor: 3 x the deviation of the
    reference's own bf16 autocast backward for that tensor + 2 x the block's median (model_checks.block_grad_bars; 2-7 % -- until
    round 6 a flat 6e-2)."""
    worst, worst_ratio, med = M.check_block_gradients("cuda", name, torch.bfloat16, tol=None)
    print("bf16 block gradients %s: worst rel-L2 %.3g, worst error / bar %.2f, reference's median deviation %.3g" % (name, worst, worst_ratio, med))


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("name", ["natural_b2", "remote_b2"])
def test_whole_net_gradients_at_real_width(name):
    """missing-item 3 of the round-4 review: the backward of MP_HSIR_Net(31,31,64,T=6) / (100,100,96,T=7) as a whole (U-Net joins,
    cat splits, prompt branches, deferred sums at real widths), batch 2: fp32 against the reference's fixture and the oracle's fp64
    autograd (every parameter < 1e-4), bf16 / fp16 against the same with a bar derived from the forward deviation of the run."""
    res = M.check_full_gradients("cuda", name, torch.bfloat16 if name == "natural_b2" else torch.float16)
    print(name, res)


@pytest.mark.timeout(2400)
def test_batch32_bf16_step_vs_oracle():
    """the benchmark's batch (32 x 64x64x31, bf16): loss and sampled parameter gradients of one step against the oracle (fp32, this host)"""
    print(M.check_batch32_step("cuda"))


def test_tiny_net_gradients_fp32():
    assert M.check_tiny_gradients("cuda") < 1e-4


@pytest.mark.parametrize("use_graph", [False, True])
def test_tiny_adamw_two_steps_vs_reference(use_graph):
    """a18: HIP forward/backward + mphsir_flat_adamw (eager, and captured in the hipGraph) reproduce the reference model
    stepped by torch.optim.AdamW: tests/golden/tiny_adamw.npz."""
    print("tiny AdamW worst relative error", M.check_tiny_adamw("cuda", use_graph=use_graph))


def test_eval_forward_with_prompt_streams_then_captured_training_step():
    """a no-grad forward forks the prompt modules on their own streams (ops.PROMPT_SIDE); the captured training step that
    follows must not wait on streams last used outside its capture (they are not tracked, and the set of tracked streams is reset
    where a backward pass begins) -- and must still reproduce the reference's two AdamW steps."""
    from mp_hsir_amd import ops
    from golden.cases import TINY_CFG
    from golden.detfill import det_fill_, seeded_input, surrogate_clip_prompt
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    assert ops.PROMPT_SIDE and not hasattr(ops, "PROMPT_SIDE_TRAIN")
    net = MP_HSIR_Net(**TINY_CFG, clip_prompt=surrogate_clip_prompt(6)).eval()
    det_fill_(net)
    net = net.cuda().set_compute_dtype(torch.float32)
    with torch.no_grad():
        net(seeded_input("smoke", (2, 8, 32, 32)).cuda(), torch.tensor([1, 4]).cuda())
    assert not any(st in (ops._SIDE.get((d, "prompt1")), ops._SIDE.get((d, "prompt2"))) for d, st in ops._SIDE_USED)
    for _ in range(2):
        M.check_tiny_adamw("cuda", use_graph=True)


def _spawn_ranks(mode, steps, out, world=2, port=29541, backend="gloo"):
    import os
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_graph_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, worker, out, mode, str(steps), backend], env=dict(env, RANK=str(r))) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    return [torch.load(out + str(r)) for r in range(world)]


def _check_world2(res, mode, steps):
    """both ranks' final parameters are bitwise equal and equal ONE process that runs both micro-batches, averages the
    gradients (DDP semantics; TVSP's batch coupling is per micro-batch) and steps torch.optim.AdamW"""
    from golden.cases import TINY_CFG
    from golden.detfill import seeded_input
    for k in res[0]["state"]:
        assert torch.equal(res[0]["state"][k], res[1]["state"][k]), "ranks diverged: " + k
    net = M.build_net(TINY_CFG, "cuda", torch.float32)
    p0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt = torch.optim.AdamW([p for p in net.parameters()], lr=2e-3)
    ref_losses = [[], []]
    for step in range(steps):
        opt.zero_grad(set_to_none=True)
        for r in range(2):
            xs = seeded_input("dp_x%d_%d" % (step, r), (2, 8, 32, 32)).cuda()
            cs = seeded_input("dp_c%d_%d" % (step, r), (2, 8, 32, 32)).cuda()
            loss = (net(xs, torch.tensor([[r + 1], [3]]).cuda()).clamp(0, 1) - cs).abs().mean()
            (loss / 2).backward()
            ref_losses[r].append(float(loss))
        opt.step()
    for r in range(2):
        assert torch.allclose(torch.tensor(res[r]["losses"]), torch.tensor(ref_losses[r]), rtol=2e-4, atol=1e-7), (r, res[r]["losses"], ref_losses[r])
    for k, v in net.state_dict().items():
        if not v.is_floating_point() or k.endswith("attn_mask"):
            continue
        d_ref, d_got = (v.detach() - p0[k]).double().cpu(), (res[0]["state"][k].cuda() - p0[k]).double().cpu()
        if float(d_ref.norm()) == 0.0:
            assert float(d_got.norm()) == 0.0, k
            continue
        assert float((d_got - d_ref).norm() / d_ref.norm()) < 2e-2, (k, float((d_got - d_ref).norm() / d_ref.norm()))


@pytest.mark.timeout(900)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL over xGMI)")
@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_data_parallel_world2_rccl(mode, tmp_path):
    """e / a19 on real hardware: two ranks, one GPU each, backend nccl (= RCCL) -- broadcast at start, bucketed gradient
    all-reduce (graph mode: started from external event nodes inside the replay, or one arena-wide message if the stack has
    none), AdamW -- against the one-process reference.  Runs wherever >= 2 GPUs are visible; the children are started
    before this process touches a GPU (device_count() does not initialise HIP)."""
    steps = 5
    res = _spawn_ranks(mode, steps, str(tmp_path / "res"), port=29551 if mode == "graph" else 29553, backend="nccl")
    print("world-2 RCCL %s mode: %d buckets, all-reduce overlapped with the replay: %s (bucket order %s)"
          % (mode, res[0]["nbuckets"], res[0]["overlap"], res[0]["bucket_order"]))
    assert res[0]["nbuckets"] >= 2
    _check_world2(res, mode, steps)


def test_checkpoint_resume_continues_bitwise(tmp_path):
    """f3: save_checkpoint after 2 steps -> a NEW model + engine, load_warm_start(resume=True) -> 2 more steps == 4 steps
    straight through, bitwise (parameters, AdamW moments, step count); without resume the same file is the reference's warm
    start: weights only, epoch 0, fresh optimizer (train.py:109-116)."""
    import importlib
    from golden.cases import TINY_CFG
    from golden.detfill import seeded_input
    from mp_hsir_amd.engine import DataParallelEngine
    T = importlib.import_module("mp_hsir_amd.train")

    def batch(step):
        return (seeded_input("ck_x%d" % step, (2, 8, 32, 32)).cuda(), seeded_input("ck_c%d" % step, (2, 8, 32, 32)).cuda(),
                torch.tensor([[1], [3]]).cuda())

    def run(net, eng, steps):
        for s in steps:
            torch.manual_seed(100 + s)           # DropPath draws: the same per step whatever ran before
            eng.train_step(*batch(s), lr=2e-3)
        torch.cuda.synchronize()

    net_a = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    eng_a = DataParallelEngine(net_a, lr=2e-3)
    run(net_a, eng_a, range(4))
    net_b = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    eng_b = DataParallelEngine(net_b, lr=2e-3)
    run(net_b, eng_b, range(2))
    path = str(tmp_path / "epoch=7.ckpt")
    T.save_checkpoint(path, net_b, eng_b, epoch=7)
    net_c = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    with torch.no_grad():
        for p in net_c.parameters():
            p.mul_(0.5)                       # everything must come from the file
    eng_c = DataParallelEngine(net_c, lr=2e-3)
    n, start = T.load_warm_start(net_c, path, torch.device("cuda"), eng_c, resume=True)
    assert start == 8 and n == len(net_c.state_dict())
    run(net_c, eng_c, range(2, 4))
    for (k, va), vc in zip(net_a.state_dict().items(), net_c.state_dict().values()):
        assert torch.equal(va, vc), k
    sa, sc = eng_a.optimizer_state(), eng_c.optimizer_state()
    assert sa["step"] == sc["step"] == 4
    for k in sa["exp_avg"]:
        assert torch.equal(sa["exp_avg"][k], sc["exp_avg"][k]) and torch.equal(sa["exp_avg_sq"][k], sc["exp_avg_sq"][k]), k
    # the same file as a warm start: weights only
    net_d = M.build_net(TINY_CFG, "cuda", torch.float32).train()
    eng_d = DataParallelEngine(net_d, lr=2e-3)
    n, start = T.load_warm_start(net_d, path, torch.device("cuda"), eng_d)
    assert start == 0 and eng_d.step_count == 0
    for (k, vb), vd in zip(net_b.state_dict().items(), net_d.state_dict().values()):
        assert torch.equal(vb, vd), k


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_data_parallel_world2_on_one_gpu(mode, tmp_path):
    """e / a19: two ranks (fresh child processes, gloo, both on cuda:0) x micro-batch 2 through the engine -- graph mode:
    captured step + arena-wide all-reduce + AdamW/repack after the replay (what bench.py --gpus N runs); eager mode:
    bucketed all-reduces from the gradient hooks -- against ONE process that runs both micro-batches, averages the
    gradients (DDP semantics; TVSP's batch coupling is per micro-batch) and steps torch.optim.AdamW."""
    from golden.cases import TINY_CFG
    from golden.detfill import seeded_input
    steps = 5
    res = _spawn_ranks(mode, steps, str(tmp_path / "res"), port=29541 if mode == "graph" else 29543)
    for k in res[0]["state"]:
        assert torch.equal(res[0]["state"][k], res[1]["state"][k]), "ranks diverged: " + k
    print("world-2 %s mode: %d buckets, all-reduce overlapped with the replay: %s (bucket order %s)"
          % (mode, res[0]["nbuckets"], res[0]["overlap"], res[0]["bucket_order"]))
    assert res[0]["nbuckets"] >= 2
    if mode == "graph":
        from mp_hsir_amd.engine import _external_events_work
        assert res[0]["overlap"] == _external_events_work(torch.device("cuda", 0))
        if res[0]["overlap"]:
            assert sorted(res[0]["bucket_order"]) == list(range(res[0]["nbuckets"]))
    _check_world2(res, mode, steps)


@pytest.mark.timeout(900)
def test_bench_two_ranks_gloo_on_one_gpu(tmp_path):
    """`bench.py --gpus 2` exactly as the driver launches it (torch.distributed.run), with the gloo test hook so that both
    ranks share this box's one GPU: exits 0 and prints one well-formed JSON line with n_gpus = 2."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MPHSIR_DIST_BACKEND="gloo", MPHSIR_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29547", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "3", "--batch", "4",
                        "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["config"]["global_batch"] == 8 and line["roofline"] is not None
    # the roofline object of the contract: algorithmic bytes only (the kernel's own split-K partials apart), where `traffic` comes from
    rf = line["roofline"]
    for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "partials_bytes_per_step", "timing"):
        assert key in rf, key
    assert 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and line["comm"]["ranks"] == 2


@pytest.mark.timeout(900)
def test_bench_starts_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher (train.py:118 `devices=opt.num_gpus`): the script starts the two ranks itself
    (gloo test hook: both on this box's GPU), relays rank 0's line with n_gpus = 2 and comm.ranks = 2; asking for more GPUs
    than the node has, without the hook, exits non-zero with a message instead of silently benchmarking one GPU."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "3", "--batch", "4",
                        "--full", "--no-cpu-baseline", "--no-roofline"], env=dict(env, MPHSIR_DIST_BACKEND="gloo", MPHSIR_SHARE_GPU="1"),
                       capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["config"]["global_batch"] == 8 and line["comm"]["ranks"] == 2
    if torch.cuda.device_count() < 8:
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "1"], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode != 0 and "GPU(s) visible" in r.stderr and not r.stdout.strip()


@pytest.mark.timeout(300)
def test_bench_plain_run_dumps_outputs(tmp_path):
    """a plain `bench.py` run times only the headline step (the --full legs stay null) and --dump-outputs writes the last step's
    loss and updated parameters as finite float32 .npy files, 64 MB at most"""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert all(line[k] is None for k in ("roofline", "roofline_spectral", "cpu_baseline", "extra_configs", "comm"))
    assert sorted(os.listdir(out)) == ["loss.npy", "params.npy"]
    loss, params = np.load(out / "loss.npy"), np.load(out / "params.npy")
    assert loss.dtype == np.float32 and params.dtype == np.float32 and np.isfinite(loss).all() and np.isfinite(params).all()
    assert params.size == sum(v.numel() for v in MP_HSIR_Net(in_channel=31, out_channel=31, dim=64, task_classes=6,
                                                              clip_prompt="surrogate").parameters())
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64e6


def test_training_step_bf16_natural_runs_and_learns():
    """three engine steps of the natural-scene net at batch 4: finite loss, parameters move, loss not exploding."""
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    torch.manual_seed(0)
    net = MP_HSIR_Net(compute_dtype=torch.bfloat16, clip_prompt="surrogate").cuda().train()
    w0 = net.output.weight.detach().clone()
    eng = DataParallelEngine(net, lr=2e-4)
    src = SyntheticPatchSource(31, 64, 4, 6, "cuda", 2024, 0)
    losses = []
    for _ in range(3):
        _, x, c, p = src.next()
        losses.append(float(eng.train_step(x, c, p)))
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < 2 * losses[0]
    assert not torch.equal(net.output.weight.detach(), w0) and len(eng.unused) == 8


def test_remote_sensing_training_step_bf16():
    """BASELINE configs[4] model (100 bands, dim 96, T=7) in bf16: two engine steps at batch 2 run through the HIP
    backward at widths 96/192/384 and head dims 48/96; loss finite, 8 gradient-less parameters detected."""
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    from mp_hsir_amd import ops
    torch.manual_seed(0)
    net = MP_HSIR_Net(100, 100, 96, task_classes=7, compute_dtype=torch.bfloat16, clip_prompt="surrogate").cuda().train()
    eng = DataParallelEngine(net, lr=1e-4)
    src = SyntheticPatchSource(100, 64, 2, 7, "cuda", 2024, 0)
    ops.ACCOUNT = {}
    losses = []
    for _ in range(2):
        _, x, c, p = src.next()
        losses.append(float(eng.train_step(x, c, p)))
    acct, ops.ACCOUNT = ops.ACCOUNT, None
    assert all(torch.isfinite(torch.tensor(losses))) and len(eng.unused) == 8
    for k in ("win_attn_bwd", "gated_mlp_bwd", "spectral_fold_bwd", "pg_gate_bwd", "gemm_tn", "conv3x3_tok"):
        assert k in acct, k
    # every one of the 22 blocks ran the HIP attention backward (C=384 / 8 heads included): 22 launches per step
    assert acct["win_attn_bwd"][0] == 2 * 22, acct["win_attn_bwd"]
    _, x, c, p = src.next()
    _, aten = M._run_profiled(lambda: eng.train_step(x, c, p))
    lib_ops = sorted(o for o in aten if o in M._LIB_GEMM_OPS)
    assert not lib_ops, "library GEMM / conv / norm ops on the training step: %s" % lib_ops


def test_remote_sensing_training_fp16_loss_scaling():
    """BASELINE configs[4]: the remote-sensing model (100 bands, dim 96, T=7), batch 16, fp16 compute with dynamic loss scaling
    (the reference's precision="16-mixed", train.py:118) through the engine: the scale adapts (overflowing steps are skipped and
    halve it), steps are taken, the loss stays finite, and the parameters with tiny gradient paths (temperature, prompt_param,
    relative_position_bias_table, text_prompt_learnable, visual_prompt) receive non-zero finite updates."""
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    torch.manual_seed(0)
    net = MP_HSIR_Net(100, 100, 96, task_classes=7, compute_dtype=torch.float16, clip_prompt="surrogate").cuda().train()
    watch = {k: p for k, p in net.named_parameters() if k.endswith(("temperature", "prompt_param", "relative_position_bias_table",
                                                                     "text_prompt_learnable", "visual_prompt"))}
    before = {k: p.detach().clone() for k, p in watch.items()}
    eng = DataParallelEngine(net, lr=1e-4)
    src = SyntheticPatchSource(100, 64, 16, 7, "cuda", 2024, 0)
    losses = []
    for _ in range(8):
        _, x, c, p = src.next()
        losses.append(float(eng.train_step(x, c, p)))
    sc = eng.scaler.cpu()
    print("fp16 losses", losses, "scaler", sc.tolist())
    assert all(torch.isfinite(torch.tensor(losses))) and eng.scaler is not None
    assert float(sc[3]) >= 3 and 1.0 <= float(sc[0]) <= 65536.0 and float(sc[2]) == 0.0, sc.tolist()
    for k, p in watch.items():
        d = (p.detach() - before[k]).abs()
        assert torch.isfinite(p).all() and float(d.max()) > 0.0, k
    assert losses[-1] < 1.5 * losses[0]


def test_full_width_forward_fp16():
    for name in FULL_CASES:
        err, dp = M.check_full_forward("cuda", name, torch.float16, tol=8e-3, dpsnr=0.05)
        print(name, "fp16 rel-L2 %.3e dPSNR %.4f" % (err, dp))


def test_512x512_172band_forward_bf16():
    """BASELINE configs[3] shape: (1,172,512,512) inpainting input through MP_HSIR_Net(172,172,96,T=7) in bf16:
    runs whole (no tiling), finite, and the 64x64 top-left crop of the output depends on the rest of the cube
    (global spectral attention reduces over all 262,144 pixels)."""
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    torch.manual_seed(0)
    net = MP_HSIR_Net(172, 172, 96, task_classes=7, compute_dtype=torch.bfloat16, clip_prompt="surrogate").cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    clean = torch.rand((1, 172, 512, 512), generator=g, device="cuda")
    x = clean * (torch.rand(clean.shape, generator=g, device="cuda") > 0.9).float()
    t = torch.tensor([4], device="cuda")
    with torch.no_grad():
        y = net(x, t)
        y_crop = net(x[:, :, :64, :64].contiguous(), t)
    assert y.shape == x.shape and torch.isfinite(y).all()
    assert not torch.allclose(y[:, :, :32, :32], y_crop[:, :, :32, :32], atol=1e-3)


def test_graph_replay_matches_eager_training():
    """the captured-and-replayed step (hipGraph) follows the same parameter trajectory as eager launches."""
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    from golden.cases import TINY_CFG
    from golden.detfill import surrogate_clip_prompt
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        net = MP_HSIR_Net(**TINY_CFG, clip_prompt=surrogate_clip_prompt(6), compute_dtype=torch.float32).cuda().eval()
        eng = DataParallelEngine(net, lr=2e-4, use_graph=use_graph, graph_warmup=2)     # eval(): no DropPath randomness
        src = SyntheticPatchSource(8, 64, 2, 6, "cuda", 2024, 0)
        losses = []
        for _ in range(5):
            _, x, c, p = src.next()
            losses.append(float(eng.train_step(x, c, p)))
        eng.finish()
        res.append((losses, net.output.weight.detach().clone(), net.encoder_level1.blocks[1].mlp.fc1.weight.detach().clone()))
    (l0, a0, b0), (l1, a1, b1) = res
    # the library GEMMs may pick another algorithm under capture (different rounding), and Adam turns rounding-level
    # gradient differences into lr-sized weight differences: the trajectories agree to ~1e-4, not bitwise
    assert l0[:3] == l1[:3] or torch.allclose(torch.tensor(l0[:3]), torch.tensor(l1[:3]), rtol=1e-6), (l0, l1)
    assert torch.allclose(torch.tensor(l0), torch.tensor(l1), rtol=2e-4, atol=1e-7), (l0, l1)
    # Adam normalises every gradient element to ~lr, so elements whose gradient is rounding noise may move by up to
    # 2*lr per step in either direction; everything else must agree closely
    for u, v in ((a0, a1), (b0, b1)):
        d = (u - v).abs()
        assert float(d.max()) < 5 * 2 * 2e-4 and float(d.mean()) < 1e-5, (float(d.max()), float(d.mean()))


def test_drop_path_factors_under_graph_replay():
    """train mode under hipGraph capture.  The per-sample DropPath factors are drawn inside the captured step
    (torch's graph-safe philox state): they must change from replay to replay, and -- same seed -- equal what the eager
    engine draws at the same step, so the captured training run follows the eager one."""
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    from golden.cases import TINY_CFG
    from golden.detfill import surrogate_clip_prompt
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(11)
        net = MP_HSIR_Net(**TINY_CFG, clip_prompt=surrogate_clip_prompt(6), compute_dtype=torch.float32).cuda().train()
        eng = DataParallelEngine(net, lr=2e-4, use_graph=use_graph, graph_warmup=2)
        src = SyntheticPatchSource(8, 32, 16, 6, "cuda", 2024, 0)
        torch.manual_seed(5)                       # the DropPath stream
        fac, losses = [], []
        for _ in range(6):
            _, x, c, p = src.next()
            losses.append(float(eng.train_step(x, c, p)))
            fac.append(net.__dict__["_dp_last"].detach().clone().cpu())
        eng.finish()
        runs.append((fac, losses))
    (fe, le), (fg, lg) = runs
    assert fg[0].shape[1:] == (2, 16) and float((fg[0] != 1).sum()) >= 0
    assert any(not torch.equal(fg[i], fg[i + 1]) for i in range(2, 5)), "the replayed graph re-used one set of DropPath factors"
    for i in range(6):
        assert torch.equal(fe[i], fg[i]), "step %d: graph-mode DropPath factors differ from the eager engine's" % i
    assert torch.allclose(torch.tensor(le), torch.tensor(lg), rtol=1e-4), (le, lg)


def test_natural_training_batch32_bf16_graph():
    """BASELINE configs[2] at its real batch size (32 per GPU; TVSP's text map depends on B): three captured bf16 steps are
    finite, and the first loss agrees with the fp32 path on the same weights and batch (bf16 forward deviation only)."""
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    torch.manual_seed(0)
    net = MP_HSIR_Net(compute_dtype=torch.bfloat16, clip_prompt="surrogate").cuda().train()
    src = SyntheticPatchSource(31, 64, 32, 6, "cuda", 2024, 0)
    _, x, c, p = src.next()
    net.eval()
    with torch.no_grad():
        l16 = float((net(x, p).clamp(0, 1) - c).abs().mean())
        net.set_compute_dtype(torch.float32)
        l32 = float((net(x, p).clamp(0, 1) - c).abs().mean())
    assert abs(l16 - l32) < 2e-2 * l32, (l16, l32)
    net.set_compute_dtype(torch.bfloat16).train()
    eng = DataParallelEngine(net, lr=2e-4, use_graph=True, graph_warmup=1)
    losses = [float(eng.train_step(x, c, p)) for _ in range(4)]
    eng.finish()
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0], losses


def test_pack_plan_matches_per_module_packers():
    M.check_pack_plan("cuda")
    M.check_pack_plan("cuda", torch.bfloat16)


def test_graphed_forward_matches_eager():
    """engine.GraphedForward (inference through a replayed hipGraph) returns exactly what the eager forward returns."""
    from mp_hsir_amd.engine import GraphedForward
    from golden.cases import TINY_CFG
    net = M.build_net(TINY_CFG, "cuda", torch.bfloat16)
    run = GraphedForward(net, warmup=1)
    g = torch.Generator(device="cuda").manual_seed(3)
    for i in range(4):
        x = torch.rand((2, 8, 64, 64), generator=g, device="cuda")
        p = torch.randint(0, 6, (2,), generator=g, device="cuda")
        with torch.no_grad():
            ref = net(x, p)
        out = run(x, p)
        assert torch.equal(out, ref), i
    assert any("graph" in e for e in run.entries.values())


def test_fused_gdfn_in_the_no_grad_forward():
    """The no_grad forward runs PromptFusion's feed-forward as ONE launch (mphsir_gdfn_fused) once the level holds >= 16384
    pixels.  Same net, same input, both forms: they agree to bf16 rounding, and against the fp32 forward of the same weights
    the fused form (t kept in fp32 on chip) is not the less accurate one."""
    from mp_hsir_amd import ops
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    torch.manual_seed(5)
    net = MP_HSIR_Net(compute_dtype=torch.bfloat16, clip_prompt="surrogate").cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.rand((4, 31, 64, 64), generator=g, device="cuda")
    p = torch.tensor([0, 1, 2, 3], device="cuda")
    calls = []
    orig = ops.gdfn_fused
    ops.gdfn_fused = lambda *a, **k: (calls.append(a[0].shape), orig(*a, **k))[1]
    keep = ops.GDFN_FUSED_MIN_PIXELS
    try:
        with torch.no_grad():
            y_fused = net(x, p)
            n_fused = len(calls)
            ops.GDFN_FUSED_MIN_PIXELS = 1 << 62
            y_chain = net(x, p)
            assert len(calls) == n_fused
            net.compute_dtype = torch.float32
            ops.bump_weight_epoch()
            y32 = net(x, p)
    finally:
        ops.gdfn_fused, ops.GDFN_FUSED_MIN_PIXELS = orig, keep
    assert n_fused >= 1, "the fused GDFN kernel did not run"
    e_f, e_c = M.rel_l2(y_fused.float().cpu(), y32.float().cpu()), M.rel_l2(y_chain.float().cpu(), y32.float().cpu())
    assert M.rel_l2(y_fused.float().cpu(), y_chain.float().cpu()) < 2e-2
    assert e_f < 4e-2 and e_f < e_c * 1.25 + 1e-4, (e_f, e_c)


@pytest.mark.parametrize("model", ["natural_scene", "remote_sensing"])
@pytest.mark.parametrize("dw_side", [0, 2])
def test_no_parameter_gradient_is_read_before_its_sum(model, dw_side, monkeypatch):
    """ops.DEBUG_DEFERRED: every parameter-gradient sum handed out before it is computed is NaN-filled first on the launch stream,
    so a consumer that read or cloned one early (AccumulateGrad on a strided / shared / hooked gradient, a backward function
    reading a leaf sum) would leave NaN in the gradient arena.  One engine step of each shipped configuration, deferred and on the
    weight-gradient branch: every gradient finite, and equal to the run without the poison."""
    from mp_hsir_amd import ops
    from mp_hsir_amd.data import SyntheticPatchSource
    from mp_hsir_amd.engine import DataParallelEngine
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    cfg = dict(natural_scene=dict(in_channel=31, out_channel=31, dim=64, task_classes=6),
               remote_sensing=dict(in_channel=100, out_channel=100, dim=96, task_classes=7))[model]
    monkeypatch.setattr(ops, "DW_SIDE", dw_side)
    grads = []
    for poison in (False, True):
        monkeypatch.setattr(ops, "DEBUG_DEFERRED", poison)
        torch.manual_seed(5)
        net = MP_HSIR_Net(**cfg, compute_dtype=torch.bfloat16, clip_prompt="surrogate").cuda().train()
        eng = DataParallelEngine(net, lr=0.0, use_graph=False)
        src = SyntheticPatchSource(cfg["in_channel"], 64, 2, cfg["task_classes"], "cuda", 2024, 0)
        for _ in range(2):                       # step 0 builds the arenas, step 1 goes through the one-launch hand-over
            torch.manual_seed(9)
            _, x, c, p = src.next()
            eng.train_step(x, c, p)
        torch.cuda.synchronize()
        assert torch.isfinite(eng.flat_g).all(), "a parameter gradient was read before its sum was launched"
        grads.append(eng.flat_g.clone())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("dw_side", [0, 2])
def test_deferred_parameter_gradient_sums_are_bitwise_the_immediate_ones(dw_side, monkeypatch):
    """The engine collects the partial-sum reductions of all parameter gradients of a backward pass and launches them together
    (ops.deferred_reductions; dw_side = 0) or issues them -- with the weight-gradient GEMMs (2) -- on a second
    stream beside the data-gradient chain.  Every gradient must be bitwise what the per-function launches produce -- in particular
    no gradient may be read (cloned by AccumulateGrad) before its sum has been launched, and nothing may be recycled under the
    side branch."""
    from mp_hsir_amd import ops
    monkeypatch.setattr(ops, "DW_SIDE", dw_side)
    from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net
    torch.manual_seed(11)
    net = MP_HSIR_Net(compute_dtype=torch.bfloat16, clip_prompt="surrogate").cuda().train()
    g = torch.Generator(device="cuda").manual_seed(12)
    xs = [torch.rand((2, 31, 64, 64), generator=g, device="cuda") for _ in range(3)]
    cs = [torch.rand((2, 31, 64, 64), generator=g, device="cuda") for _ in range(3)]
    p = torch.tensor([1, 4], device="cuda")

    def grads(i, deferred):
        net.zero_grad(set_to_none=True)
        torch.manual_seed(100 + i)                      # DropPath draws
        loss = (net(xs[i], p).clamp(0, 1) - cs[i]).abs().mean()
        if deferred:
            with ops.deferred_reductions():
                loss.backward()
        else:
            loss.backward()
        torch.cuda.synchronize()
        return {n: q.grad.clone() for n, q in net.named_parameters() if q.grad is not None}

    ref = grads(0, False)
    grads(1, True)                                      # different data through the same allocator blocks
    grads(2, False)
    got = grads(0, True)
    assert ref.keys() == got.keys() and len(ref) > 600
    bad = [n for n in ref if not torch.equal(ref[n], got[n])]
    assert not bad, bad[:8]
    if dw_side:
        return
    launches = []
    orig = ops._flush
    ops._flush = lambda segs: (launches.append(len(segs)), orig(segs))[1]
    try:
        grads(1, True)
        n_def = list(launches)
        del launches[:]
        grads(1, False)
        n_imm = list(launches)
    finally:
        ops._flush = orig
    # (the forward's own sums -- Gram partials read by the fold right away -- stay one launch each in both runs)
    assert sum(n_def) == sum(n_imm) and len([n for n in n_def if n]) < len([n for n in n_imm if n]) // 2, (n_def, len(n_imm))
