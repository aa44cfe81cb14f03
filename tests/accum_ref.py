"""Gradient accumulation (mp-hsir_amd/csrc/arena.hip multi_accum_kernel, ops.MultiCopy(micro=), engine.DataParallelEngine(accum_steps=K)):
the checks, parametrised by device.  tests/test_accum_emu.py runs them through the CPU-emulated build, tests/test_accum_gpu.py on the GPU,
tests/test_accum_host.py holds what needs neither.

What accumulation MEANS is exact: index 0 stores, every later index is one fp32 addition per element, so the arena after micro-batch j is
torch's fp32 ((g_0 + g_1) + ...) + g_j bit for bit, and K micro-batches are what K data-parallel ranks compute (at K = 2 bitwise: a + b =
b + a).  The bars that are not bitwise are copied from the checks they extend: optim_ex_ref.RefState.compare (rel-L2 2e-6 per arena), two
fp32 ulp for the reported norm, tests/test_host_logic.py's rtol 2e-5 / atol 2e-6 against torch.optim.AdamW, tests/test_gpu_model.py
_check_world2's loss rtol 2e-4 and 2e-2 relative update error."""
import contextlib
import ctypes
import io
import math
import os
import subprocess
import sys

import numpy as np
import torch

import guard
import optim_ex_ref as R
from util import bits, same_floats, ulp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "accum_worker.py")

# ---- the kernel -------------------------------------------------------------------------------------------------------------------------------
# one table of 10 rows: lengths around the 4-float vector and the 4096-float block; (src offset, dst offset) in floats off 16 bytes covers all
# four combinations, each of them at a length beyond one block
LENS = (1, 3, 4, 5, 4095, 4096, 4097, 8195, 12288, 2)
SRC_OFF = (0, 1, 0, 1, 0, 1, 0, 1, 0, 1)
DST_OFF = (0, 0, 1, 1, 0, 0, 1, 1, 0, 1)
GAP = 8                                   # floats between two destination slots: never written


def _layout():
    """-> (arena length, [(start, n)]): slot i starts DST_OFF[i] floats past a multiple of 4, GAP untouched floats lie between slots"""
    slots, o = [], GAP
    for n, d in zip(LENS, DST_OFF):
        o = (o + 3) // 4 * 4 + d
        slots.append((o, n))
        o += n + GAP
    return (o + 3) // 4 * 4, slots


def _sources(G, dev, micro, special=False):
    """fresh sources of micro-batch `micro` (CPU masters and device tensors); under the guard each lies between NaN bands and is compared
    with its master after the check"""
    masters, srcs = [], []
    for i, (n, off) in enumerate(zip(LENS, SRC_OFF)):
        g = torch.Generator().manual_seed(7100 + 16 * micro + i)
        m = torch.randn(n + off, generator=g)
        if special and n >= 5:
            m[off + 0], m[off + 2], m[off + 4] = float("nan"), float("inf"), float("-inf")
            if n > 4100:
                m[off + 4097], m[off + 4099] = float("inf"), float("-inf")
        t = G.input(m, seed=7100 + 16 * micro + i) if G is not None else m.to(dev)
        masters.append(m[off:])
        srcs.append(t[off:])
        assert srcs[-1].data_ptr() % 16 == 4 * off
    return masters, srcs


def _arena(G, dev):
    total, slots = _layout()
    arena = G.alloc((total,), torch.float32, torch.device(dev), "output", fill=float("nan")) if G is not None else torch.full((total,), float("nan"), device=dev)
    assert arena.data_ptr() % 16 == 0
    dsts = [arena[o:o + n] for o, n in slots]
    assert all(d.data_ptr() % 16 == 4 * off for d, off in zip(dsts, DST_OFF))
    gaps = torch.ones(total, dtype=torch.bool)
    for o, n in slots:
        gaps[o:o + n] = False
    return arena, dsts, gaps


def _index(form, dev, micro, cell):
    """the micro index as the host value or as the device int32 (one tensor, rewritten per call)"""
    if form == "host":
        return micro
    cell.fill_(micro)
    return cell


@guard.guarded
def check_kernel(dev, form, special=False):
    """indices 0, 1, 2 with fresh sources -> the arena bits after each.  Index 0 over a NaN-filled arena: the sources bitwise, no NaN left;
    then torch's fp32 (g0 + g1) + g2 bitwise; gaps and (through the guard) bands and sources untouched.  special: NaN and +-inf in the
    sources are stored as they are at index 0 and propagate by IEEE rules after"""
    from mp_hsir_amd import ops
    G = guard.active()
    arena, dsts, gaps = _arena(G, dev)
    gap_bits = bits(arena.cpu()[gaps])
    mc = ops.MultiCopy(torch.device(dev), len(LENS), ring=2)
    cell = torch.zeros((), dtype=torch.int32, device=dev)
    want, out = None, []
    ops.ACCOUNT = {}
    try:
        for micro in range(3):
            masters, srcs = _sources(G, dev, micro, special)
            mc(dsts, srcs, micro=_index(form, dev, micro, cell))
            want = [m.clone() for m in masters] if micro == 0 else [w + m for w, m in zip(want, masters)]
            got = arena.cpu()
            for (o, n), w, m in zip(_layout()[1], want, masters):
                if micro == 0:
                    assert bits(got[o:o + n]) == bits(m), "index 0 must store the source as it is (n %d)" % n
                    assert special or not bool(torch.isnan(got[o:o + n]).any())
                elif special:
                    assert same_floats(got[o:o + n].numpy(), w.numpy()), "index %d, n %d: NaN / inf do not propagate as IEEE addition does" % (micro, n)
                else:
                    assert bits(got[o:o + n]) == bits(w), "index %d, n %d: not the fp32 running sum" % (micro, n)
            assert bits(got[gaps]) == gap_bits, "a gap between two slots was written"
            for s, m in zip(srcs, masters):
                assert bits(s.cpu()) == bits(m), "a source changed"
            out.append(bits(got))
        assert sorted(ops.ACCOUNT) == ["multi_accum"] and ops.ACCOUNT["multi_accum"][0] == 3
        ne = float(sum(LENS))
        # 8 B per element at index 0, 12 B from index 1 on (a device index is not known to the host: counted as the read-modify-write form)
        assert ops.ACCOUNT["multi_accum"][2] == ((8.0 + 12.0 + 12.0) if form == "host" else 36.0) * ne
    finally:
        ops.ACCOUNT = None
    return out


def check_kernel_forms(dev):
    """host index and device index give the same bits, and so do two runs of either"""
    a, b, c = check_kernel(dev, "host"), check_kernel(dev, "device"), check_kernel(dev, "host")
    assert a == b, "the index as a host value and as a device int32 give different arenas"
    assert a == c, "two runs differ"
    s1, s2 = check_kernel(dev, "host", special=True), check_kernel(dev, "device", special=True)
    assert s1 == s2


@guard.guarded
def check_copy_form_is_the_old_launch(dev):
    """MultiCopy(..., micro=None) issues mphsir_multi_copy and not the new launch"""
    from mp_hsir_amd import ops
    G = guard.active()
    arena, dsts, _ = _arena(G, dev)
    masters, srcs = _sources(G, dev, 0)
    mc = ops.MultiCopy(torch.device(dev), len(LENS), ring=2)
    ops.ACCOUNT = {}
    try:
        mc(dsts, srcs)
        mc(dsts, srcs, micro=None)
        assert sorted(ops.ACCOUNT) == ["multi_copy"] and ops.ACCOUNT["multi_copy"][0] == 2, sorted(ops.ACCOUNT)
        assert ops.ACCOUNT["multi_copy"][2] == 2 * 8.0 * sum(LENS)
    finally:
        ops.ACCOUNT = None
    for d, m in zip(dsts, masters):
        assert bits(d.cpu()) == bits(m)


@guard.guarded
def check_refusals(dev):
    """every refusal: MPHSIR_EINVAL, a message that names the cause, the arena bitwise unchanged"""
    import mp_hsir_amd._lib as L
    from mp_hsir_amd import ops
    lib = L.load()
    G = guard.active()
    arena, dsts, _ = _arena(G, dev)
    masters, srcs = _sources(G, dev, 0)
    rows, blk = [], 0
    for d, s in zip(dsts, srcs):
        rows.append((s.data_ptr(), d.data_ptr(), d.numel(), blk))
        blk += (d.numel() + 4095) // 4096
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    cell = torch.ones((), dtype=torch.int32, device=dev)
    keep = bits(arena)
    stream = ops._stream(arena)

    def args(**kw):
        a = L.MultiAccumArgs(table_dev=table.data_ptr(), nseg=len(rows), total_blocks=blk, micro=1, micro_dev=None)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.mphsir_multi_accum(ctypes.byref(a), stream) == L.CONSTANTS["MPHSIR_EINVAL"], text
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()

    refused(args(struct_size=ctypes.sizeof(L.MultiAccumArgs) - 8), "struct_size")
    refused(args(struct_size=ctypes.sizeof(L.MultiAccumArgs) + 8), "struct_size")
    refused(args(table_dev=None), "null table")
    refused(args(nseg=0), "no rows")
    refused(args(nseg=-3), "no rows")
    for bad in (0, -1, 2 ** 31, 2 ** 40):
        refused(args(total_blocks=bad), "total_blocks")
    refused(args(micro=-1), "negative")
    refused(args(micro=-1, micro_dev=cell.data_ptr()), "negative")
    for call in (lambda: ops.MultiCopy(torch.device(dev), len(LENS))(dsts, srcs, micro=-1),
                 lambda: ops.MultiCopy(torch.device(dev), len(LENS))(dsts, srcs, micro=torch.zeros((), dtype=torch.int64, device=dev))):
        try:
            call()
        except (RuntimeError, AssertionError):
            pass
        else:
            raise AssertionError("the wrapper accepted what the entry point refuses")
    assert bits(arena) == keep, "something was launched"
    assert lib.mphsir_multi_accum(ctypes.byref(args(micro=0)), stream) == 0          # the same arguments with nothing wrong: it runs
    for d, m in zip(dsts, masters):
        assert bits(d.cpu()) == bits(m)


def check_kernel_graph():
    """GPU only: the launch captured ONCE with the device index, replayed three times with the index set to 0, 1, 2 and the sources
    overwritten in place between replays; capturing alone changes nothing.  -> the arena bits after each replay"""
    from mp_hsir_amd import ops
    dev = "cuda"
    arena, dsts, gaps = _arena(None, dev)
    gap_bits, start = bits(arena.cpu()[gaps]), bits(arena)
    masters, srcs = _sources(None, dev, 0)
    mc = ops.MultiCopy(torch.device(dev), len(LENS))
    cell = torch.zeros((), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        mc(dsts, srcs, micro=cell)
    torch.cuda.synchronize()
    assert bits(arena) == start, "capturing must not run the launch"
    want, out = None, []
    for micro in range(3):
        masters = _sources(None, "cpu", micro)[0]
        for s, m in zip(srcs, masters):
            s.copy_(m)
        cell.fill_(micro)
        graph.replay()
        want = [m.clone() for m in masters] if micro == 0 else [w + m for w, m in zip(want, masters)]
        got = arena.cpu()
        for (o, n), w in zip(_layout()[1], want):
            assert bits(got[o:o + n]) == bits(w), "replay %d, n %d" % (micro, n)
        assert bits(got[gaps]) == gap_bits
        out.append(bits(got))
    # no table left for a captured accumulating hand-over: a clear error, not the framework's copy
    # (the wrapper decides before it touches the device: it is asked as if a capture were running, none is started for this)
    mc.for_capture = []
    real = torch.cuda.is_current_stream_capturing
    torch.cuda.is_current_stream_capturing = lambda: True
    try:
        mc(dsts, srcs, micro=cell)
    except RuntimeError as e:
        assert "no pointer table left" in str(e), e
    else:
        raise AssertionError("an accumulating hand-over without a table under capture must raise")
    finally:
        torch.cuda.is_current_stream_capturing = real
    torch.cuda.synchronize()
    assert bits(arena) == out[-1]
    return out


# ---- the engine -------------------------------------------------------------------------------------------------------------------------------
def batch(call, dev, kind):
    from golden.detfill import seeded_input
    shape = (4, 3, 8, 8) if kind == "conv" else (2, 8, 32, 32)
    return (seeded_input("ac_x%d" % call, shape).to(dev), seeded_input("ac_c%d" % call, shape).to(dev), torch.tensor([[1], [3]]).to(dev))


def make_engine(dev, kind, dtype=torch.float32, **kw):
    from mp_hsir_amd.engine import DataParallelEngine
    net = R.make_net(kind, dev)
    if dtype != torch.float32:
        net.set_compute_dtype(dtype)
    kw.setdefault("lr", 2e-3)
    return net, DataParallelEngine(net, **kw)


def step(eng, call, dev, kind, lr=None, edit=None):
    torch.manual_seed(100 + call)
    x, c, task = batch(call, dev, kind)
    if edit is not None:
        edit(x)
    return eng.train_step(x, c, task, lr=lr)


def _launches(fn):
    """the launch list of fn() by ops.ACCOUNT: {name: launches}"""
    from mp_hsir_amd import ops
    ops.ACCOUNT = {}
    try:
        fn()
        return {k: v[0] for k, v in ops.ACCOUNT.items()}
    finally:
        ops.ACCOUNT = None


def check_off_is_off(dev, kind, use_graph=False):
    """accum_steps=1 against an engine built without the keyword, 3 steps: parameters, moments and flat_g bitwise equal, the per-step
    launch list identical, no multi_accum in it"""
    runs = []
    for kw in ({}, {"accum_steps": 1}):
        net, eng = make_engine(dev, kind, use_graph=use_graph, graph_warmup=1 if use_graph else 2, **kw)
        per_step = [_launches(lambda s=s: step(eng, s, dev, kind)) for s in range(3)]
        assert use_graph == (eng._graph is not None)
        runs.append((per_step, [bits(t) for t in (eng.flat_p, eng.flat_m, eng.flat_v, eng.flat_g)]))
        assert eng.group_loss is None
    assert runs[0][0] == runs[1][0], "the launch list changed"
    assert all("multi_accum" not in s for s in runs[1][0]) and any("multi_copy" in s for s in runs[1][0])
    assert runs[0][1] == runs[1][1]


def check_arena_holds_the_sum(dev, kind):
    """K = 3, the learning rate staged as 0: after each call flat_g is bitwise the fp32 running sum of the arenas of three accum_steps=1
    engines with the same weights run on one micro-batch each; group_loss is ((l0 + l1) + l2) * fp32(1/3).  A second group over the same
    micro-batches (weights unchanged at lr 0) must overwrite the first group's sum: nothing is zero-filled, index 0 stores"""
    from mp_hsir_amd import ops
    singles = []
    for j in range(3):
        net1, eng1 = make_engine(dev, kind)
        step(eng1, j, dev, kind, lr=0.0)
        singles.append(eng1.flat_g.clone())
    net, eng = make_engine(dev, kind, accum_steps=3)
    for group in range(2):
        running, losses, seen = None, [], {}
        for j in range(3):
            moments = None if eng.arena is None else bits(eng.flat_m)
            seen = _launches(lambda j=j: losses.append(step(eng, j, dev, kind, lr=0.0).clone()))
            running = singles[0].clone() if j == 0 else running + singles[j]
            assert bits(eng.flat_g) == bits(running), "group %d call %d: the arena is not the fp32 running sum" % (group, j)
            assert eng.step_count == group + (j == 2)
            if moments is not None:
                assert (bits(eng.flat_m) != moments) == (j == 2), "the optimizer runs on the last call of a group and on no other"
            if group == 1:
                assert seen.get("multi_accum", 0) >= 1 and "multi_copy" not in seen, seen
        want = ((losses[0] + losses[1]) + losses[2]) * torch.tensor(1.0 / 3.0, dtype=torch.float32, device=dev)
        assert eng.group_loss.dtype == torch.float32 and eng.group_loss.dim() == 0 and eng.group_loss.device.type == torch.device(dev).type
        assert bits(eng.group_loss) == bits(want), (float(eng.group_loss), float(want))
    assert ops.ACCOUNT is None


def _arena_init(eng, init):
    p0 = torch.zeros_like(eng.flat_p)
    for p, o in zip(*eng.arena[:2]):
        p0[o:o + p.numel()] = init[id(p)].reshape(-1)
    return p0


def check_the_step(dev, kind, use_graph=False):
    """K = 2, grad_clip below the measured norm, ema_decay 0.9: every group's step against optim_ex_ref.RefState (float64) stepped with the
    summed arena and grad_scale 1/2, at RefState.compare's bars; the reported norm within 2 fp32 ulp of the float64 norm of the mean
    gradient; after K - 1 calls of a group parameters, moments, EMA and step_count are bitwise what they were"""
    lr, decay = 2e-3, 0.9
    _, probe = make_engine(dev, kind, accum_steps=2, grad_clip=1e9)
    for call in range(2):
        step(probe, call, dev, kind)
    norm0 = probe.grad_stats()["norm"]
    want0 = 0.5 * math.sqrt(float(np.sum(R.f64(probe.flat_g) ** 2)))
    assert abs(norm0 - want0) <= 2 * ulp32(want0), (norm0, want0)
    clip = 0.5 * norm0
    net, eng = make_engine(dev, kind, lr=lr, accum_steps=2, grad_clip=clip, ema_decay=decay, use_graph=use_graph, graph_warmup=1)
    init = {id(p): p.detach().clone() for p in net.parameters()}
    state0 = [bits(v) for v in net.state_dict().values()]
    for group in range(3):
        before = None if eng.arena is None else [x.clone() for x in (eng.flat_p, eng.flat_m, eng.flat_v, eng.flat_ema)]
        step(eng, 2 * group, dev, kind)
        assert eng.step_count == group
        if before is None:
            assert [bits(v) for v in net.state_dict().values()] == state0 and eng.flat_ema is not None and bits(eng.flat_ema) == bits(eng.flat_p)
            before = [_arena_init(eng, init), torch.zeros_like(eng.flat_m), torch.zeros_like(eng.flat_v), _arena_init(eng, init)]
            assert bits(eng.flat_p) == bits(before[0]) and bits(eng.flat_m) == bits(before[1]) and bits(eng.flat_v) == bits(before[2])
        else:
            assert [bits(x) for x in (eng.flat_p, eng.flat_m, eng.flat_v, eng.flat_ema)] == [bits(x) for x in before], "call K - 2 of a group changed the state"
        step(eng, 2 * group + 1, dev, kind)
        t = group + 1
        assert eng.step_count == t
        ref = R.RefState(*before[:3], ema=before[3])
        norm, coef = ref.step(eng.flat_g, lr, t, max_norm=clip, grad_scale=0.5, decay=R.ema_decay_at(decay, t, True),
                              bc=(1.0 - 0.9 ** t, math.sqrt(1.0 - 0.999 ** t)))
        st = eng.grad_stats()
        print("group %d: norm %.6g (float64 %.6g) coef %.4f" % (group, st["norm"], norm, st["coef"]))
        assert abs(st["norm"] - norm) <= 2 * ulp32(norm) and abs(st["coef"] - coef) <= 2 * ulp32(coef) and st["skipped"] == 0
        if group == 0:
            assert coef < 1.0, "the test is meant to clip"
        ref.compare(eng.flat_p, eng.flat_m, eng.flat_v, eng.flat_ema, "group %d" % group)
    assert use_graph == (eng._graph is not None)


def check_eager_equals_graph(dtype, loss):
    """GPU only.  K = 2, three groups, graph_warmup=1: losses, flat_g after every call, group_loss and the final flat_p bitwise equal between
    eager and graph mode; exactly one capture"""
    from mp_hsir_amd.engine import SpectralLoss
    dev, kind = "cuda", "tiny"
    runs = []
    for use_graph in (False, True):
        kw = dict(loss_fn=SpectralLoss(sam=0.1)) if loss == "sam" else {}
        net, eng = make_engine(dev, kind, dtype=dtype, accum_steps=2, use_graph=use_graph, graph_warmup=1, **kw)
        rec, graphs = [], []
        for call in range(6):
            rec.append(bits(step(eng, call, dev, kind)))
            rec.append(bits(eng.flat_g))
            if call % 2 == 1:
                rec.append(bits(eng.group_loss))
            graphs.append(eng._graph)
        rec.append(bits(eng.flat_p))
        if use_graph:
            assert graphs[0] is None and graphs[1] is None, "the first group runs eager: the switch happens at a group boundary"
            assert graphs[2] is not None and all(g is graphs[2] for g in graphs[2:]), "one capture serves every micro-batch of every group"
            assert len(eng._multi_copy.captured) == len(eng.buckets)
        else:
            assert all(g is None for g in graphs)
        assert eng.step_count == 3 and bool(torch.isfinite(eng.flat_p).all())
        runs.append(rec)
    diff = [i for i, (a, b) in enumerate(zip(*runs)) if a != b]
    assert not diff, "eager and graph mode differ, first at record %d of %d" % (diff[0], len(runs[0]))


def check_nonfinite_micro_batch(dev, kind, scaler):
    """K = 2.  One element of micro-batch 0's input of the second group is inf: parameters and moments are bitwise unchanged after the group
    and the next clean group steps; with the loss scaler (fp32, loss_scaling=True) the scale has halved once, with grad_clip instead the
    skip count rises by exactly 1"""
    kw = dict(loss_scaling=True, init_scale=1024.0) if scaler else dict(grad_clip=1e9)
    net, eng = make_engine(dev, kind, accum_steps=2, **kw)

    def poison(x):
        x.view(-1)[x.numel() // 2 + 3] = float("inf")

    for call in range(2):
        step(eng, call, dev, kind)
    keep = [bits(x) for x in (eng.flat_p, eng.flat_m, eng.flat_v)]
    if scaler:
        assert float(eng.scaler[0]) == 1024.0
    else:
        assert eng.grad_stats()["skipped"] == 0
    step(eng, 2, dev, kind, edit=poison)
    step(eng, 3, dev, kind)
    assert not bool(torch.isfinite(eng.flat_g).all()), "the test is meant to accumulate a non-finite gradient"
    assert [bits(x) for x in (eng.flat_p, eng.flat_m, eng.flat_v)] == keep, "a group with a non-finite micro-batch must not step"
    if scaler:
        assert float(eng.scaler[0]) == 512.0, float(eng.scaler[0])
    else:
        assert eng.grad_stats()["skipped"] == 1
    for call in range(4, 6):
        step(eng, call, dev, kind)
    assert bits(eng.flat_p) != keep[0] and bool(torch.isfinite(eng.flat_p).all()) and bool(torch.isfinite(eng.flat_g).all())
    if scaler:
        assert float(eng.scaler[0]) == 512.0
    else:
        assert eng.grad_stats()["skipped"] == 1


def check_checkpoint(tmp_path):
    """GPU only.  Two groups -> save_checkpoint -> a new net and engine -> load_warm_start(resume=True) -> two more groups == four groups
    straight through, bitwise: parameters, moments, EMA; the checkpoint holds accum_steps; resuming with another value prints the note"""
    import importlib
    T = importlib.import_module("mp_hsir_amd.train")
    dev, kind = "cuda", "tiny"
    kw = dict(lr=2e-3, accum_steps=2, grad_clip=0.2, ema_decay=0.9)

    def run(eng, calls):
        for call in calls:
            step(eng, call, dev, kind, lr=2e-3)
        torch.cuda.synchronize()

    net_a, eng_a = make_engine(dev, kind, **kw)
    net_a.train()
    run(eng_a, range(8))
    net_b, eng_b = make_engine(dev, kind, **kw)
    net_b.train()
    run(eng_b, range(4))
    path = str(tmp_path / "epoch=3.ckpt")
    T.save_checkpoint(path, net_b, eng_b, epoch=3)
    ckpt = torch.load(path, map_location="cpu")
    assert ckpt["accum_steps"] == 2 and ckpt["mphsir_optimizer"]["step"] == 2
    net_c, eng_c = make_engine(dev, kind, **kw)
    net_c.train()
    with torch.no_grad():
        for p in net_c.parameters():
            p.mul_(0.5)                           # everything must come from the file
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        n, start = T.load_warm_start(net_c, path, torch.device(dev), eng_c, resume=True)
    assert start == 4 and "accum_steps" not in said.getvalue()
    run(eng_c, range(4, 8))
    for (k, va), vc in zip(net_a.state_dict().items(), net_c.state_dict().values()):
        assert torch.equal(va, vc), k
    sa, sc = eng_a.optimizer_state(), eng_c.optimizer_state()
    assert sa["step"] == sc["step"] == 4
    for k in sa["exp_avg"]:
        assert torch.equal(sa["exp_avg"][k], sc["exp_avg"][k]) and torch.equal(sa["exp_avg_sq"][k], sc["exp_avg_sq"][k]) and torch.equal(sa["ema"][k], sc["ema"][k]), k
    for other, flag in ((4, "--accum_steps 4"), (1, "--accum_steps 1")):
        net_d, eng_d = make_engine(dev, kind, **dict(kw, accum_steps=other))
        said = io.StringIO()
        with contextlib.redirect_stdout(said):
            T.load_warm_start(net_d, path, torch.device(dev), eng_d, resume=True)
        assert "the checkpoint was trained with --accum_steps 2, this run continues with %s" % flag in said.getvalue(), said.getvalue()
        assert eng_d.accum_steps == other
    # a file written with the feature off carries no new key
    net_e, eng_e = make_engine(dev, kind)
    step(eng_e, 0, dev, kind)
    T.save_checkpoint(str(tmp_path / "off.ckpt"), net_e, eng_e, epoch=0)
    assert "accum_steps" not in torch.load(str(tmp_path / "off.ckpt"), map_location="cpu")


# ---- accumulation = data parallelism ----------------------------------------------------------------------------------------------------------
def spawn_ranks(out, kind, K, steps, loss, mode, port, limit):
    """two ranks of tests/accum_worker.py over gloo, each under its own time limit -> their results"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, WORKER, out, kind, str(K), str(steps), loss, mode], env=dict(env, RANK=str(r)))
             for r in range(2)]
    codes = [p.wait(timeout=limit + 30) for p in procs]
    assert codes == [0, 0], codes
    return [torch.load(out + str(r)) for r in range(2)]


def check_emu_accumulation_is_data_parallelism(tmp_path):
    """emulator, gloo, toy net, three optimizer steps.  (1) one process with accum_steps=2 on (a_i, b_i) == two ranks with accum_steps=1
    holding a_i and b_i, parameters BITWISE: the two-rank sum is one fp32 addition and so is the accumulation.  Both sides run under
    SpectralLoss(sam=0.1), whose steps stage Adam's scalars on the device at accum_steps=1 too (under the default loss an eager
    accum_steps=1 step hands the kernel lr and the step number and the library forms the bias corrections with fp32 powf -- engine.py's
    comment on _eager_hyper -- which differs in the last bits for a reason that has nothing to do with accumulation).
    (2) two ranks x accum_steps=2 == torch.optim.AdamW on the full batch of 8 at tests/test_host_logic.py's bars; the ranks are bitwise
    identical; all-reduces per optimizer step == buckets, not K x buckets"""
    import accum_worker as W
    res = spawn_ranks(str(tmp_path / "k1_"), "emu", 1, 3, "sam", "eager", 29561, 280)
    one = W.run("emu", 2, 3, "sam", "eager")
    for k in one["state"]:
        assert torch.equal(res[0]["state"][k], res[1]["state"][k]), "ranks diverged: " + k
        assert bits(one["state"][k]) == bits(res[0]["state"][k]), "accum_steps=2 in one process differs from two ranks: " + k
    assert one["step_count"] == res[0]["step_count"] == 3 and one["allreduces"] == 0
    assert [one["losses"][0::2], one["losses"][1::2]] == [res[0]["losses"], res[1]["losses"]]
    assert res[0]["nbuckets"] >= 2 and res[0]["allreduces"] == 3 * res[0]["nbuckets"]

    res = spawn_ranks(str(tmp_path / "k2_"), "emu", 2, 3, "l1", "eager", 29563, 280)
    for k in res[0]["state"]:
        assert torch.equal(res[0]["state"][k], res[1]["state"][k]), "ranks diverged: " + k
    assert res[0]["nbuckets"] >= 2 and res[0]["unused"] == 2
    assert res[0]["allreduces"] == res[1]["allreduces"] == 3 * res[0]["nbuckets"], (res[0]["allreduces"], res[0]["nbuckets"])
    torch.manual_seed(100)
    net = W.ToyNet()
    unused0 = net.unused.weight.detach().clone()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2)
    xs, cs = W.toy_data(3)
    for i in range(3):
        opt.zero_grad(set_to_none=True)
        ((net(xs[i], None).clamp(0, 1) - cs[i]).abs().mean()).backward()
        opt.step()
    for k, v in net.state_dict().items():
        assert torch.allclose(res[0]["state"][k], v, rtol=2e-5, atol=2e-6), k
    assert torch.equal(res[0]["state"]["unused.weight"], unused0)


def check_gpu_two_ranks_equal_accum2(tmp_path):
    """MI355X, one GPU shared by two ranks over gloo (accum_steps=1, graph mode, SpectralLoss(sam=0.1)) against one in-process engine with
    accum_steps=2 on the same micro-batches: parameters after 4 optimizer steps BITWISE equal"""
    import accum_worker as W
    res = spawn_ranks(str(tmp_path / "g1_"), "gpu", 1, 4, "sam", "graph", 29565, 240)
    one = W.run("gpu", 2, 4, "sam", "graph")
    for k in one["state"]:
        assert torch.equal(res[0]["state"][k], res[1]["state"][k]), "ranks diverged: " + k
    diff = [k for k in one["state"] if bits(one["state"][k]) != bits(res[0]["state"][k])]
    assert not diff, "accum_steps=2 in one process differs from two ranks in %d tensors, first %s" % (len(diff), diff[0])
    assert [one["losses"][0::2], one["losses"][1::2]] == [res[0]["losses"], res[1]["losses"]]
    assert one["step_count"] == res[0]["step_count"] == 4


def check_gpu_two_ranks_accum2_against_torch(tmp_path):
    """two ranks x accum_steps=2 in graph mode against tests/test_gpu_model.py _check_world2's kind of reference: torch AdamW over all four
    micro-batches with loss / 4; its bars: losses rtol 2e-4, update < 2e-2 relative"""
    import accum_worker as W
    import model_checks as M
    from golden.cases import TINY_CFG
    steps = 4
    res = spawn_ranks(str(tmp_path / "g2_"), "gpu", 2, steps, "l1", "graph", 29567, 240)
    for k in res[0]["state"]:
        assert torch.equal(res[0]["state"][k], res[1]["state"][k]), "ranks diverged: " + k
    assert res[0]["step_count"] == steps
    net = M.build_net(TINY_CFG, "cuda", torch.float32)
    p0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt = torch.optim.AdamW([p for p in net.parameters()], lr=2e-3)
    ref_losses = [[], []]
    for s in range(steps):
        opt.zero_grad(set_to_none=True)
        for q in range(4):
            torch.manual_seed(100 + s * 4 + q)
            x, c, task = W.gpu_micro(s, q)
            loss = (net(x, task).clamp(0, 1) - c).abs().mean()
            (loss / 4).backward()
            ref_losses[q % 2].append(float(loss.detach()))
        opt.step()
    for r in range(2):
        want = ref_losses[r]                                     # rank r's micro-batches in call order: q = 2 j + r
        assert torch.allclose(torch.tensor(res[r]["losses"]), torch.tensor(want), rtol=2e-4, atol=1e-7), (r, res[r]["losses"], want)
    for k, v in net.state_dict().items():
        if not v.is_floating_point() or k.endswith("attn_mask"):
            continue
        d_ref, d_got = (v.detach() - p0[k]).double().cpu(), (res[0]["state"][k].cuda() - p0[k]).double().cpu()
        if float(d_ref.norm()) == 0.0:
            assert float(d_got.norm()) == 0.0, k
            continue
        assert float((d_got - d_ref).norm() / d_ref.norm()) < 2e-2, (k, float((d_got - d_ref).norm() / d_ref.norm()))
