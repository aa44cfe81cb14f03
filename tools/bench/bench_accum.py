"""Gradient accumulation (mp-hsir_amd/csrc/arena.hip multi_accum_kernel, engine.DataParallelEngine(accum_steps=K)): what the accumulating
hand-over costs and what a micro-batch costs.

    python tools/bench/bench_accum.py [handover] [step] [default]          (no argument: all legs)

handover  the gradient hand-over at the natural-scene arena, over the REAL list of gradient tensors a batch-32 bf16 step leaves (taken from a
          backward pass, not from a constant): mphsir_multi_copy, mphsir_multi_accum at micro index 0 and at index 1, a device-to-device
          copy_ of the same bytes (8 B per element), a copy_ of 1.5 x the bytes (index 1 is a read-modify-write: 12 B per element) and
          torch._foreach_add_ over the same list, which is what index 1 replaces.  COLD inputs: every call of a timed region works on another
          of SETS copies of the gradients and the arena (SETS x 115 MB, several times the 256 MB Infinity Cache), so that no call finds its
          operands where the call before left them.  Alternating, two rounds, the second is reported.  Twice: as eager calls (617 table rows
          written in Python per call: the host's time) and with every (operation, set) captured once and replayed in rotation, which is how
          the training step issues its hand-over (the device's time).
step      bench.py's workload through the engine directly (natural-scene model, bf16, batch 32, 64 x 64 patches, graph mode) at accum_steps
          1, 2, 4, 8 in one process, in alternating order: time per micro-batch, and the optimizer + plan.refresh() of a group timed alone.
default   the default path (accum_steps=1): time per step and the launch list of an eager step from ops.ACCOUNT (printed sorted, to be
          compared with another commit's).
Every time is the median of REGIONS timed regions (device events around several calls each), printed with min and max.
"""
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
import torch  # noqa: E402

from mp_hsir_amd import ops  # noqa: E402
from mp_hsir_amd.data import SyntheticPatchSource  # noqa: E402
from mp_hsir_amd.engine import DataParallelEngine  # noqa: E402
from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net  # noqa: E402

dev = torch.device("cuda")
REGIONS = 7
SETS = 8
CFG = dict(in_channel=31, out_channel=31, dim=64, task_classes=6)


def timed(fn, per_region, warm=2):
    """-> (median, min, max) milliseconds per call over REGIONS regions of per_region calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REGIONS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(per_region):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / per_region)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def fmt(t, nbytes=None):
    s = "%.4f ms [%.4f .. %.4f]" % t
    return s + (" = %.2f TB/s" % (nbytes / t[0] / 1e9) if nbytes else "")


def engine(batch=32, use_graph=True, **kw):
    torch.manual_seed(2024)
    net = MP_HSIR_Net(**CFG, compute_dtype=torch.bfloat16, clip_prompt="surrogate").to(dev).train()
    src = SyntheticPatchSource(CFG["in_channel"], 64, batch, CFG["task_classes"], dev, 2024, 0, pool=8).prefill()
    eng = DataParallelEngine(net, lr=2e-4, use_graph=use_graph, **kw)

    def step():
        _, x, c, p = src.next()
        return eng.train_step(x, c, p)
    return eng, step, src


def leg_handover():
    eng, step, src = engine(use_graph=False)
    step()
    step()                                                  # the arenas and the pack plan exist
    _, x, c, p = src.next()
    eng._loss_backward(eng.net(x, p), c)                    # a backward pass whose gradients stay where autograd left them
    torch.cuda.synchronize()
    used, offs, n = eng.arena
    ok = [q.grad is not None and q.grad.is_contiguous() and q.grad.dtype == torch.float32 for q in used]
    grads = [q.grad for q, good in zip(used, ok) if good]
    print("arena: %d fp32 elements = %.1f MB in %d gradient tensors (%d more are not contiguous fp32 and left out), %d of them not 16-byte aligned"
          % (n, 4e-6 * n, len(grads), len(ok) - sum(ok), sum(g.data_ptr() % 16 != 0 for g in grads)), flush=True)
    shapes = [(q.shape, o, q.numel()) for q, o, good in zip(used, offs, ok) if good]
    sets = []
    for _ in range(SETS):                                   # a set: its own copy of every gradient tensor and its own arena
        arena = torch.zeros(n, device=dev)
        sets.append(([arena[o:o + k].view(sh) for sh, o, k in shapes], [g.clone() for g in grads]))
    for q in used:
        q.grad = None
    del eng, step
    torch.cuda.empty_cache()
    mc = ops.MultiCopy(dev, len(grads), ring=SETS)
    big_s, big_d = torch.empty(SETS * 3 * n // 2, device=dev), torch.empty(SETS * 3 * n // 2, device=dev)
    turn = [0]

    def rot(fn):
        def call():
            turn[0] = (turn[0] + 1) % SETS
            fn(turn[0])
        return call

    def copy_of(k):                                         # a copy_ of k floats moves 8 k bytes; every call another slice
        return rot(lambda i: big_d[i * k:(i + 1) * k].copy_(big_s[i * k:(i + 1) * k]))
    elems = sum(k for _, _, k in shapes)
    calls = [
        ("multi_copy", rot(lambda i: mc(*sets[i])), 8),
        ("multi_accum index 0", rot(lambda i: mc(*sets[i], micro=0)), 8),
        ("multi_accum index 1", rot(lambda i: mc(*sets[i], micro=1)), 12),
        ("_foreach_add_", rot(lambda i: torch._foreach_add_(sets[i][0], sets[i][1])), 12),
        ("copy_ 8 B per element", copy_of(elems), 8),
        ("copy_ 12 B per element", copy_of(elems * 3 // 2), 12),
    ]
    def report(title, calls):
        rows = {}
        for rnd in range(2):
            for name, fn, bpe in calls:
                rows[name] = timed(fn, SETS)
        print(title, flush=True)
        for name, fn, bpe in calls:
            print("  %-24s %s" % (name, fmt(rows[name], bpe * elems)), flush=True)
        a1 = rows["multi_accum index 1"][0]
        print("  multi_copy / copy_ 8 B %.2f | index 0 / copy_ 8 B %.2f | index 1 / copy_ 8 B %.2f | index 1 / copy_ 12 B %.2f | index 1 / _foreach_add_ %.2f"
              % (rows["multi_copy"][0] / rows["copy_ 8 B per element"][0], rows["multi_accum index 0"][0] / rows["copy_ 8 B per element"][0],
                 a1 / rows["copy_ 8 B per element"][0], a1 / rows["copy_ 12 B per element"][0], a1 / rows["_foreach_add_"][0]), flush=True)

    # eager calls: what the host can enqueue -- the table of 617 rows is written in Python per call, the framework walks the same list
    report("eager calls (the time of a call is the host's):", calls)
    # the launches alone: each (operation, set) captured once and replayed in rotation, as the training step replays its hand-over -- the
    # table copy is a node of the graph, no Python runs
    mc = ops.MultiCopy(dev, len(grads), capture_tables=3 * SETS)
    index = [torch.full((), v, dtype=torch.int32, device=dev) for v in (0, 1)]

    def replayed(fn):
        graphs = []
        torch.cuda.synchronize()
        for i in range(SETS):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                fn(i)
            graphs.append(g)
        return rot(lambda i: graphs[i].replay())
    k8, k12 = elems, elems * 3 // 2
    report("replayed launches (device time, cold operands):", [
        ("multi_copy", replayed(lambda i: mc(*sets[i])), 8),
        ("multi_accum index 0", replayed(lambda i: mc(*sets[i], micro=index[0])), 8),
        ("multi_accum index 1", replayed(lambda i: mc(*sets[i], micro=index[1])), 12),
        ("_foreach_add_", replayed(lambda i: torch._foreach_add_(sets[i][0], sets[i][1])), 12),
        ("copy_ 8 B per element", replayed(lambda i: big_d[i * k8:(i + 1) * k8].copy_(big_s[i * k8:(i + 1) * k8])), 8),
        ("copy_ 12 B per element", replayed(lambda i: big_d[i * k12:(i + 1) * k12].copy_(big_s[i * k12:(i + 1) * k12])), 12),
    ])


def leg_step():
    ks = (1, 2, 4, 8)
    engines = {k: engine(accum_steps=k) for k in ks}
    for k in ks:
        for _ in range(4 * k):                              # eager groups, the capture, a few replays
            engines[k][1]()
    torch.cuda.synchronize()

    def group(k):
        stepk = engines[k][1]

        def run():
            for _ in range(k):
                stepk()
        return run
    for rnd in range(3):
        line = []
        for k in (ks if rnd % 2 == 0 else ks[::-1]):
            t = timed(group(k), max(1, 8 // k))
            line.append((k, tuple(v / k for v in t)))
        print("round %d: " % (rnd + 1) + " | ".join("K %d: %s per micro-batch = %.1f patches/s" % (k, fmt(t), 32e3 / t[0]) for k, t in sorted(line)), flush=True)
        per = dict(line)
        print("         non-final micro-batch, from K = 8 against K = 2: %.4f ms" % ((8 * per[8][0] - 2 * per[2][0]) / 6), flush=True)
    eng = engines[2][0]

    def tail():
        eng._optimizer_step(None, hyper=eng._hyper)
        eng.plan.refresh()
    t = timed(tail, 10)
    print("optimizer + plan.refresh() alone (plain launches, warm arenas): %s" % fmt(t), flush=True)


def leg_default():
    eng, step, _ = engine()
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    for rnd in range(3):
        t = timed(step, 10)
        print("default path, run %d: %s per step = %.1f patches/s" % (rnd + 1, fmt(t), 32e3 / t[0]), flush=True)
    del eng, step
    torch.cuda.empty_cache()
    fresh, step, _ = engine()
    step()
    ops.ACCOUNT = {}
    step()                                                  # an eager step with the arenas in place: its launches, by name
    acct, ops.ACCOUNT = ops.ACCOUNT, None
    print("launches of a default step (ops.ACCOUNT): %s" % sorted((k, v[0]) for k, v in acct.items()))


if __name__ == "__main__":
    for leg in sys.argv[1:] or ["handover", "step", "default"]:
        {"handover": leg_handover, "step": leg_step, "default": leg_default}[leg]()
