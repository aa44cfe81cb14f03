"""TEST INFRASTRUCTURE: one rank of a gloo data-parallel run for the gradient-accumulation tests (tests/accum_ref.py), or -- imported --
the same run in the calling process (world 1).

    accum_worker.py OUT KIND K STEPS LOSS MODE       KIND: emu | gpu, LOSS: l1 | sam, MODE: eager | graph

emu: the toy net of tests/test_host_logic.py's gloo worker on the CPU-emulated library.  gpu: the tiny MP-HSIR net, every rank on cuda:0
(modelled on tests/dist_graph_worker.py).  A step of the run is one OPTIMIZER step: world * K micro-batches, micro-batch j of rank r being
number q = j * world + r of the step -- so two ranks with K = 1 and one process with K = 2 see the same two micro-batches in the same
roles.  Writes rank r's losses, final state and counts to OUT<r>."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


class ToyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.b = torch.nn.Conv2d(8, 3, 3, padding=1)
        self.unused = torch.nn.Linear(5, 5)          # never receives a gradient

    def forward(self, x, prompt):
        return self.b(torch.nn.functional.gelu(self.a(x))) + x


def toy_data(steps):
    """(steps, 8, 3, 8, 8) inputs and targets: a step's batch of 8 is four micro-batches of 2"""
    g = torch.Generator().manual_seed(7)
    return torch.rand(steps, 8, 3, 8, 8, generator=g), torch.rand(steps, 8, 3, 8, 8, generator=g)


def gpu_micro(step, q):
    """micro-batch q of optimizer step `step` for the tiny net: (degraded, clean, task) on cuda:0"""
    from golden.detfill import seeded_input
    return (seeded_input("acc_x%d_%d" % (step, q), (2, 8, 32, 32)).cuda(), seeded_input("acc_c%d_%d" % (step, q), (2, 8, 32, 32)).cuda(),
            torch.tensor([[q % 5 + 1], [3]]).cuda())


def loss_kw(loss):
    from mp_hsir_amd.engine import SpectralLoss
    return dict(loss_fn=SpectralLoss(sam=0.1)) if loss == "sam" else {}


def run(kind, K, steps, loss, mode, rank=0, world=1):
    """-> dict(losses, state, nbuckets, allreduces, unused)"""
    from mp_hsir_amd.engine import DataParallelEngine
    calls = [0]
    real = dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    try:
        if kind == "emu":
            torch.manual_seed(100 + rank)           # different init per rank: the engine must broadcast rank 0's
            net = ToyNet()
            eng = DataParallelEngine(net, lr=1e-2, bucket_mb=0.0005, accum_steps=K, **loss_kw(loss))     # tiny buckets -> several all-reduces
            xs, cs = toy_data(steps)
        else:
            import model_checks as M
            from golden.cases import TINY_CFG
            net = M.build_net(TINY_CFG, "cuda", torch.float32)
            if rank != 0:
                with torch.no_grad():
                    for p in net.parameters():
                        p.mul_(1.5)
            eng = DataParallelEngine(net, lr=2e-3, use_graph=(mode == "graph"), graph_warmup=2, bucket_mb=0.25, accum_steps=K, **loss_kw(loss))
        losses = []
        for step in range(steps):
            for j in range(K):
                q = j * world + rank
                if kind == "emu":
                    losses.append(float(eng.train_step(xs[step][2 * q:2 * q + 2], cs[step][2 * q:2 * q + 2], None)))
                else:
                    torch.manual_seed(100 + step * world * K + q)
                    losses.append(float(eng.train_step(*gpu_micro(step, q))))
        if kind == "gpu":
            if mode == "graph":
                assert eng._graph is not None, "the captured step never ran"
                eng.finish()
            torch.cuda.synchronize()
    finally:
        dist.all_reduce = real
    return {"losses": losses, "state": {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, "nbuckets": len(eng.buckets),
            "allreduces": calls[0], "unused": len(eng.unused), "step_count": eng.step_count}


def main():
    out, kind, K, steps, loss, mode = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if kind == "emu":
        from emu import bind_emulator
        bind_emulator()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.save(run(kind, K, steps, loss, mode, rank, world), out + str(rank))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
