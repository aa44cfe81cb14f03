"""TEST INFRASTRUCTURE: one rank of a world-N validation pass on the CPU -- the two-convolution network of tests/optim_ex_ref.py, the
kernels through the emulated build, a gloo process group over 127.0.0.1.  Launched by tests/test_validate_host.py the way
tests/test_gpu_model.py launches tests/dist_graph_worker.py (RANK / WORLD_SIZE / MASTER_* in the environment); with WORLD_SIZE=1 it is
the one-process reference.  Writes rank r's result dict and table to <out><r>."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODES = (0, 8, 10)        # mode 10 on 3 bands masks int(0.3 * 3) = 0 of them: no image has a band to score, the mode is left out of the mean


def crops():
    import numpy as np
    return np.random.default_rng(4711).random((5, 3, 16, 16), dtype=np.float32)


def build(engine_world):
    from emu import bind_emulator
    bind_emulator()
    import optim_ex_ref as X
    from mp_hsir_amd import validate
    from mp_hsir_amd.engine import DataParallelEngine
    net = X.make_net("conv", "cpu")
    eng = DataParallelEngine(net, lr=1e-3) if engine_world else None
    vset = validate.ValidationSet.from_crops(crops(), "natural_scene", "cpu", modes=MODES, seed=7, task_classes=6)
    return net, vset, validate.Validator(net, vset, batch=2, engine=eng, weights="raw")


def main():
    out = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, _, val = build(True)
    assert val.world == world and val.idx == list(range(rank, 5, world))
    result = val.run()
    torch.save({"result": result, "table": val.last_table.clone()}, out + str(rank))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
