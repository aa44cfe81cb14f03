"""TEST INFRASTRUCTURE: checks of mp-hsir_amd/validate.py that run on the device they are given -- the two-convolution network of
tests/optim_ex_ref.py through the emulated kernels on the CPU ("conv"), model_checks.build_net(TINY_CFG) on an MI355X ("tiny")."""
import numpy as np
import torch

import spectral_loss_ref as S
from util import bits  # noqa: F401  (the tests reach it through this module)


def make_vset(dev, kind, net=None, seed=11):
    """5 seeded crops: (5,3,16,16) and modes 0, 8 for the conv net; (5,8,32,32) and modes 0, 5, 10 for the tiny net"""
    from mp_hsir_amd import validate
    shape, modes = ((5, 3, 16, 16), (0, 8)) if kind == "conv" else ((5, 8, 32, 32), (0, 5, 10))
    crops = np.random.default_rng(815).random(shape, dtype=np.float32)
    return validate.ValidationSet.from_crops(crops, "natural_scene", dev, modes=modes, seed=seed, net=net if kind != "conv" else None, task_classes=6)


def _rng_states(dev):
    out = [torch.get_rng_state()]
    if torch.device(dev).type == "cuda":
        out.append(torch.cuda.get_rng_state())
    return out


def _steps(dev, kind, use_graph, dtype, with_val, ema, account=False):
    """four steps, with a pass (two under `ema`: the averaged and the raw weights) after step 2 when asked -> what training computed"""
    from mp_hsir_amd import ops, validate
    net, eng = S.make_engine(dev, kind, use_graph, dtype, **(dict(ema_decay=0.9) if ema else {}))
    net.train()                                 # a pass has a mode to switch and to restore; the tiny net then draws drop-path factors
    torch.manual_seed(4242)                     # ... from torch's generators: both runs start from one state, and a pass must not advance it
    val = raw = None
    if with_val:
        vset = make_vset(dev, kind, net)
        val = validate.Validator(net, vset, batch=2, engine=eng, weights="ema" if ema else "auto")
        raw = validate.Validator(net, vset, batch=2, engine=eng, weights="raw") if ema else None
    rec, scores, acct = [], None, None
    graph = None
    try:
        for s in range(4):
            if account and s == 3:
                ops.ACCOUNT = {}
            rec.append((bits(eng.train_step(*S.batch(s, dev, kind)).clone()), bits(eng.flat_g)))
            if ops.ACCOUNT is not None:
                acct = {k: v[0] for k, v in ops.ACCOUNT.items()}
                ops.ACCOUNT = None
            if use_graph and s >= 1:
                assert eng._graph is not None, "the graph-mode engine never captured"
                assert graph is None or eng._graph is graph, "the engine captured again after the pass"
                graph = eng._graph
            if s == 1 and with_val:
                key, plan, dp, mode = eng._graph_key, eng.plan, net.__dict__.get("_dp_last"), net.training
                arenas = [eng.flat_p, eng.flat_m, eng.flat_v, eng.flat_g] + ([eng.flat_ema] if ema else [])
                packed = [] if plan is None else [buf for _, buf in plan.groups.values()]
                before = [bits(t) for t in arenas + packed]
                rng = _rng_states(dev)
                scores = {"auto": val.run()}
                if ema:
                    assert val.uses_ema()
                    scores["raw"] = raw.run()
                assert [bits(t) for t in arenas + packed] == before, "a pass changed parameters, moments, gradients, EMA or the packed weights"
                assert net.training == mode, "the network's mode was not restored"
                assert eng._graph is graph and eng._graph_key == key, "the captured step or its key changed"
                assert eng.plan is plan and net.__dict__.get("_dp_last") is dp, "the pack plan or the drop-path state changed"
                assert all(torch.equal(a, b) for a, b in zip(rng, _rng_states(dev))), "a pass drew random numbers"
    finally:
        ops.ACCOUNT = None
        if eng._graph is not None:              # destroyed here, not at the collector's whim (see spectral_loss_ref.run_engine)
            torch.cuda.synchronize()
            eng._graph = graph = None
    return dict(rec=rec, p=bits(eng.flat_p), ema=bits(eng.flat_ema) if ema else None, scores=scores, acct=acct)


def check_training_undisturbed(dev, kind="tiny", use_graph=False, dtype=torch.float32, ema=False):
    """four steps with a validation pass after step 2 against four steps without one: losses, gradient arenas per step, flat_p (and
    flat_ema) bitwise equal; in graph mode no second capture; under `ema` the averaged weights score differently from the raw ones"""
    a = _steps(dev, kind, use_graph, dtype, False, ema)
    b = _steps(dev, kind, use_graph, dtype, True, ema)
    print("losses equal %s, gradient arenas equal %s, parameters equal %s" % ([x[0] == y[0] for x, y in zip(a["rec"], b["rec"])],
                                                                                 [x[1] == y[1] for x, y in zip(a["rec"], b["rec"])], a["p"] == b["p"]))
    assert a["rec"] == b["rec"] and a["p"] == b["p"] and a["ema"] == b["ema"]
    first = b["scores"]["auto"]
    m0 = [m for m in first if m != "mean"][0]
    assert first[m0]["n"] == 5 and np.isfinite(first["mean"]["psnr"])
    if ema:
        raw = b["scores"]["raw"]
        print("mode %s psnr: ema %.6f raw %.6f" % (m0, first[m0]["psnr"], raw[m0]["psnr"]))
        assert first[m0]["psnr"] != raw[m0]["psnr"], "weights='ema' scored the raw weights"
    return b


def check_off_by_default(dev, kind="tiny"):
    """a training step issues the same launches whether or not a Validator exists and has run: the ops.ACCOUNT launch list of the last of
    four eager steps, with a pass after step 2 and without (and the parameters are bitwise equal)"""
    a = _steps(dev, kind, False, torch.float32, False, False, account=True)
    b = _steps(dev, kind, False, torch.float32, True, False, account=True)
    assert a["acct"] and a["acct"] == b["acct"], (a["acct"], b["acct"])
    assert "quality" not in a["acct"] and "quality_meter" not in a["acct"] and a["p"] == b["p"]
