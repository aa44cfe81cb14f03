"""In-training validation: held-out crops kept on the device, scored between two training steps without a host read-back per batch.

    vset = ValidationSet(files, "natural_scene", device, modes=None, patch=256, seed=2025, net=net)
    val = Validator(net, vset, batch=4, engine=engine)
    result = val.run()          # {mode: {psnr, ssim, sam, n, nonfinite, skipped, psnr_min, psnr_max}, "mean": {...}}

ValidationSet   reads every cube with test.py's conventions (test.load_cube, values as stored), cuts the centre patch x patch crop (or an
                evenly spread k x k grid of crops) and keeps the crops in ONE device tensor (N,C,P,P).  For each of test.py's modes 0-10
                asked for, the degraded crops are made ONCE by one degrade.SceneDegrader(model, device, seed): crop i is its call i, so
                the set is a function of (files, patch, crops, seed, opts) and can be regenerated instead of stored.  The prompt id and,
                for mode 10 (band completion), the mask of the bands that count stay resident with them.
Validator.run   eval() under no_grad; per batch -- crops of ONE mode: TVSP's prompt map couples the samples of a batch and is
                batch-invariant only under one task id -- the forward, ops.quality_bands into persistent buffers and ops.quality_meter
                into the mode's row of a device table.  Nothing is read back until the set is done; then ONE device-to-host copy.

The forward runs eagerly.  engine.GraphedForward ties a capture to the weights it was taken with and drops it when they change, which
between two validation passes of a training run is always: a pass would pay two eager calls and a capture per input shape before its
first replay ("Validation", holds the measurement).  `forward="graphed"` is there for scoring fixed weights repeatedly.

Training is not disturbed: a pass writes no parameter, moment or gradient, draws no random number (eval mode: no drop path), leaves the
captured training step and its key alone (the mode is restored before the next step) and brings the packed-weight caches to the weights
it scores the way engine._swap_ema does -- weight epoch, then the pack plan's gather -- which rewrites the plan's buffers with the
values they hold.  With EMA weights the pass runs inside engine.ema_weights(), which swaps back on exit.
"""
import contextlib
import math
import os

import torch
import torch.distributed as dist

from . import ops

FUSED_MODES = tuple(range(11))                  # test.py's modes with a fused degradation
_REFUSED = {11: "mode 11 is Poisson noise, which has no fused form", 12: "mode 12 evaluates real degraded / clean pairs, which a seeded set cannot regenerate",
            13: "mode 13 is the CASSI measurement of a one-task net, which is not part of the evaluation protocol scored here"}
SLOT = {name: i for i, name in enumerate(ops.QUALITY_METER_SLOTS)}


# ---- host logic (no device needed) -------------------------------------------------------------------------------------------------------
def crop_origins(H, W, patch, crops_per_scene=1):
    """[(y0, x0)] of the crops of an H x W cube: the centre crop, or for crops_per_scene = k * k > 1 a k x k grid whose first and last
    rows / columns touch the cube's edges and whose spacing is even (floor((H - patch) j / (k - 1)))"""
    k = math.isqrt(int(crops_per_scene))
    if k < 1 or k * k != crops_per_scene:
        raise ValueError("crops_per_scene must be a square number (1, 4, 9, ...), got %r" % (crops_per_scene,))
    if H < patch or W < patch:
        raise ValueError("a cube of %d x %d is smaller than the %d x %d crop" % (H, W, patch, patch))
    if k == 1:
        return [((H - patch) // 2, (W - patch) // 2)]
    return [((H - patch) * j // (k - 1), (W - patch) * i // (k - 1)) for j in range(k) for i in range(k)]


def check_modes(modes):
    """the modes as a tuple, each one of test.py's 0-10; 11, 12 and 13 are refused by name"""
    out = []
    for m in modes:
        m = int(m)
        if m in _REFUSED:
            raise ValueError("validation: %s" % _REFUSED[m])
        if m not in FUSED_MODES:
            raise ValueError("validation: unknown mode %d (test.py's modes 0-10)" % m)
        if m in out:
            raise ValueError("validation: mode %d is listed twice" % m)
        out.append(m)
    if not out:
        raise ValueError("validation: no mode to score")
    return tuple(out)


def default_modes(model, task_classes):
    """the modes 0-10 whose prompt id exists in a net with `task_classes` tasks"""
    from .degrade import SceneDegrader
    d = SceneDegrader.__new__(SceneDegrader)
    d.model = model
    return tuple(m for m in FUSED_MODES if d.prompt_id(m) < task_classes)


def shard(n, world, rank):
    """the crop indices rank `rank` of `world` scores: i with i % world == rank"""
    return list(range(rank, n, world))


def summarise(table, modes):
    """table: len(modes) rows of 8 floats (ops.QUALITY_METER_SLOTS) -> {mode: dict(psnr, ssim, sam, n, nonfinite, skipped, psnr_min,
    psnr_max)} plus "mean": the unweighted mean over the modes with n > 0 of the per-mode means, with `modes` (those that entered it)
    and `left_out` (those with n == 0: nothing of theirs was scored)"""
    out, used, left = {}, [], []
    for m, row in zip(modes, table):
        n = int(row[SLOT["n"]])
        d = n if n > 0 else float("nan")
        out[m] = dict(psnr=row[SLOT["psnr_sum"]] / d, ssim=row[SLOT["ssim_sum"]] / d, sam=row[SLOT["sam_sum"]] / d, n=n,
                      nonfinite=int(row[SLOT["nonfinite"]]), skipped=int(row[SLOT["skipped"]]), psnr_min=row[SLOT["psnr_min"]], psnr_max=row[SLOT["psnr_max"]])
        (used if n > 0 else left).append(m)
    k = len(used) if used else float("nan")
    out["mean"] = dict(psnr=sum(out[m]["psnr"] for m in used) / k, ssim=sum(out[m]["ssim"] for m in used) / k, sam=sum(out[m]["sam"] for m in used) / k,
                       nonfinite=sum(out[m]["nonfinite"] for m in modes), modes=list(used), left_out=list(left))
    return out


def improves(result, best):
    """the best-checkpoint rule: the mean PSNR must be finite and above the best so far (`best`: a dict with "psnr", or None), and an
    epoch with ANY image set aside as non-finite never becomes best -- its means are means over the images that behaved"""
    mean = result["mean"]
    if mean["nonfinite"] > 0 or not mean["modes"] or not math.isfinite(mean["psnr"]):
        return False
    return best is None or mean["psnr"] > best["psnr"]


def protocol_note(saved, now):
    """None when the two protocols agree, otherwise the line --resume 1 prints: the scores of the file were taken another way and its
    best does not bind this run"""
    if saved == now:
        return None
    diff = sorted(k for k in set(saved) | set(now) if saved.get(k) != now.get(k))
    return "note: the checkpoint was validated under another protocol (%s differ%s): its history is kept, the best starts anew" % (
        ", ".join(diff), "s" if len(diff) == 1 else "")


class History:
    """what a run knows about its validation passes: the protocol, one row per pass, the best so far (checkpoints carry it as `mphsir_val`)"""

    def __init__(self, protocol):
        self.protocol, self.rows, self.best = dict(protocol), [], None

    def add(self, epoch, result):
        """-> True when this pass is the best so far (improves())"""
        row = dict(epoch=int(epoch), psnr=result["mean"]["psnr"], ssim=result["mean"]["ssim"], sam=result["mean"]["sam"], nonfinite=result["mean"]["nonfinite"],
                   modes={m: dict(result[m]) for m in result if m != "mean"})
        self.rows.append(row)
        if improves(result, self.best):
            self.best = dict(epoch=row["epoch"], psnr=row["psnr"], ssim=row["ssim"], sam=row["sam"])
            return True
        return False

    def state(self):
        return {"protocol": dict(self.protocol), "history": [dict(r) for r in self.rows], "best": None if self.best is None else dict(self.best)}

    def restore(self, state):
        """adopt a checkpoint's `mphsir_val`; -> the note to print when its protocol differs (then the best starts anew), else None"""
        self.rows = [dict(r) for r in state.get("history", [])]
        note = protocol_note(state.get("protocol", {}), self.protocol)
        self.best = None if note is not None or state.get("best") is None else dict(state["best"])
        return note


def result_lines(epoch, result):
    """the lines rank 0 prints after a pass: one per mode, then the mean"""
    lines = []
    for m in (k for k in result if k != "mean"):
        r = result[m]
        lines.append("val epoch %d mode %d psnr %.4f ssim %.5f sam %.4f n %d%s" % (epoch, m, r["psnr"], r["ssim"], r["sam"], r["n"],
                                                                                  " nonfinite %d" % r["nonfinite"] if r["nonfinite"] else ""))
    mean = result["mean"]
    lines.append("val epoch %d mean psnr %.4f ssim %.5f sam %.4f" % (epoch, mean["psnr"], mean["ssim"], mean["sam"]))
    return lines


# ---- the held-out set ---------------------------------------------------------------------------------------------------------------------
class ValidationSet:
    """files: cube paths (.mat 'data' / .npy, (C,H,W)); model: "natural_scene" / "remote_sensing" (mode 10's prompt id); modes: test.py's
    modes to score (None: every mode 0-10 whose prompt id `net` has -- `net`, or its task count `task_classes`, is then needed); patch: a
    multiple of 64; crops_per_scene: 1 or k * k; seed: of the degraded set; opts: test.py's parsed flags (default: its defaults).  `bands`:
    the model's band count (default: the net's) -- a cube with another count is refused by name, and so is one smaller than `patch`."""

    def __init__(self, files, model, device, modes=None, patch=256, crops_per_scene=1, seed=2025, opts=None, net=None, bands=None, task_classes=None):
        from . import test as T
        if patch < 64 or patch % 64:
            raise ValueError("validation: patch must be a multiple of 64, got %d" % patch)
        if bands is None:
            bands = net.patch_embed.proj.weight.shape[1] if net is not None else {"natural_scene": 31, "remote_sensing": 100}[model]
        crops, names = [], []
        for f in files:
            cube = T.load_cube(f)
            name = os.path.basename(f)
            if cube.ndim != 3 or cube.shape[0] != bands:
                raise ValueError("validation: cube %s has shape %s, the model takes %s bands" % (name, tuple(cube.shape), bands))
            try:
                origins = crop_origins(cube.shape[1], cube.shape[2], patch, crops_per_scene)
            except ValueError as e:
                raise ValueError("validation: cube %s: %s" % (name, e))
            for y0, x0 in origins:
                crops.append(torch.from_numpy(cube[:, y0:y0 + patch, x0:x0 + patch].copy()))
            names.append(name)
        if not crops:
            raise ValueError("validation: no cube to score")
        self._init(torch.stack(crops), model, device, modes, seed, opts, net, task_classes)
        self.files, self.crops_per_scene = names, int(crops_per_scene)

    @classmethod
    def from_crops(cls, crops, model, device, modes=None, seed=2025, opts=None, net=None, task_classes=None):
        """a set of crops (N,C,P,P) that exist already (a tensor or an array; any P the net takes)"""
        self = cls.__new__(cls)
        self._init(torch.as_tensor(crops), model, device, modes, seed, opts, net, task_classes)
        self.files, self.crops_per_scene = [], 1
        return self

    def _init(self, crops, model, device, modes, seed, opts, net, task_classes):
        from . import test as T
        from .degrade import SceneDegrader
        assert crops.dim() == 4 and crops.shape[2] == crops.shape[3], "validation: crops (N,C,P,P), got %s" % (tuple(crops.shape),)
        if task_classes is None and net is not None:
            task_classes = net.text_prompt.task_classes
        if modes is None:
            if task_classes is None:
                raise ValueError("validation: without modes the net (or its task count) is needed to choose them")
            modes = default_modes(model, task_classes)
        self.modes = check_modes(modes)
        self.model, self.device, self.seed = model, torch.device(device), int(seed)
        self.opts = T.build_parser().parse_args([]) if opts is None else opts
        self.clean = crops.to(self.device, torch.float32).contiguous()                   # (N,C,P,P), values as stored
        self.patch = int(crops.shape[2])
        self.degraded, self.prompt, self.use = {}, {}, {}
        for m in self.modes:
            deg = SceneDegrader(model, self.device, self.seed)
            pid = deg.prompt_id(m)
            if task_classes is not None and pid >= task_classes:
                raise ValueError("validation: mode %d needs prompt id %d, the net has %d tasks" % (m, pid, task_classes))
            out = torch.empty_like(self.clean)
            for i in range(len(self.clean)):                                             # crop i is call i: the ordinal is the crop index
                out[i] = deg(self.clean[i:i + 1], m, self.opts)[0][0].float()
            self.degraded[m], self.prompt[m] = out, pid
            self.use[m] = (out == 0).flatten(2).all(dim=2).to(torch.uint8).contiguous() if m == 10 else None      # band completion: the bands
                                                                                                                   # entirely zero in the degraded crop

    def __len__(self):
        return self.clean.shape[0]

    def protocol(self, weights="auto"):
        return {"modes": list(self.modes), "patch": self.patch, "crops": self.crops_per_scene, "seed": self.seed, "weights": weights, "files": list(self.files)}


# ---- the pass -----------------------------------------------------------------------------------------------------------------------------
class Validator:
    """net: the network being trained; vset: a ValidationSet on its device; batch: crops per forward (one mode each; the last batch of a
    mode is padded with its last crop and the meter counts the first n); engine: the DataParallelEngine that trains `net`, or None;
    weights: "auto" (the EMA weights when the engine keeps them, else the current ones), "ema" or "raw"; forward: "eager" / "graphed"."""

    def __init__(self, net, vset, batch=4, engine=None, weights="auto", forward="eager"):
        if weights not in ("auto", "ema", "raw"):
            raise ValueError("validation: weights must be auto, ema or raw, got %r" % (weights,))
        if forward not in ("eager", "graphed"):
            raise ValueError("validation: forward must be eager or graphed, got %r" % (forward,))
        if weights == "ema" and engine is None:
            raise ValueError("validation: weights='ema' needs the engine that keeps them")
        self.net, self.vset, self.batch, self.engine, self.weights = net, vset, int(batch), engine, weights
        assert self.batch >= 1
        self.world = engine.world if engine is not None else 1
        self.rank = dist.get_rank(engine.pg) if self.world > 1 else 0
        self.idx = shard(len(vset), self.world, self.rank)
        dev, (N, C, P, _) = vset.device, vset.clean.shape
        if self.world > 1:                                       # this rank's crops, gathered once
            ix = torch.tensor(self.idx, dtype=torch.long, device=dev)
            take = lambda t: None if t is None else t.index_select(0, ix)          # noqa: E731
        else:
            take = lambda t: t                                                     # noqa: E731
        self._clean = take(vset.clean)
        self._degraded = {m: take(vset.degraded[m]) for m in vset.modes}
        self._use = {m: take(vset.use[m]) for m in vset.modes}
        B = self.batch
        self._prompt = {m: torch.full((B,), vset.prompt[m], dtype=torch.long, device=dev) for m in vset.modes}
        self._x, self._c = torch.empty((B, C, P, P), device=dev), torch.empty((B, C, P, P), device=dev)           # the padded last batch
        self._u = torch.empty((B, C), dtype=torch.uint8, device=dev)
        self._q = ops.quality_buffers(B, C, P, P, dev)
        self.table = torch.zeros((len(vset.modes), 8), dtype=torch.float64, device=dev)
        self._run = None
        if forward == "graphed":
            from .engine import GraphedForward
            self._run = GraphedForward(net)

    def uses_ema(self):
        """whether a pass scores the EMA weights now; weights='ema' without an EMA arena stops with a message"""
        has = self.engine is not None and getattr(self.engine, "flat_ema", None) is not None
        if self.weights == "ema" and not has:
            raise RuntimeError("validation: weights='ema', but the engine keeps no EMA weights (build it with ema_decay, and take a step first)")
        return has and self.weights in ("auto", "ema")

    @contextlib.contextmanager
    def _scored_weights(self):
        eng = self.engine
        if self.uses_ema():
            with eng.ema_weights():
                yield
            return
        if eng is not None:
            # a replayed training step updates the arena behind the per-module caches: bring them to the current weights as
            # engine._swap_ema does (the gather rewrites the plan's buffers with what the captured step left in them)
            ops.bump_weight_epoch()
            if eng.plan is not None:
                eng.plan.refresh()
        yield

    def _batches(self, m):
        """yields (x, clean, use, n) of mode m: whole batches are views of the resident tensors, the last one is padded with its last crop"""
        B, deg, use, N = self.batch, self._degraded[m], self._use[m], len(self.idx)
        for i0 in range(0, N, B):
            n = min(B, N - i0)
            if n == B:
                yield deg[i0:i0 + B], self._clean[i0:i0 + B], None if use is None else use[i0:i0 + B], n
                continue
            for buf, src in ((self._x, deg), (self._c, self._clean)) + (() if use is None else ((self._u, use),)):
                buf[:n].copy_(src[i0:i0 + n])
                buf[n:].copy_(src[N - 1:N].expand(B - n, *src.shape[1:]))
            yield self._x, self._c, None if use is None else self._u, n

    def _score(self, return_restored):
        vset, restored = self.vset, {}
        for r, m in enumerate(vset.modes):
            kept = []
            if not self.idx:
                ops.quality_meter(self.table, r, *self._q[:4], n=0, reset=True)          # a rank without crops: the row is initialised
            for j, (x, c, use, n) in enumerate(self._batches(m)):
                y = self._run(x, self._prompt[m]) if self._run is not None else self.net(x, self._prompt[m])
                y = (y if y.dtype == torch.float32 else y.float()).contiguous()
                p, s, a, npix = ops.quality_bands(y, c, out=self._q)
                ops.quality_meter(self.table, r, p, s, a, npix, use=use, n=n, reset=j == 0)
                if return_restored:
                    kept.append(y[:n].clone())
            if return_restored:
                restored[m] = torch.cat(kept) if kept else self._clean[:0]
        table = self.table
        if self.world > 1:
            # the counts and sums add up over the ranks (one small float64 all-reduce), the extremes take min and max
            sums = table.clone()
            sums[:, SLOT["psnr_min"]:SLOT["psnr_max"] + 1] = 0.0
            lo, hi = table[:, SLOT["psnr_min"]].clone(), table[:, SLOT["psnr_max"]].clone()
            dist.all_reduce(sums, group=self.engine.pg)
            dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.engine.pg)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.engine.pg)
            sums[:, SLOT["psnr_min"]], sums[:, SLOT["psnr_max"]] = lo, hi
            table = sums
        self.last_table = table.cpu()                                                    # the ONE device-to-host copy of a pass
        return summarise(self.last_table.tolist(), vset.modes), restored

    def run(self, return_restored=False):
        """one pass over the set -> the result dict (module docstring); return_restored=True: (result, {mode: restored crops (n,C,P,P)
        of this rank}), for debugging and the tests"""
        net = self.net
        was = net.training
        net.eval()
        try:
            with torch.no_grad(), self._scored_weights():
                result, restored = self._score(return_restored)
        finally:
            net.train(was)
        return (result, restored) if return_restored else result
