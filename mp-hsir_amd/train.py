#!/usr/bin/env python3
"""Training script: the reference's train.py (PromptIRModel + pl.Trainer, train.py:37-120) re-expressed as
one process per GPU with RCCL gradient all-reduce (engine.DataParallelEngine).

    python mp-hsir_amd/train.py --data_type natural_scene --epochs 100 --lr 2e-4 --batch_size 32
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 mp-hsir_amd/train.py ...

Same loss (clamp + L1, :58-61), optimizer (AdamW(lr) defaults, :69), schedule (linear warm-up over
0.1*epochs then cosine to 1e-6, stepped per epoch, :71-85 -- including lr(0) = 0), seed handling (:88-92),
warm start from a Lightning checkpoint by key+shape filtering with the `net.` prefix (:109-116) and a
checkpoint every 50 epochs (:104).  Data: --synthetic 1 (default; datasets are not available offline) feeds
data.SyntheticPatchSource; --synthetic 0 --db_path <dir> reads the reference's patch records (data.PatchDB, the LMDB
record format in a flat file); --synthetic 0 --scene_dir <dir> builds the scene pyramid of the directory's .mat / .npy cubes
once, keeps it in HBM and cuts every batch out of it on the device (scene_store.SceneStore, data.SceneStoreSource; --crop_jitter 1 moves
the origins).  Either way the per-task degradations of --*_single_de_type are synthesised on the GPU
(degrade.DegradationSynthesizer).  Checkpoints carry, besides the `net.`-prefixed state_dict, AdamW's moments and step
count and the CLIP text-embedding table the model was built with.  --ckpt_path is the reference's warm start (weights whose
key and shape match, epoch 0); --resume 1 additionally restores the optimizer state and continues at the saved epoch + 1.
--loss_sam F / --loss_sdiff F (both 0 by default: the reference's loss) add the mean spectral angle and the L1 of band-to-band
differences to the loss (engine.SpectralLoss); the log line then ends with the unweighted terms, checkpoints carry the weights as
`mphsir_loss` and --resume 1 says so when the run's weights differ from the file's.  --loss_ssim F (0 by default) adds F * (1 - SSIM), the
band-wise 7 x 7 SSIM the evaluation reports, by a launch pair of its own; the log line then also ends with ` ssim S`.
--accum_steps K (1 by default: off) takes one optimizer step per K batches (engine.DataParallelEngine(accum_steps=K)): K micro-batches are
what K data-parallel ranks compute, not one batch of K * batch_size; `it` and --log_every then count optimizer steps and `train_loss` is the
mean loss of the group.
--val_every E --val_dir DIR (0 by default: off) scores held-out crops after every E-th epoch and after the last (validate.py: the crops and
their degraded forms of test.py's modes stay on the device, a pass reads back one small table); rank 0 prints `val epoch E mode M psnr ..
ssim .. sam .. n ..` per mode and `val epoch E mean ...`, --save_best 1 writes <ckpt_dir>/best.ckpt whenever the mean PSNR improves, and
checkpoints carry protocol, history and best as `mphsir_val` (--resume 1 restores them, and says so when the protocol differs).
"""
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mp_hsir_amd import degrade  # noqa: E402
from mp_hsir_amd.data import REMOTE_SENSING_SOURCES, PatchDB, PatchDBSource, SceneStoreSource, SyntheticPatchSource  # noqa: E402
from mp_hsir_amd.engine import DataParallelEngine, SpectralLoss, warmup_cosine_lr  # noqa: E402
from mp_hsir_amd.net.MP_HSIR import _TASK_PROMPTS, MP_HSIR_Net  # noqa: E402
from mp_hsir_amd.options import options as opt  # noqa: E402
from mp_hsir_amd.scene_store import SceneStore, scene_files  # noqa: E402

MODELS = {"natural_scene": dict(in_channel=31, out_channel=31, dim=64, task_classes=6),     # train.py:44
          "remote_sensing": dict(in_channel=100, out_channel=100, dim=96, task_classes=7)}  # train.py:45


def set_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def saved_clip_table(ckpt, task_classes):
    """the CLIP text-embedding table a checkpoint of this script carries, if it fits a model with `task_classes` tasks
    (a natural-scene checkpoint, 6 x 512, warm-starting the remote-sensing model, 7 x 512, brings no table).
    ckpt: the loaded checkpoint dict, or a path."""
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt, map_location="cpu")
    table = ckpt.get("mphsir_clip_prompt")
    return table if table is not None and tuple(table.shape) == (task_classes, 512) else None


def load_warm_start(net, path, device, engine=None, resume=False):
    """The reference's warm start (train.py:109-116): keep checkpoint entries whose key AND shape match (keys carry the
    `net.` prefix), nothing else -- training starts at epoch 0 whatever wrote the checkpoint.  resume=True (--resume 1, a
    checkpoint written by save_checkpoint) also restores the optimizer state into `engine` and returns the epoch to
    continue at.  A saved CLIP table of the model's own shape must match the model's (a model built on other text
    embeddings would silently mis-evaluate); a table of another shape belongs to the other configuration and is ignored."""
    ckpt = path if isinstance(path, dict) else torch.load(path, map_location=device)      # main() loads the file once for both helpers
    state = ckpt["state_dict"]
    own = {"net." + k: v for k, v in net.state_dict().items()}
    kept = {k[4:]: v for k, v in state.items() if k in own and own[k].shape == v.shape}
    net.load_state_dict(kept, strict=False)
    table = ckpt.get("mphsir_clip_prompt")
    if table is not None and tuple(table.shape) == tuple(net.clip_prompts.shape) and \
            not torch.allclose(table.float().cpu(), net.clip_prompts.float().cpu(), atol=1e-5):
        raise RuntimeError("%s was trained with other CLIP text embeddings than this model was built with; build the model "
                           "with clip_prompt=ckpt['mphsir_clip_prompt']" % (path if not isinstance(path, dict) else "the checkpoint"))
    resume_epoch = 0
    if resume:
        if engine is None or "mphsir_optimizer" not in ckpt:
            raise RuntimeError("--resume 1 needs a checkpoint written by this script (optimizer state); %s has none"
                               % (path if not isinstance(path, dict) else "this one"))
        engine.load_optimizer_state(ckpt["mphsir_optimizer"])          # with --ema_decay: the EMA too (a state without one starts it from the weights)
        resume_epoch = int(ckpt.get("epoch", -1)) + 1
        was, now = ckpt.get("mphsir_loss") or {"sam": 0.0, "sdiff": 0.0}, loss_weights(engine)
        if was != now:
            named = "ssim" in was or "ssim" in now                    # the SSIM weight is named only when either side has one
            said = ["sam %g sdiff %g" % (w["sam"], w["sdiff"]) + (" ssim %g" % w.get("ssim", 0.0) if named else "") for w in (was, now)]
            print("note: the checkpoint was trained with loss weights %s, this run continues with %s" % tuple(said), flush=True)
        was_k, now_k = int(ckpt.get("accum_steps", 1)), getattr(engine, "accum_steps", 1)
        if was_k != now_k:
            print("note: the checkpoint was trained with --accum_steps %d, this run continues with --accum_steps %d" % (was_k, now_k), flush=True)
    return len(kept), resume_epoch


def loss_weights(engine):
    """the weights of the spectral terms of the engine's loss ({"sam": 0, "sdiff": 0}: the reference's clamp + L1), and "ssim" when the
    SSIM term is on"""
    fn = getattr(engine, "loss_fn", None)
    return fn.weights() if isinstance(fn, SpectralLoss) else {"sam": 0.0, "sdiff": 0.0}


def save_checkpoint(path, net, engine, epoch, val=None):
    """Lightning-compatible layout (`state_dict` with the `net.` prefix, `epoch`) + what resuming needs; with EMA weights on,
    `state_dict_ema` holds them in the same layout (test.py --use_ema 1).  val: a validate.History -- its protocol, rows and best so
    far are saved as `mphsir_val` (a run without validation writes the file it always wrote)."""
    ckpt = {"state_dict": {"net." + k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, "epoch": epoch,
            "mphsir_optimizer": engine.optimizer_state(), "mphsir_clip_prompt": net.clip_prompts.detach().cpu().clone(),
            "mphsir_clip_source": net.text_prompt.clip_source, "mphsir_loss": loss_weights(engine)}
    if getattr(engine, "accum_steps", 1) > 1:      # written at epoch ends: a group is never open in a checkpoint
        ckpt["accum_steps"] = engine.accum_steps
    if getattr(engine, "ema_decay", None) is not None:
        ckpt["state_dict_ema"] = {"net." + k: v.detach().cpu().clone() for k, v in engine.ema_state_dict().items()}
    if val is not None:
        ckpt["mphsir_val"] = val.state()
    torch.save(ckpt, path)


def build_validation(opt, net, eng, data_type, dev):
    """-> (validate.Validator, validate.History) of --val_dir / --val_*; every refusal ends the run with its message before any training"""
    from mp_hsir_amd import validate
    if not opt.val_dir:
        raise SystemExit("--val_every %d needs --val_dir <directory of held-out .mat / .npy cubes>" % opt.val_every)
    if opt.val_every < 0:
        raise SystemExit("--val_every must be >= 0 (0: off)")
    if opt.val_weights == "ema" and opt.ema_decay <= 0:
        raise SystemExit("--val_weights ema needs --ema_decay")
    try:
        modes = [int(m) for m in opt.val_modes.split(",") if m.strip()] or None
        vset = validate.ValidationSet(scene_files(opt.val_dir), data_type, dev, modes=modes, patch=opt.val_patch, crops_per_scene=opt.val_crops,
                                      seed=opt.val_seed, net=net)
        val = validate.Validator(net, vset, batch=opt.val_batch, engine=eng, weights=opt.val_weights)
    except ValueError as e:
        raise SystemExit(str(e))
    return val, validate.History(vset.protocol(opt.val_weights))


def main():
    rank, local, world = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("LOCAL_RANK", 0), ("WORLD_SIZE", 1)))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    if rank == 0:
        print("Options\n", opt)
    if opt.val_every and not opt.val_dir:
        raise SystemExit("--val_every %d needs --val_dir <directory of held-out .mat / .npy cubes>" % opt.val_every)
    set_seed(opt.seed)
    cfg = dict(MODELS[opt.model or opt.data_type])
    if opt.task_classes:
        cfg["task_classes"] = opt.task_classes                           # --task_classes 1: the one-task net of the cassi fine-tune
    clip_prompt = "surrogate" if opt.allow_surrogate_clip else None      # None: encode with OpenAI clip, or raise
    ckpt = None
    if opt.ckpt_path is not None:
        ckpt = torch.load(opt.ckpt_path, map_location="cpu")          # once: the CLIP table now, weights (+ optimizer) below
        saved = saved_clip_table(ckpt, cfg["task_classes"])
        clip_prompt = saved if saved is not None else clip_prompt
    dtypes = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}
    net = MP_HSIR_Net(**cfg, clip_prompt=clip_prompt, compute_dtype=dtypes[opt.precision]).to(dev).train()
    extras = opt.grad_clip > 0 or opt.ema_decay > 0
    if opt.loss_sam < 0 or opt.loss_sdiff < 0 or opt.loss_ssim < 0:
        raise SystemExit("--loss_sam / --loss_sdiff / --loss_ssim must be >= 0 (0: the term is off)")
    if opt.accum_steps < 1:
        raise SystemExit("--accum_steps must be >= 1 (1: off), got %d" % opt.accum_steps)
    spectral = opt.loss_sam > 0 or opt.loss_sdiff > 0 or opt.loss_ssim > 0      # off: the engine's default loss, the launches and the log lines of always
    eng = DataParallelEngine(net, lr=opt.lr, use_graph=bool(opt.graph), grad_clip=opt.grad_clip if opt.grad_clip > 0 else (float("inf") if extras else None),     # EMA alone: measure the norm for the log
                             ema_decay=opt.ema_decay if opt.ema_decay > 0 else None, **(dict(accum_steps=opt.accum_steps) if opt.accum_steps > 1 else {}),
                             **(dict(loss_fn=SpectralLoss(opt.loss_sam, opt.loss_sdiff, opt.loss_ssim)) if spectral else {}))
    validator = history = None
    if opt.val_every:               # 0 (default): nothing of validate.py is imported or built
        validator, history = build_validation(opt, net, eng, opt.model or opt.data_type, dev)
    start_epoch = 0
    if opt.ckpt_path is not None:
        n, start_epoch = load_warm_start(net, ckpt, dev, eng, resume=bool(opt.resume))
        if history is not None and opt.resume and ckpt.get("mphsir_val") is not None:
            note = history.restore(ckpt["mphsir_val"])
            if rank == 0:
                print("validation: %d earlier passes restored%s" % (len(history.rows), "" if history.best is None else
                                                                     ", best mean psnr %.4f at epoch %d" % (history.best["psnr"], history.best["epoch"])), flush=True)
                if note:
                    print(note, flush=True)
        if rank == 0:
            print("warm start: %d tensors from %s, %s at epoch %d" % (n, opt.ckpt_path, "resuming" if opt.resume else "starting", start_epoch))
            if not opt.resume and "mphsir_optimizer" in ckpt:
                print("note: %s also holds optimizer state of epoch %s; this run starts at epoch 0 with a fresh optimizer (the reference's "
                      "warm start, train.py:109-116) -- pass --resume 1 to continue that run instead" % (opt.ckpt_path, ckpt.get("epoch")))
        ckpt = None
        if start_epoch >= opt.epochs:
            raise SystemExit("--resume 1: %s already holds epoch %d of --epochs %d: nothing left to train" % (opt.ckpt_path, start_epoch - 1, opt.epochs))
    data_type = opt.model or opt.data_type
    de_types = opt.natural_scene_single_de_type if data_type == "natural_scene" else opt.remote_sensing_single_de_type
    cassi = None
    if "cassi" in de_types:
        cassi = dict(cassi_mask=degrade.CassiMask(dev, opt.cassi_mask or None, seed=opt.seed), cassi_step=opt.cassi_step)
        at, sentences = de_types.index("cassi"), net.text_prompt.task_text_prompts             # the prompt id is the index into the menu
        if rank == 0 and (at >= len(sentences) or sentences[at] != _TASK_PROMPTS["cassi"]):
            print("warning: 'cassi' is task %d of the menu, and task %d of this net is %s: build the one-task net with --task_classes 1" %
                  (at, at, repr(sentences[at]) if at < len(sentences) else "missing"), flush=True)
    if opt.synthetic:
        src = SyntheticPatchSource(cfg["in_channel"], opt.patch_size, opt.batch_size, cfg["task_classes"], dev, opt.seed, rank,
                                   de_types=de_types, data_type=data_type, fused_degrade=bool(opt.fused_degrade), cassi=cassi)
        steps_per_epoch = opt.steps_per_epoch
    else:
        if opt.db_path and opt.scene_dir:
            raise SystemExit("--db_path and --scene_dir both given: train from the patch database OR from the scene store")
        if not opt.db_path and not opt.scene_dir:
            raise SystemExit("--synthetic 0 needs --db_path <directory with data.bin + meta_info.txt> (data.write_patch_db) or --scene_dir "
                             "<directory of .mat / .npy cubes>")
        if opt.scene_dir:
            P = opt.patch_size
            files = scene_files(opt.scene_dir)
            if data_type == "remote_sensing" and not opt.all_sources:            # the filter --db_path applies to its records (dataset_utils.py:56)
                files = [f for f in files if os.path.basename(f).startswith(REMOTE_SENSING_SOURCES)]
                if not files:
                    raise SystemExit("--scene_dir %s holds no scene of %s (pass --all_sources 1 to train on every file)" % (opt.scene_dir, ", ".join(REMOTE_SENSING_SOURCES)))
            store = SceneStore(files, data_type, dev, patch=P, strides=(P, P // 2, P // 2))
            if rank == 0:
                print("scene store: %d records from %d levels, %.1f MB resident, %d degenerate" %
                      (len(store), store.levels_host.shape[0], store.nbytes / 1e6, store.degenerate), flush=True)
            src = SceneStoreSource(store, opt.batch_size, de_types, data_type, dev, opt.seed, rank, world, opt.repeat,
                                   fused_degrade=bool(opt.fused_degrade), jitter=bool(opt.crop_jitter), cassi=cassi)
        else:
            keep_all = data_type == "natural_scene" or opt.all_sources          # dataset_utils.py:56 filters remote-sensing sources
            db = PatchDB(opt.db_path, dataset_names=None if keep_all else REMOTE_SENSING_SOURCES)
            src = PatchDBSource(db, opt.batch_size, de_types, data_type, dev, opt.seed, rank, world, opt.repeat, fused_degrade=bool(opt.fused_degrade), cassi=cassi)
        steps_per_epoch = src.steps_per_epoch()
    K = opt.accum_steps
    if K > 1:
        # --accum_steps: an epoch draws the source's batches in the order of always, K per optimizer step; a trailing partial group is not
        # drawn (no group is ever open at an epoch end, where checkpoints are written)
        if rank == 0 and steps_per_epoch % K:
            print("note: --accum_steps %d: %d batches per epoch -> %d optimizer steps, %d not drawn" % (K, steps_per_epoch, steps_per_epoch // K, steps_per_epoch % K), flush=True)
        steps_per_epoch //= K
    for epoch in range(start_epoch, opt.epochs):
        lr = warmup_cosine_lr(epoch, opt.lr, opt.epochs)
        running = 0.0
        for it in range(steps_per_epoch):       # optimizer steps
            for _micro in range(K):
                _, degraded, clean, prompt = src.next()
                loss = eng.train_step(degraded, clean, prompt, lr=lr)
            if (it + 1) % opt.log_every == 0:
                if K > 1:
                    loss = eng.group_loss.clone()                   # the mean loss of the group's micro-batches, formed on the device
                if world > 1:
                    dist.all_reduce(loss, op=dist.ReduceOp.AVG)       # self.log(..., sync_dist=True), train.py:65
                running = float(loss)
                parts = ""
                if rank == 0 and spectral:          # one more small read-back per logged step: this rank's unweighted terms
                    lc = eng.loss_components()
                    parts = " l1 %.5f sam_deg %.4f sdiff %.5f" % (lc["l1"], lc["sam_deg"], lc["sdiff"])
                    if "ssim" in lc:
                        parts += " ssim %.4f" % lc["ssim"]
                if rank == 0 and extras:
                    gst = eng.grad_stats()          # one small read-back per logged step (the norm is the unclipped one)
                    print("epoch %d it %d lr %.3e grad_norm %.4f clip %.3f train_loss %.5f%s" % (epoch, it + 1, lr, gst["norm"], gst["coef"], running, parts), flush=True)
                elif rank == 0:
                    print("epoch %d it %d lr %.3e train_loss %.5f%s" % (epoch, it + 1, lr, running, parts), flush=True)
        if validator is not None and ((epoch + 1) % opt.val_every == 0 or epoch == opt.epochs - 1):
            result = validator.run()                                  # every rank takes part and gets the same dict
            if rank == 0:
                from mp_hsir_amd.validate import result_lines
                print("\n".join(result_lines(epoch, result)), flush=True)
                if history.add(epoch, result) and opt.save_best and opt.ckpt_dir:
                    os.makedirs(opt.ckpt_dir, exist_ok=True)
                    save_checkpoint(os.path.join(opt.ckpt_dir, "best.ckpt"), net, eng, epoch, val=history)
        if rank == 0 and opt.ckpt_dir and (epoch + 1) % 50 == 0:      # ModelCheckpoint(every_n_epochs=50), train.py:104
            os.makedirs(opt.ckpt_dir, exist_ok=True)
            save_checkpoint(os.path.join(opt.ckpt_dir, "epoch=%d.ckpt" % epoch), net, eng, epoch, val=history)
    eng.finish()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
