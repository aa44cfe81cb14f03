"""Command-line flags of the training script -- same names, types and defaults as the reference's
options.py (options.py:6-37), so its command lines (README.md:36,38) work unchanged:

    python train.py --epochs 100 --lr 2e-4 --batch_size 32 --data_type natural_scene ...

Like the reference, the namespace is built at import time (`from options import options as opt`);
unknown flags are tolerated so that importing this module under pytest/torchrun does not abort.
Additions (not present in the reference, all optional): --model, --precision, --steps_per_epoch, --graph,
--synthetic, --log_every, --allow_surrogate_clip, --all_sources, --resume, --fused_degrade, --scene_dir, --crop_jitter, --grad_clip, --ema_decay, --task_classes, --cassi_mask, --cassi_step, --loss_sam, --loss_sdiff, --loss_ssim, --val_dir, --val_every, --val_patch, --val_crops, --val_batch, --val_modes, --val_seed, --val_weights,
--save_best, --accum_steps.  Reference hazards kept on purpose: `--num_gpus type=list` turns "01"
into ['0','1'] (options.py:36) and `--classifier type=bool` treats any non-empty string as True.
--fused_degrade 1 works at every --patch_size: a patch of up to 128 x 128 is degraded by the plane form of the launch, a larger one (256
out of a --scene_dir store, say) by its tiled form, with the same plan and the same element values.
The reference's "unseen task" fine-tune (its task_classes == 1 branch, net/MP_HSIR.py:503-506, and 'cassi' in its menu, dataset_utils.py:112):
    python train.py --data_type natural_scene --natural_scene_single_de_type cassi --task_classes 1 --ckpt_path ALLINONE.ckpt
"""
import argparse

_FLAGS = [
    # name, kwargs                                                                       (reference line)
    ("--cuda", dict(type=int, default=0)),                                               # :6
    ("--seed", dict(type=int, default=2024)),                                            # :7
    ("--epochs", dict(type=int, default=100, help="maximum number of epochs to train the total model.")),
    ("--batch_size", dict(type=int, default=32, help="Batch size to use per GPU")),
    ("--lr", dict(type=float, default=2e-4, help="learning rate of encoder.")),
    ("--init", dict(type=str, default="xu", choices=["kn", "ku", "xn", "xu"], help="which init scheme to choose.")),
    ("--mode", dict(type=int, default=0, help="Degraded Mode.")),
    ("--natural_scene_single_de_type", dict(nargs="+", default=["gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"],
                                            help="which type of single degradation is training and testing for.")),
    ("--remote_sensing_single_de_type", dict(nargs="+", default=["gaussianN", "complexN", "blur", "sr", "inpaint", "haze", "bandmiss"],
                                             help="which type of single degradation is training and testing for.")),
    ("--patch_size", dict(type=int, default=64, help="patchsize of input.")),
    ("--num_workers", dict(type=int, default=16, help="number of workers.")),
    ("--data_type", dict(type=str, default="remote_sensing", help="Types of data used for training.")),
    ("--classifier", dict(type=bool, default=False, help="")),
    ("--db_path", dict(type=str, default="", help="where clean HSIs of remote_sensing saves.")),
    ("--classifier_path", dict(type=str, default="", help="")),
    ("--output_path", dict(type=str, default="output/", help="output save path")),
    ("--ckpt_path", dict(type=str, default=None, help="checkpoint save path")),
    ("--ckpt_dir", dict(type=str, default="", help="Name of the Directory where the checkpoint is to be saved")),
    ("--num_gpus", dict(type=list, default=[0], help="Number of GPUs to use for training")),
    ("--repeat", dict(type=int, default=1, help="")),
    # ---- additions -------------------------------------------------------------------------------
    ("--model", dict(type=str, default=None, choices=[None, "natural_scene", "remote_sensing"],
                     help="which MP_HSIR_Net to build (the reference edits train.py:44-45 by hand); default: --data_type")),
    ("--precision", dict(type=str, default="bf16", choices=["bf16", "f32", "f16"], help="compute dtype of the HIP kernels "
                         "(f16 = the reference's 16-mixed: fp16 compute + dynamic loss scaling)")),
    ("--allow_surrogate_clip", dict(type=int, default=0, help="1: build the model on a seeded stand-in for the CLIP text "
                                    "embeddings when the OpenAI clip package is missing (benchmarks only)")),
    ("--all_sources", dict(type=int, default=0, help="1: do not filter remote-sensing records by source file name")),
    ("--steps_per_epoch", dict(type=int, default=100, help="synthetic source: optimisation steps per epoch")),
    ("--synthetic", dict(type=int, default=1, help="1: GPU-side synthetic patch source (no datasets offline)")),
    ("--log_every", dict(type=int, default=10)),
    ("--graph", dict(type=int, default=1, help="1: capture the training step in a hipGraph after two eager steps and replay it")),
    ("--resume", dict(type=int, default=0, help="1: --ckpt_path also restores the optimizer state and continues at the saved "
                      "epoch + 1 (a checkpoint written by this script); 0 (default) = the reference's warm start: weights only, epoch 0")),
    ("--fused_degrade", dict(type=int, default=0, help="1: degrade every training batch in one HIP launch from a plan built without host "
                             "synchronisation (degrade.DegradationSynthesizer(fused=True); no poissonN; any --patch_size: patches beyond "
                             "128 x 128 go through the tiled form of the launch); 0 (default): the tensor programs")),
    ("--scene_dir", dict(type=str, default="", help="with --synthetic 0: a directory of .mat / .npy cubes; the scene pyramid is built once, kept in "
                         "HBM, and every batch is cut out of it on the device (scene_store.SceneStore); excludes --db_path")),
    ("--crop_jitter", dict(type=int, default=0, help="1 (with --scene_dir): move every patch origin by a uniform offset below its level's stride")),
    ("--grad_clip", dict(type=float, default=0.0, help="> 0: clip the global L2 norm of the gradient to this value (clip_grad_norm_'s rule, on the "
                         "device; a step with a non-finite norm is skipped); 0 (default): off")),
    ("--task_classes", dict(type=int, default=0, help="0 (default): the model's own task set (6 natural-scene, 7 remote-sensing); 1: the one-task "
                            "net of the cassi fine-tune (the warm start drops the tensors whose shapes differ)")),
    ("--cassi_mask", dict(type=str, default="", help="'cassi' degradation: the coded-aperture mask, a .mat file with a 'mask' entry (as the reference "
                          "reads it) or a .npy file; default: a seeded Bernoulli(0.5) binary mask of 256 x 256")),
    ("--cassi_step", dict(type=int, default=2, help="'cassi' degradation: dispersion step in columns per band (the reference: 2)")),
    ("--ema_decay", dict(type=float, default=0.0, help="> 0: keep an exponential moving average of the weights with this decay (warmed up as "
                         "min(decay, (1 + t) / (10 + t))), saved as `state_dict_ema` and evaluated by test.py --use_ema 1; 0 (default): off")),
    ("--loss_sam", dict(type=float, default=0.0, help="> 0: add this weight times the mean spectral angle (radians) of the restored patch against the "
                        "clean one to the clamp + L1 loss (engine.SpectralLoss, one fused launch pair); 0 (default): off")),
    ("--loss_sdiff", dict(type=float, default=0.0, help="> 0: add this weight times the L1 of the band-to-band differences; 0 (default): off")),
    ("--loss_ssim", dict(type=float, default=0.0, help="> 0: add this weight times (1 - SSIM), the band-wise 7 x 7 SSIM that test.py and the in-training "
                         "validation report (one more fused launch pair; patches of at least 7 x 7); 0 (default): off")),
    # in-training validation (validate.py); --val_every 0 (default): off, the run does what it always did
    ("--val_dir", dict(type=str, default="", help="directory of held-out .mat / .npy cubes")),
    ("--val_every", dict(type=int, default=0, help="0 (default): no validation; E: score the held-out set after every E-th epoch and after the last")),
    ("--val_patch", dict(type=int, default=256, help="side of the crops cut out of the held-out cubes (a multiple of 64)")),
    ("--val_crops", dict(type=int, default=1, help="crops per cube: 1 (the centre) or k * k (an evenly spread grid)")),
    ("--val_batch", dict(type=int, default=4, help="crops per validation forward (one degradation mode each)")),
    ("--val_modes", dict(type=str, default="", help="test.py's modes to score, comma separated (0,5,7,...); default: every mode 0-10 whose prompt id the net has")),
    ("--val_seed", dict(type=int, default=2025, help="seed of the degraded held-out set")),
    ("--val_weights", dict(type=str, default="auto", choices=["auto", "ema", "raw"], help="the weights a pass scores: auto = the EMA weights "
                           "under --ema_decay, else the current ones")),
    ("--save_best", dict(type=int, default=0, help="1 (with --ckpt_dir): write best.ckpt whenever the mean validation PSNR improves")),
    ("--accum_steps", dict(type=int, default=1, help="K > 1: gradient accumulation, K micro-batches of --batch_size per optimizer step (the gradients "
                           "summed on the device, one AdamW step on their mean).  K micro-batches equal K data-parallel ranks, not one batch of "
                           "K * batch_size, because TVSP couples the samples of a batch; the learning rate is the user's to scale, as with more "
                           "GPUs.  An epoch takes steps_per_epoch // K optimizer steps; --log_every counts them.  1 (default): off")),
]


def build_parser():
    p = argparse.ArgumentParser()
    for name, kw in _FLAGS:
        p.add_argument(name, **kw)
    return p


options = build_parser().parse_known_args()[0]
