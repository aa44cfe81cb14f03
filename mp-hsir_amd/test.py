#!/usr/bin/env python3
"""Evaluation script: the 13 degradation modes of the reference's test.py (test.py:80-530, dispatch :580-645), batch-1
forward under no_grad, band-wise PSNR / SSIM on the device (metrics.py = utils/val_utils.py:49-105 without skimage).

  mode  degradation (utils/dataset_utils.py)                              prompt id   flag
   0    Gaussian noise sigma (:277-305)                                    0          --gaussian_noise_sigma 70
   1    non-iid Gaussian noise, per-band sigma from a list (:307-340)      1          --gaussian_noise_sigmas
   2    non-iid Gaussian + stripes (:342-406)                              1          --stripe_nosie_ratio
   3    non-iid Gaussian + deadlines (:408-466)                            1          --deadline_nosie_ratio
   4    non-iid Gaussian + impulse (:468-522)                              1          --impulse_nosie_ratio
   5    Gaussian blur, kernel size (:571-622)                              2          --gaussian_blur_radius 15
   6    motion blur (kernel size, angle) (:624-679)                        0          --motion_blur_radius
   7    bicubic down x nearest up (:681-726)                               3          --downsample_factor 8
   8    random mask (:728-769)                                             4          --mask_ratio 0.9
   9    haze (:771-840)                                                    5          --haze_omega 1
  10    missing bands, scored on the missing bands only (:842-879)         5 (6 RS)   --bandmis_ratio 0.3
  11    Poisson noise scale 10 (:243-275)                                  0
  12    real degraded / clean pairs from --test_degrad_dir (:197-241)      1
  13    CASSI snapshot measurement of the whole cube (an ADDITION: the     0          --cassi_mask --cassi_step 2
        reference has the task, degradation_utils.py:202-225, and no
        test mode for it); for a net built with --task_classes 1

Test cubes: --test_dir with .mat ('data' key, as the reference) or .npy cubes; without it, synthetic cubes (no datasets offline).
Without --tile every cube is centre-cropped to multiples of 64 (crop_img, utils/image_utils.py:58-70) and restored in one forward,
as the reference does.  With --tile N (an addition: the reference has no tiled path) cubes are NOT cropped: the degradation runs on
the whole cube, restoration goes through scene.SceneRestorer (overlapping N x N tiles, --tile_overlap, gathered and blended on the
GPU) and PSNR / SSIM are taken over the whole scene.  --quality fused scores through the fused HIP kernel (metrics.compute_quality:
the same PSNR / SSIM in one pass over the two cubes, plus the mean spectral angle SAM in degrees, which the reference does not
report); the default, --quality torch, is the tensor-program path and prints what it always printed.  --ensemble 4 / 8 (an addition
too) restores every tile under 4 (flips, half turn) or 8 (all flips and rotations; square tiles only) transforms of the training
augmentation and averages the results mapped back (scene.SceneRestorer(ensemble=...)); without --tile the cropped cube is then a
one-tile scene of that restorer, which for ensemble 1 is bitwise the plain forward.  --save_restored 1 writes
<output_path>/<mode label>/restored_<name>.npy (fp32, (C,H,W)) in either case.  The degradations are the GPU functions of degrade.py;
--fused_degrade 1 (an addition, default 0) degrades every cube of modes 0-10 in ONE HIP launch instead (degrade.SceneDegrader: the
same element values, no cube-sized temporary, no library convolution, draws that depend on --seed and the cube's ordinal only -- other
random streams than the tensor programs', so other scores within the noise; with or without --tile / --ensemble).  Mode 11 (Poisson
noise) has no fused form and ends the run with a message; mode 12 degrades nothing and ignores the flag.
Mode 13 measures the cube through the coded aperture --cassi_mask (a .mat with a 'mask' entry or a .npy; default: a seeded binary mask of
max(256, H) x max(256, W)) at a crop origin drawn from --seed, with the tensor form (degrade.cassi_measure) or, under --fused_degrade 1,
the HIP launch pair (ops.cassi): the same values either way, since the measurement has no per-element draws.  A mask file smaller
than the cube ends the run with a message.
A cube whose band count is not the model's (Urban's 210 bands under the 100-band model, say) is degraded and scored on its own bands and
restored through windows along the spectral axis (an addition: scene.SceneRestorer(bands=...), --band_overlap; windows of the model's band
count, blended with linear ramps, one mirror-padded window for a cube with fewer bands): with --tile as windows x tiles, without it as one
spatial tile, the cropped cube.  What windows cost in quality is unmeasured.  Mode 13 collapses the bands into one measurement and ends
the run with a message for such a cube, as does mode 9 beyond the 100 bands of its wavelength table.
--ckpt_path evaluates a Lightning checkpoint of the reference (`net.` key prefix).
"""
import argparse
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mp_hsir_amd import degrade as D  # noqa: E402
from mp_hsir_amd.engine import GraphedForward  # noqa: E402
from mp_hsir_amd.metrics import compute_psnr_ssim, compute_psnr_ssim2, compute_quality  # noqa: E402
from mp_hsir_amd.net.MP_HSIR import MP_HSIR_Net  # noqa: E402
from mp_hsir_amd.scene import SceneRestorer  # noqa: E402


def psnr_bandwise(restored, clean):
    return compute_psnr_ssim(restored, clean)[0]


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--cuda", type=int, default=0)                       # reference default 4 (test.py:543): box specific
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--mode", type=int, default=0, help="Used to select degradation mode.")
    p.add_argument("--test_dir", type=str, default="", help="where clean HSIs of test saves.")
    p.add_argument("--test_degrad_dir", type=str, default="", help="where real degraded HSIs of test saves.")
    p.add_argument("--degrad_id", type=int, default=1)
    p.add_argument("--gaussian_noise_sigma", type=int, default=70, help="Gaussian Noise intensity")
    p.add_argument("--gaussian_noise_sigmas", type=int, nargs="+", default=[10, 30, 50, 70], help="Gaussian Noise inid intensity")
    p.add_argument("--stripe_nosie_ratio", type=float, nargs=2, default=[0.05, 0.15], help="Stripe ratio")
    p.add_argument("--deadline_nosie_ratio", type=float, nargs=2, default=[0.05, 0.15], help="Deadline ratio")
    p.add_argument("--impulse_nosie_ratio", type=float, nargs="+", default=[0.1, 0.3, 0.5, 0.7], help="Impulse ratio")
    p.add_argument("--gaussian_blur_radius", type=int, default=15, help="Gaussian Blur")
    p.add_argument("--motion_blur_radius", type=int, nargs=2, default=(15, 45), help="Motion Blur")
    p.add_argument("--downsample_factor", type=int, default=8, help="factor")
    p.add_argument("--mask_ratio", type=float, default=0.9, help="Inpaint Mask Ratio")
    p.add_argument("--haze_omega", type=float, default=1, help="haze")
    p.add_argument("--bandmis_ratio", type=float, default=0.3, help="Bandmis Ratio")
    p.add_argument("--select_bands", type=list, default=[27, 15, 9])
    p.add_argument("--output_path", type=str, default="output/")
    p.add_argument("--ckpt_path", type=str, default=None)
    p.add_argument("--rank", type=int, default=31)
    # additions
    p.add_argument("--model", type=str, default="natural_scene", choices=["natural_scene", "remote_sensing"])
    p.add_argument("--size", type=int, default=512, help="synthetic cube height/width (reference test cubes: 512)")
    p.add_argument("--cubes", type=int, default=4)
    p.add_argument("--precision", type=str, default="f32", choices=["bf16", "f32"])
    p.add_argument("--allow_surrogate_clip", type=int, default=0)
    p.add_argument("--tile", type=int, default=0, help="0: crop to multiples of 64 and restore the cube in one forward (the reference); "
                   "N (a multiple of 64): keep the whole scene and restore it as overlapping N x N tiles")
    p.add_argument("--tile_overlap", type=int, default=32, help="nominal overlap of neighbouring tiles (at most tile // 2)")
    p.add_argument("--quality", type=str, default="torch", choices=["torch", "fused"], help="torch: PSNR / SSIM by the tensor programs of "
                   "metrics.py; fused: PSNR / SSIM / SAM by the fused HIP kernel (adds a sam column)")
    p.add_argument("--ensemble", type=int, default=1, choices=[1, 4, 8], help="self-ensemble: the mean over 4 (flips and the half turn) or 8 (all "
                   "flips and rotations; needs square tiles) transformed restorations of every tile, mapped back; 1: off")
    p.add_argument("--fused_degrade", type=int, default=0, help="1: degrade every cube of modes 0-10 in one HIP launch (degrade.SceneDegrader; no "
                   "Poisson mode 11); 0 (default): the tensor programs of degrade.py")
    p.add_argument("--use_ema", type=int, default=0, help="1: evaluate the EMA weights of the checkpoint (`state_dict_ema`, written by train.py "
                   "--ema_decay) instead of `state_dict`; a checkpoint without them ends the run")
    p.add_argument("--task_classes", type=int, default=0, help="0: the model's own task set (6 / 7); 1: the one-task net of the cassi fine-tune (mode 13)")
    p.add_argument("--cassi_mask", type=str, default="", help="mode 13: coded-aperture mask, a .mat ('mask') or .npy file; default: a seeded binary mask")
    p.add_argument("--cassi_step", type=int, default=2, help="mode 13: dispersion step in columns per band (the reference: 2)")
    p.add_argument("--band_overlap", type=int, default=-1, help="a cube whose band count is not the model's is restored through windows along the "
                   "spectral axis (scene.SceneRestorer(bands=...)): nominal overlap of neighbouring windows in bands, at most bands // 2; "
                   "-1 (default): bands // 4 -- the default of an option, not a tuned value")
    p.add_argument("--save_restored", type=int, default=0, help="1: write <output_path>/<mode label>/restored_<name>.npy (fp32, (C,H,W))")
    return p


def crop_img(x, base=64):
    """(C,H,W) centre crop to multiples of `base` (utils/image_utils.py:58-70)"""
    h, w = x.shape[-2:]
    ch, cw = h % base, w % base
    return x[..., ch // 2:h - ch + ch // 2, cw // 2:w - cw + cw // 2]


def load_cube(path):
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32)
    import scipy.io as sio
    return np.array(sio.loadmat(path)["data"]).astype(np.float32)


def cube_source(o, bands, dev, gen):
    """yields (name, clean (1,C,H,W) on dev[, real degraded]); cropped to multiples of 64 unless --tile keeps the whole scene"""
    crop = (lambda x: x) if o.tile > 0 else crop_img
    if o.test_dir:
        for fn in sorted(os.listdir(o.test_dir)):
            clean = torch.from_numpy(crop(load_cube(os.path.join(o.test_dir, fn)))).to(dev)[None]
            real = None
            if o.mode == 12:
                real = torch.from_numpy(crop(load_cube(os.path.join(o.test_degrad_dir, fn)))).to(dev)[None]
            yield fn.split(".")[0], clean, real
    else:
        if o.mode == 12:
            raise SystemExit("mode 12 evaluates real degraded/clean pairs: pass --test_dir and --test_degrad_dir")
        if o.tile > 0 and o.size < 64:
            raise SystemExit("--size %d: a synthetic cube must be at least 64 x 64" % o.size)
        for i in range(o.cubes):
            yield "synthetic_%d" % i, torch.rand((1, bands, o.size, o.size), generator=gen, device=dev), None


def degrade_for_mode(o, clean, d, model):
    """-> (degraded, prompt id) for one clean cube (1,C,H,W); d = degrade.Draws"""
    B, C, H, W = clean.shape
    nb = int(np.floor(C / 3))

    def non_iid(x, sigmas=(10, 30, 50, 70)):
        return D.gaussian_noise_non_iid(x, d.choice([s / 255.0 for s in sigmas], B * C).reshape(B, C), d.randn(B, C, H, W))
    m = o.mode
    if m == 0:
        return D.gaussian_noise(clean, torch.full((B,), o.gaussian_noise_sigma / 255.0, device=clean.device), d.randn(B, C, H, W)), 0
    if m == 1:
        return non_iid(clean, o.gaussian_noise_sigmas), 1
    if m == 2:
        lo, hi = o.stripe_nosie_ratio
        bands = d.band_subset(B, C, nb)
        n = d.randint(int(lo * W), max(int(hi * W), int(lo * W) + 1), (B, C))
        cols = d.column_subsets(B, C, W, n)
        return D.stripe_noise(non_iid(clean), bands, (d.rand(B, C, W) * 0.5 - 0.25) * cols), 1
    if m == 3:
        lo, hi = o.deadline_nosie_ratio
        bands = d.band_subset(B, C, nb)
        n = d.randint(int(np.ceil(lo * W)), max(int(np.ceil(hi * W)), int(np.ceil(lo * W)) + 1), (B, C))
        return D.deadline_noise(non_iid(clean), d.column_subsets(B, C, W, n) & bands[:, :, None]), 1
    if m == 4:
        bands = d.band_subset(B, C, nb)
        p = d.choice(list(o.impulse_nosie_ratio), B).reshape(B, 1, 1, 1)
        return D.impulse_noise(non_iid(clean), (d.rand(B, C, H, W) < p) & bands[:, :, None, None], d.rand(B, C, H, W) < 0.5), 1
    if m == 5:
        return D.blur(clean, D.gaussian_kernel2d(o.gaussian_blur_radius)), 2
    if m == 6:
        return D.blur(clean, D.motion_kernel2d(*o.motion_blur_radius)), 0
    if m == 7:
        return D.super_resolution_input(clean, o.downsample_factor), 3
    if m == 8:
        return D.random_mask(clean, d.rand(B, C, H, W), torch.full((B,), o.mask_ratio, device=clean.device)), 4
    if m == 9:
        low = d.rand(B, 1, max(H // 16, 2), max(W // 16, 2))
        cirrus = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=True)[:, 0]
        return D.haze(clean, cirrus, torch.full((B,), float(o.haze_omega), device=clean.device)), 5
    if m == 10:
        n = int(o.bandmis_ratio * C)
        return D.band_loss(clean, d.rand(B, C).argsort(dim=1).argsort(dim=1) < n), (5 if model == "natural_scene" else 6)
    if m == 11:
        return D.poisson_noise(clean, 10.0, generator=d.gen), 0
    if m == 13:
        try:
            mask = D.scene_cassi_mask(o, clean.device, H, W)
        except ValueError as e:
            raise SystemExit(str(e))
        return D.cassi_measure(clean, mask.mask, mask.origins(d, B, H, W), o.cassi_step), 0
    raise SystemExit("unknown mode %d" % m)


MODE_LABEL = {0: "Denoise sigma=%(gaussian_noise_sigma)s", 1: "Denoise sigma=%(gaussian_noise_sigmas)s",
              2: "Destripe stripe ratio=%(stripe_nosie_ratio)s", 3: "Deadline denoise deadline ratio=%(deadline_nosie_ratio)s",
              4: "Impulse denoise impulse ratio=%(impulse_nosie_ratio)s", 5: "Gaussian deblur sigma=%(gaussian_blur_radius)s",
              6: "Motion deblur motion radius=%(motion_blur_radius)s", 7: "Super resolution downsample factor=%(downsample_factor)s",
              8: "Inpaint mask ratio=%(mask_ratio)s", 9: "Dehaze haze omega=%(haze_omega)s", 10: "Bandmiss ratio=%(bandmis_ratio)s",
              11: "Degrad_Id=%(degrad_id)s", 12: "Degrad_Id=%(degrad_id)s", 13: "CASSI step=%(cassi_step)s"}


def mode_dir(o):
    """directory name of a run's outputs under --output_path: the mode's label line with everything but [A-Za-z0-9=.,-] folded to _"""
    return re.sub(r"[^A-Za-z0-9=.,-]+", "_", MODE_LABEL[o.mode] % vars(o)).strip("_")


def check_whole_scene(o, name, clean):
    """with --tile cubes keep their extent, so a degradation with a divisibility need of its own is checked before it runs"""
    H, W = clean.shape[-2:]
    if min(H, W) < 64:
        raise SystemExit("cube %s is %d x %d: smaller than 64 x 64" % (name, H, W))
    if o.mode == 7 and (H % o.downsample_factor or W % o.downsample_factor):
        raise SystemExit("cube %s is %d x %d: mode 7 downsamples by --downsample_factor %d, which does not divide both extents "
                         "(crop the cube, or run without --tile)" % (name, H, W, o.downsample_factor))


def scene_restorer(o, net, cache, name, H, W):
    """the SceneRestorer of a cube: --tile's, or (--ensemble without --tile) one whose single tile is the cropped cube itself"""
    T, ov = (o.tile, o.tile_overlap) if o.tile > 0 else (max(H, W), 0)
    if T not in cache:
        try:
            cache[T] = SceneRestorer(net, tile=T, overlap=ov, ensemble=o.ensemble,    # tiles of one shape: one captured forward serves every scene
                                     band_overlap=None if o.band_overlap < 0 else o.band_overlap)
        except ValueError as e:
            if "band overlap" in str(e):
                raise SystemExit("--band_overlap %d: %s" % (o.band_overlap, e))
            if o.tile > 0:
                raise SystemExit("--tile %d --tile_overlap %d: %s" % (o.tile, o.tile_overlap, e))
            raise SystemExit("cube %s is %d x %d: --ensemble %d restores it as one %d x %d tile: %s" % (name, H, W, o.ensemble, T, T, e))
    p = cache[T].plan(H, W)
    if o.ensemble == 8 and p.th != p.tw:
        raise SystemExit("cube %s is %d x %d and is restored as %d x %d tiles: --ensemble 8 turns tiles by 90 degrees and needs square ones "
                         "(use --ensemble 4: the flips and the half turn)" % (name, H, W, p.th, p.tw))
    return cache[T]


def check_other_band_count(o, name, Cs, bands):
    """a cube of Cs bands under a model of `bands`: degraded and scored on its own Cs bands, restored through spectral windows -- unless the
    mode's degradation is not defined for that band count"""
    if o.mode == 13:
        raise SystemExit("cube %s has %d bands, the model %d: mode 13 (the CASSI measurement) collapses the bands into one measurement "
                         "and cannot be restored through spectral windows" % (name, Cs, bands))
    if o.mode == 9 and Cs > 100:
        raise SystemExit("cube %s has %d bands: mode 9 (haze) takes its wavelengths from a table of 100 bands and is not defined "
                         "beyond them" % (name, Cs))


def evaluate(o, net, dev):
    """-> (mean psnr, mean ssim, number of cubes); prints one line per cube"""
    p, s, _, n = evaluate_quality(o, net, dev)
    return p, s, n


def evaluate_quality(o, net, dev):
    """-> (mean psnr, mean ssim, mean sam in degrees or None under --quality torch, number of cubes); prints one line per cube"""
    fused = o.quality == "fused"
    cfg_bands = net.patch_embed.proj.weight.shape[1]
    gen = torch.Generator(device=dev).manual_seed(o.seed)
    d = D.Draws(dev, o.seed + 1)
    fused_degrader = None
    if o.fused_degrade and o.mode != 12:
        if o.mode == 11:
            raise SystemExit("--fused_degrade 1: mode 11 is Poisson noise, which has no fused form (run it with --fused_degrade 0)")
        fused_degrader = D.SceneDegrader(o.model, dev, o.seed + 1)
    scenes = o.tile > 0 or o.ensemble > 1
    restorers = {}
    if o.tile > 0:
        scene_restorer(o, net, restorers, "", o.tile, o.tile)      # a bad --tile / --tile_overlap ends the run before any cube is loaded
    elif not scenes:
        run = GraphedForward(net)        # cubes of one shape: captured after two eager calls, then replayed
    out_dir = os.path.join(o.output_path, mode_dir(o))
    if o.save_restored:
        os.makedirs(out_dir, exist_ok=True)
    ps = ss = sa = 0.0
    n = 0
    for name, clean, real in cube_source(o, cfg_bands, dev, gen):
        if o.tile > 0:
            check_whole_scene(o, name, clean)
        windows = clean.shape[1] != cfg_bands          # another band count: spectral windows, through the restorer with or without --tile
        if windows:
            check_other_band_count(o, name, clean.shape[1], cfg_bands)
        if o.mode == 12:
            degraded, pid = real, 1
        elif fused_degrader is not None:
            try:
                degraded, pid = fused_degrader(clean, o.mode, o)
            except ValueError as e:
                if o.mode != 13:
                    raise
                raise SystemExit(str(e))                    # a mask file smaller than the cube
        else:
            degraded, pid = degrade_for_mode(o, clean, d, o.model)
        if scenes or windows:
            restored = scene_restorer(o, net, restorers, name, *clean.shape[-2:])(degraded.float().contiguous(), pid)
        else:
            restored = run(degraded.float().contiguous(), torch.tensor([pid], device=dev))
        if o.save_restored:
            np.save(os.path.join(out_dir, "restored_%s.npy" % name), restored[0].float().cpu().numpy())
        clean_c = clean.clamp(0, 1)
        if fused:
            q = compute_quality(restored, clean_c, degraded if o.mode == 10 else None)
            p, s, cnt = q["psnr"], q["ssim"], q["count"]
            sa += q["sam"] * cnt
        elif o.mode == 10:
            p, s, cnt = compute_psnr_ssim2(restored, clean_c, degraded)      # only the completed bands (test.py:523)
        else:
            p, s, cnt = compute_psnr_ssim(restored, clean_c)
        ps, ss, n = ps + p * cnt, ss + s * cnt, n + cnt
        if fused:
            print("%s psnr %.2f ssim %.4f sam %.3f" % (name, p, s, q["sam"]))
        else:
            print("%s psnr %.2f ssim %.4f" % (name, p, s))
    return ps / max(n, 1), ss / max(n, 1), (sa / max(n, 1) if fused else None), n


def checkpoint_weights(ckpt, use_ema=False, path="the checkpoint"):
    """the network's state_dict out of a loaded checkpoint (`net.` prefix removed, the reference's test.py:575); use_ema: the averaged
    weights train.py --ema_decay saved beside them -- a checkpoint without any ends the run with a message"""
    key = "state_dict_ema" if use_ema else "state_dict"
    if key not in ckpt:
        raise SystemExit("--use_ema 1: %s holds no state_dict_ema (it was not trained with --ema_decay)" % path)
    return {k[4:]: v for k, v in ckpt[key].items() if k.startswith("net.")}


def main():
    o = build_parser().parse_args()
    torch.manual_seed(o.seed)
    np.random.seed(o.seed)
    dev = torch.device("cuda", o.cuda)
    cfg = dict(in_channel=31, out_channel=31, dim=64, task_classes=6) if o.model == "natural_scene" else \
        dict(in_channel=100, out_channel=100, dim=96, task_classes=7)
    clip_prompt = "surrogate" if o.allow_surrogate_clip else None
    ckpt = torch.load(o.ckpt_path, map_location="cpu") if o.ckpt_path else None
    if o.use_ema and ckpt is None:
        raise SystemExit("--use_ema 1 needs --ckpt_path")
    if ckpt is not None and ckpt.get("mphsir_clip_prompt") is not None:
        clip_prompt = ckpt["mphsir_clip_prompt"]          # the table the checkpoint was trained with
    if o.task_classes:
        cfg["task_classes"] = o.task_classes
    net = MP_HSIR_Net(**cfg, clip_prompt=clip_prompt, compute_dtype=torch.float32 if o.precision == "f32" else torch.bfloat16).to(dev).eval()
    if ckpt is not None:
        net.load_state_dict(checkpoint_weights(ckpt, bool(o.use_ema), o.ckpt_path), strict=False)   # test.py:575
        print("CKPT name : {}".format(o.ckpt_path))
    p, s, sam, n = evaluate_quality(o, net, dev)
    print((MODE_LABEL[o.mode] % vars(o)) + ": psnr: %.2f, ssim: %.4f" % (p, s) + ("" if sam is None else ", sam: %.3f" % sam))


if __name__ == "__main__":
    main()
