#!/usr/bin/env python3
"""Score the restoration paths of a trained DDPM / dDDPM checkpoint against ground truth: degrade a test
set, restore it with RePaint inpainting (``--task inpaint``, section 3.5) or DDNM super-resolution (``--task sr``, section 3.6) and
report PSNR and SSIM of the result and of network-free baselines, as mean and standard error over the images.

Loads the checkpoint as evaluate_ddpm.py does (``--synthetic CONFIG`` builds closed-form weights instead; their scores mean
nothing).  The images are ``--images file.npy`` (uint8 [N, H, W, C] of the model's size) or, by default, the dataset's test split
through utils/data.py; ``--max_batches`` keeps the first max_batches * batch_size of them.

  * ``--task inpaint``: ``--mask`` as in inpaint_model_samples.py, chain options ``--timestep_respacing``, ``--jump_length``,
    ``--jump_n_sample``.  Baseline: hidden pixels filled with the mean of the known ones.  Also the PSNR over the hidden pixels only.
  * ``--task sr``: the images are average-pooled by ``--scale``, chain options ``--timestep_respacing``, ``--use_ddim``, ``--eta``
    as in upscale_model_samples.py.  Baselines: replication and bicubic upsampling.  Also the consistency max |pool(x_out) - y| in
    uint8 levels, of the chain's float output and of the uint8 image that is scored.
  * ``--task sr --downsample bicubic`` (DDPM checkpoints; section 3.15): the images are reduced by antialiased bicubic downsampling,
    the degradation of the super-resolution benchmarks, instead of pooled, and ``model.super_resolve(downsample="bicubic")`` restores
    them.  Same baselines; the consistency is max |A(x_out) - y| in uint8 levels with that operator; the settings gain ``downsample``.
    Not with ``--mask``, ``--dpm_solver`` or ``--sigma_y``.
  * ``--task inpaint --method ddnm``: DDNM for a mask (section 3.8) instead of RePaint, with ``--use_ddim`` / ``--eta`` and without
    the ``--jump_*`` options; ``--task sr --mask KIND``: masked super-resolution, the mask applied to the pooled image, restored
    with ``model.restore``; the baselines mean-fill the same holes before they upsample.
  * ``--dpm_solver`` (DDNM only, not with ``--use_ddim`` / ``--eta``): DDNM on the DPM-Solver++(2M) chain (section 3.9,
    ``model.restore_solver``) over the ``--timestep_respacing`` grid (e.g. ``logsnr20``); ``method`` then reads ``ddnm_dpmpp2m``.
  * ``--sigma_y S`` (DDNM only, not with ``--dpm_solver``): the measurement is noisy (section 3.10).  N(0, S^2) noise, seeded by
    ``--seed``, is added to the measurement in its [-1, 1] scale after degrading; ``model.restore_noisy`` (DDNM+) restores it, the
    baselines see the same noisy measurement, ``method`` reads ``ddnm_plus``, the settings gain ``sigma_y``, and the consistency
    becomes the RMS of pool(x_out) - y_clean over the measured pixels in uint8 levels.  ``--sigma_y 0`` changes nothing.
  * ``--task colorize`` (3-channel DDPM checkpoints; section 3.11): the images are greyed with ``--weights`` (``mean`` or ``luma``)
    and average-pooled by ``--scale`` (default 1: plain colourisation), ``--mask`` applies to that measurement, ``model.colorize``
    restores it with ``--timestep_respacing``, ``--use_ddim``, ``--eta`` and ``--sigma_y``.  Baselines: the grey image copied into
    the three channels, replicated or bicubic-upsampled at ``--scale`` > 1.  The consistency is max |A(x_out) - y| in uint8 levels
    (with ``--sigma_y``: the RMS against the clean y); ``method`` reads ``ddnm_gray`` and the settings gain ``weights``.
  * ``--task deblur --kernel K`` (DDPM checkpoints; section 3.14): the images are blurred with the separable kernel K (``uniform``,
    ``gauss`` or ``aniso``; zero padding; the task has no default kernel) and ``model.deblur`` restores them with ``--tol``, ``--timestep_respacing``, ``--use_ddim`` and
    ``--eta``.  Baselines: the blurred image itself and A+ y clipped to [-1, 1].  The consistency is max |A(x_out) - y| in uint8
    levels; ``method`` reads ``ddnm_blur`` and the settings gain ``kernel`` and ``tol``.
  * ``--task cs --ratio R [--perm_seed S]`` (DDPM checkpoints; section 3.17): every colour plane is measured by the first
    m = 4 round(R N / 4) coefficients of the orthonormal Walsh-Hadamard transform of its pixels permuted with seed S (default 0), and
    ``model.restore_cs`` restores it with ``--timestep_respacing``, ``--use_ddim`` and ``--eta``.  Baseline: ``adjoint``, A^T y clipped
    to [-1, 1].  The consistency is max |A(x_out) - y| in the measurement's own scale; ``method`` reads ``ddnm_cs`` and the settings
    gain ``ratio``, ``perm_seed`` and ``m``.  No ``--scale``, ``--mask``, ``--sigma_y``, ``--dpm_solver``, ``--method``, ``--kernel``
    or ``--tol``.
  * ``--task deconv --psf P [--tol T]`` (DDPM checkpoints; section 3.18): the images are blurred by the 2-D point-spread function P
    (``diag``, ``disk`` or a ``.npy`` file of a 2-D array with odd sides; periodic boundary) and ``model.deconvolve`` restores them
    with ``--tol`` (default 0.03), ``--timestep_respacing``, ``--use_ddim`` and ``--eta``.  Baselines: the blurred image itself and
    ``pinv``, A+ y clipped to [-1, 1].  The consistency is max |A+ A x_out - A+ y|; ``method`` reads ``ddnm_deconv`` and the settings
    gain ``psf`` and ``tol``.  ``--psf`` belongs to this task alone; it takes no ``--scale``, ``--mask``, ``--sigma_y``,
    ``--dpm_solver``, ``--method`` or ``--kernel``.
  * ``--task deconv_noisy --psf P --sigma_y S [--tol T]`` (DDPM checkpoints; section 3.19), S > 0: the images are blurred as for
    ``deconv``, N(0, S^2) noise seeded by ``--seed`` is added in the [-1, 1] scale, and ``model.deconvolve_noisy`` (DDNM+ per
    frequency) restores them.  Baselines, all from the noisy image: the blurred image, ``pinv`` (which shows the amplification of
    the noise by 1 / |K^|) and ``tikhonov``, conj K^ / (|K^|^2 + S^2).  ``method`` reads ``ddnm_plus``, the settings gain ``psf``,
    ``tol`` and ``sigma_y``, and the consistency is the RMS of A(x_out) - y_clean in uint8 levels.  Needs a chain that draws; keep
    ``--tol`` at or above S.  ``--task deconv`` itself keeps refusing ``--sigma_y``.
  * ``--method dps --zeta Z [--saturate GAIN] [--sigma_y S]`` (DDPM and dDDPM checkpoints; section 3.22), for ``--task inpaint``
    (``--mask``), ``sr`` (``--scale`` 1, 2, 4 or 8), ``deblur`` (``--kernel``) and ``deconv`` (``--psf``): Diffusion Posterior Sampling,
    ``model.restore_guided``.  The images are measured by the task's operator, through a sensor that clips at GAIN with ``--saturate``,
    with N(0, S^2) noise added; every reverse step is followed by a gradient step of size Z.  Baseline: ``measured``.  The consistency
    is the RMS of phi(A x_out) - y_clean in uint8 levels; ``method`` reads ``dps`` and the settings gain ``zeta`` and
    ``unet_backwards`` (one input-gradient backward per forward).  No ``--dpm_solver``, ``--downsample``, ``--tol`` or ``--jump_*``.
  * batch g draws x_T and its Philox key from ``--seed`` + g.

Prints one JSON object, the settings that produced it (among them ``method`` and ``unet_forwards``, the UNet forwards per image, so
that two runs compare on cost as well as on PSNR) beside the metrics; ``--json OUT`` also writes it to a file.  One process,
one GPU.
"""
import argparse
import json
import time

import numpy as np
import torch

from utils import sampling_cli as cli
from utils.restoration_metrics import BLUR_KERNELS, CS_TASK, DEBLUR_TASK, DECONV_NOISY_TASK, DECONV_TASK, DOWNSAMPLES, DPS_METHOD, DPS_TASKS, GRAY_WEIGHTS, MASKS, METHODS, TASKS, evaluate_restoration, load_mask, report, to_u8


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="PSNR / SSIM of RePaint inpainting or DDNM super-resolution against ground truth.",
                                 epilog="--method dps (inpaint, sr, deblur, deconv; DDPM and dDDPM checkpoints) has two options of its own: "
                                        "--zeta Z, the step size of the gradient step after every reverse step (required there), and "
                                        "--saturate GAIN, a sensor that clips: y = clamp(GAIN A x, -1, 1).")
    cli.add_chain_flags(ap, solver=True, out_dir=False, prefix="ddnm: ", respacing_help='run K of the T steps: "N", "n1,n2,..." sections or (sr) "ddimN"',
                        sigma_y="ddnm: add N(0, sigma_y^2) noise to the measurement ([-1, 1] scale) and restore with DDNM+; not with --dpm_solver")
    ap.add_argument("--images", default=None, help="uint8 [N, H, W, C] .npy of the model's size (default: the dataset's test split)")
    ap.add_argument("--task", required=True, choices=(*TASKS, DEBLUR_TASK, CS_TASK, DECONV_TASK, DECONV_NOISY_TASK))
    ap.add_argument("--mask", default=None, help=f"one of {', '.join(MASKS)} or a .npy file of {{0, 1}} (1 = known); inpaint: default "
                                                 "center; sr: masked super-resolution, the mask is of the pooled image (default: none)")
    ap.add_argument("--method", default=None, choices=(*METHODS, DPS_METHOD), help="inpaint: repaint (default) or ddnm; sr: ddnm; dps: gradient-"
                                                                                   "guided restoration of inpaint, sr, deblur and deconv")
    # (the two options of --method dps are described in the epilog, not in the option list: the list is what every method shares)
    ap.add_argument("--zeta", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--saturate", type=float, default=None, metavar="GAIN", help=argparse.SUPPRESS)
    ap.add_argument("--scale", type=int, default=None, help="sr: the pooling factor (default 4); colorize: default 1")
    ap.add_argument("--downsample", default=None, choices=DOWNSAMPLES, help="sr: how the images are reduced (default mean: average pooling)")
    ap.add_argument("--weights", default=None, choices=tuple(GRAY_WEIGHTS), help="colorize: the grey image's channel weights (default mean)")
    ap.add_argument("--kernel", default=None, choices=BLUR_KERNELS, help="deblur: the separable blur (required there)")
    ap.add_argument("--tol", type=float, default=None, help="deblur: singular values below tol * s_max are dropped, per axis (default 0.03)")
    ap.add_argument("--psf", default=None, help="deconv: the 2-D point-spread function, diag, disk or a .npy file (required there)")
    ap.add_argument("--ratio", type=float, default=None, help="cs: the sampling ratio in (0, 1] (required there)")
    ap.add_argument("--perm_seed", type=int, default=None, help="cs: seed of the pixel permutation (default 0)")
    ap.add_argument("--jump_length", type=int, default=10, help="inpaint: RePaint jump length")
    ap.add_argument("--jump_n_sample", type=int, default=10, help="inpaint: RePaint resamplings per jump")
    ap.add_argument("--max_batches", type=int, default=None, help="stop after this many batches of images")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    args = ap.parse_args(argv)
    if args.batch_size < 1 or (args.max_batches is not None and args.max_batches < 1):
        ap.error("--batch_size and --max_batches must be >= 1")
    if args.method == DPS_METHOD:
        return check_dps(ap, args)
    if args.zeta is not None or args.saturate is not None:
        ap.error("--zeta and --saturate belong to --method dps")
    del args.zeta, args.saturate          # the other methods' namespace is what it was: these two exist under --method dps only
    if args.psf is not None and args.task not in (DECONV_TASK, DECONV_NOISY_TASK):
        ap.error("--psf belongs to --task deconv and --task deconv_noisy")
    if args.task in (DECONV_TASK, DECONV_NOISY_TASK):
        if args.psf is None:
            ap.error(f"--task {args.task} needs --psf: the point-spread function is part of the task, there is no default")
        if args.psf not in ("diag", "disk") and not args.psf.endswith(".npy"):
            ap.error("--psf must be diag, disk or a .npy file")
        if args.task == DECONV_NOISY_TASK and not args.sigma_y > 0:
            ap.error("--task deconv_noisy needs --sigma_y > 0: the noise level is part of the task (--sigma_y 0 is --task deconv)")
        if args.method is not None or args.dpm_solver or (args.task == DECONV_TASK and args.sigma_y != 0.0) or args.mask is not None or args.scale is not None or \
                args.kernel is not None:
            ap.error("--task deconv has one method, ddnm on ancestral or DDIM steps, and takes no --method, --mask, --scale, --sigma_y, "
                     "--dpm_solver or --kernel")
        if args.tol is None:
            args.tol = 3e-2
        if not (0 <= args.tol < 1):
            ap.error("--tol must be in [0, 1)")
    if (args.ratio is not None or args.perm_seed is not None) and args.task != CS_TASK:
        ap.error("--ratio and --perm_seed belong to --task cs")
    if args.task == CS_TASK:
        if args.ratio is None:
            ap.error("--task cs needs --ratio: the sampling ratio is part of the task, there is no default")
        if not (0 < args.ratio <= 1):
            ap.error("--ratio must be in (0, 1]")
        if args.perm_seed is None:
            args.perm_seed = 0
        if args.perm_seed < 0:
            ap.error("--perm_seed must be >= 0")
        if args.method is not None or args.dpm_solver or args.sigma_y != 0.0 or args.mask is not None or args.scale is not None or \
                args.kernel is not None or args.tol is not None:
            ap.error("--task cs has one method, ddnm on ancestral or DDIM steps, and takes no --method, --mask, --scale, --sigma_y, "
                     "--dpm_solver, --kernel or --tol")
    if args.method is None:
        args.method = "repaint" if args.task == "inpaint" else "ddnm"
    if args.downsample is not None and args.task != "sr":
        ap.error("--downsample belongs to --task sr")
    if args.downsample == "bicubic" and (args.mask is not None or args.dpm_solver or args.sigma_y != 0.0):
        ap.error("--downsample bicubic takes no --mask, --dpm_solver or --sigma_y")
    if args.weights is not None and args.task != "colorize":
        ap.error("--weights belongs to --task colorize")
    if (args.kernel is not None or args.tol is not None) and args.task not in (DEBLUR_TASK, DECONV_TASK, DECONV_NOISY_TASK):
        ap.error("--kernel and --tol belong to --task deblur")
    if args.task == DEBLUR_TASK:
        if args.kernel is None:
            ap.error("--task deblur needs --kernel: the blur is part of the task, there is no default")
        if args.tol is None:
            args.tol = 3e-2
        if not (0 <= args.tol < 1):
            ap.error("--tol must be in [0, 1)")
        if args.method != "ddnm" or args.dpm_solver or args.sigma_y != 0.0 or args.mask is not None or args.scale is not None:
            ap.error("--task deblur has one method, ddnm on ancestral or DDIM steps, and takes no --mask, --scale or --sigma_y")
    elif args.task in (CS_TASK, DECONV_TASK, DECONV_NOISY_TASK):
        pass                      # checked above
    elif args.task == "sr":
        if args.scale is None:
            args.scale = 4
        if args.method != "ddnm":
            ap.error("--task sr has one method, ddnm")
        if args.scale < 2:
            ap.error("--scale must be >= 2")
    elif args.task == "colorize":
        if args.scale is None:
            args.scale = 1
        if args.weights is None:
            args.weights = "mean"
        if args.method != "ddnm" or args.dpm_solver:
            ap.error("--task colorize has one method, ddnm on ancestral or DDIM steps")
        if args.scale not in (1, 2, 4, 8):
            ap.error("--scale must be 1, 2, 4 or 8")
    else:
        if args.scale is None:
            args.scale = 4
        if args.mask is None:
            args.mask = "center"
    cli.check_chain_flags(ap, args, "sigma_y")
    if args.method == "ddnm":
        cli.check_chain_flags(ap, args, "solver sigma_y_solver sigma_y_draws eta")
        if args.jump_length != ap.get_default("jump_length") or args.jump_n_sample != ap.get_default("jump_n_sample"):
            ap.error("--jump_length and --jump_n_sample belong to --method repaint (DDNM has no jumps)")
    else:
        if args.use_ddim or args.eta != 0.0 or args.dpm_solver or args.sigma_y != 0.0:
            ap.error("--use_ddim, --eta, --dpm_solver and --sigma_y belong to DDNM (RePaint runs ancestral steps)")
        if args.jump_length < 1 or args.jump_n_sample < 1:
            ap.error("--jump_length and --jump_n_sample must be >= 1")
    return args


def check_dps(ap, args):
    """--method dps: the four tasks it restores, each with its own operator flag, on ancestral or DDIM steps"""
    if args.task not in DPS_TASKS:
        ap.error(f"--method dps restores --task {', '.join(DPS_TASKS)}")
    if args.zeta is None or not np.isfinite(args.zeta) or args.zeta < 0:
        ap.error("--method dps needs --zeta, a finite step size >= 0")
    if args.saturate is not None and not (np.isfinite(args.saturate) and args.saturate > 0):
        ap.error("--saturate must be a finite gain > 0")
    own = {"inpaint": "mask", "sr": "scale", DEBLUR_TASK: "kernel", DECONV_TASK: "psf"}
    for task, flag in own.items():
        if task != args.task and getattr(args, flag) is not None:
            ap.error(f"--method dps: --{flag} belongs to --task {task}")
    if args.dpm_solver or args.downsample is not None or args.weights is not None or args.tol is not None or args.ratio is not None or \
            args.perm_seed is not None or args.jump_length != ap.get_default("jump_length") or args.jump_n_sample != ap.get_default("jump_n_sample"):
        ap.error("--method dps takes no --dpm_solver, --downsample, --weights, --tol, --ratio, --perm_seed or --jump_* (it has no pseudo-inverse "
                 "to truncate and no jumps)")
    if args.task == "inpaint" and args.mask is None:
        args.mask = "center"
    if args.task == "sr":
        if args.scale is None:
            args.scale = 4
        if args.scale not in (1, 2, 4, 8):
            ap.error("--method dps: --scale must be 1, 2, 4 or 8")
    if args.task == DEBLUR_TASK and args.kernel is None:
        ap.error("--task deblur needs --kernel: the blur is part of the task, there is no default")
    if args.task == DECONV_TASK:
        if args.psf is None:
            ap.error("--task deconv needs --psf: the point-spread function is part of the task, there is no default")
        if args.psf not in ("diag", "disk") and not args.psf.endswith(".npy"):
            ap.error("--psf must be diag, disk or a .npy file")
    cli.check_chain_flags(ap, args, "sigma_y eta")
    return args


def chain_options(args):
    """the task's keywords for evaluate_restoration, also the chain settings the result records"""
    steps = cli.chain_kwargs(args)
    if args.method == DPS_METHOD:
        kw = dict(steps, zeta=args.zeta)
        for name in ("saturate", "scale", "kernel", "psf"):
            if getattr(args, name) is not None:
                kw[name] = getattr(args, name)
        if args.sigma_y != 0.0:
            kw.update(sigma_y=args.sigma_y)
        return kw
    kw = dict(respacing=steps.pop("respacing"))
    if args.task in ("sr", "colorize"):
        kw.update(scale=args.scale)
    if args.task == "colorize":
        kw.update(weights=args.weights)
    if args.downsample == "bicubic":
        kw.update(downsample="bicubic")
    if args.task == DEBLUR_TASK:
        kw.update(kernel=args.kernel, tol=args.tol)
    if args.task == CS_TASK:
        kw.update(ratio=args.ratio, perm_seed=args.perm_seed)
    if args.task in (DECONV_TASK, DECONV_NOISY_TASK):
        kw.update(psf=args.psf, tol=args.tol)
    if args.dpm_solver:
        kw.update(dpm_solver=True)                 # (evaluate_restoration's own keyword for chain_kwargs' solver="dpm++2m")
    elif args.method == "ddnm":
        kw.update(steps)
    else:
        kw.update(jump_length=args.jump_length, jump_n_sample=args.jump_n_sample)
    if args.sigma_y != 0.0:
        kw.update(sigma_y=args.sigma_y)
    return kw


def load_model(args, device):
    return cli.load_model(args.saved_model, args.synthetic, args.batch_size, device, default_force_latent=True)[:3]


def load_images(args, config, channels):
    """uint8 [N, H, W, C]: the file, or the test split (floats in [-1, 1], rounded to the uint8 grid the metrics are defined on)"""
    size = int(config["image_size"])
    limit = None if args.max_batches is None else args.max_batches * args.batch_size
    if args.images:
        return cli.load_uint8_images(args.images, ((size, size, channels),))[:limit]
    from utils import DATA_DIR, get_dataloader
    loader = get_dataloader(config, data_root=DATA_DIR, device="cpu", train=False)[0]
    out = []
    for g, (x, _) in enumerate(loader):
        if args.max_batches is not None and g >= args.max_batches:
            break
        out.append(to_u8(x).numpy())
    return np.concatenate(out)


def main():
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    model, config, channels = load_model(args, device)
    images = load_images(args, config, channels)
    n, h, w, _ = images.shape
    kw = chain_options(args)
    if args.task == "inpaint":
        kw["mask"] = args.mask if args.mask in MASKS else load_mask(args.mask, n, h, w, channels)
    elif args.mask is not None and args.task not in (DEBLUR_TASK, CS_TASK, DECONV_TASK, DECONV_NOISY_TASK):
        kw["sr_mask"] = args.mask if args.mask in MASKS else load_mask(args.mask, n, h // args.scale, w // args.scale, 1)

    print(f"Scoring {args.task} on {n} images with {'synthetic weights' if args.synthetic else args.saved_model}.")
    t0 = time.time()
    result = evaluate_restoration(model, images, args.task, batch_size=args.batch_size, seed=args.seed, method=args.method, **kw)
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    settings = dict(checkpoint=None if args.synthetic else args.saved_model, synthetic=args.synthetic, model=config["model"],
                    task=args.task, images=args.images or f"{config['dataset']} test split", n_images=n, batch_size=args.batch_size,
                    seed=args.seed, method=result["method"], unet_forwards=result["unet_forwards"], **chain_options(args))
    if args.mask is not None:
        settings["mask"] = args.mask
    if "m" in result:
        settings["m"] = result["m"]
    if "unet_backwards" in result:
        settings["unet_backwards"] = result["unet_backwards"]
    out = dict(settings=settings, metrics=report(result))
    print(json.dumps(out, indent=4))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=4)


if __name__ == "__main__":
    main()
