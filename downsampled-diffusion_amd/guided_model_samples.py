"""Restore degraded images with a trained, unconditional DDPM or dDDPM checkpoint by Diffusion Posterior Sampling (Chung et al.,
ICLR 2023): gradient-guided restoration, DESIGN.md section 3.22.

Loads the checkpoint as generate_model_samples.py does (``--synthetic CONFIG`` builds closed-form weights instead) and runs
``model.restore_guided``.  A dDDPM checkpoint is welcome: its chain runs in the latent and the measurement is taken in pixels, behind
the decoder.

  * ``--task inpaint``: ``--mask`` as in inpaint_model_samples.py (default ``center``; 1 = known);
    ``--task sr``: ``--scale`` x ``--scale`` block means (1, 2, 4 or 8 -- default 4);
    ``--task deblur``: ``--kernel`` ``uniform``, ``gauss`` or ``aniso``, the separable blur with zero padding of deblur_model_samples.py;
    ``--task deconv``: ``--psf`` ``diag``, ``disk`` or a ``.npy`` file of a 2-D array with odd sides, periodic boundary;
  * ``--zeta Z``: the step size of the gradient step after every reverse step (required; the paper uses 0.3 to 1.0 with its own
    normalisation -- here the distance is taken per image);
  * ``--saturate GAIN``: the sensor clips, y = clamp(GAIN A x, -1, 1) -- an over-exposed photograph -- and the chain is told so;
  * ``--images file.npy`` holds uint8 images [N, H, W, C] of the measurement's size; with ``--measure_input`` they are clean images of
    the model's size that are measured here first, on the GPU, with the operator, the response and ``--sigma_y``;
  * ``--sigma_y S``: with ``--measure_input``, N(0, S^2) noise from a generator seeded by ``--seed`` is added to the measurement in its
    [-1, 1] scale.  That is all it does: DPS needs no noise level, the chain is the same for every S;
  * ``--timestep_respacing``, ``--use_ddim`` and ``--eta`` choose the chain as in generate_model_samples.py;
  * batch g draws x_T and its Philox key from ``--seed`` + g.

Writes ``{saved_model}_guided_{task}_{tag}_z{zeta}_{spec}.npy`` through the sampling driver's output stage (utils.OutputStage: float32
[N, H, W, C], each image min-max scaled to [0, 255] like the sample files) and ``..._measured.npy``, the uint8 [N, h, w, C] measurement
it started from (unmeasured pixels black).  One process, one GPU.
"""
import argparse
import os

import numpy as np
import torch

from ddk import ops
from models.diffusion import blur, psf
from utils import sampling_cli as cli
from utils.restoration_metrics import MASKS, load_mask, make_mask

TASKS = ("inpaint", "sr", "deblur", "deconv")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Restore degraded images with a trained DDPM / dDDPM checkpoint by Diffusion Posterior Sampling.")
    cli.add_chain_flags(ap, sigma_y="with --measure_input: standard deviation of the noise added to the measurement, [-1, 1] scale "
                                    "(the chain itself needs no noise level)")
    ap.add_argument("--task", required=True, choices=TASKS)
    ap.add_argument("--images", required=True, help="uint8 .npy [N, H, W, C]: measurements, or clean images with --measure_input")
    ap.add_argument("--zeta", type=float, required=True, help="step size of the gradient step after every reverse step (>= 0)")
    ap.add_argument("--saturate", type=float, default=None, metavar="GAIN", help="the sensor clips: y = clamp(GAIN A x, -1, 1)")
    ap.add_argument("--measure_input", action="store_true", help="the file holds clean images: measure them first")
    ap.add_argument("--mask", default=None, help=f"inpaint: one of {', '.join(MASKS)} or a .npy file of {{0, 1}} (1 = known; default center)")
    ap.add_argument("--scale", type=int, default=None, help="sr: the side of the averaged blocks, 1, 2, 4 or 8 (default 4)")
    ap.add_argument("--kernel", default=None, choices=blur.PRESETS, help="deblur: the separable blur (required there)")
    ap.add_argument("--psf", default=None, help=f"deconv: one of {', '.join(psf.PRESETS)} or a .npy file of a 2-D array with odd sides (required there)")
    args = ap.parse_args(argv)
    cli.check_chain_flags(ap, args, "eta sigma_y")
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    if not np.isfinite(args.zeta) or args.zeta < 0:
        ap.error("--zeta must be a finite number >= 0")
    if args.saturate is not None and not (np.isfinite(args.saturate) and args.saturate > 0):
        ap.error("--saturate must be a finite gain > 0")
    if args.sigma_y != 0.0 and not args.measure_input:
        ap.error("--sigma_y only adds noise to a measurement made here: it needs --measure_input")
    own = dict(inpaint="mask", sr="scale", deblur="kernel", deconv="psf")
    for task, flag in own.items():
        if task != args.task and getattr(args, flag) is not None:
            ap.error(f"--{flag} belongs to --task {task}")
    if args.task == "inpaint" and args.mask is None:
        args.mask = "center"
    if args.task == "inpaint" and args.mask not in MASKS and not args.mask.endswith(".npy"):
        ap.error(f"--mask must be one of {', '.join(MASKS)} or a .npy file")
    if args.task == "sr":
        if args.scale is None:
            args.scale = 4
        if args.scale not in ops.MEASURE_BLOCKS:
            ap.error("--scale must be 1, 2, 4 or 8")
    if args.task == "deblur" and args.kernel is None:
        ap.error("--task deblur needs --kernel: the blur is part of the task, there is no default")
    if args.task == "deconv":
        if args.psf is None:
            ap.error("--task deconv needs --psf: the point-spread function is part of the task, there is no default")
        if args.psf not in psf.PRESETS and not args.psf.endswith(".npy"):
            ap.error(f"--psf must be one of {', '.join(psf.PRESETS)} or a .npy file")
    return args


def operator_spec(args):
    """(restore_guided's `operator` argument, the tag of the output's name)"""
    if args.task == "inpaint":
        return ("mean", 1), args.mask if args.mask in MASKS else os.path.splitext(os.path.basename(args.mask))[0]
    if args.task == "sr":
        return ("mean", args.scale), f"x{args.scale}"
    if args.task == "deblur":
        return args.kernel, args.kernel
    if args.psf in psf.PRESETS:
        return ("psf", args.psf), args.psf
    return ("psf", psf.psf_array(np.load(args.psf))), os.path.splitext(os.path.basename(args.psf))[0]


def guided_kwargs(args):
    """the keywords of model.restore_guided the flags stand for (without the mask, which depends on the images)"""
    kw = dict(zeta=args.zeta, **cli.chain_kwargs(args))
    if args.saturate is not None:
        kw.update(response="saturate", gain=args.saturate)
    return kw


def main():
    from models.diffusion import guidance as G
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    model, config, c, _ = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device, default_force_latent=True)
    size = int(config["image_size"])
    spec, tag = operator_spec(args)
    kw = guided_kwargs(args)
    op = G.make_operator(spec, (c, size, size), response=kw.get("response", "linear"), gain=kw.get("gain", 1.0))
    _, h, w = op.out_shape
    if args.measure_input:
        x_all = cli.u8_to_unit(cli.load_uint8_images(args.images, ((size, size, c),)))           # NHWC, clean
    else:
        x_all = cli.u8_to_unit(cli.load_uint8_images(args.images, ((h, w, c),)))                 # NHWC, the measurement
    n = x_all.shape[0]
    mask = None
    if args.task == "inpaint":
        mask = (make_mask(args.mask, n, h, w) if args.mask in MASKS else load_mask(args.mask, n, h, w, 1))[:, 0].contiguous()
    if args.measure_input:
        ys = []
        for i in range(0, n, args.batch_size):
            op.mask = None if mask is None else mask[i:i + args.batch_size].to(device)
            ys.append(op.measure(x_all[i:i + args.batch_size].to(device).contiguous()).cpu())
        y_all = torch.cat(ys)
        if args.sigma_y > 0:
            noise = args.sigma_y * torch.randn(y_all.shape, generator=torch.Generator().manual_seed(args.seed))
            y_all = y_all + (noise if mask is None else noise * mask.unsqueeze(-1))
    else:
        y_all = x_all if mask is None else x_all * mask.unsqueeze(-1)

    chain = cli.chain_spec(args)
    sat = f"_sat{args.saturate:g}" if args.saturate is not None else ""
    print(f"Restoring {n} images ({args.task} {tag}{sat}, zeta {args.zeta:g}, {chain} steps) with {args.saved_model}.")
    restored = cli.run_batches(n, args.batch_size, args.seed, lambda i: model.restore_guided(
        y_all[i:i + args.batch_size].permute(0, 3, 1, 2).contiguous(), spec, mask=None if mask is None else mask[i:i + args.batch_size], **kw))
    base = cli.save_outputs(args.out_dir, f"{args.saved_model}_guided_{args.task}_{tag}{sat}_z{args.zeta:g}_{chain}", restored, "_measured",
                            cli.unit_to_u8(y_all))
    print(f"Reconstructions saved to {base}.npy, measurements to {base}_measured.npy")


if __name__ == "__main__":
    main()
