"""Colourise grey images, or upscale small grey ones, with a trained, unconditional 3-channel DDPM checkpoint: zero-shot DDNM for the
operator mask o pooling o grey (Wang, Yu, Zhang, ICLR 2023), DESIGN.md section 3.11.

Loads the checkpoint as generate_model_samples.py does (``--synthetic CONFIG`` builds closed-form weights instead), reads
``--images file.npy`` and runs ``model.colorize`` on it:

  * uint8 [N, h, w] or [N, h, w, 1] images are taken as the grey measurement y, of the model's size divided by ``--scale``;
    uint8 [N, H, W, 3] images of the model's full size are first greyed with ``--weights`` and average-pooled by ``--scale`` (so a
    test set can be degraded and restored in one go);
  * ``--weights mean`` (the three channels averaged, DDNM's own operator) or ``luma`` (BT.601, what grey photographs are);
  * ``--scale`` is 1 (plain colourisation), 2, 4 or 8;
  * ``--mask center|left|half|lines`` or ``--mask file.npy`` ({0, 1}, 1 = measured, of y's size) hides part of y;
  * ``--timestep_respacing``, ``--use_ddim`` and ``--eta`` choose the chain as in generate_model_samples.py;
  * ``--sigma_y S`` declares that y carries noise of standard deviation S in the model's [-1, 1] scale (DDNM+, section 3.10), and
    the file names gain ``_sy{S}``;
  * batch g draws x_T and its Philox key from ``--seed`` + g.

A dDDPM checkpoint is refused: its chain runs in a latent whose channels are not colours.

Writes ``{saved_model}_color{scale}_{weights}_{spec}.npy`` through the sampling driver's output stage (utils.OutputStage: float32
[N, H, W, 3], each image min-max scaled to [0, 255] like the sample files) and ``..._gray.npy``, the uint8 grey images it started
from.  One process, one GPU.
"""
import argparse
import os

import numpy as np
import torch

from utils import sampling_cli as cli
from utils.restoration_metrics import GRAY_WEIGHTS, MASKS, gray, load_mask, make_mask, pool

NEEDS_COLOURS = "colourisation needs a 3-channel pixel model (a ddpm checkpoint): a dddpm samples in a latent whose channels are not colours"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Colourise grey images with a trained 3-channel DDPM checkpoint (DDNM).")
    cli.add_chain_flags(ap, sigma_y="the noise level of the grey images in the [-1, 1] scale (DDNM+)")
    ap.add_argument("--images", required=True, help="uint8 .npy: grey [N, h, w] / [N, h, w, 1], or colour [N, H, W, 3] to be greyed first")
    ap.add_argument("--weights", default="mean", choices=tuple(GRAY_WEIGHTS), help="the grey image's channel weights")
    ap.add_argument("--scale", type=int, default=1, help="1: colourisation; 2, 4, 8: the grey image is that much smaller")
    ap.add_argument("--mask", default=None, help=f"one of {', '.join(MASKS)} or a .npy file of {{0, 1}} (1 = measured), of the grey image's size")
    args = ap.parse_args(argv)
    cli.check_chain_flags(ap, args, "eta sigma_y sigma_y_draws")
    if args.batch_size < 1 or args.scale not in (1, 2, 4, 8):
        ap.error("--batch_size must be >= 1 and --scale 1, 2, 4 or 8")
    return args


def main():
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    model, config, color_channels, _ = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device, pixel_only=NEEDS_COLOURS)
    if color_channels != 3:
        raise SystemExit(NEEDS_COLOURS)

    size, s = int(config["image_size"]), args.scale
    if size % s:
        raise SystemExit(f"--scale {s} does not divide the model's image size {size}")
    hs = size // s
    imgs = np.load(args.images)
    if imgs.dtype == np.uint8 and imgs.ndim == 3:
        imgs = imgs[..., None]
    if imgs.dtype != np.uint8 or imgs.ndim != 4 or (imgs.shape[1:] != (hs, hs, 1) and imgs.shape[1:] != (size, size, 3)):
        raise SystemExit(f"--images: expected uint8 [N, {hs}, {hs}] / [N, {hs}, {hs}, 1] or [N, {size}, {size}, 3], got {imgs.dtype} {imgs.shape}")
    y_all = cli.u8_to_unit(imgs).permute(0, 3, 1, 2)
    if imgs.shape[3] == 3:
        y_all = gray(y_all, args.weights)
        if s > 1:
            y_all = pool(y_all, s)
    n = y_all.shape[0]
    mask_all, mask_name = None, ""
    if args.mask is not None:
        if args.mask in MASKS:
            mask_all, mask_name = make_mask(args.mask, n, hs, hs), args.mask
        else:
            mask_all, mask_name = load_mask(args.mask, n, hs, hs, 1), os.path.splitext(os.path.basename(args.mask))[0]
        mask_all = mask_all.amin(dim=1)

    spec = cli.chain_spec(args, mid=f"_{mask_name}" if mask_name else "")
    kw = dict(weights=args.weights, sigma_y=args.sigma_y, **cli.chain_kwargs(args))
    print(f"Colourising {n} images ({args.weights} grey, x{s}, {spec} steps) with {args.saved_model}.")

    def restore(i):
        mk = None if mask_all is None else mask_all[i:i + args.batch_size].to(device)
        return model.colorize(y_all[i:i + args.batch_size].to(device), mk, s, **kw)
    restored = cli.run_batches(n, args.batch_size, args.seed, restore)

    base = cli.save_outputs(args.out_dir, f"{args.saved_model}_color{s}_{args.weights}_{spec}", restored, "_gray",
                            cli.unit_to_u8(y_all.permute(0, 2, 3, 1)))
    print(f"Colourised images saved to {base}.npy, grey inputs to {base}_gray.npy")


if __name__ == "__main__":
    main()
