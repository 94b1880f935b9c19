"""Deblur images with a trained, unconditional DDPM checkpoint: zero-shot deblurring with DDNM (Wang, Yu, Zhang, ICLR 2023) for a
separable blur with zero padding, DESIGN.md section 3.14.

Loads the checkpoint as generate_model_samples.py does (``--synthetic CONFIG`` builds closed-form weights instead), reads
``--images file.npy`` (uint8 [N, H, W, C] of the model's size) and runs ``model.deblur`` on it:

  * ``--kernel`` is ``uniform`` (9 x 9 box), ``gauss`` (5 x 5, sigma 10) or ``aniso`` (9 taps, sigma 20 down the rows, sigma 1
    along them); ``--tol`` drops the singular values of each axis below tol * s_max from the pseudo-inverse;
  * the images are taken as already blurred; with ``--blur_input`` they are sharp and are blurred here first, on the GPU and in
    float (ops.separable_apply), so a test set can be degraded and restored in one go;
  * ``--timestep_respacing``, ``--use_ddim`` and ``--eta`` choose the chain as in generate_model_samples.py;
  * batch g draws x_T and its Philox key from ``--seed`` + g;
  * a dDDPM checkpoint is refused: a blur of its latent is not a blur of the image.

Writes ``{saved_model}_deblur_{kernel}_{spec}.npy`` through the sampling driver's output stage (utils.OutputStage: float32
[N, H, W, C], each image min-max scaled to [0, 255] like the sample files) and ``..._blurred.npy``, the uint8 blurred images it
started from.  One process, one GPU.
"""
import argparse

import torch

from ddk import ops
from models.diffusion import blur
from utils import sampling_cli as cli


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Deblur images with a trained DDPM checkpoint (DDNM, separable blur).")
    cli.add_chain_flags(ap)
    ap.add_argument("--images", required=True, help="uint8 .npy [N, H, W, C] of the model's size: blurred, or sharp with --blur_input")
    ap.add_argument("--kernel", choices=blur.PRESETS, default="gauss")
    ap.add_argument("--tol", type=float, default=blur.DEFAULT_TOL, help="singular values below tol * s_max are dropped, per axis")
    ap.add_argument("--blur_input", action="store_true", help="the images are sharp: blur them first")
    args = ap.parse_args(argv)
    cli.check_chain_flags(ap, args, "eta")
    if not (0 <= args.tol < 1):
        ap.error("--tol must be in [0, 1)")
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    return args


def main():
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    model, config, c, _ = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device, pixel_only=(
        "deblurring needs a pixel model (ddpm), this checkpoint is a {model}: a blur of a latent is not a blur of the image"))

    size = int(config["image_size"])
    y_all = cli.u8_to_unit(cli.load_uint8_images(args.images, ((size, size, c),)))          # NHWC
    n = y_all.shape[0]
    if args.blur_input:
        A_h, A_w = (m.to(device) for m in blur.blur_operands(args.kernel, size, size, args.tol)[:2])
        y_all = torch.cat([ops.separable_apply(y_all[i:i + args.batch_size].to(device).contiguous(), A_h, A_w).cpu()
                           for i in range(0, n, args.batch_size)])
    blurred = cli.unit_to_u8(y_all)
    y_all = y_all.permute(0, 3, 1, 2).contiguous()

    spec = cli.chain_spec(args)
    kw = dict(tol=args.tol, **cli.chain_kwargs(args))
    print(f"Deblurring {n} images ({args.kernel} kernel, {spec} steps) with {args.saved_model}.")
    restored = cli.run_batches(n, args.batch_size, args.seed, lambda i: model.deblur(y_all[i:i + args.batch_size].to(device), args.kernel, **kw))

    base = cli.save_outputs(args.out_dir, f"{args.saved_model}_deblur_{args.kernel}_{spec}", restored, "_blurred", blurred)
    print(f"Deblurred images saved to {base}.npy, blurred inputs to {base}_blurred.npy")


if __name__ == "__main__":
    main()
