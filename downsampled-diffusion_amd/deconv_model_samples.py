"""Deconvolve images blurred by a 2-D point-spread function with a trained, unconditional DDPM checkpoint: zero-shot deconvolution
with DDNM (Wang, Yu, Zhang, ICLR 2023) for a circular convolution, DESIGN.md section 3.18.

Loads the checkpoint as generate_model_samples.py does (``--synthetic CONFIG`` builds closed-form weights instead) and runs
``model.deconvolve``:

  * ``--psf`` is ``diag`` (9 x 9, a 45 degree motion), ``disk`` (9 x 9 defocus of radius 3.5) or a ``.npy`` file holding a 2-D array
    with odd sides (a measured point-spread function); the boundary is periodic;
  * ``--images file.npy`` holds uint8 images [N, H, W, C] of the model's size, already blurred; with ``--blur_input`` they are sharp
    images that are blurred here first, on the GPU (ops.circular_conv), so a test set can be blurred and restored in one go;
  * ``--tol``: frequencies whose |K^| is below tol * max |K^| are dropped from the pseudo-inverse (default 0.03);
  * ``--sigma_y S`` declares that the blurred images carry noise of standard deviation S (in the [-1, 1] scale) and restores them
    with ``model.deconvolve_noisy`` (DDNM+); with ``--blur_input`` that noise, N(0, S^2) from a generator
    seeded by ``--seed``, is added here after blurring.  The output names gain ``_sy<S>``.  S = 0 (the default) is the exact
    measurement: today's chain, outputs and names.  S > 0 needs a chain that draws (not ``--use_ddim`` with ``--eta 0``); keep
    ``--tol`` at or above S;
  * ``--timestep_respacing``, ``--use_ddim`` and ``--eta`` choose the chain as in generate_model_samples.py;
  * batch g draws x_T and its Philox key from ``--seed`` + g;
  * a dDDPM checkpoint is refused: a convolution of its latent is not a convolution of the image.

Writes ``{saved_model}_deconv_{psf}_{spec}.npy`` through the sampling driver's output stage (utils.OutputStage: float32
[N, H, W, C], each image min-max scaled to [0, 255] like the sample files) and ``..._blurred.npy``, the uint8 [N, H, W, C] blurred
images it started from.  One process, one GPU.
"""
import argparse
import os

import numpy as np
import torch

from ddk import ops
from models.diffusion import blur, psf
from utils import sampling_cli as cli


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Deconvolve images blurred by a 2-D point-spread function with a trained DDPM checkpoint (DDNM).")
    cli.add_chain_flags(ap, sigma_y="standard deviation of the noise in the blurred images, [-1, 1] scale (0: exact, DDNM)")
    ap.add_argument("--images", required=True, help="uint8 .npy [N, H, W, C]: blurred images, or sharp ones with --blur_input")
    ap.add_argument("--psf", required=True, help=f"one of {', '.join(psf.PRESETS)} or a .npy file of a 2-D array with odd sides")
    ap.add_argument("--blur_input", action="store_true", help="the file holds sharp images: blur them first")
    ap.add_argument("--tol", type=float, default=blur.DEFAULT_TOL, help="frequencies below tol * max |K^| are dropped (default 0.03)")
    args = ap.parse_args(argv)
    cli.check_chain_flags(ap, args, "eta")
    if args.psf not in psf.PRESETS and not args.psf.endswith(".npy"):
        ap.error(f"--psf must be one of {', '.join(psf.PRESETS)} or a .npy file")
    if not (0 <= args.tol < 1):
        ap.error("--tol must be in [0, 1)")
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    cli.check_chain_flags(ap, args, "sigma_y sigma_y_draws",
                          sigma_y_draws="--sigma_y > 0 needs a chain that draws: ancestral steps, or --use_ddim with --eta > 0")
    return args


def load_psf(name):
    """the preset's name, or the array of a .npy file (checked by psf.psf_array)"""
    return name if name in psf.PRESETS else psf.psf_array(np.load(name))


def main():
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    model, config, c, _ = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device, pixel_only=(
        "deconvolution needs a pixel model (ddpm), this checkpoint is a {model}: a convolution of a latent is not a convolution of the image"))

    size = int(config["image_size"])
    if not psf.size_ok(c, size, size):
        raise SystemExit(f"deconvolution needs an image size that is a power of two in [16, 256], this model's is {size}")
    k = load_psf(args.psf)
    y_all = cli.u8_to_unit(cli.load_uint8_images(args.images, ((size, size, c),)))          # NHWC
    if args.blur_input:
        K = torch.from_numpy(psf.interleave(psf.psf_spectrum(k, size, size))).to(device)
        y_all = torch.cat([ops.circular_conv(y_all[i:i + args.batch_size].to(device).contiguous(), K).cpu()
                           for i in range(0, y_all.shape[0], args.batch_size)])
        if args.sigma_y > 0:
            y_all = y_all + args.sigma_y * torch.randn(y_all.shape, generator=torch.Generator().manual_seed(args.seed))
    n = y_all.shape[0]

    spec = cli.chain_spec(args)                     # with _sy{S} for a noisy measurement
    kw = dict(tol=args.tol, **cli.chain_kwargs(args))
    tag = args.psf if args.psf in psf.PRESETS else os.path.splitext(os.path.basename(args.psf))[0]
    noisy = args.sigma_y > 0
    if noisy:
        kw["sigma_y"] = args.sigma_y
    run = model.deconvolve_noisy if noisy else model.deconvolve
    print(f"Deconvolving {n} images (psf {tag}, tol {args.tol:g}, {spec} steps) with {args.saved_model}.")
    restored = cli.run_batches(n, args.batch_size, args.seed,
                               lambda i: run(y_all[i:i + args.batch_size].permute(0, 3, 1, 2).contiguous().to(device), k, **kw))

    base = cli.save_outputs(args.out_dir, f"{args.saved_model}_deconv_{tag}_{spec}", restored, "_blurred",
                            cli.unit_to_u8(y_all))          # (noisy images may leave [-1, 1]: clamped to [0, 255])
    print(f"Reconstructions saved to {base}.npy, blurred images to {base}_blurred.npy")


if __name__ == "__main__":
    main()
