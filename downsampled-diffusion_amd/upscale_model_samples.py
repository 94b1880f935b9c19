"""Upscale low-resolution images with a trained, unconditional DDPM / dDDPM checkpoint: zero-shot super-resolution with DDNM
(Wang, Yu, Zhang, ICLR 2023), DESIGN.md section 3.6.

Loads the checkpoint as generate_model_samples.py does (``--synthetic CONFIG`` builds closed-form weights instead), reads
``--images file.npy`` (uint8 [N, h, w, C]) and runs ``model.super_resolve`` on it:

  * images of the model's size divided by ``--scale`` are taken as the low-resolution input; images of the model's full size
    are first average-pooled by ``--scale`` (so a test set can be degraded and restored in one go);
  * ``--scale`` is 2, 4 or 8 for a DDPM; a dDDPM holds the constraint in its latent and takes 2, 4 or 8 times its reduction;
  * ``--timestep_respacing``, ``--use_ddim`` and ``--eta`` choose the chain as in generate_model_samples.py; ``--dpm_solver``
    (not with ``--use_ddim`` / ``--eta``) runs ``model.restore_solver`` instead, DDNM on the DPM-Solver++(2M) chain (section 3.9;
    use a log-SNR grid, e.g. ``logsnr20``), and adds ``_dpmpp2m`` to the file names;
  * ``--sigma_y S`` (not with ``--dpm_solver``) declares that the low-resolution images carry noise of standard deviation S in the
    model's [-1, 1] scale (S = 2 s / 255 for s uint8 levels): ``model.restore_noisy`` (DDNM+, section 3.10) runs instead, and the
    file names gain ``_sy{S}``;
  * ``--downsample bicubic`` (DDPM checkpoints; not with ``--dpm_solver`` / ``--sigma_y``): the low-resolution images are antialiased
    bicubic reductions, what image libraries and the super-resolution benchmarks make, and ``model.super_resolve(downsample="bicubic")``
    holds that constraint instead of block means (section 3.15); full-size inputs are reduced by the same matrix, and the file names
    gain ``_bicubic`` behind the scale;
  * batch g draws x_T and its Philox key from ``--seed`` + g.

Writes ``{saved_model}_sr{scale}_{spec}.npy`` through the sampling driver's output stage (utils.OutputStage: float32
[N, H, W, C], each image min-max scaled to [0, 255] like the sample files) and ``..._lowres.npy``, the uint8 low-resolution
images it started from.  One process, one GPU.
"""
import argparse

import torch

from utils import sampling_cli as cli
from utils.restoration_metrics import DOWNSAMPLES, pool, resize


def output_base(saved_model, scale, downsample, spec):
    """the output files' name without directory and extension"""
    return f"{saved_model}_sr{scale}{'_bicubic' if downsample == 'bicubic' else ''}_{spec}"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Upscale images with a trained DDPM / dDDPM checkpoint (DDNM super-resolution).")
    cli.add_chain_flags(ap, solver=True, sigma_y="the noise level of the low-resolution images in the [-1, 1] scale (DDNM+); not with --dpm_solver")
    ap.add_argument("--images", required=True, help="uint8 .npy [N, h, w, C]: low-resolution, or full-resolution to be pooled first")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--downsample", default="mean", choices=DOWNSAMPLES,
                    help="what the low-resolution images are: block means (default) or antialiased bicubic reductions")
    args = ap.parse_args(argv)
    if args.downsample == "bicubic" and (args.dpm_solver or args.sigma_y != 0.0):
        ap.error("--downsample bicubic runs ancestral or DDIM steps on an exact measurement: not with --dpm_solver or --sigma_y")
    cli.check_chain_flags(ap, args, "solver eta sigma_y sigma_y_solver sigma_y_draws")
    if args.batch_size < 1 or args.scale < 2:
        ap.error("--batch_size must be >= 1 and --scale >= 2")
    return args


def main():
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    model, config, c, _ = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device)

    size, s = int(config["image_size"]), args.scale
    if size % s:
        raise SystemExit(f"--scale {s} does not divide the model's image size {size}")
    imgs = cli.load_uint8_images(args.images, ((size // s, size // s, c), (size, size, c)))
    y_all = cli.u8_to_unit(imgs).permute(0, 3, 1, 2)
    if imgs.shape[1] == size:
        y_all = resize(y_all, s, device) if args.downsample == "bicubic" else pool(y_all, s)
    n = y_all.shape[0]

    spec = cli.chain_spec(args)
    kw = cli.chain_kwargs(args)
    if args.downsample == "bicubic":
        kw.update(downsample="bicubic")
    print(f"Upscaling {n} images x{s} ({spec} steps) with {args.saved_model}.")

    def restore(i):
        y = y_all[i:i + args.batch_size].to(device)
        if args.sigma_y != 0.0:
            return model.restore_noisy(y, None, s, sigma_y=args.sigma_y, **kw)
        return model.restore_solver(y, None, s, **kw) if args.dpm_solver else model.super_resolve(y, s, **kw)
    restored = cli.run_batches(n, args.batch_size, args.seed, restore)

    base = cli.save_outputs(args.out_dir, output_base(args.saved_model, s, args.downsample, spec), restored, "_lowres",
                            cli.unit_to_u8(y_all.permute(0, 2, 3, 1)))
    print(f"Upscaled images saved to {base}.npy, low-resolution inputs to {base}_lowres.npy")


if __name__ == "__main__":
    main()
