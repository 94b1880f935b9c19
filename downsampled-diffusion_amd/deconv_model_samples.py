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
import json
import os
import time

import numpy as np
import torch

from ddk import ops
from models import DDPM, Unet
from models.diffusion import blur, psf
from utils import CHECKPOINT_DIR, SAMPLE_DIR, OutputStage, get_color_channels, get_model_state_dict, load_checkpoint_file
from utils import synthetic as syn


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Deconvolve images blurred by a 2-D point-spread function with a trained DDPM checkpoint (DDNM).")
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--images", required=True, help="uint8 .npy [N, H, W, C]: blurred images, or sharp ones with --blur_input")
    ap.add_argument("--psf", required=True, help=f"one of {', '.join(psf.PRESETS)} or a .npy file of a 2-D array with odd sides")
    ap.add_argument("--blur_input", action="store_true", help="the file holds sharp images: blur them first")
    ap.add_argument("--tol", type=float, default=blur.DEFAULT_TOL, help="frequencies below tol * max |K^| are dropped (default 0.03)")
    ap.add_argument("--sigma_y", type=float, default=0.0, help="standard deviation of the noise in the blurred images, [-1, 1] scale (0: exact, DDNM)")
    ap.add_argument("--timestep_respacing", default="", help='run K of the T steps: "ddimN", "N" or "n1,n2,..." sections')
    ap.add_argument("--use_ddim", action="store_true", help="DDIM steps instead of ancestral ones")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise scale (0: deterministic)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234, help="base seed: batch g draws from seed + g")
    ap.add_argument("--out_dir", default=None)
    args = ap.parse_args(argv)
    if args.eta < 0 or (args.eta != 0.0 and not args.use_ddim):
        ap.error("--eta needs --use_ddim and a value >= 0")
    if args.psf not in psf.PRESETS and not args.psf.endswith(".npy"):
        ap.error(f"--psf must be one of {', '.join(psf.PRESETS)} or a .npy file")
    if not (0 <= args.tol < 1):
        ap.error("--tol must be in [0, 1)")
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    if not (np.isfinite(args.sigma_y) and args.sigma_y >= 0):
        ap.error("--sigma_y must be a finite number >= 0")
    if args.sigma_y > 0 and args.use_ddim and args.eta == 0:
        ap.error("--sigma_y > 0 needs a chain that draws: ancestral steps, or --use_ddim with --eta > 0")
    return args


def load_psf(name):
    """the preset's name, or the array of a .npy file (checked by psf.psf_array)"""
    return name if name in psf.PRESETS else psf.psf_array(np.load(name))


def main():
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    if args.synthetic:
        with open(args.synthetic) as f:
            config = json.load(f)
        model_state_dict = None
    else:
        save_data = load_checkpoint_file(os.path.join(CHECKPOINT_DIR, f"{args.saved_model}.pt"))
        model_state_dict = get_model_state_dict(save_data)
        config = save_data["config"]
    config["batch_size"] = args.batch_size
    color_channels = get_color_channels(config["dataset"])
    if config["model"] != "ddpm":
        raise SystemExit(f"deconvolution needs a pixel model (ddpm), this checkpoint is a {config['model']}: a convolution of a latent is "
                         "not a convolution of the image")
    model = DDPM(config, Unet(config), device, color_channels)
    if model_state_dict is None:
        model_state_dict = syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS)
    model.load_state_dict(model_state_dict)
    model = model.to(device).eval()
    model.rng_stream_id = 0

    c, size = color_channels, int(config["image_size"])
    if not psf.size_ok(c, size, size):
        raise SystemExit(f"deconvolution needs an image size that is a power of two in [16, 256], this model's is {size}")
    k = load_psf(args.psf)
    data = np.load(args.images)
    if data.dtype != np.uint8 or data.ndim != 4 or data.shape[1:] != (size, size, c):
        raise SystemExit(f"--images: expected uint8 [N, {size}, {size}, {c}], got {data.dtype} {data.shape}")
    y_all = torch.from_numpy(data.astype(np.float32)) / 255 * 2 - 1          # NHWC
    if args.blur_input:
        K = torch.from_numpy(psf.interleave(psf.psf_spectrum(k, size, size))).to(device)
        y_all = torch.cat([ops.circular_conv(y_all[i:i + args.batch_size].to(device).contiguous(), K).cpu()
                           for i in range(0, y_all.shape[0], args.batch_size)])
        if args.sigma_y > 0:
            y_all = y_all + args.sigma_y * torch.randn(y_all.shape, generator=torch.Generator().manual_seed(args.seed))
    n = y_all.shape[0]

    spec = (args.timestep_respacing.replace(",", "-") or "full") + (f"_ddim_eta{args.eta:g}" if args.use_ddim else "")
    kw = dict(tol=args.tol, respacing=args.timestep_respacing or None, ddim=args.use_ddim, eta=args.eta)
    tag = args.psf if args.psf in psf.PRESETS else os.path.splitext(os.path.basename(args.psf))[0]
    noisy = args.sigma_y > 0
    if noisy:
        kw["sigma_y"] = args.sigma_y
        spec += f"_sy{args.sigma_y:g}"
    restore = model.deconvolve_noisy if noisy else model.deconvolve
    print(f"Deconvolving {n} images (psf {tag}, tol {args.tol:g}, {spec} steps) with {args.saved_model}.")
    stage = OutputStage()
    t0 = time.time()
    for g, i in enumerate(range(0, n, args.batch_size)):
        torch.manual_seed(args.seed + g)          # x_T and the Philox key of batch g
        stage.submit(restore(y_all[i:i + args.batch_size].permute(0, 3, 1, 2).contiguous().to(device), k, **kw))
    batches = stage.finish()
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    out_dir = args.out_dir or SAMPLE_DIR
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, f"{args.saved_model}_deconv_{tag}_{spec}")
    np.save(base + ".npy", np.concatenate(batches).astype(np.float32), allow_pickle=False)
    blurred = ((y_all.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8).numpy()
    np.save(base + "_blurred.npy", blurred, allow_pickle=False)
    print(f"Reconstructions saved to {base}.npy, blurred images to {base}_blurred.npy")


if __name__ == "__main__":
    main()
