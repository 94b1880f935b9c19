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
import json
import os
import time

import numpy as np
import torch

from models import DDPM, DownsampleDDPM, Unet
from utils import CHECKPOINT_DIR, SAMPLE_DIR, OutputStage, get_color_channels, get_model_state_dict, load_checkpoint_file
from utils import synthetic as syn
from utils.restoration_metrics import DOWNSAMPLES, pool, resize


def output_base(saved_model, scale, downsample, spec):
    """the output files' name without directory and extension"""
    return f"{saved_model}_sr{scale}{'_bicubic' if downsample == 'bicubic' else ''}_{spec}"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Upscale images with a trained DDPM / dDDPM checkpoint (DDNM super-resolution).")
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--images", required=True, help="uint8 .npy [N, h, w, C]: low-resolution, or full-resolution to be pooled first")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--downsample", default="mean", choices=DOWNSAMPLES,
                    help="what the low-resolution images are: block means (default) or antialiased bicubic reductions")
    ap.add_argument("--timestep_respacing", default="", help='run K of the T steps: "ddimN", "N" or "n1,n2,..." sections')
    ap.add_argument("--use_ddim", action="store_true", help="DDIM steps instead of ancestral ones")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise scale (0: deterministic)")
    ap.add_argument("--dpm_solver", action="store_true",
                    help='DPM-Solver++(2M) steps over the --timestep_respacing grid (e.g. "logsnr20"); not with --use_ddim / --eta')
    ap.add_argument("--sigma_y", type=float, default=0.0,
                    help="the noise level of the low-resolution images in the [-1, 1] scale (DDNM+); not with --dpm_solver")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234, help="base seed: batch g draws from seed + g")
    ap.add_argument("--out_dir", default=None)
    args = ap.parse_args(argv)
    if args.downsample == "bicubic" and (args.dpm_solver or args.sigma_y != 0.0):
        ap.error("--downsample bicubic runs ancestral or DDIM steps on an exact measurement: not with --dpm_solver or --sigma_y")
    if args.dpm_solver and (args.use_ddim or args.eta != 0.0):
        ap.error("--dpm_solver is its own deterministic update: it cannot be combined with --use_ddim or --eta")
    if args.eta < 0 or (args.eta != 0.0 and not args.use_ddim):
        ap.error("--eta needs --use_ddim and a value >= 0")
    if not np.isfinite(args.sigma_y) or args.sigma_y < 0:
        ap.error("--sigma_y must be a finite number >= 0")
    if args.sigma_y != 0.0 and args.dpm_solver:
        ap.error("--sigma_y and --dpm_solver are exclusive (the solver draws nothing, so there is no variance to trade)")
    if args.sigma_y != 0.0 and args.use_ddim and args.eta == 0.0:
        ap.error("--sigma_y needs a chain that draws: ancestral steps, or --use_ddim with --eta > 0")
    if args.batch_size < 1 or args.scale < 2:
        ap.error("--batch_size must be >= 1 and --scale >= 2")
    return args


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
    if config["model"] == "ddpm":
        model = DDPM(config, Unet(config), device, color_channels)
    elif config["model"] == "dddpm":
        model = DownsampleDDPM(config, Unet(config), device, color_channels)
    else:
        raise NotImplementedError(config["model"])
    if model_state_dict is None:
        model_state_dict = syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS)
    model.load_state_dict(model_state_dict)
    model = model.to(device).eval()
    model.rng_stream_id = 0

    c, size, s = color_channels, int(config["image_size"]), args.scale
    if size % s:
        raise SystemExit(f"--scale {s} does not divide the model's image size {size}")
    imgs = np.load(args.images)
    if imgs.dtype != np.uint8 or imgs.ndim != 4 or imgs.shape[3] != c or imgs.shape[1:3] not in ((size, size), (size // s, size // s)):
        raise SystemExit(f"--images: expected uint8 [N, {size // s}, {size // s}, {c}] or [N, {size}, {size}, {c}], got {imgs.dtype} {imgs.shape}")
    y_all = torch.from_numpy(imgs.astype(np.float32)).permute(0, 3, 1, 2) / 255 * 2 - 1
    if imgs.shape[1] == size:
        y_all = resize(y_all, s, device) if args.downsample == "bicubic" else pool(y_all, s)
    n = y_all.shape[0]
    lowres = ((y_all + 1) * 127.5).round().clamp(0, 255).permute(0, 2, 3, 1).numpy().astype(np.uint8)

    spec = (args.timestep_respacing.replace(",", "-") or "full") + (f"_ddim_eta{args.eta:g}" if args.use_ddim else "") + \
        ("_dpmpp2m" if args.dpm_solver else "") + (f"_sy{args.sigma_y:g}" if args.sigma_y != 0.0 else "")
    if args.dpm_solver:
        kw = dict(respacing=args.timestep_respacing or None, solver="dpm++2m")
    else:
        kw = dict(respacing=args.timestep_respacing or None, ddim=args.use_ddim, eta=args.eta)
        if args.downsample == "bicubic":
            kw.update(downsample="bicubic")
    print(f"Upscaling {n} images x{s} ({spec} steps) with {args.saved_model}.")
    stage = OutputStage()
    t0 = time.time()
    for g, i in enumerate(range(0, n, args.batch_size)):
        torch.manual_seed(args.seed + g)          # x_T and the Philox key of batch g
        y = y_all[i:i + args.batch_size].to(device)
        if args.sigma_y != 0.0:
            out = model.restore_noisy(y, None, s, sigma_y=args.sigma_y, **kw)
        else:
            out = model.restore_solver(y, None, s, **kw) if args.dpm_solver else model.super_resolve(y, s, **kw)
        stage.submit(out[0] if config["model"] == "dddpm" else out)
    batches = stage.finish()
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    out_dir = args.out_dir or SAMPLE_DIR
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, output_base(args.saved_model, s, args.downsample, spec))
    np.save(base + ".npy", np.concatenate(batches).astype(np.float32), allow_pickle=False)
    np.save(base + "_lowres.npy", lowres, allow_pickle=False)
    print(f"Upscaled images saved to {base}.npy, low-resolution inputs to {base}_lowres.npy")


if __name__ == "__main__":
    main()
