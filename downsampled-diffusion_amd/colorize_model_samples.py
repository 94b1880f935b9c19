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
import json
import os
import time

import numpy as np
import torch

from models import DDPM, Unet
from utils import CHECKPOINT_DIR, SAMPLE_DIR, OutputStage, get_color_channels, get_model_state_dict, load_checkpoint_file
from utils import synthetic as syn
from utils.restoration_metrics import GRAY_WEIGHTS, MASKS, gray, load_mask, make_mask, pool


def main():
    ap = argparse.ArgumentParser(description="Colourise grey images with a trained 3-channel DDPM checkpoint (DDNM).")
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--images", required=True, help="uint8 .npy: grey [N, h, w] / [N, h, w, 1], or colour [N, H, W, 3] to be greyed first")
    ap.add_argument("--weights", default="mean", choices=tuple(GRAY_WEIGHTS), help="the grey image's channel weights")
    ap.add_argument("--scale", type=int, default=1, help="1: colourisation; 2, 4, 8: the grey image is that much smaller")
    ap.add_argument("--mask", default=None, help=f"one of {', '.join(MASKS)} or a .npy file of {{0, 1}} (1 = measured), of the grey image's size")
    ap.add_argument("--timestep_respacing", default="", help='run K of the T steps: "ddimN", "N" or "n1,n2,..." sections')
    ap.add_argument("--use_ddim", action="store_true", help="DDIM steps instead of ancestral ones")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise scale (0: deterministic)")
    ap.add_argument("--sigma_y", type=float, default=0.0, help="the noise level of the grey images in the [-1, 1] scale (DDNM+)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234, help="base seed: batch g draws from seed + g")
    ap.add_argument("--out_dir", default=None)
    args = ap.parse_args()
    if args.eta < 0 or (args.eta != 0.0 and not args.use_ddim):
        ap.error("--eta needs --use_ddim and a value >= 0")
    if not np.isfinite(args.sigma_y) or args.sigma_y < 0:
        ap.error("--sigma_y must be a finite number >= 0")
    if args.sigma_y != 0.0 and args.use_ddim and args.eta == 0.0:
        ap.error("--sigma_y needs a chain that draws: ancestral steps, or --use_ddim with --eta > 0")
    if args.batch_size < 1 or args.scale not in (1, 2, 4, 8):
        ap.error("--batch_size must be >= 1 and --scale 1, 2, 4 or 8")

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
    if config["model"] != "ddpm" or color_channels != 3:
        raise SystemExit("colourisation needs a 3-channel pixel model (a ddpm checkpoint): a dddpm samples in a latent whose channels are "
                         "not colours")
    model = DDPM(config, Unet(config), device, color_channels)
    if model_state_dict is None:
        model_state_dict = syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS)
    model.load_state_dict(model_state_dict)
    model = model.to(device).eval()
    model.rng_stream_id = 0

    size, s = int(config["image_size"]), args.scale
    if size % s:
        raise SystemExit(f"--scale {s} does not divide the model's image size {size}")
    hs = size // s
    imgs = np.load(args.images)
    if imgs.dtype == np.uint8 and imgs.ndim == 3:
        imgs = imgs[..., None]
    if imgs.dtype != np.uint8 or imgs.ndim != 4 or (imgs.shape[1:] != (hs, hs, 1) and imgs.shape[1:] != (size, size, 3)):
        raise SystemExit(f"--images: expected uint8 [N, {hs}, {hs}] / [N, {hs}, {hs}, 1] or [N, {size}, {size}, 3], got {imgs.dtype} {imgs.shape}")
    y_all = torch.from_numpy(imgs.astype(np.float32)).permute(0, 3, 1, 2) / 255 * 2 - 1
    if imgs.shape[3] == 3:
        y_all = gray(y_all, args.weights)
        if s > 1:
            y_all = pool(y_all, s)
    n = y_all.shape[0]
    grey_u8 = ((y_all + 1) * 127.5).round().clamp(0, 255).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    mask_all, mask_name = None, ""
    if args.mask is not None:
        if args.mask in MASKS:
            mask_all, mask_name = make_mask(args.mask, n, hs, hs), args.mask
        else:
            mask_all, mask_name = load_mask(args.mask, n, hs, hs, 1), os.path.splitext(os.path.basename(args.mask))[0]
        mask_all = mask_all.amin(dim=1)

    spec = (args.timestep_respacing.replace(",", "-") or "full") + (f"_ddim_eta{args.eta:g}" if args.use_ddim else "") + \
        (f"_{mask_name}" if mask_name else "") + (f"_sy{args.sigma_y:g}" if args.sigma_y != 0.0 else "")
    kw = dict(weights=args.weights, sigma_y=args.sigma_y, respacing=args.timestep_respacing or None, ddim=args.use_ddim, eta=args.eta)
    print(f"Colourising {n} images ({args.weights} grey, x{s}, {spec} steps) with {args.saved_model}.")
    stage = OutputStage()
    t0 = time.time()
    for g, i in enumerate(range(0, n, args.batch_size)):
        torch.manual_seed(args.seed + g)          # x_T and the Philox key of batch g
        mk = None if mask_all is None else mask_all[i:i + args.batch_size].to(device)
        stage.submit(model.colorize(y_all[i:i + args.batch_size].to(device), mk, s, **kw))
    batches = stage.finish()
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    out_dir = args.out_dir or SAMPLE_DIR
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, f"{args.saved_model}_color{s}_{args.weights}_{spec}")
    np.save(base + ".npy", np.concatenate(batches).astype(np.float32), allow_pickle=False)
    np.save(base + "_gray.npy", grey_u8, allow_pickle=False)
    print(f"Colourised images saved to {base}.npy, grey inputs to {base}_gray.npy")


if __name__ == "__main__":
    main()
