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
import json
import os
import time

import numpy as np
import torch

from ddk import ops
from models import DDPM, Unet
from models.diffusion import blur
from utils import CHECKPOINT_DIR, SAMPLE_DIR, OutputStage, get_color_channels, get_model_state_dict, load_checkpoint_file
from utils import synthetic as syn


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Deblur images with a trained DDPM checkpoint (DDNM, separable blur).")
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--images", required=True, help="uint8 .npy [N, H, W, C] of the model's size: blurred, or sharp with --blur_input")
    ap.add_argument("--kernel", choices=blur.PRESETS, default="gauss")
    ap.add_argument("--tol", type=float, default=blur.DEFAULT_TOL, help="singular values below tol * s_max are dropped, per axis")
    ap.add_argument("--blur_input", action="store_true", help="the images are sharp: blur them first")
    ap.add_argument("--timestep_respacing", default="", help='run K of the T steps: "ddimN", "N" or "n1,n2,..." sections')
    ap.add_argument("--use_ddim", action="store_true", help="DDIM steps instead of ancestral ones")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise scale (0: deterministic)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234, help="base seed: batch g draws from seed + g")
    ap.add_argument("--out_dir", default=None)
    args = ap.parse_args(argv)
    if args.eta < 0 or (args.eta != 0.0 and not args.use_ddim):
        ap.error("--eta needs --use_ddim and a value >= 0")
    if not (0 <= args.tol < 1):
        ap.error("--tol must be in [0, 1)")
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
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
    if config["model"] != "ddpm":
        raise SystemExit(f"deblurring needs a pixel model (ddpm), this checkpoint is a {config['model']}: a blur of a latent is not a blur "
                         "of the image")
    model = DDPM(config, Unet(config), device, color_channels)
    if model_state_dict is None:
        model_state_dict = syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS)
    model.load_state_dict(model_state_dict)
    model = model.to(device).eval()
    model.rng_stream_id = 0

    c, size = color_channels, int(config["image_size"])
    imgs = np.load(args.images)
    if imgs.dtype != np.uint8 or imgs.ndim != 4 or imgs.shape[1:] != (size, size, c):
        raise SystemExit(f"--images: expected uint8 [N, {size}, {size}, {c}], got {imgs.dtype} {imgs.shape}")
    y_all = torch.from_numpy(imgs.astype(np.float32)) / 255 * 2 - 1          # NHWC
    n = y_all.shape[0]
    if args.blur_input:
        A_h, A_w = (m.to(device) for m in blur.blur_operands(args.kernel, size, size, args.tol)[:2])
        y_all = torch.cat([ops.separable_apply(y_all[i:i + args.batch_size].to(device).contiguous(), A_h, A_w).cpu()
                           for i in range(0, n, args.batch_size)])
    blurred = ((y_all + 1) * 127.5).round().clamp(0, 255).numpy().astype(np.uint8)
    y_all = y_all.permute(0, 3, 1, 2).contiguous()

    spec = (args.timestep_respacing.replace(",", "-") or "full") + (f"_ddim_eta{args.eta:g}" if args.use_ddim else "")
    kw = dict(tol=args.tol, respacing=args.timestep_respacing or None, ddim=args.use_ddim, eta=args.eta)
    print(f"Deblurring {n} images ({args.kernel} kernel, {spec} steps) with {args.saved_model}.")
    stage = OutputStage()
    t0 = time.time()
    for g, i in enumerate(range(0, n, args.batch_size)):
        torch.manual_seed(args.seed + g)          # x_T and the Philox key of batch g
        stage.submit(model.deblur(y_all[i:i + args.batch_size].to(device), args.kernel, **kw))
    batches = stage.finish()
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    out_dir = args.out_dir or SAMPLE_DIR
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, f"{args.saved_model}_deblur_{args.kernel}_{spec}")
    np.save(base + ".npy", np.concatenate(batches).astype(np.float32), allow_pickle=False)
    np.save(base + "_blurred.npy", blurred, allow_pickle=False)
    print(f"Deblurred images saved to {base}.npy, blurred inputs to {base}_blurred.npy")


if __name__ == "__main__":
    main()
