"""Reconstruct images from compressed-sensing measurements with a trained, unconditional DDPM checkpoint: zero-shot compressed sensing
with DDNM (Wang, Yu, Zhang, ICLR 2023) for a subsampled, permuted Walsh-Hadamard transform, DESIGN.md section 3.17.

Loads the checkpoint as generate_model_samples.py does (``--synthetic CONFIG`` builds closed-form weights instead) and runs
``model.restore_cs``:

  * every colour plane is flattened row-major, read through the pixel permutation of ``--perm_seed``
    (models.diffusion.hadamard.cs_perm) and transformed by the orthonormal Walsh-Hadamard matrix in natural order; the measurement is
    the first m = 4 round(ratio N / 4) coefficients (``--ratio`` in (0, 1]; the paper's are 0.5, 0.25 and 0.1);
  * ``--images file.npy`` holds float32 measurements [N, C, m]; with ``--measure_input`` it holds uint8 images [N, H, W, C] of the
    model's size, which are measured here first, on the GPU (ops.hadamard_measure), so a test set can be measured and restored in
    one go;
  * ``--timestep_respacing``, ``--use_ddim`` and ``--eta`` choose the chain as in generate_model_samples.py;
  * batch g draws x_T and its Philox key from ``--seed`` + g;
  * a dDDPM checkpoint is refused: a transform of its latent is not a transform of the image.

Writes ``{saved_model}_cs_r{ratio}_p{perm_seed}_{spec}.npy`` through the sampling driver's output stage (utils.OutputStage: float32
[N, H, W, C], each image min-max scaled to [0, 255] like the sample files) and ``..._measurements.npy``, the float32 [N, C, m]
measurements it started from.  One process, one GPU.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from ddk import ops
from models import DDPM, Unet
from models.diffusion import hadamard
from utils import CHECKPOINT_DIR, SAMPLE_DIR, OutputStage, get_color_channels, get_model_state_dict, load_checkpoint_file
from utils import synthetic as syn


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Reconstruct images from Walsh-Hadamard measurements with a trained DDPM checkpoint (DDNM).")
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--images", required=True, help="float32 .npy [N, C, m] of measurements, or uint8 [N, H, W, C] images with --measure_input")
    ap.add_argument("--ratio", type=float, default=0.25, help="sampling ratio in (0, 1]: m = 4 round(ratio H W / 4) coefficients per plane")
    ap.add_argument("--perm_seed", type=int, default=0, help="seed of the pixel permutation")
    ap.add_argument("--measure_input", action="store_true", help="the file holds images: measure them first")
    ap.add_argument("--timestep_respacing", default="", help='run K of the T steps: "ddimN", "N" or "n1,n2,..." sections')
    ap.add_argument("--use_ddim", action="store_true", help="DDIM steps instead of ancestral ones")
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM noise scale (0: deterministic)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234, help="base seed: batch g draws from seed + g")
    ap.add_argument("--out_dir", default=None)
    args = ap.parse_args(argv)
    if args.eta < 0 or (args.eta != 0.0 and not args.use_ddim):
        ap.error("--eta needs --use_ddim and a value >= 0")
    if not (0 < args.ratio <= 1):
        ap.error("--ratio must be in (0, 1]")
    if args.perm_seed < 0:
        ap.error("--perm_seed must be >= 0")
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
        raise SystemExit(f"compressed sensing needs a pixel model (ddpm), this checkpoint is a {config['model']}: a transform of a latent is "
                         "not a transform of the image")
    model = DDPM(config, Unet(config), device, color_channels)
    if model_state_dict is None:
        model_state_dict = syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS)
    model.load_state_dict(model_state_dict)
    model = model.to(device).eval()
    model.rng_stream_id = 0

    c, size = color_channels, int(config["image_size"])
    if not hadamard.size_ok(c, size, size):
        raise SystemExit(f"compressed sensing needs an image size that is a power of two in [16, 256], this model's is {size}")
    N = size * size
    m = hadamard.cs_rows(args.ratio, N)
    perm = hadamard.cs_perm(N, args.perm_seed)
    data = np.load(args.images)
    if args.measure_input:
        if data.dtype != np.uint8 or data.ndim != 4 or data.shape[1:] != (size, size, c):
            raise SystemExit(f"--images: expected uint8 [N, {size}, {size}, {c}] with --measure_input, got {data.dtype} {data.shape}")
        x_all = torch.from_numpy(data.astype(np.float32)) / 255 * 2 - 1          # NHWC
        pd = torch.from_numpy(perm).to(device)
        y_all = torch.cat([ops.hadamard_measure(x_all[i:i + args.batch_size].to(device).contiguous(), pd, m).cpu()
                           for i in range(0, x_all.shape[0], args.batch_size)])
    else:
        if data.dtype.kind != "f" or data.ndim != 3 or data.shape[1:] != (c, m):
            raise SystemExit(f"--images: expected float [N, {c}, {m}] measurements (ratio {args.ratio:g} of {N}), got {data.dtype} {data.shape}")
        y_all = torch.from_numpy(data.astype(np.float32))
    n = y_all.shape[0]

    spec = (args.timestep_respacing.replace(",", "-") or "full") + (f"_ddim_eta{args.eta:g}" if args.use_ddim else "")
    kw = dict(respacing=args.timestep_respacing or None, ddim=args.use_ddim, eta=args.eta)
    print(f"Reconstructing {n} images from {m} of {N} coefficients per plane ({spec} steps) with {args.saved_model}.")
    stage = OutputStage()
    t0 = time.time()
    for g, i in enumerate(range(0, n, args.batch_size)):
        torch.manual_seed(args.seed + g)          # x_T and the Philox key of batch g
        stage.submit(model.restore_cs(y_all[i:i + args.batch_size].to(device), perm, **kw))
    batches = stage.finish()
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    out_dir = args.out_dir or SAMPLE_DIR
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, f"{args.saved_model}_cs_r{args.ratio:g}_p{args.perm_seed}_{spec}")
    np.save(base + ".npy", np.concatenate(batches).astype(np.float32), allow_pickle=False)
    np.save(base + "_measurements.npy", y_all.numpy().astype(np.float32), allow_pickle=False)
    print(f"Reconstructions saved to {base}.npy, measurements to {base}_measurements.npy")


if __name__ == "__main__":
    main()
