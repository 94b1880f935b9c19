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

import numpy as np
import torch

from ddk import ops
from models.diffusion import hadamard
from utils import sampling_cli as cli


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Reconstruct images from Walsh-Hadamard measurements with a trained DDPM checkpoint (DDNM).")
    cli.add_chain_flags(ap)
    ap.add_argument("--images", required=True, help="float32 .npy [N, C, m] of measurements, or uint8 [N, H, W, C] images with --measure_input")
    ap.add_argument("--ratio", type=float, default=0.25, help="sampling ratio in (0, 1]: m = 4 round(ratio H W / 4) coefficients per plane")
    ap.add_argument("--perm_seed", type=int, default=0, help="seed of the pixel permutation")
    ap.add_argument("--measure_input", action="store_true", help="the file holds images: measure them first")
    args = ap.parse_args(argv)
    cli.check_chain_flags(ap, args, "eta")
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
    model, config, c, _ = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device, pixel_only=(
        "compressed sensing needs a pixel model (ddpm), this checkpoint is a {model}: a transform of a latent is not a transform of the image"))

    size = int(config["image_size"])
    if not hadamard.size_ok(c, size, size):
        raise SystemExit(f"compressed sensing needs an image size that is a power of two in [16, 256], this model's is {size}")
    N = size * size
    m = hadamard.cs_rows(args.ratio, N)
    perm = hadamard.cs_perm(N, args.perm_seed)
    if args.measure_input:
        x_all = cli.u8_to_unit(cli.load_uint8_images(args.images, ((size, size, c),), expected=f"[N, {size}, {size}, {c}] with --measure_input"))
        pd = torch.from_numpy(perm).to(device)
        y_all = torch.cat([ops.hadamard_measure(x_all[i:i + args.batch_size].to(device).contiguous(), pd, m).cpu()          # (x_all is NHWC)
                           for i in range(0, x_all.shape[0], args.batch_size)])
    else:
        data = np.load(args.images)
        if data.dtype.kind != "f" or data.ndim != 3 or data.shape[1:] != (c, m):
            raise SystemExit(f"--images: expected float [N, {c}, {m}] measurements (ratio {args.ratio:g} of {N}), got {data.dtype} {data.shape}")
        y_all = torch.from_numpy(data.astype(np.float32))
    n = y_all.shape[0]

    spec = cli.chain_spec(args)
    kw = cli.chain_kwargs(args)
    print(f"Reconstructing {n} images from {m} of {N} coefficients per plane ({spec} steps) with {args.saved_model}.")
    restored = cli.run_batches(n, args.batch_size, args.seed, lambda i: model.restore_cs(y_all[i:i + args.batch_size].to(device), perm, **kw))

    base = cli.save_outputs(args.out_dir, f"{args.saved_model}_cs_r{args.ratio:g}_p{args.perm_seed}_{spec}", restored, "_measurements",
                            y_all.numpy().astype(np.float32))
    print(f"Reconstructions saved to {base}.npy, measurements to {base}_measurements.npy")


if __name__ == "__main__":
    main()
