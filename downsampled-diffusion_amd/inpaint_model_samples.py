"""Inpaint images with a trained DDPM / dDDPM checkpoint: RePaint (Lugmayr et al., CVPR 2022), DESIGN.md section 3.5, or with
``--method ddnm`` DDNM for a mask (Wang et al., ICLR 2023), section 3.8: K UNet forwards instead of RePaint's K + (r - 1) j ... .

Loads the checkpoint as generate_model_samples.py does (``--synthetic CONFIG`` builds closed-form weights instead), reads
``--images file.npy`` (uint8 or float [N, H, W, C] in [0, 255], the on-disk format of the sample files; mapped by
u8 / 255 * 2 - 1 as the training data is), hides the region given by ``--mask`` and fills it with ``model.inpaint``:

  * ``--mask center|left|half|lines`` (1 = known): hide the central square of half the side, the left half, the bottom half,
    or every second row; or ``--mask file.npy``: {0, 1} of shape [H, W], [N, H, W] or [N, H, W, 1|C];
  * ``--timestep_respacing`` (e.g. "250"), ``--jump_length`` and ``--jump_n_sample`` set the RePaint schedule;
  * ``--method ddnm`` fills with ``model.restore`` (scale 1) instead: ``--use_ddim`` and ``--eta`` choose DDIM steps, the
    ``--jump_*`` options must stay at their defaults, and a mask that differs between the channels counts a pixel as known only
    where every channel is; ``--dpm_solver`` (with ``--method ddnm`` only, not with ``--use_ddim`` / ``--eta``) fills with
    ``model.restore_solver``, DDNM on the DPM-Solver++(2M) chain (section 3.9; use a log-SNR grid, e.g. ``logsnr20``);
  * ``--sigma_y S`` (with ``--method ddnm`` only, not with ``--dpm_solver``) declares that the known pixels of the given images
    carry noise of standard deviation S in the model's [-1, 1] scale (S = 2 s / 255 for s uint8 levels): the fill is
    ``model.restore_noisy`` (DDNM+, section 3.10), which never pastes the noisy pixels back, and the names gain ``_sy{S}``;
  * batch g draws x_T and its Philox key from ``--seed`` + g.

Writes ``{saved_model}_inpaint_{mask}_{spec}_j{j}r{r}.npy`` (float32 [N, H, W, C] in [0, 255]; with ``--method ddnm``
``{saved_model}_inpaint_{mask}_{spec}_ddnm[_ddim_eta{eta}|_dpmpp2m][_sy{S}].npy``) and, beside it, the masked inputs for viewing
(``..._masked.npy``, hidden pixels 0).  One process, one GPU.
"""
import argparse
import os
import time

import numpy as np
import torch

from utils import sampling_cli as cli
from utils import synthetic as syn
from utils.restoration_metrics import MASKS, load_mask, make_mask


def to_u8_range(x):
    """[-1, 1] NCHW -> float32 NHWC in [0, 255]."""
    return ((x.clamp(-1, 1) + 1) * 127.5).permute(0, 2, 3, 1).cpu().numpy().astype(np.float32)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Inpaint images with a trained DDPM / dDDPM checkpoint (RePaint).")
    cli.add_chain_flags(ap, solver=True, prefix="ddnm: ", respacing_help='run the schedule over K of the T steps, e.g. "250" (default: all T)',
                        sigma_y="ddnm: the noise level of the known pixels in the [-1, 1] scale (DDNM+); not with --dpm_solver")
    ap.add_argument("--images", default=None, help="[N, H, W, C] .npy in [0, 255] (default with --synthetic: synthetic images)")
    ap.add_argument("--n_images", type=int, default=4, help="number of synthetic images when --images is not given")
    ap.add_argument("--mask", default="center", help=f"one of {', '.join(MASKS)} or a .npy file of {{0, 1}} (1 = known)")
    ap.add_argument("--method", default="repaint", choices=("repaint", "ddnm"), help="repaint (section 3.5) or ddnm (section 3.8)")
    ap.add_argument("--jump_length", type=int, default=10)
    ap.add_argument("--jump_n_sample", type=int, default=10)
    args = ap.parse_args(argv)
    if args.jump_length < 1 or args.jump_n_sample < 1 or args.batch_size < 1:
        ap.error("--jump_length, --jump_n_sample and --batch_size must be >= 1")
    cli.check_chain_flags(ap, args, "sigma_y")
    if args.method == "ddnm":
        if args.jump_length != ap.get_default("jump_length") or args.jump_n_sample != ap.get_default("jump_n_sample"):
            ap.error("--jump_length and --jump_n_sample belong to --method repaint (DDNM has no jumps)")
        cli.check_chain_flags(ap, args, "sigma_y_solver sigma_y_draws solver eta")
    elif args.use_ddim or args.eta != 0.0 or args.dpm_solver or args.sigma_y != 0.0:
        ap.error("--use_ddim, --eta, --dpm_solver and --sigma_y belong to --method ddnm (RePaint runs ancestral steps)")
    if args.images is None and not args.synthetic:
        ap.error("--images is required unless --synthetic is given")
    return args


def main():
    args = parse_args()
    device = "cuda:0"
    torch.cuda.set_device(0)
    model, config, color_channels, _ = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device)

    c, h, w = color_channels, int(config["image_size"]), int(config["image_size"])
    if args.images:
        imgs = np.load(args.images)
        if imgs.ndim != 4 or imgs.shape[1:] != (h, w, c):
            raise SystemExit(f"--images: expected [N, {h}, {w}, {c}], got {imgs.shape}")
        x_all = cli.u8_to_unit(imgs).permute(0, 3, 1, 2)
    else:
        x_all = syn.synthetic_normal((args.n_images, c, h, w), "inpaint.images").clamp(-1, 1)
    n = x_all.shape[0]
    if args.mask in MASKS:
        mask_all, mask_name = make_mask(args.mask, n, h, w), args.mask
    else:
        mask_all, mask_name = load_mask(args.mask, n, h, w, c), os.path.splitext(os.path.basename(args.mask))[0]

    spec = cli.respacing_name(args)
    ddnm = args.method == "ddnm"
    if ddnm:
        kw = cli.chain_kwargs(args)
        tail = "_ddnm" + cli.step_tags(args)
        what = "DDNM on DPM-Solver++(2M)" if args.dpm_solver else "DDNM"
        if args.sigma_y != 0.0:
            kw.update(sigma_y=args.sigma_y)
            what = f"DDNM+ for sigma_y = {args.sigma_y:g}"
        print(f"Inpainting {n} images ({mask_name} mask, {spec} steps, {what}{', DDIM eta ' + format(args.eta, 'g') if args.use_ddim else ''}) "
              f"with {args.saved_model}.")
        run = model.restore_solver if args.dpm_solver else model.restore_noisy if args.sigma_y != 0.0 else model.restore
        restore = lambda i: run(x_all[i:i + args.batch_size].to(device), mask_all[i:i + args.batch_size].to(device).amin(dim=1), 1, **kw)
    else:
        kw = dict(respacing=args.timestep_respacing or None, jump_length=args.jump_length, jump_n_sample=args.jump_n_sample)
        tail = f"_j{args.jump_length}r{args.jump_n_sample}"
        print(f"Inpainting {n} images ({mask_name} mask, {spec} steps, j = {args.jump_length}, r = {args.jump_n_sample}) "
              f"with {args.saved_model}.")
        restore = lambda i: model.inpaint(x_all[i:i + args.batch_size].to(device), mask_all[i:i + args.batch_size].to(device), **kw)
    # no output stage here: the known pixels keep their values, so the images are clamped and scaled, not min-max normalised each
    t0 = time.time()
    outs = [to_u8_range(out) for out in cli.seeded_batches(n, args.batch_size, args.seed, restore)]
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    masked = to_u8_range(x_all) * mask_all.expand(-1, c, -1, -1).permute(0, 2, 3, 1).numpy()
    base = cli.save_outputs(args.out_dir, f"{args.saved_model}_inpaint_{mask_name}_{spec}{tail}", np.concatenate(outs), "_masked",
                            masked.astype(np.float32))
    print(f"Inpainted images saved to {base}.npy, masked inputs to {base}_masked.npy")


if __name__ == "__main__":
    main()
