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
import json
import os
import time

import numpy as np
import torch

from models import DDPM, DownsampleDDPM, Unet
from utils import CHECKPOINT_DIR, SAMPLE_DIR, get_color_channels, get_model_state_dict, load_checkpoint_file
from utils import synthetic as syn
from utils.restoration_metrics import MASKS, load_mask, make_mask


def to_u8_range(x):
    """[-1, 1] NCHW -> float32 NHWC in [0, 255]."""
    return ((x.clamp(-1, 1) + 1) * 127.5).permute(0, 2, 3, 1).cpu().numpy().astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description="Inpaint images with a trained DDPM / dDDPM checkpoint (RePaint).")
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--images", default=None, help="[N, H, W, C] .npy in [0, 255] (default with --synthetic: synthetic images)")
    ap.add_argument("--n_images", type=int, default=4, help="number of synthetic images when --images is not given")
    ap.add_argument("--mask", default="center", help=f"one of {', '.join(MASKS)} or a .npy file of {{0, 1}} (1 = known)")
    ap.add_argument("--timestep_respacing", default="", help='run the schedule over K of the T steps, e.g. "250" (default: all T)')
    ap.add_argument("--method", default="repaint", choices=("repaint", "ddnm"), help="repaint (section 3.5) or ddnm (section 3.8)")
    ap.add_argument("--use_ddim", action="store_true", help="ddnm: DDIM steps instead of ancestral ones")
    ap.add_argument("--eta", type=float, default=0.0, help="ddnm: DDIM noise scale (0: deterministic)")
    ap.add_argument("--dpm_solver", action="store_true",
                    help='ddnm: DPM-Solver++(2M) steps over the --timestep_respacing grid (e.g. "logsnr20"); not with --use_ddim / --eta')
    ap.add_argument("--sigma_y", type=float, default=0.0,
                    help="ddnm: the noise level of the known pixels in the [-1, 1] scale (DDNM+); not with --dpm_solver")
    ap.add_argument("--jump_length", type=int, default=10)
    ap.add_argument("--jump_n_sample", type=int, default=10)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1234, help="base seed: batch g draws from seed + g")
    ap.add_argument("--out_dir", default=None)
    args = ap.parse_args()
    if args.jump_length < 1 or args.jump_n_sample < 1 or args.batch_size < 1:
        ap.error("--jump_length, --jump_n_sample and --batch_size must be >= 1")
    if not np.isfinite(args.sigma_y) or args.sigma_y < 0:
        ap.error("--sigma_y must be a finite number >= 0")
    if args.method == "ddnm":
        if args.jump_length != ap.get_default("jump_length") or args.jump_n_sample != ap.get_default("jump_n_sample"):
            ap.error("--jump_length and --jump_n_sample belong to --method repaint (DDNM has no jumps)")
        if args.sigma_y != 0.0 and args.dpm_solver:
            ap.error("--sigma_y and --dpm_solver are exclusive (the solver draws nothing, so there is no variance to trade)")
        if args.sigma_y != 0.0 and args.use_ddim and args.eta == 0.0:
            ap.error("--sigma_y needs a chain that draws: ancestral steps, or --use_ddim with --eta > 0")
        if args.dpm_solver and (args.use_ddim or args.eta != 0.0):
            ap.error("--dpm_solver is its own deterministic update: it cannot be combined with --use_ddim or --eta")
        if args.eta < 0 or (args.eta != 0.0 and not args.use_ddim):
            ap.error("--eta needs --use_ddim and a value >= 0")
    elif args.use_ddim or args.eta != 0.0 or args.dpm_solver or args.sigma_y != 0.0:
        ap.error("--use_ddim, --eta, --dpm_solver and --sigma_y belong to --method ddnm (RePaint runs ancestral steps)")
    if args.images is None and not args.synthetic:
        ap.error("--images is required unless --synthetic is given")

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

    c, h, w = color_channels, int(config["image_size"]), int(config["image_size"])
    if args.images:
        imgs = np.load(args.images)
        if imgs.ndim != 4 or imgs.shape[1:] != (h, w, c):
            raise SystemExit(f"--images: expected [N, {h}, {w}, {c}], got {imgs.shape}")
        x_all = torch.from_numpy(imgs.astype(np.float32)).permute(0, 3, 1, 2) / 255 * 2 - 1
    else:
        x_all = syn.synthetic_normal((args.n_images, c, h, w), "inpaint.images").clamp(-1, 1)
    n = x_all.shape[0]
    if args.mask in MASKS:
        mask_all, mask_name = make_mask(args.mask, n, h, w), args.mask
    else:
        mask_all, mask_name = load_mask(args.mask, n, h, w, c), os.path.splitext(os.path.basename(args.mask))[0]

    spec = args.timestep_respacing.replace(",", "-") or "full"
    ddnm = args.method == "ddnm"
    if ddnm and args.dpm_solver:
        kw = dict(respacing=args.timestep_respacing or None, solver="dpm++2m")
        tail = "_ddnm_dpmpp2m"
        print(f"Inpainting {n} images ({mask_name} mask, {spec} steps, DDNM on DPM-Solver++(2M)) with {args.saved_model}.")
    elif ddnm:
        kw = dict(respacing=args.timestep_respacing or None, ddim=args.use_ddim, eta=args.eta)
        tail = "_ddnm" + (f"_ddim_eta{args.eta:g}" if args.use_ddim else "")
        what = "DDNM"
        if args.sigma_y != 0.0:
            kw.update(sigma_y=args.sigma_y)
            tail += f"_sy{args.sigma_y:g}"
            what = f"DDNM+ for sigma_y = {args.sigma_y:g}"
        print(f"Inpainting {n} images ({mask_name} mask, {spec} steps, {what}{', DDIM eta ' + format(args.eta, 'g') if args.use_ddim else ''}) "
              f"with {args.saved_model}.")
    else:
        kw = dict(respacing=args.timestep_respacing or None, jump_length=args.jump_length, jump_n_sample=args.jump_n_sample)
        tail = f"_j{args.jump_length}r{args.jump_n_sample}"
        print(f"Inpainting {n} images ({mask_name} mask, {spec} steps, j = {args.jump_length}, r = {args.jump_n_sample}) "
              f"with {args.saved_model}.")
    outs = []
    t0 = time.time()
    for g, i in enumerate(range(0, n, args.batch_size)):
        torch.manual_seed(args.seed + g)          # x_T and the Philox key of batch g
        x, m = x_all[i:i + args.batch_size].to(device), mask_all[i:i + args.batch_size].to(device)
        if ddnm:
            run = model.restore_solver if args.dpm_solver else model.restore_noisy if args.sigma_y != 0.0 else model.restore
            out = run(x, m.amin(dim=1), 1, **kw)
        else:
            out = model.inpaint(x, m, **kw)
        if config["model"] == "dddpm":
            out = out[0]
        outs.append(to_u8_range(out))
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")

    out_dir = args.out_dir or SAMPLE_DIR
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, f"{args.saved_model}_inpaint_{mask_name}_{spec}{tail}")
    np.save(base + ".npy", np.concatenate(outs), allow_pickle=False)
    masked = to_u8_range(x_all) * mask_all.expand(-1, c, -1, -1).permute(0, 2, 3, 1).numpy()
    np.save(base + "_masked.npy", masked.astype(np.float32), allow_pickle=False)
    print(f"Inpainted images saved to {base}.npy, masked inputs to {base}_masked.npy")


if __name__ == "__main__":
    main()
