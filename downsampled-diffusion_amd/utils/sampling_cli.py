"""What the sampling and evaluation scripts share (generate / inpaint / upscale / colorize / deblur / cs / deconv _model_samples.py,
evaluate_restoration.py, evaluate_ddpm.py): the model load, the chain flags with their checks, the file-name fragment and the keywords
the flags stand for, the uint8 input images, the seeded batch loop and the two output files.  Plain functions; what only one script
does stays in that script."""
import json
import os
import time

import numpy as np
import torch

from .eval_helpers import OutputStage
from .paths import CHECKPOINT_DIR, SAMPLE_DIR

RESPACING_HELP = 'run K of the T steps: "ddimN", "N" or "n1,n2,..." sections'


# ------------------------------------------------------------------ model
def load_model(saved_model, synthetic, batch_size, device, *, default_force_latent=False, pixel_only=None, fill=True):
    """``{saved_model}.pt`` from CHECKPOINT_DIR (EMA weights preferred), or closed-form synthetic weights for the JSON config file
    ``synthetic``, rebuilt from its config on ``device`` in eval mode.  Returns (model, config, color_channels, step).

    batch_size None keeps the config's.  default_force_latent: a dDDPM config from before that key gets ``force_latent = False``
    (reference evaluate_ddpm.py:24-28).  pixel_only: the SystemExit message ("{model}" is filled in) for a config that is no pixel
    ddpm.  fill=False leaves the weights as constructed, for a rank that receives them by broadcast."""
    from models import DDPM, DownsampleDDPM, Unet
    from . import synthetic as syn
    from .data import get_color_channels
    from .utils import get_model_state_dict, load_checkpoint_file
    step = 0
    if synthetic:
        with open(synthetic) as f:
            config = json.load(f)
        model_state_dict = None
    else:
        save_data = load_checkpoint_file(os.path.join(CHECKPOINT_DIR, f"{saved_model}.pt"))
        model_state_dict = get_model_state_dict(save_data)
        config = save_data["config"]
        step = save_data.get("step", 0)
    if default_force_latent and config["model"] == "dddpm" and "force_latent" not in config:
        config["force_latent"] = False
    if batch_size is not None:
        config["batch_size"] = batch_size
    color_channels = get_color_channels(config["dataset"])
    if pixel_only is not None and config["model"] != "ddpm":
        raise SystemExit(pixel_only.format(model=config["model"]))
    if config["model"] == "ddpm":
        model = DDPM(config, Unet(config), device, color_channels)
    elif config["model"] == "dddpm":
        model = DownsampleDDPM(config, Unet(config), device, color_channels)
    else:
        raise NotImplementedError(config["model"])
    if fill:
        if model_state_dict is None:
            model_state_dict = syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS)
        model.load_state_dict(model_state_dict)
    model = model.to(device).eval()
    model.rng_stream_id = 0
    return model, config, color_channels, step


# ------------------------------------------------------------------ flags
def add_chain_flags(ap, *, batch_size=32, solver=False, sigma_y=None, out_dir=True, prefix="", respacing_help=RESPACING_HELP):
    """the flags every chain script has: checkpoint, chain, batch and seed; ``solver`` adds --dpm_solver, ``sigma_y`` (its help text)
    adds --sigma_y, ``out_dir`` adds --out_dir.  ``prefix`` goes before the help of the flags that only one of a script's methods takes."""
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--timestep_respacing", default="", help=respacing_help)
    ap.add_argument("--use_ddim", action="store_true", help=prefix + "DDIM steps instead of ancestral ones")
    ap.add_argument("--eta", type=float, default=0.0, help=prefix + "DDIM noise scale (0: deterministic)")
    if solver:
        ap.add_argument("--dpm_solver", action="store_true", help=prefix + 'DPM-Solver++(2M) steps over the --timestep_respacing grid (e.g. '
                                                                           '"logsnr20"); not with --use_ddim / --eta')
    if sigma_y:
        ap.add_argument("--sigma_y", type=float, default=0.0, help=sigma_y)
    ap.add_argument("--batch_size", type=int, default=batch_size)
    ap.add_argument("--seed", type=int, default=1234, help="base seed: batch g draws from seed + g")
    if out_dir:
        ap.add_argument("--out_dir", default=None)


CHAIN_RULES = {
    "eta": (lambda a: a.eta < 0 or (a.eta != 0.0 and not a.use_ddim),
            "--eta needs --use_ddim and a value >= 0"),
    "solver": (lambda a: a.dpm_solver and (a.use_ddim or a.eta != 0.0),
               "--dpm_solver is its own deterministic update: it cannot be combined with --use_ddim or --eta"),
    "sigma_y": (lambda a: not np.isfinite(a.sigma_y) or a.sigma_y < 0,
                "--sigma_y must be a finite number >= 0"),
    "sigma_y_solver": (lambda a: a.sigma_y != 0.0 and a.dpm_solver,
                       "--sigma_y and --dpm_solver are exclusive (the solver draws nothing, so there is no variance to trade)"),
    "sigma_y_draws": (lambda a: a.sigma_y != 0.0 and a.use_ddim and a.eta == 0.0,
                      "--sigma_y needs a chain that draws: ancestral steps, or --use_ddim with --eta > 0"),
}


def check_chain_flags(ap, args, rules, **messages):
    """ap.error for the first of ``rules`` (names of CHAIN_RULES, in the caller's order: a script's first complaint about a command
    line is part of its interface) that ``args`` breaks; ``messages`` replaces a rule's wording by the script's own."""
    for name in rules.split():
        broken, message = CHAIN_RULES[name]
        if broken(args):
            ap.error(messages.get(name, message))


# ------------------------------------------------------------------ flags -> names and keywords
def respacing_name(args):
    return args.timestep_respacing.replace(",", "-") or "full"


def step_tags(args, mid=""):
    """``_ddim_eta{eta}``, ``_dpmpp2m``, the caller's ``mid``, ``_sy{sigma_y}``: what follows the respacing in a file name"""
    sigma_y = getattr(args, "sigma_y", 0.0)
    return (f"_ddim_eta{args.eta:g}" if args.use_ddim else "") + ("_dpmpp2m" if getattr(args, "dpm_solver", False) else "") + mid + \
        (f"_sy{sigma_y:g}" if sigma_y != 0.0 else "")


def chain_spec(args, mid=""):
    """the chain's fragment of a file name, e.g. ``10-5_ddim_eta0.5_sy0.1``"""
    return respacing_name(args) + step_tags(args, mid)


def chain_kwargs(args):
    """the chain flags as the keywords of model.sample and the restore methods"""
    if getattr(args, "dpm_solver", False):
        return dict(respacing=args.timestep_respacing or None, solver="dpm++2m")
    return dict(respacing=args.timestep_respacing or None, ddim=args.use_ddim, eta=args.eta)


# ------------------------------------------------------------------ images
def load_uint8_images(path, shapes_allowed, flag="--images", expected=None):
    """the uint8 [N, H, W, C] array of a .npy file whose [H, W, C] is one of ``shapes_allowed``, or SystemExit"""
    imgs = np.load(path)
    if imgs.dtype != np.uint8 or imgs.ndim != 4 or imgs.shape[1:] not in shapes_allowed:
        expected = expected or " or ".join(f"[N, {h}, {w}, {c}]" for h, w, c in shapes_allowed)
        raise SystemExit(f"{flag}: expected uint8 {expected}, got {imgs.dtype} {imgs.shape}")
    return imgs


def u8_to_unit(imgs):
    """uint8 array -> float32 tensor in [-1, 1], as the training data is mapped; the layout stays"""
    return torch.from_numpy(imgs.astype(np.float32)) / 255 * 2 - 1


def unit_to_u8(y):
    """tensor in [-1, 1] (values outside are clamped) -> uint8 array, rounded to nearest; the layout stays"""
    return ((y + 1) * 127.5).round().clamp(0, 255).numpy().astype(np.uint8)


# ------------------------------------------------------------------ batches and files
def seeded_batches(n, batch_size, seed, restore):
    """restore(i) for the batches starting at image i = 0, batch_size, ... of n, batch g seeded with seed + g"""
    for g, i in enumerate(range(0, n, batch_size)):
        torch.manual_seed(seed + g)          # x_T and the Philox key of batch g
        out = restore(i)
        yield out[0] if isinstance(out, tuple) else out      # a dDDPM returns (x_out, z)


def run_batches(n, batch_size, seed, restore):
    """seeded_batches through the sampling driver's output stage: float32 [N, H, W, C], each image min-max scaled to [0, 255]"""
    stage = OutputStage()
    t0 = time.time()
    for out in seeded_batches(n, batch_size, seed, restore):
        stage.submit(out)
    batches = stage.finish()
    torch.cuda.synchronize()
    print(f"Total time: {time.time() - t0:.2f} s")
    return np.concatenate(batches).astype(np.float32)


def save_outputs(out_dir, name, restored, suffix, companion):
    """``{name}.npy`` and ``{name}{suffix}.npy`` (the input the run started from) in out_dir (default SAMPLE_DIR); returns their base"""
    out_dir = out_dir or SAMPLE_DIR
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, name)
    np.save(base + ".npy", restored, allow_pickle=False)
    np.save(base + suffix + ".npy", companion, allow_pickle=False)
    return base
