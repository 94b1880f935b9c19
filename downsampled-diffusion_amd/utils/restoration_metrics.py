"""Full-reference scoring of the two restoration paths: degrade a set of ground-truth images, restore them
with ``model.inpaint`` (RePaint, section 3.5) or ``model.super_resolve`` (DDNM, section 3.6) and measure PSNR and SSIM of the result
and of network-free baselines against the originals.  The metrics are ``ddk.ops.image_metrics`` (HIP); torch does the degradations,
the baselines and the bookkeeping.

Images travel as uint8 [N, H, W, C], the format the CLIs write; a model sees u8 / 255 * 2 - 1 in NCHW, as the training data is
mapped.  The mask kinds and the pooling live here and the CLIs (inpaint_model_samples.py, upscale_model_samples.py,
evaluate_restoration.py) import them, so a score is of the degradation the sampling CLIs apply.
"""
import math

import numpy as np
import torch

from .sampling_cli import seeded_batches

MASKS = ("center", "left", "half", "lines")
TASKS = ("inpaint", "sr", "colorize")
DEBLUR_TASK = "deblur"          # evaluate_restoration's fourth task (section 3.14), with kernels of its own instead of masks and scales
BLUR_KERNELS = ("uniform", "gauss", "aniso")
CS_TASK = "cs"                  # ... and its fifth (section 3.17), with a sampling ratio and a permutation seed
DECONV_TASK = "deconv"          # ... and its sixth (section 3.18), with a 2-D point-spread function
DECONV_NOISY_TASK = "deconv_noisy"      # ... and its seventh (section 3.19): the blurred image carries noise
METHODS = ("repaint", "ddnm")
GRAY_WEIGHTS = {"mean": (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0), "luma": (0.299, 0.587, 0.114)}     # DDPM.colorize's two operators
DOWNSAMPLES = ("mean", "bicubic")     # task "sr": block means (section 3.6) or the antialiased bicubic reduction (section 3.15)


# ------------------------------------------------------------------ degradations
def make_mask(kind, n, h, w):
    """[N, 1, H, W] float {0, 1}, 1 = known."""
    m = torch.ones(n, 1, h, w)
    if kind == "center":
        m[:, :, h // 4:h - h // 4, w // 4:w - w // 4] = 0
    elif kind == "left":
        m[:, :, :, :w // 2] = 0
    elif kind == "half":
        m[:, :, h // 2:, :] = 0
    elif kind == "lines":
        m[:, :, 1::2, :] = 0
    else:
        raise ValueError(f"unknown mask {kind!r}: one of {MASKS} or a .npy file")
    return m


def load_mask(path, n, h, w, c):
    a = np.load(path)
    if a.ndim == 2:
        a = a[None]
    if a.ndim == 3:
        a = a[..., None]
    if a.ndim != 4 or a.shape[1:3] != (h, w) or a.shape[3] not in (1, c) or a.shape[0] not in (1, n):
        raise ValueError(f"mask file {path}: expected [H, W], [N, H, W] or [N, H, W, 1|C] with H, W = {h}, {w}, got {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).float().expand(n, -1, -1, -1)


def pool(x, scale):
    """scale x scale average pooling of [N, C, H, W]: the degradation of the super-resolution task (A of section 3.6)."""
    return torch.nn.functional.avg_pool2d(x, scale)


def resize_matrices(h, w, scale):
    """(A_h [h / scale, h], A_w [w / scale, w]) fp32: the antialiased bicubic reduction of section 3.15, one matrix per axis"""
    from models.diffusion import blur
    return tuple(torch.tensor(blur.resize_matrix(n, scale), dtype=torch.float32) for n in (h, w))


def resize(x, scale, device, batch_size=256):
    """the antialiased bicubic reduction by ``scale`` of [N, C, H, W] (A of section 3.15), on ``device`` through
    ops.separable_apply_rect: what DDPM.super_resolve(downsample="bicubic") inverts.  Returns a CPU tensor [N, C, H/scale, W/scale]."""
    from ddk import ops
    A_h, A_w = (m.to(device) for m in resize_matrices(x.shape[2], x.shape[3], scale))
    out = [ops.nhwc_to_nchw(ops.separable_apply_rect(ops.nchw_to_nhwc(x[i:i + batch_size].to(device).float().contiguous()), A_h, A_w)).cpu()
           for i in range(0, x.shape[0], batch_size)]
    return torch.cat(out)


def gray(x, weights):
    """the grey image [N, 1, H, W] of [N, 3, H, W]: the channels' weighted sum (the grey_w of section 3.11)"""
    if weights not in GRAY_WEIGHTS:
        raise ValueError(f"unknown weights {weights!r}: one of {tuple(GRAY_WEIGHTS)}")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"a grey image needs 3 channels, got {tuple(x.shape)}")
    return (x * x.new_tensor(GRAY_WEIGHTS[weights]).reshape(1, 3, 1, 1)).sum(dim=1, keepdim=True)


# ------------------------------------------------------------------ uint8 <-> model range
def from_u8(images):
    """uint8 [N, H, W, C] (numpy or torch) -> float32 [N, C, H, W] in [-1, 1]."""
    t = torch.as_tensor(images)
    if t.dtype != torch.uint8 or t.dim() != 4:
        raise ValueError(f"images must be uint8 [N, H, W, C], got {t.dtype} {tuple(t.shape)}")
    return t.float().permute(0, 3, 1, 2) / 255 * 2 - 1


def to_u8(x):
    """[N, C, H, W] in [-1, 1] (values outside are clamped) -> uint8 [N, H, W, C], rounded to nearest; inverts from_u8 exactly."""
    return ((x.float() + 1) * 127.5).round().clamp(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous()


# ------------------------------------------------------------------ baselines (no network)
def replicate(y, scale):
    """nearest upsampling: every low-resolution pixel repeated scale x scale (A+ of section 3.6)."""
    return y.repeat_interleave(scale, dim=2).repeat_interleave(scale, dim=3)


def bicubic(y, scale):
    return torch.nn.functional.interpolate(y, scale_factor=scale, mode="bicubic", align_corners=False)


def mean_fill(x, mask):
    """hidden pixels (mask 0) take their image's per-channel mean over the known pixels (0 if nothing is known)."""
    m = mask.expand_as(x)
    mean = (x * m).sum(dim=(2, 3), keepdim=True) / m.sum(dim=(2, 3), keepdim=True).clamp(min=1)
    return torch.where(m != 0, x, mean.expand_as(x))


# ------------------------------------------------------------------ scoring
def summarise(values):
    """mean and standard error of the mean (sample standard deviation / sqrt(n); nan for one image) of per-image values; images
    without a value (nan, e.g. the hidden-pixel PSNR of an image with nothing hidden) are left out."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return dict(mean=math.nan, stderr=math.nan, n=0)
    with np.errstate(invalid="ignore"):            # inf - inf: identical images have no spread to report
        stderr = float(v.std(ddof=1) / math.sqrt(v.size)) if v.size > 1 else math.nan
    return dict(mean=float(v.mean()), stderr=stderr, n=int(v.size))


def _score(ops, cand_u8, ref_u8, hidden, device):
    m = ops.image_metrics(cand_u8.to(device), ref_u8.to(device))
    out = dict(psnr=m["psnr"].numpy(), ssim=m["ssim"].double().numpy())
    if hidden is not None:
        out["psnr_hidden"] = ops.image_metrics(cand_u8.to(device), ref_u8.to(device), mask=hidden.to(device))["psnr"].numpy()
    return out


# ------------------------------------------------------------------ what the task evaluators share
def _setup(model, images_uint8, batch_size):
    """(x_all float [N, C, H, W] in [-1, 1], ref uint8 [N, H, W, C], the model's device) of the ground truth"""
    x_all = from_u8(images_uint8)
    if x_all.shape[0] < 1 or batch_size < 1:
        raise ValueError("evaluate_restoration needs at least one image and batch_size >= 1")
    return x_all, torch.as_tensor(images_uint8).contiguous(), model.betas.device


def _unet_forwards(model, chain, method="ddnm"):
    """UNet forwards per image of the chain that ``chain``'s keywords choose: the number of its steps"""
    respacing = chain.get("respacing")
    if "solver" in chain:
        return len(model._solver_tables(respacing, chain["solver"])[1])
    if method == "repaint":
        return len(model._inpaint_tables(respacing, chain.get("jump_length", 10), chain.get("jump_n_sample", 10))[1])
    if respacing is not None or chain.get("ddim"):
        return len(model._spaced_tables(respacing, chain.get("ddim", False), chain.get("eta", 0.0))[1])
    return int(model.timesteps)


def _restore_all(n, batch_size, seed, restore, images):
    """(x_out, images with "restored" in front): restore(i) over the seeded batches, as the sampling CLIs run them"""
    x_out = torch.cat([out.float().cpu() for out in seeded_batches(n, batch_size, seed, restore)])
    return x_out, dict(restored=to_u8(x_out), **images)


def _result(images, ref, hidden, device, method, extra):
    from ddk import ops
    methods = {name: _score(ops, img, ref, hidden, device) for name, img in images.items()}
    return dict(n_images=ref.shape[0], method=method, methods=methods, images={k: v.numpy() for k, v in images.items()}, **extra)


@torch.no_grad()
def evaluate_restoration(model, images_uint8, task, *, batch_size=32, seed=1234, mask="center", scale=None, method=None, sr_mask=None,
                         dpm_solver=False, sigma_y=0.0, downsample="mean", **chain):
    """Degrade, restore and score ``images_uint8`` (uint8 [N, H, W, C] of the model's size).

    task "inpaint": ``mask`` is one of MASKS or a {0, 1} tensor broadcastable to [N, 1|C, H, W] (1 = known); ``chain`` goes to
    ``model.inpaint`` (respacing, jump_length, jump_n_sample).  Baseline: mean_fill.  Every method also gets psnr_hidden, the PSNR
    over the hidden pixels only.
    task "sr": the images are average-pooled by ``scale`` (default 4); ``chain`` goes to ``model.super_resolve`` (respacing, ddim, eta).
    Baselines: replicate, bicubic.  consistency: per image max |pool(x_out) - y| * 127.5 (uint8 levels) of the model's float output,
    consistency_u8 the same of the uint8 image that is scored (rounding alone may cost 0.5, clamping to [0, 255] more).
    method (default: "repaint" for inpaint, "ddnm" for sr): "ddnm" with task "inpaint" fills with ``model.restore`` at scale 1
    (DDNM for a mask, section 3.8; ``chain``: respacing, ddim, eta; a pixel counts as known where every channel is).  Task "sr"
    with ``sr_mask`` is masked super-resolution: the mask (a kind of MASKS or a {0, 1} tensor broadcastable to
    [N, 1, H/scale, W/scale]) applies to the pooled image, ``model.restore`` upscales it, and the baselines mean-fill the pooled
    image's holes before they upsample it, so they are scored on the same degraded input.  The consistency is then over the
    measured pixels.  Without a mask, task "sr" is ``model.super_resolve`` as before.
    dpm_solver (method "ddnm" only; ``chain``: respacing alone, no ddim / eta): DDNM on the DPM-Solver++(2M) chain (section 3.9),
    ``model.restore_solver`` in place of ``restore`` / ``super_resolve``; the returned method is then "ddnm_dpmpp2m".
    sigma_y > 0 (method "ddnm" only, not with dpm_solver): the measurement is noisy (section 3.10).  N(0, sigma_y^2) noise from a
    generator seeded with ``seed`` is added to the float measurement (the image of task "inpaint", the pooled image of task "sr")
    after degrading and before restoring; ``model.restore_noisy`` restores it and the baselines are built from the same noisy
    measurement.  The returned method is "ddnm_plus" and "sigma_y" is returned; "consistency" / "consistency_u8" are then, per
    image, the RMS of pool(x_out) - y_clean over the measured pixels in uint8 levels (how far the result is from the clean
    measurement; task "inpaint" gets them too), since the result is not meant to reproduce the noisy one.  sigma_y = 0: exactly
    the result without it.
    task "colorize" (3-channel pixel models; section 3.11): the images are greyed with ``weights`` ("mean" or "luma") and
    average-pooled by ``scale`` (1, the default there: plain colourisation); ``sr_mask`` applies to that measurement as in task
    "sr"; ``model.colorize`` restores it (``chain``: respacing, ddim, eta), with ``sigma_y`` as above.  Baselines: "replicate", the
    grey image copied into the three channels (and every pixel repeated scale x scale), and at scale > 1 "bicubic".  consistency /
    consistency_u8: max |A(x_out) - y| over the measured pixels in uint8 levels (with sigma_y: the RMS against the clean y).  The
    returned method is "ddnm_gray", and "weights" is returned.
    task "deblur" (pixel models; section 3.14): the images are blurred with the separable ``kernel`` (required: "uniform", "gauss",
    "aniso"; zero padding) and ``model.deblur`` restores them (``chain``: tol, respacing, ddim, eta).  Baselines: "blurred", the measurement
    itself, and "pinv", A+ y clipped to [-1, 1] (the truncated pseudo-inverse alone, no network).  consistency / consistency_u8:
    max |A(x_out) - y| in uint8 levels, which the truncation keeps above zero.  The returned method is "ddnm_blur", and "kernel" and
    "tol" are returned.
    task "cs" (pixel models; section 3.17): every plane is measured by the first m = cs_rows(``ratio``, H W) coefficients of the
    orthonormal Walsh-Hadamard transform of its pixels permuted with ``perm_seed`` (default 0), on the device
    (ops.hadamard_measure), and ``model.restore_cs`` restores it (``chain``: respacing, ddim, eta).  Baseline: "adjoint", A^T y
    clipped to [-1, 1].  consistency: per image max |A(x_out) - y| of the model's float output, in the measurement's own scale.  The
    returned method is "ddnm_cs", and "ratio", "perm_seed" and "m" are returned.
    task "deconv" (pixel models; section 3.18): the images are blurred by the 2-D point-spread function ``psf`` ("diag", "disk", a
    .npy path or an array; periodic boundary) on the device (ops.circular_conv) and ``model.deconvolve`` restores them (``tol``;
    ``chain``: respacing, ddim, eta).  Baselines: "blurred" and "pinv", A+ y clipped to [-1, 1].  consistency: per image
    max |A+ A x_out - A+ y| of the model's float output.  The returned method is "ddnm_deconv", and "psf" and "tol" are returned.
    task "deconv_noisy" (pixel models; section 3.19): task "deconv" with N(0, sigma_y^2) noise, sigma_y > 0, from a generator seeded by
    ``seed`` added to the blurred images, restored by ``model.deconvolve_noisy``.  Baselines, all from the noisy image: "blurred",
    "pinv" (which shows the amplification) and "tikhonov", conj K^ / (|K^|^2 + sigma_y^2) applied through ops.circular_conv.  The
    returned method is "ddnm_plus", "sigma_y" is returned, and consistency / consistency_u8 are the RMS of A(x_out) - y_clean in
    uint8 levels: the result is not meant to reproduce the noisy image.
    downsample "bicubic" (task "sr" on a pixel model, without sr_mask, dpm_solver or sigma_y; section 3.15): the images are reduced
    by the antialiased bicubic matrix (``resize``) instead of pooled and ``model.super_resolve(downsample="bicubic")`` restores them.
    The baselines stay (replicate, bicubic upsampling); consistency / consistency_u8 are max |A(x_out) - y| in uint8 levels with that
    matrix, and "downsample" is returned.  The default, "mean", is the result without the argument.
    Batch g draws x_T and its Philox key from seed + g, as the sampling CLIs do.

    "method" and "unet_forwards" (UNet forwards per image: the chain's steps; the batch shares each forward) are returned too.
    Returns {"n_images", "methods": {name: {"psnr": [N], "ssim": [N], ...}}, "images": {name: uint8 [N, H, W, C]}} and, for "sr",
    "consistency" / "consistency_u8" [N]; "restored" is the model's entry."""
    if method == DPS_METHOD:
        if dpm_solver or sr_mask is not None or downsample != "mean":
            raise ValueError("method 'dps' runs ancestral or DDIM steps on an unmasked measurement (task 'inpaint': its mask): no dpm_solver, "
                             "sr_mask or downsample")
        return _evaluate_dps(model, images_uint8, task, batch_size=batch_size, seed=seed, mask=mask, scale=scale, sigma_y=sigma_y, **chain)
    if "zeta" in chain or "saturate" in chain:
        raise ValueError("zeta and saturate belong to method 'dps'")
    if downsample not in DOWNSAMPLES:
        raise ValueError(f"unknown downsample {downsample!r}: one of {DOWNSAMPLES}")
    if downsample != "mean" and (task != "sr" or sr_mask is not None or dpm_solver or sigma_y):
        raise ValueError("downsample 'bicubic' belongs to task 'sr' without a mask, dpm_solver or sigma_y")
    if task == DEBLUR_TASK:
        if method not in (None, "ddnm") or dpm_solver or sigma_y or sr_mask is not None or scale is not None:
            raise ValueError("task 'deblur' has one method, ddnm on ancestral or DDIM steps, and no mask, scale or sigma_y")
        if "kernel" not in chain or not hasattr(model, "deblur"):
            raise ValueError("task 'deblur' needs a kernel and a model with a deblur method (a pixel DDPM)")
        return _evaluate_deblur(model, images_uint8, batch_size=batch_size, seed=seed, **chain)
    if task == DECONV_TASK:
        if method not in (None, "ddnm") or dpm_solver or sigma_y or sr_mask is not None or scale is not None or "kernel" in chain:
            raise ValueError("task 'deconv' has one method, ddnm on ancestral or DDIM steps, and no mask, scale, kernel or sigma_y")
        if "psf" not in chain or not hasattr(model, "deconvolve"):
            raise ValueError("task 'deconv' needs a psf and a model with a deconvolve method (a pixel DDPM)")
        return _evaluate_deconv(model, images_uint8, batch_size=batch_size, seed=seed, **chain)
    if task == DECONV_NOISY_TASK:
        if method not in (None, "ddnm") or dpm_solver or sr_mask is not None or scale is not None or "kernel" in chain:
            raise ValueError("task 'deconv_noisy' has one method, ddnm on ancestral or DDIM (eta > 0) steps, and no mask, scale or kernel")
        if "psf" not in chain or not hasattr(model, "deconvolve_noisy"):
            raise ValueError("task 'deconv_noisy' needs a psf and a model with a deconvolve_noisy method (a pixel DDPM)")
        if isinstance(sigma_y, bool) or not isinstance(sigma_y, (int, float, np.integer, np.floating)) or not math.isfinite(sigma_y) or sigma_y <= 0:
            raise ValueError(f"task 'deconv_noisy' needs a finite sigma_y > 0 (sigma_y = 0 is task 'deconv'), got {sigma_y!r}")
        return _evaluate_deconv(model, images_uint8, batch_size=batch_size, seed=seed, sigma_y=float(sigma_y), **chain)
    if "psf" in chain:
        raise ValueError("psf belongs to task 'deconv'")
    if "kernel" in chain or "tol" in chain:
        raise ValueError("kernel and tol belong to task 'deblur'")
    if task == CS_TASK:
        if method not in (None, "ddnm") or dpm_solver or sigma_y or sr_mask is not None or scale is not None:
            raise ValueError("task 'cs' has one method, ddnm on ancestral or DDIM steps, and no mask, scale or sigma_y")
        if "ratio" not in chain or not hasattr(model, "restore_cs"):
            raise ValueError("task 'cs' needs a ratio and a model with a restore_cs method (a pixel DDPM)")
        return _evaluate_cs(model, images_uint8, batch_size=batch_size, seed=seed, **chain)
    if "ratio" in chain or "perm_seed" in chain:
        raise ValueError("ratio and perm_seed belong to task 'cs'")
    if task not in TASKS:
        raise ValueError(f"unknown task {task!r}: one of {(*TASKS, DEBLUR_TASK, CS_TASK, DECONV_TASK, DECONV_NOISY_TASK)}")
    if task == "colorize":
        return _evaluate_colorize(model, images_uint8, batch_size=batch_size, seed=seed, scale=1 if scale is None else scale, method=method,
                                  sr_mask=sr_mask, dpm_solver=dpm_solver, sigma_y=sigma_y, **chain)
    if "weights" in chain:
        raise ValueError("weights belongs to task 'colorize'")
    x_all, ref, device = _setup(model, images_uint8, batch_size)
    n, c, h, w = x_all.shape
    images, extra, hidden = {}, {}, None
    if method is None:
        method = "repaint" if task == "inpaint" else "ddnm"
    if method not in METHODS or (task == "sr" and method != "ddnm"):
        raise ValueError(f"unknown method {method!r} for task {task!r}: one of {METHODS} (sr: ddnm only)")
    if isinstance(sigma_y, bool) or not isinstance(sigma_y, (int, float, np.integer, np.floating)) or not math.isfinite(sigma_y) or sigma_y < 0:
        raise ValueError(f"sigma_y must be a finite real number >= 0, got {sigma_y!r}")
    sigma_y = float(sigma_y)
    if sigma_y and (method != "ddnm" or dpm_solver):
        raise ValueError("sigma_y needs method 'ddnm' on ancestral or DDIM (eta > 0) steps: not RePaint, not dpm_solver")
    if dpm_solver:
        if method != "ddnm" or chain.get("ddim") or chain.get("eta", 0.0) != 0.0:
            raise ValueError("dpm_solver runs DDNM on its own deterministic update: method 'ddnm', no ddim, no eta")
        chain = dict({k: v for k, v in chain.items() if k not in ("ddim", "eta")}, solver="dpm++2m")
    run = model.restore_solver if dpm_solver else model.restore
    K = _unet_forwards(model, chain, method)
    noise = None
    if sigma_y:
        run = lambda y, m, s, **kw: model.restore_noisy(y, m, s, sigma_y=sigma_y, **kw)
        noise = lambda like: sigma_y * torch.randn(like.shape, generator=torch.Generator().manual_seed(seed))
    if task == "inpaint":
        m_all = make_mask(mask, n, h, w) if isinstance(mask, str) else torch.as_tensor(mask).float().expand(n, -1, h, w)
        if method == "ddnm":
            m_all = m_all.amin(dim=1, keepdim=True)
            x_meas = x_all + noise(x_all) if sigma_y else x_all
            restore = lambda i: run(x_meas[i:i + batch_size].to(device), m_all[i:i + batch_size, 0].to(device), 1, **chain)
        else:
            restore = lambda i: model.inpaint(x_all[i:i + batch_size].to(device), m_all[i:i + batch_size].to(device), **chain)
        extra["unet_forwards"] = K
        images["mean_fill"] = to_u8(mean_fill(x_meas if sigma_y else x_all, m_all))
        hidden = (m_all.amin(dim=1) == 0).to(torch.uint8).contiguous()
    else:
        scale = 4 if scale is None else int(scale)
        if scale < 2 or h % scale or w % scale:
            raise ValueError(f"scale {scale} must be >= 2 and divide the image size {h} x {w}")
        if downsample == "bicubic":
            A_h, A_w = resize_matrices(h, w, scale)
            degrade = lambda x: torch.einsum("ih,bchw,jw->bcij", A_h, x, A_w)
            y_all = resize(x_all, scale, device)
            chain = dict(chain, downsample="bicubic")
            extra["downsample"] = "bicubic"
        else:
            degrade = lambda x: pool(x, scale)
            y_all = degrade(x_all)
        y_meas = y_all + noise(y_all) if sigma_y else y_all
        extra["unet_forwards"] = K
        my_all = None
        if sr_mask is None:
            restore = (lambda i: run(y_meas[i:i + batch_size].to(device), None, scale, **chain)) if dpm_solver or sigma_y else \
                (lambda i: model.super_resolve(y_all[i:i + batch_size].to(device), scale, **chain))
            y_base = y_meas
        else:
            hs, ws = h // scale, w // scale
            my_all = make_mask(sr_mask, n, hs, ws) if isinstance(sr_mask, str) else torch.as_tensor(sr_mask).float().expand(n, -1, hs, ws)
            my_all = my_all.amin(dim=1, keepdim=True)
            restore = lambda i: run(y_meas[i:i + batch_size].to(device), my_all[i:i + batch_size, 0].to(device), scale, **chain)
            y_base = mean_fill(y_meas, my_all)            # the baselines see the same holes
        images["replicate"] = to_u8(replicate(y_base, scale))
        images["bicubic"] = to_u8(bicubic(y_base, scale))
    x_out, images = _restore_all(n, batch_size, seed, restore, images)
    if sigma_y:
        # the result is not meant to reproduce the noisy measurement: its RMS distance from the CLEAN one over the measured pixels
        s1, y_clean = (1, x_all) if task == "inpaint" else (scale, y_all)
        meas = (m_all if task == "inpaint" else torch.ones_like(y_all[:, :1]) if my_all is None else my_all).expand_as(y_clean)
        rms = lambda x: ((((pool(x, s1) if s1 > 1 else x) - y_clean) ** 2 * meas).sum(dim=(1, 2, 3)) / meas.sum(dim=(1, 2, 3)).clamp(min=1)).sqrt() * 127.5
        extra["consistency"] = rms(x_out).double().numpy()
        extra["consistency_u8"] = rms(from_u8(images["restored"])).double().numpy()
        extra["sigma_y"] = sigma_y
    elif task == "sr":
        meas = 1.0 if my_all is None else my_all      # the constraint holds where y is measured
        extra["consistency"] = (((degrade(x_out) - y_all) * meas).abs().amax(dim=(1, 2, 3)) * 127.5).double().numpy()
        extra["consistency_u8"] = (((degrade(from_u8(images["restored"])) - y_all) * meas).abs().amax(dim=(1, 2, 3)) * 127.5).double().numpy()
    return _result(images, ref, hidden, device, method + ("_dpmpp2m" if dpm_solver else "_plus" if sigma_y else ""), extra)


DPS_METHOD = "dps"
DPS_TASKS = ("inpaint", "sr", DEBLUR_TASK, DECONV_TASK)


def dps_operator(task, *, mask=None, scale=None, kernel=None, psf=None):
    """(restore_guided's `operator` argument, the mask kind or tensor or None) of one of DPS_TASKS"""
    if task == "inpaint":
        return ("mean", 1), ("center" if mask is None else mask)
    if task == "sr":
        return ("mean", 4 if scale is None else int(scale)), None
    if task == DEBLUR_TASK:
        if kernel not in BLUR_KERNELS:
            raise ValueError(f"task 'deblur' needs a kernel, one of {BLUR_KERNELS}, got {kernel!r}")
        return kernel, None
    if task == DECONV_TASK:
        if psf is None:
            raise ValueError("task 'deconv' needs a psf")
        return ("psf", np.load(psf) if isinstance(psf, str) and psf.endswith(".npy") else psf), None
    raise ValueError(f"method 'dps' restores the tasks {DPS_TASKS}, got {task!r}")


@torch.no_grad()
def _evaluate_dps(model, images_uint8, task, *, batch_size, seed, mask, scale, sigma_y, zeta=None, saturate=None, kernel=None, psf=None,
                  **chain):
    """evaluate_restoration with method "dps" (Diffusion Posterior Sampling), for DDPM and dDDPM models alike:
    the images are measured on the device by the task's operator (guidance.Operator.measure: mask, block means, the separable blur or the
    circular convolution, then -- with ``saturate`` = GAIN -- clamp(GAIN u, -1, 1)), N(0, sigma_y^2) noise seeded by ``seed`` is added,
    and ``model.restore_guided(..., zeta=zeta)`` restores them (``chain``: respacing, ddim, eta).  Baseline: "measured", the measurement
    brought to the image's size (block means replicated; unmeasured pixels mean-filled).  consistency / consistency_u8: per image the RMS
    of phi(A x_out) - y_clean over the measured elements in uint8 levels (DPS approaches the measurement, it does not hold it).  The
    returned method is "dps"; "zeta", "unet_forwards" and "unet_backwards" (one input-gradient backward per forward) are returned."""
    from models.diffusion import guidance as G
    if zeta is None:
        raise ValueError("method 'dps' needs zeta, the step size of its gradient step")
    if isinstance(sigma_y, bool) or not isinstance(sigma_y, (int, float, np.integer, np.floating)) or not math.isfinite(sigma_y) or sigma_y < 0:
        raise ValueError(f"sigma_y must be a finite real number >= 0, got {sigma_y!r}")
    if set(chain) - {"respacing", "ddim", "eta"}:
        raise ValueError(f"method 'dps' takes respacing, ddim and eta, not {sorted(set(chain) - {'respacing', 'ddim', 'eta'})}")
    spec, mask = dps_operator(task, mask=mask, scale=scale, kernel=kernel, psf=psf)
    x_all, ref, device = _setup(model, images_uint8, batch_size)
    n, c, h, w = x_all.shape
    kw = dict(response="saturate", gain=float(saturate)) if saturate is not None else {}
    op = G.make_operator(spec, (c, h, w), **kw)
    m_all = None
    if mask is not None:
        m_all = (make_mask(mask, n, h, w) if isinstance(mask, str) else torch.as_tensor(mask).float().expand(n, -1, h, w)).amin(dim=1).contiguous()
    ys = []
    for i in range(0, n, batch_size):
        op.mask = None if m_all is None else m_all[i:i + batch_size].to(device)
        ys.append(op.measure(x_all[i:i + batch_size].permute(0, 2, 3, 1).contiguous().to(device)).permute(0, 3, 1, 2).cpu())
    y_clean = torch.cat(ys)
    meas = torch.ones_like(y_clean[:, :1]) if m_all is None else m_all.unsqueeze(1)
    y_meas = y_clean
    if sigma_y:
        y_meas = y_clean + float(sigma_y) * torch.randn(y_clean.shape, generator=torch.Generator().manual_seed(seed)) * meas
    restore = lambda i: model.restore_guided(y_meas[i:i + batch_size], spec, zeta=zeta, mask=None if m_all is None else m_all[i:i + batch_size],
                                             **kw, **chain)
    s = op.out_shape[1] and h // op.out_shape[1]
    base = replicate(y_meas, s) if s > 1 else y_meas
    images = dict(measured=to_u8(base if m_all is None else mean_fill(base, meas)))
    x_out, images = _restore_all(n, batch_size, seed, restore, images)

    def rms(x):
        out = []
        for i in range(0, n, batch_size):
            op.mask = None if m_all is None else m_all[i:i + batch_size].to(device)
            out.append(op.measure(x[i:i + batch_size].permute(0, 2, 3, 1).contiguous().to(device)).permute(0, 3, 1, 2).cpu())
        d = (torch.cat(out) - y_clean) ** 2 * meas
        return (d.sum(dim=(1, 2, 3)) / meas.expand_as(d).sum(dim=(1, 2, 3)).clamp(min=1)).sqrt() * 127.5
    K = _unet_forwards(model, chain)
    extra = dict(unet_forwards=K, unet_backwards=K, zeta=zeta, consistency=rms(x_out).double().numpy(),
                 consistency_u8=rms(from_u8(images["restored"])).double().numpy())
    if saturate is not None:
        extra["saturate"] = float(saturate)
    if sigma_y:
        extra["sigma_y"] = float(sigma_y)
    hidden = None if m_all is None else (m_all == 0).to(torch.uint8).contiguous()
    return _result(images, ref, hidden, device, DPS_METHOD, extra)


@torch.no_grad()
def _evaluate_colorize(model, images_uint8, *, batch_size, seed, scale, method, sr_mask, dpm_solver, sigma_y, weights="mean", **chain):
    """evaluate_restoration's task "colorize" (see there)"""
    x_all, ref, device = _setup(model, images_uint8, batch_size)
    n, c, h, w = x_all.shape
    if method not in (None, "ddnm") or dpm_solver:
        raise ValueError("task 'colorize' has one method, ddnm on ancestral or DDIM steps (no RePaint, no dpm_solver)")
    if isinstance(sigma_y, bool) or not isinstance(sigma_y, (int, float, np.integer, np.floating)) or not math.isfinite(sigma_y) or sigma_y < 0:
        raise ValueError(f"sigma_y must be a finite real number >= 0, got {sigma_y!r}")
    sigma_y = float(sigma_y)
    scale = int(scale)
    if scale < 1 or h % scale or w % scale:
        raise ValueError(f"scale {scale} must be >= 1 and divide the image size {h} x {w}")
    A = lambda x: pool(gray(x, weights), scale) if scale > 1 else gray(x, weights)
    y_all = A(x_all)
    y_meas = y_all + sigma_y * torch.randn(y_all.shape, generator=torch.Generator().manual_seed(seed)) if sigma_y else y_all
    K = _unet_forwards(model, chain)
    my_all, y_base = None, y_meas
    if sr_mask is not None:
        hs, ws = h // scale, w // scale
        my_all = make_mask(sr_mask, n, hs, ws) if isinstance(sr_mask, str) else torch.as_tensor(sr_mask).float().expand(n, -1, hs, ws)
        my_all = my_all.amin(dim=1, keepdim=True)
        y_base = mean_fill(y_meas, my_all)                # the baselines see the same holes
    images = {"replicate": to_u8(replicate(y_base, scale).expand(-1, 3, -1, -1))}
    if scale > 1:
        images["bicubic"] = to_u8(bicubic(y_base, scale).expand(-1, 3, -1, -1))
    mk = lambda i: None if my_all is None else my_all[i:i + batch_size, 0].to(device)
    x_out, images = _restore_all(n, batch_size, seed, lambda i: model.colorize(y_meas[i:i + batch_size].to(device), mk(i), scale, weights=weights,
                                                                               sigma_y=sigma_y, **chain), images)
    meas = torch.ones_like(y_all) if my_all is None else my_all
    extra = dict(unet_forwards=K, weights=weights)
    if sigma_y:
        rms = lambda x: (((A(x) - y_all) ** 2 * meas).sum(dim=(1, 2, 3)) / meas.sum(dim=(1, 2, 3)).clamp(min=1)).sqrt() * 127.5
        extra.update(consistency=rms(x_out).double().numpy(), consistency_u8=rms(from_u8(images["restored"])).double().numpy(), sigma_y=sigma_y)
    else:
        dev = lambda x: (((A(x) - y_all) * meas).abs().amax(dim=(1, 2, 3)) * 127.5).double().numpy()
        extra.update(consistency=dev(x_out), consistency_u8=dev(from_u8(images["restored"])))
    return _result(images, ref, None, device, "ddnm_gray", extra)


@torch.no_grad()
def _evaluate_deblur(model, images_uint8, *, batch_size, seed, kernel, tol=3e-2, **chain):
    """evaluate_restoration's task "deblur" (see there)"""
    from models.diffusion import blur
    x_all, ref, device = _setup(model, images_uint8, batch_size)
    n, c, h, w = x_all.shape
    A_h, A_w, Q_h, Q_w = blur.blur_operands(kernel, h, w, tol)[:4]
    sep = lambda x, L, R: torch.einsum("ih,bchw,jw->bcij", L, x, R)
    y_all = sep(x_all, A_h, A_w)
    images = {"blurred": to_u8(y_all), "pinv": to_u8(sep(y_all, Q_h, Q_w).clamp(-1, 1))}
    x_out, images = _restore_all(n, batch_size, seed, lambda i: model.deblur(y_all[i:i + batch_size].to(device), kernel, tol=tol, **chain), images)
    dev = lambda x: ((sep(x, A_h, A_w) - y_all).abs().amax(dim=(1, 2, 3)) * 127.5).double().numpy()
    extra = dict(unet_forwards=_unet_forwards(model, chain), kernel=kernel if isinstance(kernel, str) else "custom", tol=float(tol),
                 consistency=dev(x_out), consistency_u8=dev(from_u8(images["restored"])))
    return _result(images, ref, None, device, "ddnm_blur", extra)


@torch.no_grad()
def _evaluate_cs(model, images_uint8, *, batch_size, seed, ratio, perm_seed=0, **chain):
    """evaluate_restoration's task "cs" (see there)"""
    from ddk import ops
    from models.diffusion import hadamard
    x_all, ref, device = _setup(model, images_uint8, batch_size)
    n, c, h, w = x_all.shape
    if not hadamard.size_ok(c, h, w):
        raise ValueError(f"task 'cs' needs H and W powers of two in [16, 256] and 1 to 8 channels, got {c} x {h} x {w}")
    m = hadamard.cs_rows(ratio, h * w)
    perm = hadamard.cs_perm(h * w, perm_seed)
    pd = torch.from_numpy(perm).to(device)
    batches = lambda f, v: torch.cat([f(v[i:i + batch_size].to(device).contiguous()).cpu() for i in range(0, n, batch_size)])
    A = lambda x: batches(lambda v: ops.hadamard_measure(ops.nchw_to_nhwc(v), pd, m), x)
    y_all = A(x_all)
    images = {"adjoint": to_u8(batches(lambda v: ops.nhwc_to_nchw(ops.hadamard_adjoint(v, pd, h, w)), y_all).clamp(-1, 1))}
    x_out, images = _restore_all(n, batch_size, seed, lambda i: model.restore_cs(y_all[i:i + batch_size].to(device), perm, **chain), images)
    extra = dict(unet_forwards=_unet_forwards(model, chain), ratio=float(ratio), perm_seed=int(perm_seed), m=m,
                 consistency=(A(x_out) - y_all).abs().amax(dim=(1, 2)).double().numpy())
    return _result(images, ref, None, device, "ddnm_cs", extra)


@torch.no_grad()
def _evaluate_deconv(model, images_uint8, *, batch_size, seed, psf, tol=3e-2, sigma_y=0.0, **chain):
    """evaluate_restoration's tasks "deconv" and (sigma_y > 0) "deconv_noisy" (see there)"""
    from ddk import ops
    from models.diffusion import psf as P
    x_all, ref, device = _setup(model, images_uint8, batch_size)
    n, c, h, w = x_all.shape
    if not P.size_ok(c, h, w):
        raise ValueError(f"task 'deconv' needs H and W powers of two in [16, 256] and 1 to 8 channels, got {c} x {h} x {w}")
    name = psf if isinstance(psf, str) else "custom"
    k = P.psf_array(np.load(psf) if isinstance(psf, str) and psf.endswith(".npy") else psf)
    Kd, Pd, Md, _ = (torch.from_numpy(v).to(device) for v in P.psf_operands(k, h, w, tol))
    Md = torch.stack([Md, torch.zeros_like(Md)], dim=-1).contiguous()      # the projection A+ A as a multiplier
    batches = lambda S, v: torch.cat([ops.nhwc_to_nchw(ops.circular_conv(ops.nchw_to_nhwc(v[i:i + batch_size].to(device).contiguous()), S)).cpu()
                                      for i in range(0, n, batch_size)])
    y_clean = batches(Kd, x_all)
    y_all = y_clean + sigma_y * torch.randn(y_clean.shape, generator=torch.Generator().manual_seed(seed)) if sigma_y else y_clean
    yp_all = batches(Pd, y_all)
    images = {"blurred": to_u8(y_all.clamp(-1, 1)), "pinv": to_u8(yp_all.clamp(-1, 1))}
    if sigma_y:
        Kc = P.psf_spectrum(k, h, w)
        Wd = torch.from_numpy(P.interleave(np.conj(Kc) / (np.abs(Kc) ** 2 + sigma_y ** 2))).to(device)
        images["tikhonov"] = to_u8(batches(Wd, y_all).clamp(-1, 1))
    restore = (lambda y: model.deconvolve_noisy(y, k, sigma_y=sigma_y, tol=tol, **chain)) if sigma_y else (lambda y: model.deconvolve(y, k, tol=tol, **chain))
    x_out, images = _restore_all(n, batch_size, seed, lambda i: restore(y_all[i:i + batch_size].to(device)), images)
    extra = dict(unet_forwards=_unet_forwards(model, chain), psf=name, tol=float(tol))
    if sigma_y:
        rms = lambda x: ((batches(Kd, x) - y_clean) ** 2).mean(dim=(1, 2, 3)).sqrt() * 127.5
        extra.update(sigma_y=float(sigma_y), consistency=rms(x_out).double().numpy(), consistency_u8=rms(from_u8(images["restored"])).double().numpy())
    else:
        extra.update(consistency=(batches(Md, x_out) - yp_all).abs().amax(dim=(1, 2, 3)).double().numpy())
    return _result(images, ref, None, device, "ddnm_plus" if sigma_y else "ddnm_deconv", extra)


def report(result):
    """evaluate_restoration's per-image arrays as {"mean", "stderr", "n"} entries, JSON-ready."""
    out = {name: {k: summarise(v) for k, v in m.items()} for name, m in result["methods"].items()}
    for k in ("consistency", "consistency_u8"):
        if k in result:
            out[k] = dict(summarise(result[k]), max=float(np.max(result[k])))
    return out
