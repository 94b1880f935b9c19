#!/usr/bin/env python3
"""Respaced / DDIM sampling at the benchmark's shape: cfg4 (dDDPM-x3, unet_chan 128, 8x32x32 latents, B = 32, T = 1000), synthetic
weights, default plan options, the native graph sampler.

For each K in {50, 100, 250} a DDIM chain (respacing "ddimK", eta 0; the step is the same captured graph whatever the tables) and a
plain chain of the same K steps (t = 999 .. 1000 - K, the benchmark's own call) are timed ALTERNATELY in this process, REPS times
each, every chain from the same x_T and bracketed by device synchronisation; the per-step figure is the median.  The clock is
settled first by running plain steps for a while (measuring-on-mi355x: warm up by time).  images/s = B / (K * ms_step + t_decode),
with the x3 decode (tanh(upsample(z))) timed in the same run; T = 1000 is the plain chain's per-step time x 1000.  One JSON line on
stdout.  GPU-box tool.

--solver: the cost of a DPM-Solver++(2M) step against a DDIM (eta 0) step on the same "logsnrK" grid, K in {20, 50}, timed
alternately the same way (the two chains differ only in the step's last kernel: a history load and store instead of a draw).

--restore: the cost of a DDNM super-resolution step against an ancestral step of the same respaced "50"
chain, n = 2 and 4 (the fused tail) and, for the record, the same two with the fused tail switched off and n = 8 (always the
unfused tail), timed alternately the same way (the chains differ only in the step's last kernel).

--restore-masked: the cost of a masked DDNM step at n = 1 (inpainting, the fused tail; and with the fused
tail switched off) and n = 2 with a mask, against an ancestral step of the same respaced "50" chain, timed the same way, and the
images/s of "100"-step DDIM (eta 0) DDNM inpainting with the decode, for the comparison with RePaint's 2410 ops.

--restore-solver: the cost of a DDNM step on the DPM-Solver++(2M) chain at n = 1 with the center mask and n = 2
without a mask, against a plain 2M step on the same "logsnr20" grid, timed alternately the same way, and the end-to-end images/s of
each with the decode.

--restore-noisy: the cost of a DDNM+ step for a noisy measurement (sigma_y = 0.1) at n = 1 with the center
mask (the fused tail; and with the fused tail switched off) and n = 2 with the mask, against an ancestral step of the same respaced
"50" chain, timed alternately the same way.

--restore-gray: the cost of a colourisation step ("luma" weights, sigma_y = 0, no mask) on a 128-wide
3-channel pixel DDPM with 32 x 32 images at n = 1 (the fused tail; and with the fused tail switched off) and n = 2, against an
ancestral step of the same model's respaced "50" chain, timed alternately the same way.

--restore-blur: the cost of a DDNM deblurring step ("gauss" kernel) against an ancestral step of the same
respaced chain, timed alternately the same way, on a 128-wide 3-channel pixel DDPM with 32 x 32 images at B = 32 ("50" steps; the
one-launch form of the update) and on a 32-wide one with 256 x 256 images at B = 8 ("20" steps; the two-launch form).  Every
deblurring step ends in the unfused tail (the operator couples a whole plane), so the ratio holds the plain tail's extra launch as
well as the two matrix products.

--restore-sep: the same two models with the size-changing operator of DESIGN.md section 3.15, antialiased bicubic reduction by 4
(y 8 x 8 and 64 x 64): the cost of a step of the restore_sep chain against an ancestral step, timed alternately the same way (the step
is the deblurring step: its figure is expected), and the one-time cost of forming Yp = Q_h y Q_w^T with separable_apply_rect, the
median of five timings of 200 back-to-back calls each between two device events (two launches per call; where the
kernels are shorter than a launch takes to enqueue, the figure is the enqueue's).

--restore-cs: the cost of a DDNM compressed-sensing step (ratio 0.25, perm seed 0) against an ancestral step of
the same respaced chain on --restore-blur's two models: 3 x 32 x 32 at B = 32 (the plane form, one launch) and 3 x 256 x 256 at B = 8
(the scratch form, three launches).  The ancestral, compressed-sensing and deblurring chains alternate in one process, medians of
five each, so the deblurring step's ratio from the same run stands beside it as the natural neighbour.

--restore-fft: the cost of a DDNM deconvolution step (the disk point-spread function, tol 3e-2) against an
ancestral step of the same respaced chain on the same two models: 3 x 32 x 32 at B = 32, "50" steps (the plane form, one launch) and
3 x 256 x 256 at B = 8, "20" steps (the multi-launch form, three launches).  The ancestral, deconvolution and compressed-sensing
chains alternate in one process, medians of five each; the result is also written to profiles/restore_fft_bench.json.

--restore-fft-noisy: the cost of a DDNM+ deconvolution step (the disk point-spread function, tol 3e-2, sigma_y
0.05) against an ancestral step and against the deconvolution step of the same respaced chain, on --restore-fft's two models and
steps.  The ancestral, deconvolution and noisy deconvolution chains alternate in one process, medians of five each; the result is
also written to profiles/restore_fft_noisy_bench.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]
import torch

import bench
from ddk import ops
from models import DDPM, DownsampleDDPM, Unet
from utils import synthetic as syn

DEV = "cuda"
B, C, S, T = 32, 8, 32, 1000
KS = (50, 100, 250)
SOLVER_KS = (20, 50)
REPS = 5
NOISY_SIGMA_Y = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solver", action="store_true", help="2M step against DDIM step on logsnrK grids")
    ap.add_argument("--restore", action="store_true", help="DDNM super-resolution step against an ancestral step, respacing 50")
    ap.add_argument("--restore-masked", action="store_true", help="masked DDNM step (n = 1, 2) against an ancestral step, respacing 50")
    ap.add_argument("--restore-noisy", action="store_true", help="DDNM+ step (n = 1, 2; sigma_y 0.1) against an ancestral step, respacing 50")
    ap.add_argument("--restore-gray", action="store_true", help="colourisation step (n = 1, 2; luma) against an ancestral step, respacing 50, on a 3-channel pixel model")
    ap.add_argument("--restore-blur", action="store_true", help="deblurring step (gauss) against an ancestral step on 3x32x32 (B 32) and 3x256x256 (B 8) pixel models")
    ap.add_argument("--restore-sep", action="store_true", help="bicubic x4 restore_sep step against an ancestral step, and the cost of forming Yp, on the --restore-blur models")
    ap.add_argument("--restore-cs", action="store_true", help="compressed-sensing step (ratio 0.25) and deblurring step against an ancestral step on the --restore-blur models")
    ap.add_argument("--restore-fft", action="store_true", help="deconvolution step (disk PSF) and compressed-sensing step against an ancestral step on the --restore-blur models")
    ap.add_argument("--restore-fft-noisy", action="store_true", help="DDNM+ deconvolution step (disk PSF, sigma_y 0.05) against an ancestral and a deconvolution step on the --restore-blur models")
    ap.add_argument("--restore-solver", action="store_true", help="DDNM step on the 2M chain (n = 1 center mask, n = 2) against a 2M step, logsnr20")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.restore_gray:
        return restore_gray_ab()
    if args.restore_blur:
        return restore_blur_ab()
    if args.restore_sep:
        return restore_sep_ab()
    if args.restore_cs:
        return restore_cs_ab()
    if args.restore_fft:
        return restore_fft_ab()
    if args.restore_fft_noisy:
        return restore_fft_noisy_ab()
    cfg = bench.cfg4()
    model = DownsampleDDPM(cfg, Unet(cfg), DEV, 3)
    model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
    model = model.to(DEV).eval()
    plan = model.latent_model.plan()
    tables = model._tables()
    x0 = ops.randn((B, S, S, C), DEV, seed=1234, step=T, stream_id=0)
    x = x0.clone()

    ys = {n: torch.nn.functional.avg_pool2d(ops.nhwc_to_nchw(x0).clamp(-1, 1), n).permute(0, 2, 3, 1).contiguous() for n in (2, 4, 8)}

    ys[1] = ops.nhwc_to_nchw(x0).clamp(-1, 1).permute(0, 2, 3, 1).contiguous()
    ii, jj = torch.meshgrid(torch.arange(S, device=DEV), torch.arange(S, device=DEV), indexing="ij")
    center = ((ii < S // 4) | (ii >= S - S // 4) | (jj < S // 4) | (jj >= S - S // 4)).float()      # the CLI's "center" mask
    mks = {n: center[::n, ::n].expand(B, -1, -1).contiguous() for n in (1, 2)}

    def chain(kind, K):
        x.copy_(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "plain":
            plan.sample_nhwc(x, tables, T - 1, T - K, seed=1234, stream_id=0)
        elif kind == "ddim_logsnr":
            sp, use = model._spaced_tables(f"logsnr{K}", True, 0.0)
            plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
        elif kind == "2m":
            sp, use = model._solver_tables(f"logsnr{K}", "dpm++2m")
            plan.sample_multistep_nhwc(x, sp, K - 1, 0, stream_id=0, timesteps=use)
        elif kind == "anc":
            sp, use = model._spaced_tables(str(K), False, 0.0)
            plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
        elif kind.startswith("rsolver"):                 # DDNM on the 2M chain: n = 1 with the center mask, n >= 2 without a mask
            n = int(kind[len("rsolver"):])
            sp, use = model._solver_tables(f"logsnr{K}", "dpm++2m")
            plan.sample_restore_multistep_nhwc(x, ys[n], mks[n] if n == 1 else None, n, sp, K - 1, stream_id=0, timesteps=use)
        elif kind.startswith("noisy"):                   # DDNM+ on ancestral steps, the center mask
            n = int(kind[len("noisy"):])
            sp, use = model._noisy_tables(str(K), False, 0.0, NOISY_SIGMA_Y)
            plan.sample_restore_noisy_nhwc(x, ys[n], mks[n], n, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
        elif kind.startswith("masked"):                  # "masked<n>" ancestral, "maskedddim<n>" DDIM eta 0
            ddim = kind.startswith("maskedddim")
            n = int(kind[len("maskedddim" if ddim else "masked"):])
            sp, use = model._spaced_tables(str(K), ddim, 0.0)
            plan.sample_restore_masked_nhwc(x, ys[n], mks[n], n, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
        elif kind.startswith("restore"):
            n = int(kind[len("restore"):])
            sp, use = model._spaced_tables(str(K), False, 0.0)
            plan.sample_restore_nhwc(x, ys[n], n, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
        else:
            sp, use = model._spaced_tables(f"ddim{K}", True, 0.0)
            plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def decode():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = model.rescaled_upsample(ops.nhwc_to_nchw(x))
        torch.cuda.synchronize()
        assert torch.isfinite(img).all() and img.shape == (B, 3, 256, 256)
        return (time.perf_counter() - t0) * 1e3

    if args.solver:
        return solver_ab(chain, decode)
    if args.restore:
        return restore_ab(chain, plan)
    if args.restore_masked:
        return restore_masked_ab(chain, plan, decode)
    if args.restore_solver:
        return restore_solver_ab(chain, plan, decode)
    if args.restore_noisy:
        return restore_noisy_ab(chain, plan)

    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}, DDIM eta 0", "reps": REPS, "per_K": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:          # settle the clock on the step's own load
            chain("plain", 96)
        decode_ms = min(decode() for _ in range(3))
        plain_all = []
        for K in KS:
            chain("plain", K)
            chain("ddim", K)                                 # captures this K's graphs outside the timed calls
            plain, spaced = [], []
            for _ in range(REPS):
                plain.append(chain("plain", K) / K)
                spaced.append(chain("ddim", K) / K)
            assert torch.isfinite(x).all()
            p, s = statistics.median(plain), statistics.median(spaced)
            plain_all += plain
            res["per_K"][str(K)] = {"plain_ms_per_step": round(p, 4), "spaced_ms_per_step": round(s, 4),
                                    "spaced_over_plain": round(s / p, 4), "spaced_min_max_ms": [round(min(spaced), 4), round(max(spaced), 4)],
                                    "plain_min_max_ms": [round(min(plain), 4), round(max(plain), 4)],
                                    "images_per_sec": round(B / ((K * s + decode_ms) / 1e3), 2)}
        p_all = statistics.median(plain_all)
        res["decode_ms"] = round(decode_ms, 3)
        res["T1000_images_per_sec"] = round(B / ((T * p_all + decode_ms) / 1e3), 2)
        res["max_spaced_over_plain"] = max(v["spaced_over_plain"] for v in res["per_K"].values())
    print(json.dumps(res), flush=True)


def solver_ab(chain, decode):
    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}, logsnrK grids, DPM-Solver++(2M) vs DDIM eta 0",
           "reps": REPS, "per_K": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:
            chain("plain", 96)
        decode_ms = min(decode() for _ in range(3))
        for K in SOLVER_KS:
            chain("ddim_logsnr", K)                      # captures both chains' graphs outside the timed calls
            chain("2m", K)
            ddim, ms = [], []
            for _ in range(REPS):
                ddim.append(chain("ddim_logsnr", K) / K)
                ms.append(chain("2m", K) / K)
            d, m = statistics.median(ddim), statistics.median(ms)
            res["per_K"][str(K)] = {"ddim_ms_per_step": round(d, 4), "dpm2m_ms_per_step": round(m, 4), "dpm2m_over_ddim": round(m / d, 4),
                                    "ddim_min_max_ms": [round(min(ddim), 4), round(max(ddim), 4)],
                                    "dpm2m_min_max_ms": [round(min(ms), 4), round(max(ms), 4)],
                                    "dpm2m_images_per_sec": round(B / ((K * m + decode_ms) / 1e3), 2)}
        res["decode_ms"] = round(decode_ms, 3)
        res["max_dpm2m_over_ddim"] = max(v["dpm2m_over_ddim"] for v in res["per_K"].values())
    print(json.dumps(res), flush=True)


def restore_ab(chain, plan):
    K = 50
    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}, respacing {K}, DDNM restore step vs ancestral step",
           "reps": REPS, "per_n": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:
            chain("plain", 96)
        for n, fused in ((2, True), (4, True), (2, False), (4, False), (8, True)):
            plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, int(fused))
            tail = "fused" if plan.restore_tail_parts(B, S, S, n) > 0 else "unfused"
            chain("anc", K)                              # captures both chains' graphs outside the timed calls
            chain(f"restore{n}", K)
            anc, rst = [], []
            for _ in range(REPS):
                anc.append(chain("anc", K) / K)
                rst.append(chain(f"restore{n}", K) / K)
            a, r = statistics.median(anc), statistics.median(rst)
            res["per_n"][f"{n}_{tail}"] = {"ancestral_ms_per_step": round(a, 4), "restore_ms_per_step": round(r, 4),
                                           "restore_over_ancestral": round(r / a, 4),
                                           "ancestral_min_max_ms": [round(min(anc), 4), round(max(anc), 4)],
                                           "restore_min_max_ms": [round(min(rst), 4), round(max(rst), 4)]}
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    print(json.dumps(res), flush=True)


def restore_masked_ab(chain, plan, decode):
    K = 50
    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}, respacing {K}, masked DDNM step vs ancestral step, center mask",
           "reps": REPS, "per_n": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:
            chain("plain", 96)
        for n, fused in ((1, True), (2, True), (1, False)):
            plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, int(fused))
            tail = "fused" if plan.restore_masked_tail_parts(B, S, S, n) > 0 else "unfused"
            chain("anc", K)                              # captures both chains' graphs outside the timed calls
            chain(f"masked{n}", K)
            anc, rst = [], []
            for _ in range(REPS):
                anc.append(chain("anc", K) / K)
                rst.append(chain(f"masked{n}", K) / K)
            a, r = statistics.median(anc), statistics.median(rst)
            res["per_n"][f"{n}_{tail}"] = {"ancestral_ms_per_step": round(a, 4), "masked_ms_per_step": round(r, 4),
                                           "masked_over_ancestral": round(r / a, 4),
                                           "ancestral_min_max_ms": [round(min(anc), 4), round(max(anc), 4)],
                                           "masked_min_max_ms": [round(min(rst), 4), round(max(rst), 4)]}
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
        # "100" DDIM eta 0 DDNM inpainting, end to end with the decode: what a user runs instead of RePaint's 2410 ops
        K = 100
        chain("maskedddim1", K)
        runs = [chain("maskedddim1", K) for _ in range(REPS)]
        decode_ms = min(decode() for _ in range(3))
        ms = statistics.median(runs)
        res["ddim100_inpaint"] = {"chain_ms": round(ms, 3), "chain_min_max_ms": [round(min(runs), 3), round(max(runs), 3)],
                                  "decode_ms": round(decode_ms, 3), "unet_forwards": K,
                                  "images_per_sec": round(B / ((ms + decode_ms) / 1e3), 2)}
    print(json.dumps(res), flush=True)


def restore_noisy_ab(chain, plan):
    K = 50
    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}, respacing {K}, DDNM+ step (sigma_y {NOISY_SIGMA_Y}) vs ancestral "
                    "step, center mask", "reps": REPS, "per_n": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:
            chain("plain", 96)
        for n, fused in ((1, True), (2, True), (1, False)):
            plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, int(fused))
            tail = "fused" if plan.restore_noisy_tail_parts(B, S, S, n) > 0 else "unfused"
            chain("anc", K)                              # captures both chains' graphs outside the timed calls
            chain(f"noisy{n}", K)
            anc, rst = [], []
            for _ in range(REPS):
                anc.append(chain("anc", K) / K)
                rst.append(chain(f"noisy{n}", K) / K)
            a, r = statistics.median(anc), statistics.median(rst)
            res["per_n"][f"{n}_{tail}"] = {"ancestral_ms_per_step": round(a, 4), "noisy_ms_per_step": round(r, 4),
                                           "noisy_over_ancestral": round(r / a, 4),
                                           "ancestral_min_max_ms": [round(min(anc), 4), round(max(anc), 4)],
                                           "noisy_min_max_ms": [round(min(rst), 4), round(max(rst), 4)]}
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    print(json.dumps(res), flush=True)


def restore_gray_ab():
    """its own model: the grey operator needs three colour channels, which cfg4's 8-channel latent does not have"""
    K, weights = 50, "luma"
    cfg = dict(unet_chan=128, unet_in=3, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=S, T=T, loss_type="simple",
               beta_schedule="linear", loss_flat="sum")
    model = DDPM(cfg, Unet(cfg), DEV, 3)
    model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
    model = model.to(DEV).eval()
    plan = model.latent_model.plan()
    x0 = ops.randn((B, S, S, 3), DEV, seed=1234, step=T, stream_id=0)
    x = x0.clone()
    w = torch.tensor([0.299, 0.587, 0.114], device=DEV)
    g = (x0.clamp(-1, 1) * w).sum(dim=3)                                                    # [B, S, S]
    ys = {1: g.contiguous(), 2: torch.nn.functional.avg_pool2d(g.unsqueeze(1), 2)[:, 0].contiguous()}

    def chain(kind):
        x.copy_(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "anc":
            sp, use = model._spaced_tables(str(K), False, 0.0)
            plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
        else:
            n = int(kind[len("gray"):])
            sp, use = model._gray_tables(str(K), False, 0.0, 0.0)
            plan.sample_restore_gray_nhwc(x, ys[n], None, n, weights, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {"shape": f"DDPM unet_chan 128, 3x{S}x{S} images, B={B}, T={T}, respacing {K}, colourisation step ({weights}, sigma_y 0, no mask) vs "
                    "ancestral step", "reps": REPS, "per_n": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:
            chain("anc")
        for n, fused in ((1, True), (2, True), (1, False)):
            plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, int(fused))
            tail = "fused" if plan.restore_gray_tail_parts(B, S, S, n) > 0 else "unfused"
            chain("anc")                                 # captures both chains' graphs outside the timed calls
            chain(f"gray{n}")
            anc, rst = [], []
            for _ in range(REPS):
                anc.append(chain("anc") / K)
                rst.append(chain(f"gray{n}") / K)
            a, r = statistics.median(anc), statistics.median(rst)
            res["per_n"][f"{n}_{tail}"] = {"ancestral_ms_per_step": round(a, 4), "gray_ms_per_step": round(r, 4),
                                           "gray_over_ancestral": round(r / a, 4),
                                           "ancestral_min_max_ms": [round(min(anc), 4), round(max(anc), 4)],
                                           "gray_min_max_ms": [round(min(rst), 4), round(max(rst), 4)]}
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    assert torch.isfinite(x).all()
    print(json.dumps(res), flush=True)


def restore_blur_ab():
    """its own models: the blur is an operator on pixels, which cfg4's latent is not"""
    from models.diffusion import blur
    res = {"shape": f"pixel DDPMs, T={T}, deblurring step (gauss kernel, tol 3e-2) vs ancestral step of the same respaced chain", "reps": REPS,
           "per_case": {}}
    for name, chan, size, b, K in (("3x32x32_B32_chan128_one_launch", 128, 32, 32, 50), ("3x256x256_B8_chan32_two_launches", 32, 256, 8, 20)):
        cfg = dict(unet_chan=chan, unet_in=3, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=size, T=T, loss_type="simple",
                   beta_schedule="linear", loss_flat="sum")
        model = DDPM(cfg, Unet(cfg), DEV, 3)
        model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
        model = model.to(DEV).eval()
        plan = model.latent_model.plan()
        x0 = ops.randn((b, size, size, 3), DEV, seed=1234, step=T, stream_id=0)
        x = x0.clone()
        m = {k: v.to(DEV) for k, v in zip(("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w"), blur.blur_operands("gauss", size, size))}
        y = ops.separable_apply(x0.clamp(-1, 1), m["A_h"], m["A_w"])
        sp, use = model._spaced_tables(str(K), False, 0.0)

        def chain(kind):
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "anc":
                plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
            else:
                plan.sample_restore_blur_nhwc(x, y, m["P_h"], m["P_w"], m["Q_h"], m["Q_w"], sp, K - 1, seed=1234, stream_id=0, timesteps=use)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        with torch.no_grad():
            t_settle = time.perf_counter()
            while time.perf_counter() - t_settle < 2.0:
                chain("anc")
            chain("blur")                                # both chains' graphs are captured outside the timed calls
            anc, rst = [], []
            for _ in range(REPS):
                anc.append(chain("anc") / K)
                rst.append(chain("blur") / K)
        assert torch.isfinite(x).all() and plan.restore_blur_tail_parts(b, size, size) == 0
        a, r = statistics.median(anc), statistics.median(rst)
        res["per_case"][name] = {"ancestral_ms_per_step": round(a, 4), "blur_ms_per_step": round(r, 4), "blur_over_ancestral": round(r / a, 4),
                                 "ancestral_min_max_ms": [round(min(anc), 4), round(max(anc), 4)],
                                 "blur_min_max_ms": [round(min(rst), 4), round(max(rst), 4)], "steps": K}
        del model, plan
    print(json.dumps(res), flush=True)


def restore_cs_ab():
    """restore_blur_ab's models: the ancestral, compressed-sensing and deblurring chains alternating"""
    from models.diffusion import blur, hadamard
    ratio = 0.25
    res = {"shape": f"pixel DDPMs, T={T}, compressed-sensing step (ratio {ratio}, perm seed 0) and deblurring step (gauss kernel, tol 3e-2) vs "
                    "ancestral step of the same respaced chain", "reps": REPS, "per_case": {}}
    for name, chan, size, b, K in (("3x32x32_B32_chan128_plane_form", 128, 32, 32, 50), ("3x256x256_B8_chan32_scratch_form", 32, 256, 8, 20)):
        cfg = dict(unet_chan=chan, unet_in=3, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=size, T=T, loss_type="simple",
                   beta_schedule="linear", loss_flat="sum")
        model = DDPM(cfg, Unet(cfg), DEV, 3)
        model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
        model = model.to(DEV).eval()
        plan = model.latent_model.plan()
        x0 = ops.randn((b, size, size, 3), DEV, seed=1234, step=T, stream_id=0)
        x = x0.clone()
        mats = {k: v.to(DEV) for k, v in zip(("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w"), blur.blur_operands("gauss", size, size))}
        y_blur = ops.separable_apply(x0.clamp(-1, 1), mats["A_h"], mats["A_w"])
        perm = torch.from_numpy(hadamard.cs_perm(size * size, 0)).to(DEV)
        m = hadamard.cs_rows(ratio, size * size)
        y_cs = ops.hadamard_measure(x0.clamp(-1, 1), perm, m)
        sp, use = model._spaced_tables(str(K), False, 0.0)

        def chain(kind):
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "anc":
                plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
            elif kind == "cs":
                plan.sample_restore_cs_nhwc(x, y_cs, perm, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
            else:
                plan.sample_restore_blur_nhwc(x, y_blur, mats["P_h"], mats["P_w"], mats["Q_h"], mats["Q_w"], sp, K - 1, seed=1234, stream_id=0,
                                              timesteps=use)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        with torch.no_grad():
            t_settle = time.perf_counter()
            while time.perf_counter() - t_settle < 2.0:
                chain("anc")
            chain("cs")                                  # every chain's graphs are captured outside the timed calls
            chain("blur")
            times = {"anc": [], "cs": [], "blur": []}
            for _ in range(REPS):
                for kind in times:
                    times[kind].append(chain(kind) / K)
        assert torch.isfinite(x).all() and plan.restore_cs_tail_parts(b, size, size) == 0
        a, c, r = (statistics.median(times[k]) for k in ("anc", "cs", "blur"))
        res["per_case"][name] = {"ancestral_ms_per_step": round(a, 4), "cs_ms_per_step": round(c, 4), "blur_ms_per_step": round(r, 4),
                                 "cs_over_ancestral": round(c / a, 4), "blur_over_ancestral": round(r / a, 4), "m": m, "steps": K,
                                 **{f"{k}_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}
        del model, plan
    print(json.dumps(res), flush=True)


def restore_fft_ab():
    """restore_blur_ab's models: the ancestral, deconvolution and compressed-sensing chains alternating"""
    from models.diffusion import hadamard, psf
    ratio, name_psf, tol = 0.25, "disk", 3e-2
    res = {"shape": f"pixel DDPMs, T={T}, deconvolution step ({name_psf} point-spread function, tol {tol}) and compressed-sensing step (ratio {ratio}, "
                    "perm seed 0) vs ancestral step of the same respaced chain", "reps": REPS, "per_case": {}}
    for name, chan, size, b, K in (("3x32x32_B32_chan128_plane_form", 128, 32, 32, 50), ("3x256x256_B8_chan32_multi_launch_form", 32, 256, 8, 20)):
        cfg = dict(unet_chan=chan, unet_in=3, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=size, T=T, loss_type="simple",
                   beta_schedule="linear", loss_flat="sum")
        model = DDPM(cfg, Unet(cfg), DEV, 3)
        model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
        model = model.to(DEV).eval()
        plan = model.latent_model.plan()
        x0 = ops.randn((b, size, size, 3), DEV, seed=1234, step=T, stream_id=0)
        x = x0.clone()
        Kd, Pd, Md, _ = (torch.from_numpy(v).to(DEV) for v in psf.psf_operands(name_psf, size, size, tol))
        y_fft = ops.circular_conv(x0.clamp(-1, 1), Kd)
        perm = torch.from_numpy(hadamard.cs_perm(size * size, 0)).to(DEV)
        m = hadamard.cs_rows(ratio, size * size)
        y_cs = ops.hadamard_measure(x0.clamp(-1, 1), perm, m)
        sp, use = model._spaced_tables(str(K), False, 0.0)

        def chain(kind):
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "anc":
                plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
            elif kind == "fft":
                plan.sample_restore_fft_nhwc(x, y_fft, Md, Pd, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
            else:
                plan.sample_restore_cs_nhwc(x, y_cs, perm, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        with torch.no_grad():
            t_settle = time.perf_counter()
            while time.perf_counter() - t_settle < 2.0:
                chain("anc")
            chain("fft")                                 # every chain's graphs are captured outside the timed calls
            chain("cs")
            times = {"anc": [], "fft": [], "cs": []}
            for _ in range(REPS):
                for kind in times:
                    times[kind].append(chain(kind) / K)
        assert torch.isfinite(x).all() and plan.restore_fft_tail_parts(b, size, size) == 0
        a, f, c = (statistics.median(times[k]) for k in ("anc", "fft", "cs"))
        res["per_case"][name] = {"ancestral_ms_per_step": round(a, 4), "fft_ms_per_step": round(f, 4), "cs_ms_per_step": round(c, 4),
                                 "fft_over_ancestral": round(f / a, 4), "cs_over_ancestral": round(c / a, 4), "kept": int(Md.sum().item()),
                                 "steps": K, **{f"{k}_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}
        del model, plan
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "restore_fft_bench.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


def restore_fft_noisy_ab():
    """restore_fft_ab's models and steps: the ancestral, deconvolution and noisy deconvolution chains alternating"""
    from models.diffusion import psf
    name_psf, tol, sigma_y = "disk", 3e-2, 0.05
    res = {"shape": f"pixel DDPMs, T={T}, DDNM+ deconvolution step ({name_psf} point-spread function, tol {tol}, sigma_y {sigma_y}) vs deconvolution "
                    "step and ancestral step of the same respaced chain", "reps": REPS, "per_case": {}}
    for name, chan, size, b, K in (("3x32x32_B32_chan128_plane_form", 128, 32, 32, 50), ("3x256x256_B8_chan32_multi_launch_form", 32, 256, 8, 20)):
        cfg = dict(unet_chan=chan, unet_in=3, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=size, T=T, loss_type="simple",
                   beta_schedule="linear", loss_flat="sum")
        model = DDPM(cfg, Unet(cfg), DEV, 3)
        model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
        model = model.to(DEV).eval()
        plan = model.latent_model.plan()
        x0 = ops.randn((b, size, size, 3), DEV, seed=1234, step=T, stream_id=0)
        x = x0.clone()
        Kd, Pd, Md, _ = (torch.from_numpy(v).to(DEV) for v in psf.psf_operands(name_psf, size, size, tol))
        sp, use = model._spaced_tables(str(K), False, 0.0)
        gd, nd = (torch.from_numpy(v).to(DEV) for v in psf.psf_noisy_operands(name_psf, size, size, tol, sigma_y, sp["c1"]))
        y_fft = ops.circular_conv(x0.clamp(-1, 1), Kd)
        y_noisy = y_fft + sigma_y * ops.randn(tuple(x0.shape), DEV, seed=99, step=1, stream_id=0)

        def chain(kind):
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "anc":
                plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
            elif kind == "fft":
                plan.sample_restore_fft_nhwc(x, y_fft, Md, Pd, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
            else:
                plan.sample_restore_fft_noisy_nhwc(x, y_noisy, Md, Pd, gd, nd, sp, K - 1, seed=1234, stream_id=0, timesteps=use)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        with torch.no_grad():
            t_settle = time.perf_counter()
            while time.perf_counter() - t_settle < 2.0:
                chain("anc")
            chain("fft")                                 # every chain's graphs are captured outside the timed calls
            chain("noisy")
            times = {"anc": [], "fft": [], "noisy": []}
            for _ in range(REPS):
                for kind in times:
                    times[kind].append(chain(kind) / K)
        assert torch.isfinite(x).all() and plan.restore_fft_noisy_tail_parts(b, size, size) == 0
        a, f, n = (statistics.median(times[k]) for k in ("anc", "fft", "noisy"))
        res["per_case"][name] = {"ancestral_ms_per_step": round(a, 4), "fft_ms_per_step": round(f, 4), "noisy_ms_per_step": round(n, 4),
                                 "noisy_over_ancestral": round(n / a, 4), "noisy_over_fft": round(n / f, 4), "fft_over_ancestral": round(f / a, 4),
                                 "kept": int(Md.sum().item()), "steps": K,
                                 **{f"{k}_min_max_ms": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}
        del model, plan
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "restore_fft_noisy_bench.json")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


def restore_sep_ab():
    """restore_blur_ab's models and chains with the bicubic x4 operator, and the cost of forming Yp from the small y"""
    from models.diffusion import blur
    scale = 4
    res = {"shape": f"pixel DDPMs, T={T}, restore_sep step (antialiased bicubic x{scale}, tol 3e-2) vs ancestral step of the same respaced chain; "
                    "form_yp: separable_apply_rect(y, Q_h, Q_w), per call", "reps": REPS, "per_case": {}}
    for name, chan, size, b, K in (("3x32x32_B32_chan128_from_8x8", 128, 32, 32, 50), ("3x256x256_B8_chan32_from_64x64", 32, 256, 8, 20)):
        cfg = dict(unet_chan=chan, unet_in=3, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=size, T=T, loss_type="simple",
                   beta_schedule="linear", loss_flat="sum")
        model = DDPM(cfg, Unet(cfg), DEV, 3)
        model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
        model = model.to(DEV).eval()
        plan = model.latent_model.plan()
        x0 = ops.randn((b, size, size, 3), DEV, seed=1234, step=T, stream_id=0)
        x = x0.clone()
        A = blur.resize_matrix(size, scale)
        m = {k: v.to(DEV) for k, v in zip(("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w"), blur.separable_operands(A, A)[:6])}
        y = ops.separable_apply_rect(x0.clamp(-1, 1), m["A_h"], m["A_w"])
        sp, use = model._spaced_tables(str(K), False, 0.0)

        def chain(kind):
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "anc":
                plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
            else:
                plan.sample_restore_sep_nhwc(x, y, m["P_h"], m["P_w"], m["Q_h"], m["Q_w"], sp, K - 1, seed=1234, stream_id=0, timesteps=use)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def form_yp(calls=200):
            out = torch.empty_like(x0)
            ops.separable_apply_rect(y, m["Q_h"], m["Q_w"], out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                ops.separable_apply_rect(y, m["Q_h"], m["Q_w"], out=out)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls

        with torch.no_grad():
            t_settle = time.perf_counter()
            while time.perf_counter() - t_settle < 2.0:
                chain("anc")
            chain("sep")                                 # both chains' graphs are captured outside the timed calls
            anc, rst = [], []
            for _ in range(REPS):
                anc.append(chain("anc") / K)
                rst.append(chain("sep") / K)
            yp = [form_yp() for _ in range(REPS)]
        assert torch.isfinite(x).all() and plan.restore_blur_tail_parts(b, size, size) == 0
        a, r = statistics.median(anc), statistics.median(rst)
        res["per_case"][name] = {"ancestral_ms_per_step": round(a, 4), "sep_ms_per_step": round(r, 4), "sep_over_ancestral": round(r / a, 4),
                                 "ancestral_min_max_ms": [round(min(anc), 4), round(max(anc), 4)],
                                 "sep_min_max_ms": [round(min(rst), 4), round(max(rst), 4)], "steps": K,
                                 "form_yp_ms": round(statistics.median(yp), 4), "form_yp_min_max_ms": [round(min(yp), 4), round(max(yp), 4)],
                                 "form_yp_over_step": round(statistics.median(yp) / r, 4)}
        del model, plan
    print(json.dumps(res), flush=True)


def restore_solver_ab(chain, plan, decode):
    K = 20
    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}, logsnr{K}, DDNM on DPM-Solver++(2M) step vs plain 2M step; "
                    "n = 1: center mask, n = 2: no mask", "reps": REPS, "per_n": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:
            chain("plain", 96)
        decode_ms = min(decode() for _ in range(3))
        for n in (1, 2):
            tail = "fused" if plan.restore_multistep_tail_parts(B, S, S, n) > 0 else "unfused"
            chain("2m", K)                               # captures both chains' graphs outside the timed calls
            chain(f"rsolver{n}", K)
            ms, rs = [], []
            for _ in range(REPS):
                ms.append(chain("2m", K) / K)
                rs.append(chain(f"rsolver{n}", K) / K)
            m, r = statistics.median(ms), statistics.median(rs)
            res["per_n"][f"{n}_{tail}"] = {"dpm2m_ms_per_step": round(m, 4), "restore_solver_ms_per_step": round(r, 4),
                                           "restore_solver_over_dpm2m": round(r / m, 4),
                                           "dpm2m_min_max_ms": [round(min(ms), 4), round(max(ms), 4)],
                                           "restore_solver_min_max_ms": [round(min(rs), 4), round(max(rs), 4)],
                                           "unet_forwards": K, "images_per_sec": round(B / ((K * r + decode_ms) / 1e3), 2),
                                           "dpm2m_images_per_sec": round(B / ((K * m + decode_ms) / 1e3), 2)}
        res["decode_ms"] = round(decode_ms, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
