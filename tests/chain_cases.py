"""What the sampler-chain GPU tests share, each written once: the tiny model, masks and measurements, the hand-made row tables, the
device's Philox draws, the use_graph / native_sampler toggles, the SamplerArgs struct with its timestep map and workspace, the
"chains share a workspace" driver and the command-line set-up.  Plain functions and context managers; a test module keeps its own
constants, bars, operands, fixtures, assertions and prints, and a thin module-scoped fixture where it wants one of these cached."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

import restore_ref as RR
from ddk import lib as L
from helpers import dddpm_cfg, ddpm_cfg, det_load, to_nchw
from oracle import philox_ref as PR
from oracle import unet_ref as U
from utils import synthetic as syn

DEV = "cuda"
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "downsampled-diffusion_amd")
BASE_TABLES = (("c_recip", 3.0), ("c_recipm1", 2.0), ("c1", 1.0), ("c2", 1.0), ("sigma", 0.5))


# ---------------------------------------------------------------- the model, masks, measurements
def tiny_ddpm(cfg, channels=3):
    """(a DDPM with deterministic weights on the device in eval mode, its eps model restated by oracle/unet_ref on the CPU)"""
    from models import DDPM, Unet
    m = det_load(DDPM(cfg, Unet(cfg), DEV, channels)).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    return m, (lambda x, t: U.unet_forward(sd, cfg, x, t, pre="latent_model."))


def mask(kind, b, h, w):
    """[b, h, w] {0, 1}: a checkerboard, a single measured block / pixel, a single hidden one (at another place per image)"""
    i, j = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if kind == "checker":
        return torch.stack([((i + j + k) % 2).float() for k in range(b)])
    m = torch.zeros(b, h, w) if kind == "one_measured" else torch.ones(b, h, w)
    for k in range(b):
        m[k, (k * 3 + 1) % h, (k * 5 + w - 1) % w] = 1.0 - m[k, 0, 0]
    return m


def pooled_y(shape, n, name):
    """the n x n block means of a clamped synthetic image"""
    return RR.pool(syn.synthetic_normal(shape, name).clamp(-1, 1), n).contiguous()


def sel(mk, y):
    """the mask [b, h, w] as a boolean selection of y [b, c, h, w]"""
    return (mk != 0).unsqueeze(1).expand_as(y)


def argmax(x):
    return x.reshape(x.shape[0], -1).argmax(dim=1)


# ---------------------------------------------------------------- the lone ops' inputs
def hand_tables(g, noisy=False):
    """8 rows, made by hand, drawn from g in this order: c_recip, c_recipm1, c1, c2, sigma, with row 0 of c1, c2 set to 1, 0; with
    noisy, then lam (strictly between 0 and 1 in rows 1, 2, 5, 6, 7, exactly 1 in rows 3 and 4, 0 in row 0) and sgm (!= sigma
    everywhere, 0 in row 0).  tests/test_chain_cases_cpu.py pins the bits."""
    tab = {k: torch.rand(8, generator=g) * s for k, s in BASE_TABLES}
    tab["c1"][0], tab["c2"][0] = 1.0, 0.0
    if noisy:
        tab["lam"] = 0.1 + 0.8 * torch.rand(8, generator=g)
        tab["lam"][3] = tab["lam"][4] = 1.0
        tab["lam"][0] = 0.0
        tab["sgm"] = tab["sigma"] * (0.1 + 0.8 * torch.rand(8, generator=g))
        tab["sgm"][0] = 0.0
        assert ((tab["lam"][[1, 2, 5, 6, 7]] > 0) & (tab["lam"][[1, 2, 5, 6, 7]] < 1)).all() and (tab["sgm"][1:] != tab["sigma"][1:]).all()
    return tab


def philox_draws(B, c, h, w, t, seed, stream):
    """the device's own draws (ddk_randn: the ops' Philox call and keying), image b at row t[b], checked against oracle/philox_ref;
    NCHW on the CPU"""
    from ddk import ops
    z_dev = torch.stack([ops.randn((B, h, w, c), DEV, seed, int(tb), stream)[b] for b, tb in enumerate(t)]).cpu()
    z_ref = torch.from_numpy(np.stack([PR.philox_normal(B * h * w * c, seed, int(tb), stream).reshape(B, h, w, c)[b]
                                       for b, tb in enumerate(t)]))
    assert float((z_dev - z_ref).abs().max()) < 1e-5
    return to_nchw(z_dev)


@contextlib.contextmanager
def toggled(model, attr, value):
    """model.attr = value inside the block (use_graph = False: eager launches; native_sampler = False: the Python loop)"""
    old = getattr(model, attr)
    setattr(model, attr, value)
    try:
        yield
    finally:
        setattr(model, attr, old)


# ---------------------------------------------------------------- the C chain entries
def timestep_map(use):
    return (C.c_int64 * len(use))(*[int(v) for v in use])


def fresh_workspace(nbytes):
    return torch.empty(nbytes // 4 + 4, device=DEV)


@contextlib.contextmanager
def workspace(plan, nbytes):
    """a fresh workspace, released on the way out: the plan's cached graphs and shift table point into it, so they are dropped before
    the memory goes back"""
    ws = fresh_workspace(nbytes)
    try:
        yield ws
    finally:
        assert plan._lib.ddk_sampler_release_workspace(plan.handle, L.ptr(ws)) == 0


def sampler_args(plan, x, tables, t_start, ws, nbytes, *, seed, stream_id=0, graph=0, noise=None, shape=None):
    """ddk_sampler_args for a chain on the NHWC state x from t_start down to 0; shape overrides x's (B, H, W)"""
    b, h, w = shape or x.shape[:3]
    return L.SamplerArgs(plan.handle, L.ptr(plan.packed), L.ptr(x), L.ptr(noise), L.ptr(tables["c_recip"]), L.ptr(tables["c_recipm1"]),
                         L.ptr(tables["c1"]), L.ptr(tables["c2"]), L.ptr(tables.get("sigma")), b, h, w, t_start, 0, seed, stream_id, graph,
                         L.ptr(ws), nbytes)


class SharedWorkspace:
    """Chains of several kinds on one plan, state buffer, timestep map and t_start, launched on a side stream.
    launch(what, args_ref, tmap, stream_ptr) -> rc is the kind-specific part; tables is the chains' row tables, or what -> tables
    where the kinds differ in them."""

    def __init__(self, plan, tables, use, x_T_nhwc, nbytes, seed, launch):
        self.plan, self.tables, self.nbytes, self.seed, self.launch = plan, tables, nbytes, seed, launch
        self.tmap, self.t_start = timestep_map(use), len(use) - 1
        self.x0, self.x = x_T_nhwc, torch.empty_like(x_T_nhwc)
        self.side = torch.cuda.Stream()

    def run(self, ws, what, graph=1):
        self.x.copy_(self.x0)
        torch.cuda.synchronize()
        tables = self.tables(what) if callable(self.tables) else self.tables
        a = sampler_args(self.plan, self.x, tables, self.t_start, ws, self.nbytes, seed=self.seed, graph=graph)
        with torch.cuda.stream(self.side):
            rc = self.launch(what, C.byref(a), self.tmap, self.side.cuda_stream)
        assert rc == 0, L.last_error()
        self.side.synchronize()
        return self.x.clone()

    def alone(self, what):
        with workspace(self.plan, self.nbytes) as ws:
            return self.run(ws, what)

    def interleaved(self, order, single):
        """the jobs of order on one fresh workspace: each equals its own single run bit for bit"""
        with workspace(self.plan, self.nbytes) as ws:
            for what in order:
                got = self.run(ws, what)
                assert torch.equal(got, single[what]), (order, what, float((got - single[what]).abs().max()))


# ---------------------------------------------------------------- the command lines
def cli_cfg(model="ddpm"):
    """the scripts' --synthetic config: the tiny DDPM on 16 x 16 images, or the smallest dDDPM on 32 x 32, T = 100"""
    cfg = ddpm_cfg(32, 3, 16, T=100) if model == "ddpm" else dict(dddpm_cfg(32, 32, 2), T=100)
    cfg.update(model=model, dataset="celeba")
    return cfg


def cli_files(tmp_path, cfg, n_images, size, rng_seed=0):
    """cfg.json and (n_images > 0) a uint8 imgs.npy under tmp_path: (cfg_path, images_path, images, env of the child process)"""
    cfg_path = tmp_path / "cfg.json"
    cfg_path.write_text(json.dumps(cfg))
    images_path = images = None
    if n_images:
        images = (np.random.default_rng(rng_seed).random((n_images, size, size, 3)) * 255).astype(np.uint8)
        images_path = tmp_path / "imgs.npy"
        np.save(images_path, images)
    return cfg_path, images_path, images, dict(os.environ, PYTHONPATH=PKG)


def run_script(name, *argv, env, timeout=300, check=True):
    """a script of the package in a fresh process; unless check is False its exit status must be 0"""
    r = subprocess.run([sys.executable, os.path.join(PKG, name), *map(str, argv)], capture_output=True, text=True, env=env, timeout=timeout)
    if check:
        assert r.returncode == 0, r.stderr[-2000:]
    return r
