"""The dDDPM in the 'deterministic' and 'convolutional' resampler modes on the device: the reference's own outputs, the losses and
every gradient against a float64 composition of oracle/ and tests/resample_ref.py, the trainer (device graph, EMA, checkpoint),
sampling, restoration and the sample-generation CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resample_ref as RR
from helpers import dddpm_cfg, det_load, golden, rel_err
from oracle import diffusion_ref as D
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
CASES = [("deterministic", 3, 2), ("deterministic", 3, 3), ("convolutional", 3, 2), ("convolutional", 3, 3), ("convolutional", 8, 2),
         ("convolutional", 8, 3)]


def _cfg(d_mode, u_mode, unet_in, n_down, size=32, chan=32, T=1000, **extra):
    cfg = dddpm_cfg(chan, size, n_down, T)
    cfg.update(d_mode=d_mode, u_mode=u_mode, unet_in=unet_in, **extra)
    return cfg


def _model(cfg, ae=False):
    from models import DownsampleDDPM, DownsampleDDPMAutoencoder, Unet
    return det_load((DownsampleDDPMAutoencoder if ae else DownsampleDDPM)(cfg, Unet(cfg), DEV, 3)).to(DEV)


# ---------------------------------------------------------------- the reference's own outputs
@pytest.mark.parametrize("mode,unet_in,n_down", CASES)
def test_rescaled_resamplers_match_the_reference(mode, unet_in, n_down):
    g = golden("g11_resampler_modes")
    tag = f"{mode}_u{unet_in}_n{n_down}"
    m = _model(_cfg(mode, mode, unet_in, n_down)).eval()
    x = syn.synthetic_input((2, 3, 32, 32), f"g11.x{n_down}").to(DEV)
    with torch.no_grad():
        z = m.rescaled_downsample(x)
        x_hat = m.rescaled_upsample(torch.from_numpy(g[f"{tag}_z"]).to(DEV))
        raw = m.downsample(x)
    assert rel_err(raw.cpu(), g[f"{tag}_raw"]) < 2e-5
    assert rel_err(z.cpu(), g[f"{tag}_z"]) < 2e-5
    assert rel_err(x_hat.cpu(), g[f"{tag}_x"]) < 2e-5


# ---------------------------------------------------------------- losses and gradients
T_LOSS = torch.tensor([0, 10, 30, 49])            # both sides of t_rec_max = 25


def _wgrad_bound(name, x, dy):
    """(N + 8) 2^-24 sum |dy| |x| for the weight and the bias gradient of one conv layer, N = B Hout Wout, from the float64 layer
    input x and upstream gradient dy (tests/test_resampler_ops_gpu.py derives the bound)"""
    fn = RR.conv_down if name.startswith("downsample") else RR.conv_up
    cin, cout = x.shape[1], dy.shape[1]
    shape = (cout, cin, 3, 3) if name.startswith("downsample") else (cin, cout, 4, 4)
    w = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad(fn(x.detach().abs(), w, b), (w, b), dy.abs())
    n = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return (n + 8) * U * gw, (n + 8) * U * gb


@pytest.mark.parametrize("mode,ae", [("deterministic", False), ("convolutional", False), ("convolutional", True), ("deterministic", True)])
def test_losses_and_every_gradient_against_float64(mode, ae):
    """losses(x, t) and the gradient of every parameter, the draw re-made from the same seed, against the float64 composition.

    Measured on an MI355X: see the figures this test prints (pytest -s) and DESIGN.md section 3.12."""
    unet_in = 3 if mode == "deterministic" else 8
    cfg = _cfg(mode, mode, unet_in, 1, size=16, T=50, t_rec_max=25)
    model = _model(cfg, ae).train()
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    x = syn.synthetic_input((4, 3, 16, 16), "rm.loss.x")
    tt = T_LOSS.to(DEV)
    torch.manual_seed(11)
    obj, extra = model.losses(x.to(DEV), tt)
    obj.backward()
    torch.manual_seed(11)
    eps = torch.randn((4, unet_in, 8, 8), device=DEV).cpu().double()           # the draw losses() made: torch.randn_like(z), first use of the generator

    names = [k for k, _ in model.named_parameters()]
    leaves = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    buf = {k: v.double() for k, v in D.schedule_buffers("linear", 50).items()}
    tape = []
    obj_r, extra_r = RR.losses(leaves, buf, cfg, x.double(), T_LOSS, eps, ae, tape)
    obj_r.backward()
    print(f"\n{mode} ae={ae}: obj {float(obj):.7g} / {float(obj_r.detach()):.7g}  latent {float(extra['latent']):.7g} / {float(extra_r['latent'].detach()):.7g}"
          f"  recon {float(extra['recon']):.7g} / {float(extra_r['recon'].detach()):.7g}")
    assert abs(float(obj) / float(obj_r.detach()) - 1) < 1e-4
    assert abs(float(extra["latent"]) / float(extra_r["latent"].detach()) - 1) < 1e-4 and abs(float(extra["recon"]) / float(extra_r["recon"].detach()) - 1) < 1e-4

    params = dict(model.named_parameters())
    worst_unet, failures = 0.0, []
    for k in names:
        got, want = params[k].grad, leaves[k].grad
        if k.startswith("latent_model."):
            assert got is not None and want is not None, k
            worst_unet = max(worst_unet, rel_err(got.cpu(), want))
    layers = {name: (xin, y.grad) for name, xin, y in tape}
    assert set(layers) == {k.rsplit(".", 1)[0] for k in names if not k.startswith("latent_model.")}
    for name, (xin, dy) in layers.items():
        bw, bb = _wgrad_bound(name, xin, dy)
        for k, bound in ((name + ".weight", bw), (name + ".bias", bb)):
            err = (params[k].grad.cpu().double() - leaves[k].grad).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            print(f"  {k}: max |err| {float(err.max()):.3g}, largest err / bound {ratio:.3g}, rel_err {rel_err(params[k].grad.cpu(), leaves[k].grad):.3g}")
            if ratio > 1.0:
                failures.append((k, ratio))
    print(f"  UNet parameters: worst rel_err {worst_unet:.3g}")
    assert worst_unet < 1e-3                          # the bar of the G6 gradient test (tests/test_backward_gpu.py)
    assert not failures, failures


# ---------------------------------------------------------------- the trainer
def _graph_vs_eager(cfg, ae, xshape, eshape):
    from trainers.graph_step import GraphedAccumulation
    from trainers.optim import FusedAdam
    tt = torch.tensor([0, 11, 30, 49], device=DEV)
    orig = torch.randn_like
    results, moved = {}, None
    try:
        for how in ("eager", "graph"):
            model = _model(cfg, ae).train()
            eps = syn.synthetic_normal(eshape, "rm.graph.eps").to(DEV)
            model.t_sample = lambda n, tt=tt: tt
            torch.randn_like = lambda z, eps=eps: eps
            opt = FusedAdam(model, lr=2e-4, max_grad_norm=1.0)
            before = {k: v.detach().clone() for k, v in model.named_parameters() if not k.startswith("latent_model.")}
            batches = [syn.synthetic_input(xshape, f"rm.graph.x{mb}").to(DEV) for mb in range(2)]
            ga = GraphedAccumulation(model, 2)
            if how == "graph":
                ga.capture(batches)
                opt.zero_grad()
            out = []
            for step in range(2):
                if how == "graph":
                    rows = ga.replay(batches).clone()
                else:
                    ga.static_x = batches
                    rows = ga._run()
                out.append((rows.cpu(), opt.fp.grad.clone().cpu()))
                opt.step()
                opt.zero_grad()
                for m in model.modules():
                    if hasattr(m, "invalidate_plan"):
                        m.invalidate_plan()
            results[how] = out
            after = dict(model.named_parameters())
            moved = {k: not torch.equal(v, after[k].detach()) for k, v in before.items()}
    finally:
        torch.randn_like = orig
    for step in range(2):
        assert torch.equal(results["eager"][step][0], results["graph"][step][0]), step
        assert torch.equal(results["eager"][step][1], results["graph"][step][1]), step
    assert not torch.equal(results["graph"][0][1], results["graph"][1][1])
    return moved


@pytest.mark.parametrize("d_mode,u_mode,unet_in", [("convolutional", "convolutional", 8), ("deterministic", "convolutional_res", 3)])
def test_graph_replayed_step_equals_the_eager_one(d_mode, u_mode, unet_in):
    cfg = _cfg(d_mode, u_mode, unet_in, 1, size=16, T=50, t_rec_max=25)
    moved = _graph_vs_eager(cfg, True, (4, 3, 16, 16), (4, unet_in, 8, 8))
    assert moved and all(moved.values()), moved               # every resampler parameter moved
    if d_mode == "deterministic":
        assert not any(k.startswith("downsample.") for k in moved)


@pytest.mark.parametrize("d_mode,u_mode,unet_in", [("convolutional", "convolutional", 8), ("deterministic", "convolutional_res", 3)])
def test_trainer_two_steps_ema_and_checkpoint(tmp_path, monkeypatch, d_mode, u_mode, unet_in):
    import trainers.trainer as T
    import trainers.trainer_ddpm as TD
    for mod in (T, TD):
        monkeypatch.setattr(mod, "LOGGING_DIR", str(tmp_path) + "/", raising=True)
    # the loader feeds from the test's own process: its four workers are not what this test is about, and forking them from a
    # process that holds a whole suite's device mappings takes most of a minute
    import utils.data as UD
    real_loader = UD.DataLoader
    monkeypatch.setattr(UD, "DataLoader", lambda ds, **kw: real_loader(ds, **{**kw, "num_workers": 0, "pin_memory": False}))
    from trainers import setup_trainer
    config = dict(model="dddpm", dataset="celeba", n_steps=2, batch_size=4, image_size=16, n_downsamples=1, lr=2e-4, unet_chan=32,
                  unet_dims=(1, 2, 2, 2), unet_dropout=0.0, T=100, loss_type="simple", beta_schedule="linear", ema_decay=0.995,
                  loss_flat="sum", val_split=0, n_samples=4, d_mode=d_mode, u_mode=u_mode, d_dropout=0, d_chans=64, d_n_blocks=1,
                  u_n_blocks=1, unet_in=unet_in, ae_loss=True, t_rec_max=100, force_latent=True)
    trainer, config = setup_trainer(config, True, str(tmp_path), "unit", seed=0)
    names = [k for k, _ in trainer.model.named_parameters() if not k.startswith("latent_model.")]
    assert names and config["model_size"] == sum(p.numel() for p in trainer.model.parameters())
    before = {k: v.detach().clone() for k, v in trainer.model.named_parameters()}
    losses = trainer.train()
    assert len(losses) == 2 and all(np.isfinite(losses)) and trainer.step == 2
    after = dict(trainer.model.named_parameters())
    for k in names:
        assert not torch.equal(before[k], after[k].detach()), k
    assert torch.equal(trainer.ema._flat_ema().flat, trainer.opt.fp.flat)          # step < 2000: the EMA is reset to the live weights
    ck = torch.load(trainer.checkpoint_name, map_location="cpu", weights_only=False)
    assert list(ck["model"].keys()) == list(trainer.model.state_dict().keys()) == list(ck["ema_model"].keys())
    for k in names:
        assert torch.equal(ck["model"][k], after[k].detach().cpu()), k
    trainer2, _ = setup_trainer(dict(ck["config"]), True, str(tmp_path), "unit", seed=0)
    trainer2.load_checkpoint(ck)
    assert trainer2.step == 2 and torch.equal(trainer2.opt.fp.flat.cpu(), trainer.opt.fp.flat.cpu())
    assert torch.equal(trainer2.ema._flat_ema().flat.cpu(), trainer.ema._flat_ema().flat.cpu())
    xs, zs = trainer2.sample()
    assert xs.shape == (4, 3, 16, 16) and zs.shape == (4, unet_in, 8, 8) and bool(torch.isfinite(xs).all())


# ---------------------------------------------------------------- sampling, restoration, CLI
@pytest.mark.parametrize("mode,unet_in", [("deterministic", 3), ("convolutional", 8)])
def test_sample_decodes_its_latent(mode, unet_in):
    cfg = _cfg(mode, mode, unet_in, 1, size=16, T=50)
    m = _model(cfg).eval()
    x, z = m.sample(2, respacing="ddim5", ddim=True)
    assert x.shape == (2, 3, 16, 16) and z.shape == (2, unet_in, 8, 8)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    assert rel_err(x.cpu(), RR.rescaled_upsample(sd, cfg, z.cpu().double())) < 2e-5


def test_restoration_on_a_deterministic_model():
    cfg = _cfg("deterministic", "deterministic", 3, 1, size=16, T=50)
    m = _model(cfg).eval()
    y = syn.synthetic_input((2, 3, 4, 4), "rm.sr.y")
    x, z = m.super_resolve(y.to(DEV), 4, respacing="5", seed=3)
    assert x.shape == (2, 3, 16, 16) and z.shape == (2, 3, 8, 8) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(z).all())
    mask = torch.ones(16, 16)
    mask[:, 8:] = 0
    y = syn.synthetic_input((2, 3, 16, 16), "rm.restore.y")
    x, z = m.restore(y.to(DEV), mask, 1, respacing="5", seed=3)
    assert x.shape == (2, 3, 16, 16) and z.shape == (2, 3, 8, 8) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(z).all())
    assert torch.equal(x[..., :8].cpu(), y[..., :8])                    # paste: the measured half comes back as given


def test_generate_model_samples_cli_on_a_deterministic_config(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = _cfg("deterministic", "deterministic", 3, 1, size=16, T=50)
    cfg.update(model="dddpm", dataset="celeba")
    cfg_path = tmp_path / "cfg.json"
    cfg_path.write_text(json.dumps(cfg))
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "downsampled-diffusion_amd"))
    r = subprocess.run([sys.executable, os.path.join(root, "downsampled-diffusion_amd", "generate_model_samples.py"), "--synthetic", str(cfg_path),
                        "--saved_model", "det", "--fid_samples", "4", "--batch_size", "2", "--timestep_respacing", "ddim5", "--use_ddim",
                        "--out_dir", str(tmp_path)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(p.name for p in tmp_path.glob("det*.npy"))
    imgs = [np.load(tmp_path / f) for f in files if "latent" not in f]
    assert len(imgs) == 1 and imgs[0].shape == (2, 2, 16, 16, 3) and imgs[0].dtype == np.float32 and np.isfinite(imgs[0]).all(), files
