"""Whole T = 1000 chains on the GPU vs the reference's own (tests/golden/g10_long.npz, tools/gen_golden.py:g10_long).

The tiny DDPM (unet_chan 32, 3x16x16, linear schedule, T = 1000, B = 2).  The native graph sampler replays its captured
16-step graphs about 63 times here, so the step counter, the t indexing and the t == 0 mask all cross graph boundaries; the
likelihood sweep runs all 1000 timesteps ([T][B][nslot] partials, 1000 finalize workgroups).  Both with injected draws, so
the reference's trajectory is reproduced element for element.

Bar: the 50-step chains' 1e-4 abs (test_sampler_gpu.py) holds over 1000 steps (measured 2.6e-6 after 1000; changing one draw
misses by 0.61); the sweep keeps g9's 5e-5 relative (measured 3e-7)."""
import numpy as np
import pytest
import torch

from helpers import ddpm_cfg, det_load, golden, rel_err
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SNAPS = (1, 500, 900, 990, 999, 1000)
CHAIN_TOL = 1e-4
LOSS_TOL = 5e-5
KEYS = ("vlb_t", "prior", "vlb", "L_simple_t", "L_simple")


@pytest.fixture(scope="module")
def tiny():
    from models import DDPM, Unet
    cfg = ddpm_cfg(32, 3, 16)
    return det_load(DDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()


@pytest.fixture(scope="module")
def chain_draws():
    x_T = syn.synthetic_normal((2, 3, 16, 16), "g10.chain.xT")
    noise = torch.stack([syn.synthetic_normal((2, 3, 16, 16), f"g10.chain.n{k}") for k in range(1000)])
    return x_T, noise


def g10_x():
    """tools/gen_golden.py:g10_x"""
    x = syn.synthetic_input((2, 3, 16, 16), "g9.x").clamp(-1, 1)
    x[0, 0, 0, :6] = torch.tensor([-1.0, 1.0, -0.9995, 0.9995, -0.999, 0.999])
    return x


def test_chain_1000_steps_vs_reference(tiny, chain_draws):
    """snapshot k = a native run of the first k steps (early_stop = 1000 - k, noise[:k]); the last is the whole chain with its
    noise-free t == 0 step.  Then the argmax pixel and the uint8 image, as test_chain_tiny_50_steps judges them."""
    g = golden("g10_long")
    x_T, noise = chain_draws
    errs = {}
    for k in SNAPS:
        x = tiny.p_sample_loop((2, 3, 16, 16), early_stop=1000 - k, x_T=x_T, noise=noise[:k])
        errs[k] = float(np.abs(x.cpu().numpy() - g[f"chain_step{k}"]).max())
    print("g10 chain max abs error per snapshot:", errs)
    assert all(e < CHAIN_TOL for e in errs.values()), errs
    assert np.array_equal(x.reshape(2, -1).argmax(dim=1).cpu().numpy(), g["argmax"])
    from utils import fix_samples
    fixed = fix_samples(x)
    assert np.abs(fixed - g["fixed"]).max() < 2e-2
    assert (np.round(fixed) != np.round(g["fixed"])).mean() < 2e-3      # identical uint8 images (<=1 LSB on <0.2%)


def test_chain_1000_steps_detects_one_changed_draw(tiny, chain_draws):
    """negative control: draw k = 700 (t = 299) replaced, everything else equal -- the final state must miss the reference by
    more than 10x the bar, so the bar above can see a single wrong step anywhere in the chain."""
    g = golden("g10_long")
    x_T, noise = chain_draws
    bad = noise.clone()
    bad[700] = syn.synthetic_normal((2, 3, 16, 16), "g10.chain.control")
    x = tiny.p_sample_loop((2, 3, 16, 16), x_T=x_T, noise=bad)
    err = float(np.abs(x.cpu().numpy() - g["chain_step1000"]).max())
    print("g10 chain, draw 700 changed: max abs error", err)
    assert err > 10 * CHAIN_TOL


def test_test_losses_1000_steps_vs_reference(tiny):
    """the likelihood sweep over all 1000 timesteps (one injected draw g10.eps{k} per step) vs the reference's test_losses_;
    the t = 0 column (the discretised NLL: -1, +1, +-0.9995 and the exact +-0.999 boundary in image 0) on its own too."""
    g = golden("g10_long")
    noise = torch.stack([syn.synthetic_normal((2, 3, 16, 16), f"g10.eps{k}") for k in range(1000)]).to(DEV)
    res = tiny.test_losses(g10_x().to(DEV), noise=noise)
    assert res["vlb_t"].shape == (2, 1000) and res["L_simple_t"].shape == (1000,)
    errs = {k: rel_err(res[k].cpu(), g[f"losses_{k}"]) for k in KEYS}
    errs["vlb_t[:, -1]"] = rel_err(res["vlb_t"][:, -1].cpu(), g["losses_vlb_t"][:, -1])
    print("g10 test_losses relative error:", errs)
    assert all(e < LOSS_TOL for e in errs.values()), errs
