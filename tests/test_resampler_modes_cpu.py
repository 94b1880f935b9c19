"""The 'deterministic' and 'convolutional' resampler modes of the dDDPM (reference models/downsampled/wrapper.py:22-26,49-55), the
parts that need no device: the factories and their state_dict contract against the reference's own key list, the float64
restatement (tests/resample_ref.py) against the reference's own outputs (tests/golden/g11_*), the host-built tap tables against
the restatement, and the FLOP counts."""
import json
import os

import numpy as np
import pytest
import torch

import resample_ref as RR
from helpers import GOLD, dddpm_cfg, det_state, golden, rel_err
from utils import synthetic as syn

MODES = ("convolutional_res", "convolutional", "deterministic")
CASES = [("deterministic", 3, 2), ("deterministic", 3, 3), ("convolutional", 3, 2), ("convolutional", 3, 3), ("convolutional", 8, 2),
         ("convolutional", 8, 3)]


def _keys():
    with open(os.path.join(GOLD, "g11_state_dict_keys.json")) as f:
        return json.load(f)


def _cfg(mode_d, mode_u, unet_in, n_down, size=32, chan=32, T=1000):
    cfg = dddpm_cfg(chan, size, n_down, T)
    cfg.update(d_mode=mode_d, u_mode=mode_u, unet_in=unet_in)
    return cfg


def _model(cfg, ae=False):
    from models import DownsampleDDPM, DownsampleDDPMAutoencoder, Unet
    return (DownsampleDDPMAutoencoder if ae else DownsampleDDPM)(cfg, Unet(cfg), "cpu", 3)


@pytest.mark.parametrize("d_mode", MODES)
@pytest.mark.parametrize("u_mode", MODES)
def test_factories_build_all_nine_mode_pairs(d_mode, u_mode):
    from models.downsampled import get_downsampling, get_upsampling
    from models.downsampled.convblocks import ConvResNet, Interpolate, SimpleDownConv, SimpleUpConv
    unet_in = 3 if "deterministic" in (d_mode, u_mode) else 8
    cfg = _cfg(d_mode, u_mode, unet_in, 2)
    down, up = get_downsampling(cfg, (3, 32, 32)), get_upsampling(cfg, (3, 32, 32))
    kinds = {"convolutional_res": (ConvResNet, ConvResNet), "convolutional": (SimpleDownConv, SimpleUpConv), "deterministic": (Interpolate, Interpolate)}
    assert type(down) is kinds[d_mode][0] and type(up) is kinds[u_mode][1]
    if d_mode == "deterministic":
        assert down.size == (8, 8) and not list(down.state_dict()) and not list(down.buffers())
    if u_mode == "deterministic":
        assert up.size == (32, 32) and not list(up.state_dict())
    # the channel chain the reference's call gives: unet_in is the simple stacks' `dim`
    if d_mode == "convolutional":
        assert [(c.in_channels, c.out_channels) for c in down.conv] == [(3, unet_in), (unet_in, unet_in)]
        assert all(c.kernel_size == (3, 3) and c.stride == (2, 2) and c.padding == (1, 1) for c in down.conv)
    if u_mode == "convolutional":
        assert [(c.in_channels, c.out_channels) for c in up.conv] == [(unet_in, unet_in), (unet_in, 3)]
        assert all(c.kernel_size == (4, 4) and c.stride == (2, 2) and c.padding == (1, 1) for c in up.conv)
    m = _model(cfg)            # ... and the whole model builds with the pair
    assert m.sample_shape == [unet_in, 8, 8]


@pytest.mark.parametrize("mode,unet_in,n_down", CASES)
def test_state_dict_keys_equal_the_references_and_load_strictly(mode, unet_in, n_down):
    ref = _keys()
    want = dict(ref[f"{mode}_u{unet_in}_n{n_down}"])
    want.update(ref[f"latent_model_u{unet_in}"])
    for ae in (False, True):
        m = _model(_cfg(mode, mode, unet_in, n_down), ae)
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == want
        sd = det_state({k: tuple(s) for k, s in want.items()})
        sd.update({k: v for k, v in m.state_dict().items() if k in syn.SCHEDULE_KEYS})
        m.load_state_dict(sd, strict=True)
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k


def test_bad_modes_are_refused_at_construction():
    from models.downsampled import get_downsampling, get_upsampling
    for which, fn in (("d_mode", get_downsampling), ("u_mode", get_upsampling)):
        cfg = _cfg("convolutional_res", "convolutional_res", 8, 2)
        cfg[which] = "deterministic"
        with pytest.raises(ValueError, match="unet_in"):
            fn(cfg, (3, 32, 32))
        cfg[which] = "nearest"
        with pytest.raises(NotImplementedError):
            fn(cfg, (3, 32, 32))
    with pytest.raises(ValueError, match="unet_in"):
        _model(_cfg("deterministic", "convolutional", 8, 2))
    # the reference's assertion on an even downsampled size stays (wrapper.py:52): 24 / 8 = 3
    with pytest.raises(AssertionError, match="even"):
        get_downsampling(_cfg("deterministic", "deterministic", 3, 3, size=24), (3, 24, 24))


@pytest.mark.parametrize("mode,unet_in,n_down", CASES)
def test_restatement_reproduces_the_references_outputs(mode, unet_in, n_down):
    """tests/resample_ref.py (float64) == the reference's downsample / rescaled_downsample / rescaled_upsample (fp32, torch's CPU
    kernels; bicubic computes t in fp32): the bar the g8 resampler goldens are held to"""
    g = golden("g11_resampler_modes")
    tag = f"{mode}_u{unet_in}_n{n_down}"
    cfg = _cfg(mode, mode, unet_in, n_down)
    shapes = {k: tuple(s) for k, s in _keys()[tag].items() if k not in syn.SCHEDULE_KEYS}
    sd = {k: v.double() for k, v in det_state(shapes).items()}
    x = syn.synthetic_input((2, 3, 32, 32), f"g11.x{n_down}").double()
    assert rel_err(RR.downsample(sd, cfg, x), g[f"{tag}_raw"]) < 2e-5
    z = RR.rescaled_downsample(sd, cfg, x)
    assert rel_err(z, g[f"{tag}_z"]) < 2e-5
    assert rel_err(RR.rescaled_upsample(sd, cfg, torch.from_numpy(g[f"{tag}_z"]).double()), g[f"{tag}_x"]) < 2e-5


def test_restatement_equals_torch_interpolate():
    import torch.nn.functional as F
    for n_in, n_out in ((16, 8), (8, 16), (32, 8), (8, 32), (12, 6), (6, 12), (2, 1), (1, 2), (256, 32)):
        x = syn.synthetic_normal((2, 3, n_in, n_in), f"rr.{n_in}.{n_out}").double()
        want = F.interpolate(x, size=(n_out, n_out), mode="bicubic", align_corners=True)
        assert rel_err(RR.bicubic(x, (n_out, n_out)), want) < 1e-12


@pytest.mark.parametrize("n_in,n_out", [(8, 4), (32, 4), (4, 32), (24, 6), (2, 1)])
def test_host_built_tap_tables_equal_the_restatement(n_in, n_out):
    from ddk import ops
    idx, w = ops.bicubic_taps(n_in, n_out)
    assert idx.shape == (n_out, 4) and w.shape == (n_out, 4) and idx.dtype == np.int32 and w.dtype == np.float32
    assert idx.min() >= 0 and idx.max() <= n_in - 1
    want = RR.bicubic_matrix(n_in, n_out)
    dense = np.zeros((n_out, n_in))
    for o in range(n_out):
        for k in range(4):
            dense[o, idx[o, k]] += float(w[o, k])          # clamped taps add their weights
    assert np.abs(dense - want).max() <= 2.0 ** -24 * 4        # four fp32 roundings of weights below 2 in magnitude at the most
    assert np.abs(want.sum(axis=1) - 1).max() < 1e-14 and np.abs(dense.sum(axis=1) - 1).max() < 4 * 2.0 ** -24
    # the transposed lists hold the same matrix: every (input, output) pair once, outputs ascending
    start, oi, wt = ops.bicubic_taps_transposed(n_in, n_out)
    assert start.shape == (n_in + 1,) and start[0] == 0 and start[-1] == len(oi) == len(wt)
    dense_t = np.zeros((n_out, n_in))
    for i in range(n_in):
        outs = oi[start[i]:start[i + 1]]
        assert list(outs) == sorted(set(outs))
        dense_t[outs, i] = wt[start[i]:start[i + 1]]
    assert np.abs(dense_t - dense).max() <= 2.0 ** -24 * 2


def test_flops_are_the_hand_counts():
    from models.downsampled.convblocks import Interpolate, SimpleDownConv, SimpleUpConv
    # 3 -> 8 at 10x6 -> 5x3, then 8 -> 8 at 5x3 -> 3x2
    assert SimpleDownConv(8, 3, 2).flops(2, 10, 6) == 2 * 2 * (5 * 3 * 9 * 3 * 8 + 3 * 2 * 9 * 8 * 8)
    # 8 -> 8 at 4x4 -> 8x8, then 8 -> 3 at 8x8 -> 16x16: four taps per output element
    assert SimpleUpConv(8, 3, 2).flops(2, 4, 4) == 2 * 2 * (8 * 8 * 4 * 8 * 8 + 16 * 16 * 4 * 8 * 3)
    # 16 taps per output element whatever the input size
    assert Interpolate((8, 8), 3).flops(2, 32, 32) == 2 * 16 * 2 * 3 * 8 * 8
    m = _model(_cfg("convolutional", "deterministic", 3, 2))
    assert m.downsample.flops(1, 32, 32) > 0 and m.upsample.flops(1, 8, 8) == 2 * 16 * 3 * 32 * 32


def test_cpu_tensors_are_refused():
    from ddk import ops
    from ddk.lib import DDKError
    x = torch.zeros(1, 3, 8, 8)
    calls = [lambda: ops.bicubic_resize(x, (4, 4)), lambda: ops.bicubic_resize_grad(x, (16, 16)),
             lambda: ops.conv_small_s2(x, torch.zeros(3, 3, 3, 3), torch.zeros(3)), lambda: ops.convt_small_s2(x, torch.zeros(3, 3, 4, 4), torch.zeros(3)),
             lambda: ops.conv_small_s2_dgrad(torch.zeros(1, 3, 4, 4), torch.zeros(3, 3, 3, 3), (8, 8)),
             lambda: ops.convt_small_s2_dgrad(x, torch.zeros(3, 3, 4, 4)),
             lambda: ops.conv_small_s2_wgrad(x, torch.zeros(1, 3, 4, 4)), lambda: ops.convt_small_s2_wgrad(x, torch.zeros(1, 3, 16, 16))]
    for call in calls:
        with pytest.raises(DDKError, match="CPU tensor"):
            call()
