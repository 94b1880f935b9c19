"""DDNM super-resolution on the CPU: the restatement's projection (tests/restore_ref.py) has the two properties the method rests
on, every argument error of DDPM.super_resolve / DownsampleDDPM.super_resolve comes before any device work, and the header, the
ctypes signatures and the built library agree on the new entries.

The bound of the projection, in units of 2^-24, for |x0| <= 1 and |y| <= 1: each of the n^2 - 1 roundings of the block sum is at
most half an ulp of a value below n^2, which is 1 after the exact scaling by 1 / n^2; d = y - m is below 2 in size (half an ulp: 1);
x0' = x0 + d is below 4 in size (half an ulp: 2), and the block mean of those last errors is no larger than one of them.  In all
n^2 + 2, within the (n^2 + 4) 2^-24 the tests hold the projection to; pooling the result in float64 adds nothing visible."""
import ctypes
import os
import re

import pytest
import torch

import restore_ref as RR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from ddk import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddk_p_sample_update_restore", "ddk_sampler_restore_workspace_bytes", "ddk_sampler_run_restore")


def _bound(n):
    return (n * n + 4) * 2.0 ** -24


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_projection_hits_y_and_is_idempotent(n, seed):
    g = torch.Generator().manual_seed(100 * n + seed)
    x0 = (1.5 * torch.randn(3, 4, 8 * n, 4 * n, generator=g)).clamp(-1, 1)
    y = torch.rand(3, 4, 8, 4, generator=g) * 2 - 1
    once = RR.project(x0, y, n)
    assert once.dtype == torch.float32
    err = float((RR.pool(once.double(), n) - y.double()).abs().max())
    print(f"n = {n}: |avg_pool(x0') - y| max {err:.3g} (bound {_bound(n):.3g})")
    assert err <= _bound(n)
    twice = RR.project(once, y, n)
    err2 = float((twice - once).abs().max())
    print(f"n = {n}: |P(P(x0)) - P(x0)| max {err2:.3g}")
    assert err2 <= _bound(n)
    # the null-space part is kept: x0' - A+ A x0' equals x0 - A+ A x0 up to rounding
    null = lambda v: v.double() - RR.replicate(RR.pool(v.double(), n), n)
    assert float((null(once) - null(x0)).abs().max()) <= 2 * _bound(n)


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


def _dd():
    cfg = dddpm_cfg(32, 32, 2)
    return DownsampleDDPM(cfg, Unet(cfg), "cpu", 3)


@pytest.mark.parametrize("scale", [0, 1, 3, 16, 2.0, True, "2", None])
def test_bad_scale_raises(scale):
    with pytest.raises(ValueError):
        _tiny().super_resolve(torch.zeros(2, 3, 8, 8), scale)


@pytest.mark.parametrize("y", [torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 4, 4), torch.zeros(3, 4, 4), torch.zeros(2, 3, 4, 8),
                               torch.zeros(2, 3, 4, 4, dtype=torch.long), torch.full((2, 3, 4, 4), float("nan")),
                               torch.full((2, 3, 4, 4), float("inf")), [[0.0]]])
def test_bad_y_raises(y):
    with pytest.raises(ValueError):
        _tiny().super_resolve(y, 4)


@pytest.mark.parametrize("kw", [dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(solver="dpm++2m"), dict(noise=torch.zeros(1)),
                                dict(early_stop=10), dict(jump_length=3)])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(ValueError):
        _tiny().super_resolve(torch.zeros(2, 3, 4, 4), 4, **kw)


def test_good_arguments_reach_the_device_check():
    """everything valid: the first complaint is the missing device, not an argument"""
    with pytest.raises(L.DDKError):
        _tiny().super_resolve(torch.zeros(2, 3, 4, 4), 4, respacing="20", ddim=True, eta=0.5, seed=1)


@pytest.mark.parametrize("y,scale,kw", [
    (torch.zeros(1, 3, 8, 8), 4, {}),                      # n_lat = 4 / 4 = 1
    (torch.zeros(1, 3, 16, 16), 2, {}),                    # scale below dim_reduc
    (torch.zeros(1, 3, 4, 4), 12, {}),                     # not a multiple of dim_reduc
    (torch.zeros(1, 3, 1, 1), 64, {}),                     # n_lat = 16
    (torch.zeros(1, 8, 1, 1), 8, {}),                      # a latent is not an image
    (torch.zeros(1, 3, 8, 8), 8, {}),                      # 32 / 8 = 4, not 8
    (torch.full((1, 3, 4, 4), float("nan")), 8, {}),
    (torch.zeros(1, 3, 4, 4), 8, dict(solver="dpm++2m")),
    (torch.zeros(1, 3, 4, 4), 8, dict(noise=torch.zeros(1))),
    (torch.zeros(1, 3, 4, 4), 8, dict(early_stop=3)),
    (torch.zeros(1, 3, 4, 4), 8, dict(eta=0.3)),
])
def test_dddpm_bad_arguments_raise(y, scale, kw):
    with pytest.raises(ValueError):
        _dd().super_resolve(y, scale, **kw)


def test_dddpm_good_arguments_reach_the_device_check():
    with pytest.raises(L.DDKError):
        _dd().super_resolve(torch.zeros(1, 3, 4, 4), 8)


@pytest.mark.parametrize("kw", [dict(respacing=None), dict(respacing="20"), dict(respacing="20", ddim=True),
                                dict(respacing="ddim50", ddim=True, eta=0.7)])
def test_row_0_of_every_table_set_returns_x0(kw):
    """c1[0] == 1 and c2[0] == 0 in fp32, so the last step's result is x0' itself: what the consistency of the output rests on"""
    m = _tiny()
    spaced = kw["respacing"] is not None or kw.get("ddim", False)
    tables = m._spaced_tables(kw["respacing"], kw.get("ddim", False), kw.get("eta", 0.0))[0] if spaced else m._tables()
    assert float(tables["c1"][0]) == 1.0 and float(tables["c2"][0]) == 0.0


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW + ("ddk_sampler_restore_tail_parts",):
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(L.SIGNATURES["ddk_p_sample_update_restore"][1]) == 17
    assert len(L.SIGNATURES["ddk_sampler_run_restore"][1]) == 5
    assert L.load().ddk_version() == L.ABI_VERSION == 400


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only: the restore workspace holds y behind the sampler layout, and the fused tail's eligibility is
    128 % (W n) == 0 on top of the plain tail's (cfg4: 128 channels, 32 x 32 latent; 256 channels: never)"""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 8, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    plain = lib.ddk_sampler_workspace_bytes(h, 32, 32, 32, 49)
    assert lib.ddk_sampler_restore_workspace_bytes(h, 32, 32, 32, 49) >= plain + 32 * 32 * 32 * 8 // 4 * 4
    assert lib.ddk_sampler_restore_workspace_bytes(h, 32, 30, 32, 49) == 0
    parts = {n: lib.ddk_sampler_restore_tail_parts(h, 32, 32, 32, n) for n in (2, 4, 8)}
    assert parts[2] == parts[4] == 8 and parts[8] == 0, parts
    assert lib.ddk_sampler_restore_tail_parts(h, 32, 64, 64, 2) in (0, 32)          # W n = 128: eligible where the final conv is
    assert lib.ddk_sampler_restore_tail_parts(h, 32, 64, 64, 4) == 0
    assert lib.ddk_unet_set_option(h, 12, 0) == 0
    assert lib.ddk_sampler_restore_tail_parts(h, 32, 32, 32, 2) == 0
    assert lib.ddk_unet_set_option(h, 12, 1) == 0
    u256 = Unet(ddpm_cfg(256, 8, 32))
    u256.flops(1, 32, 32)
    assert lib.ddk_sampler_restore_tail_parts(u256._plan.handle, 32, 32, 32, 2) == 0
