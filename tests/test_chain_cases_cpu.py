"""The pure parts of tests/chain_cases.py, which every sampler-chain GPU test builds its inputs with: the masks, the hand-made row
tables (their bits pinned, so that an edit cannot silently change every lone-op test's inputs), the timestep map, the toggle and the
field order of the SamplerArgs struct."""
import ctypes
import hashlib
import types

import pytest
import torch

import chain_cases as CC

BASE = tuple(k for k, _ in CC.BASE_TABLES)
# sha256 of the tables' bytes in the order c_recip, c_recipm1, c1, c2, sigma (, lam, sgm), as the functions this module replaced made
# them from torch.Generator().manual_seed(seed): test_restore_noisy_gpu._hand_tables(g), and the tables of
# test_restore_blur_gpu._inputs(3, 16, 16, 3, seed), which come after x, e and yp from the same generator
NOISY = {23: "5f1700ac01d613e9b6f2bda464f43b2a420ad458b85ea2152e4f82821794588e", 613: "bd46ef958d9233770549b4a5e572984faa7092607b051a55225d6d5529808a5f"}
AFTER_INPUTS = {23: "35482ddee933bf3e434bd352c18393ef65b341da7a5d9f6afc5f100e32052a75", 613: "a25ca4dc284a9b4bb8c0d9763134e286ac275f2c9610d56df0c2a94e7a2cf2d5"}


def _digest(tab, keys):
    return hashlib.sha256(b"".join(tab[k].numpy().tobytes() for k in keys)).hexdigest()


@pytest.mark.parametrize("b,h,w", [(3, 16, 16), (2, 4, 8), (16, 32, 32)])
def test_masks(b, h, w):
    checker = CC.mask("checker", b, h, w)
    assert checker.shape == (b, h, w) and set(checker.unique().tolist()) == {0.0, 1.0}
    assert [int(v) for v in checker.sum(dim=(1, 2))] == [h * w // 2] * b
    assert torch.equal(checker[1], 1 - checker[0])                            # another phase per image
    for kind, ones in (("one_measured", 1), ("one_hidden", h * w - 1)):
        mk = CC.mask(kind, b, h, w)
        assert mk.shape == (b, h, w) and [int(v) for v in mk.sum(dim=(1, 2))] == [ones] * b
        odd = [int(mk[k].flatten().argmax() if kind == "one_measured" else mk[k].flatten().argmin()) for k in range(b)]
        assert len(set(odd)) == b                                             # at another place per image


def test_sel_and_argmax():
    mk = CC.mask("checker", 2, 4, 8)
    y = torch.zeros(2, 3, 4, 8)
    s = CC.sel(mk, y)
    assert s.shape == y.shape and s.dtype == torch.bool and int(s.sum()) == 3 * int(mk.sum())
    x = torch.zeros(2, 3, 4, 8)
    x[0, 1, 2, 3], x[1, 2, 3, 7] = 1.0, 2.0
    assert CC.argmax(x).tolist() == [1 * 32 + 2 * 8 + 3, 2 * 32 + 3 * 8 + 7]


@pytest.mark.parametrize("seed", [23, 613])
def test_hand_tables_have_their_properties_and_their_bits(seed):
    tab = CC.hand_tables(torch.Generator().manual_seed(seed), noisy=True)
    assert list(tab) == list(BASE) + ["lam", "sgm"] and all(v.shape == (8,) and v.dtype == torch.float32 for v in tab.values())
    assert float(tab["c1"][0]) == 1.0 and float(tab["c2"][0]) == 0.0 and float(tab["lam"][0]) == 0.0 and float(tab["sgm"][0]) == 0.0
    assert tab["lam"][[3, 4]].tolist() == [1.0, 1.0]
    assert ((tab["lam"][[1, 2, 5, 6, 7]] > 0) & (tab["lam"][[1, 2, 5, 6, 7]] < 1)).all() and (tab["sgm"][1:] != tab["sigma"][1:]).all()
    assert _digest(tab, BASE + ("lam", "sgm")) == NOISY[seed]
    # the five base tables are the same draws with and without the two more
    plain = CC.hand_tables(torch.Generator().manual_seed(seed))
    assert list(plain) == list(BASE) and all(torch.equal(plain[k], tab[k]) for k in BASE)
    # after a lone op's other inputs, as the plane-wide kinds' tests draw them
    g = torch.Generator().manual_seed(seed)
    shape = (3, 3, 16, 16)
    _ = 2 * torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.rand(shape, generator=g)      # x, e, yp
    assert _digest(CC.hand_tables(g), BASE) == AFTER_INPUTS[seed]


def test_timestep_map():
    tmap = CC.timestep_map(torch.tensor([0, 50, 999]))
    assert len(tmap) == 3 and list(tmap) == [0, 50, 999] and tmap._type_ is ctypes.c_int64
    assert list(CC.timestep_map([7])) == [7]


def test_toggled_restores_when_the_body_raises():
    m = types.SimpleNamespace(use_graph=True, native_sampler=True)
    with CC.toggled(m, "use_graph", False):
        assert m.use_graph is False and m.native_sampler is True
    assert m.use_graph is True
    with pytest.raises(RuntimeError, match="inside"):
        with CC.toggled(m, "native_sampler", False):
            assert m.native_sampler is False
            raise RuntimeError("inside")
    assert m.native_sampler is True


def test_sampler_args_field_order(monkeypatch):
    """every field against L.SamplerArgs._fields_, with host tensors standing in for device ones: ddk.lib.ptr refuses a CPU tensor, so
    here it is replaced by the address alone"""
    monkeypatch.setattr(CC.L, "ptr", lambda t: None if t is None else t.data_ptr())
    plan = types.SimpleNamespace(handle=0x1230, packed=torch.zeros(4))
    x, ws, noise = torch.zeros(2, 16, 24, 3), torch.zeros(8), torch.zeros(1)
    tables = {k: torch.zeros(8) for k in BASE}
    a = CC.sampler_args(plan, x, tables, 19, ws, 4096, seed=613, stream_id=5, graph=1, noise=noise)
    want = dict(unet=0x1230, packed=plan.packed.data_ptr(), x=x.data_ptr(), noise=noise.data_ptr(), B=2, H=16, W=24, t_start=19, t_end=0,
                seed=613, stream_id=5, use_graph=1, workspace=ws.data_ptr(), workspace_bytes=4096, **{k: tables[k].data_ptr() for k in BASE})
    assert [name for name, _ in CC.L.SamplerArgs._fields_] == list(want)[:4] + list(BASE) + list(want)[4:14]
    assert {name: getattr(a, name) for name in want} == want
    assert len({v for k, v in want.items() if k in BASE + ("packed", "x", "noise", "workspace")}) == 9      # no two fields share a pointer
    # the defaults, a table without sigma, and an overriding shape
    b = CC.sampler_args(plan, x, {k: tables[k] for k in BASE[:4]}, 7, ws, 64, seed=1, shape=(2, 48, 16))
    assert (b.noise, b.sigma, b.stream_id, b.use_graph, b.B, b.H, b.W, b.t_start, b.seed) == (None, None, 0, 0, 2, 48, 16, 7, 1)
