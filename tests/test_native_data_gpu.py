"""The image-batch kernel (csrc/image_batch.hip) and the loader built on it, on the device: every shape of
tests/image_batch_ref.py against the float64 restatement evaluated at the fp32-rounded weights, bands, position independence, flips,
out-of-range indices, guard bands and poisoned outputs, NativeImageLoader against its own host path, and two trainer steps fed by it."""
import functools

import numpy as np
import pytest
import torch

import image_batch_ref as R
from guard import guard_bands
from poison import WORDS, poisoned_allocations

from ddk import lib as L
from ddk import ops
from utils import image_batch as IB
from utils.data import NativeImageLoader, get_dataloader

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, INDEX = 6, [5, 0, 3, 3, 0]                      # first, last, repeats
CASES = [(hs, ws, s, c) for hs, ws, s in R.SHAPES for c in (1, 3)]
# beside the list: the kernel's other paths.  (512, 512, 128) x 3 is LDS-limited to 3 rows per band, so its last band is partial
# (128 = 42 * 3 + 2) and every band re-reads rows of its neighbours; (128, 128, 32) is a 4x reduction, the largest the kernel must take
EXTRA = [(512, 512, 128, 3), (128, 128, 32, 1)]


@functools.lru_cache(maxsize=None)
def _case(hs, ws, s, c):
    """(u8 [N, hs, ws, c], Transform, float64 reference [N, c, s, s] without flips): computed once, never written"""
    u8 = R.images(N, hs, ws, c, seed=hs * 7919 + ws * 31 + c)
    tf = IB.Transform(hs, ws, s)
    a_h, a_w = tf.matrices()
    ref = R.transform(u8, a_h, a_w)
    ref.setflags(write=False)
    u8.setflags(write=False)
    return u8, tf, ref


def _tables(tf):
    return tuple(torch.from_numpy(t).to(DEV) for t in (tf.row_start, tf.row_w, tf.col_start, tf.col_w))


def _run(u8, tf, index, flip=False, seed=0, epoch=0):
    images = torch.from_numpy(np.array(u8)).to(DEV)
    idx = torch.tensor(index, dtype=torch.int64).to(DEV)
    return ops.image_batch(images, idx, _tables(tf), tf.S, flip, seed, epoch)


def _bands(tf, hs, ws, c):
    r = ops.image_batch_rows_per_group(hs, ws, c, tf.S, tf.row_taps, tf.col_taps)
    assert r >= 1
    return r, -(-tf.S // r)


@pytest.mark.parametrize("hs,ws,s,c", CASES + EXTRA)
def test_kernel_against_the_float64_restatement(hs, ws, s, c):
    u8, tf, ref = _case(hs, ws, s, c)
    got = _run(u8, tf, INDEX)
    assert got.shape == (5, c, s, s) and got.dtype == torch.float32 and got.is_contiguous()
    err = float(np.abs(got.double().cpu().numpy() - ref[INDEX]).max())
    bound = R.bound(tf.row_taps, tf.col_taps)
    print(f"{hs}x{ws}x{c} -> {s}: taps {tf.row_taps}, {tf.col_taps}; max abs error {err:.3e}, bound {bound:.3e} ({err / bound:.2f} of it)")
    assert err <= bound
    if hs == ws == s:
        want = torch.from_numpy(np.array(u8)).permute(0, 3, 1, 2).float().div(255).mul(2).sub(1)[INDEX]
        assert torch.equal(got.cpu(), want)                                   # bit for bit u8 / 255 * 2 - 1


def test_bands():
    for hs, ws, s in ((218, 178, 64), (64, 64, 16)):
        for c in (1, 3):
            assert _bands(IB.Transform(hs, ws, s), hs, ws, c)[1] >= 2
    # no listed shape is cut by the LDS budget, and a band of max(4, S / 4) rows divides S: the added shape has the partial last band
    partial = [(hs, ws, s, c) for hs, ws, s, c in CASES + EXTRA if s % _bands(IB.Transform(hs, ws, s), hs, ws, c)[0]]
    assert (512, 512, 128, 3) in partial
    r, n = _bands(IB.Transform(512, 512, 128), 512, 512, 3)
    assert n >= 2 and 0 < 128 - (n - 1) * r < r


@pytest.mark.parametrize("hs,ws,s,c", [(218, 178, 64, 3), (7, 5, 4, 3), (33, 47, 16, 1), (512, 512, 128, 3)])
def test_position_independence(hs, ws, s, c):
    u8, tf, _ = _case(hs, ws, s, c)
    got = _run(u8, tf, INDEX)
    alone = _run(u8, tf, [3])
    assert torch.equal(got[2], got[3]) and torch.equal(got[2], alone[0])      # image 3 at positions 2, 3 and alone
    assert torch.equal(got[1], got[4])


def test_an_image_array_at_an_odd_address():
    """the array starts one byte into its allocation: every image's base is odd"""
    u8, tf, ref = _case(21, 13, 8, 3)
    flat = torch.zeros(u8.size + 1, dtype=torch.uint8)
    flat[1:] = torch.from_numpy(np.array(u8)).reshape(-1)
    images = flat.to(DEV)[1:].view(N, 21, 13, 3)
    assert images.data_ptr() % 2 == 1
    got = ops.image_batch(images, torch.tensor(INDEX).to(DEV), _tables(tf), 8)
    assert torch.equal(got, _run(u8, tf, INDEX))
    assert np.abs(got.double().cpu().numpy() - ref[INDEX]).max() <= R.bound(tf.row_taps, tf.col_taps)


@pytest.mark.parametrize("hs,ws,s,c", [(218, 178, 64, 3), (13, 21, 8, 1), (7, 5, 4, 3)])
def test_flips(hs, ws, s, c):
    u8, tf, _ = _case(hs, ws, s, c)
    index = [0, 1, 2, 3, 4, 5, 3]
    plain = _run(u8, tf, index)
    sets = []
    for seed, epoch in ((11, 0), (11, 1), (0xFEDC_BA98_7654_3210, 0)):
        want = R.flips(index, seed, epoch)
        got = _run(u8, tf, index, True, seed, epoch)
        for b, m in enumerate(want):
            assert torch.equal(got[b], plain[b].flip(-1) if m else plain[b]), (seed, epoch, b)
        sets.append(tuple(want))
    assert 0 < sum(sets[0]) < len(index) and sets[0] != sets[1]               # a second epoch mirrors another set


@pytest.mark.parametrize("hs,ws,s,c", [(218, 178, 64, 3), (7, 5, 4, 1)])
def test_out_of_range_indices(hs, ws, s, c):
    u8, tf, _ = _case(hs, ws, s, c)
    clean = _run(u8, tf, [5, 0, 3])
    got = _run(u8, tf, [5, N, 0, -1, 3, 2 ** 40])
    for b in (1, 3, 5):
        assert bool(torch.isnan(got[b]).all())
    assert torch.equal(got[[0, 2, 4]], clean)


@pytest.mark.parametrize("hs,ws,s,c", [(218, 178, 64, 3), (7, 5, 4, 3), (9, 9, 16, 1), (512, 512, 128, 3)])
def test_guard_bands_and_poison(hs, ws, s, c):
    u8, tf, _ = _case(hs, ws, s, c)
    plain = _run(u8, tf, INDEX, True, 5, 0)
    for word in WORDS:
        for skew in (0, 16):
            with guard_bands(word, skew=skew) as g:
                got = _run(u8, tf, INDEX, True, 5, 0)                         # images, index, tables and out all lie between bands
                assert g.check() == [] and not g.unbanded and g.count >= 7
            assert torch.equal(got, plain), (hex(word), skew)
        with poisoned_allocations(word) as p:
            got = _run(u8, tf, INDEX, True, 5, 0)
            assert p.count >= 1
        assert torch.equal(got, plain), hex(word)                             # every element of out was written


def test_argument_errors_leave_out_untouched():
    u8, tf, _ = _case(21, 13, 8, 3)
    images, idx, t = torch.from_numpy(np.array(u8)).to(DEV), torch.tensor(INDEX).to(DEV), _tables(tf)
    out = torch.full((5, 3, 8, 8), 7.0, device=DEV)
    call = lambda **k: L.load().ddk_image_batch(*[k.get(n, v) for n, v in (          # noqa: E731
        ("images", L.ptr(images)), ("n", N), ("hs", 21), ("ws", 13), ("c", 3), ("index", L.ptr(idx)), ("b", 5), ("rs", L.ptr(t[0])),
        ("rw", L.ptr(t[1])), ("rt", tf.row_taps), ("cs", L.ptr(t[2])), ("cw", L.ptr(t[3])), ("ct", tf.col_taps), ("s", 8), ("flip", 0),
        ("seed", 0), ("epoch", 0), ("out", L.ptr(out)), ("stream", L.stream()))])
    for bad in (dict(c=5), dict(s=6), dict(rt=33), dict(ct=0), dict(b=0), dict(images=None), dict(out=out.data_ptr() + 4), dict(hs=2)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0 and not bool((out == 7.0).any())


# ------------------------------------------------------------------ the loader
@pytest.fixture
def small_file(tmp_path):
    u8 = R.images(10, 12, 20, 3, seed=11)
    path = tmp_path / "train.npy"
    np.save(path, u8)
    return str(path)


def test_native_loader_on_the_device(small_file):
    from trainers.train_helpers import cycle
    tf = IB.Transform(12, 20, 8)
    dev = NativeImageLoader(small_file, 8, 4, DEV, shuffle=True, flip=True, seed=5)
    cpu = NativeImageLoader(small_file, 8, 4, "cpu", shuffle=True, flip=True, seed=5)
    assert len(dev) == 2 and dev.data.images.is_cuda and dev.data.images.dtype == torch.uint8
    for _ in range(2):                                                        # two epochs
        pairs = list(zip(dev, cpu))
        assert len(pairs) == 2 and torch.equal(dev.last_order, cpu.last_order)
        for (x, y), (xc, _) in pairs:
            assert x.is_cuda and x.shape == (4, 3, 8, 8) and x.dtype == torch.float32
            assert y.is_cuda and y.dtype == torch.int64 and y.shape == (4,) and not bool(y.any())
            assert x.to(DEV) is x                                             # the trainer's x.to(device) is a no-op
            assert float((x.cpu() - xc).abs().max()) <= R.bound(tf.row_taps, tf.col_taps)
    it = cycle(NativeImageLoader(small_file, 8, 4, DEV, shuffle=True))
    seen = [next(it)[0] for _ in range(5)]                                    # into the third epoch
    assert all(b.shape == (4, 3, 8, 8) and bool(torch.isfinite(b).all()) for b in seen) and seen[0].data_ptr() != seen[1].data_ptr()


@pytest.mark.parametrize("split", [True, False])
def test_trainer_on_an_image_file(tmp_path, monkeypatch, split):
    """the smallest configuration of tests/test_trainer_gpu.py on <data_root>/cifar10/train.npy.  16 images, not 12: a quarter of 12 is
    3 images, no batch of 4 for the validation loader (drop_last), which NativeImageLoader refuses outright (cycle() over an empty
    loader never yields)"""
    import trainers.trainer as T
    import trainers.trainer_ddpm as TD
    for mod in (T, TD):
        monkeypatch.setattr(mod, "LOGGING_DIR", str(tmp_path) + "/", raising=True)
    from trainers import setup_trainer
    (tmp_path / "cifar10").mkdir()
    u8 = R.images(16, 20, 24, 3, seed=21)
    np.save(tmp_path / "cifar10" / "train.npy", u8)
    config = dict(model="ddpm", dataset="cifar10", n_steps=2, batch_size=4, image_size=16, n_downsamples=0, lr=2e-4, unet_chan=32,
                  unet_dims=(1, 2, 2, 2), unet_dropout=0.1, T=100, loss_type="simple", beta_schedule="linear", ema_decay=0.995,
                  loss_flat="sum", val_split=0.25 if split else 0, n_samples=4, rnd_flip=split)
    trainer, config = setup_trainer(config, True, str(tmp_path), "unit", seed=0)
    losses = trainer.train()
    assert len(losses) == 2 and all(np.isfinite(losses)) and trainer.step == 2
    assert trainer._graph                                                     # the step graph was captured
    # val_batch is one image of the file through the training transform, repeated n_samples times
    tf = IB.Transform(20, 24, 16)
    a_h, a_w = tf.matrices()
    ref = R.transform(u8, a_h, a_w)
    vb = trainer.val_batch.double().cpu().numpy()
    assert vb.shape == (4, 3, 16, 16) and np.array_equal(vb[0], vb[3])
    close = [i for i in range(16) if min(np.abs(vb[0] - ref[i]).max(), np.abs(vb[0] - ref[i][..., ::-1]).max()) <= R.bound(tf.row_taps, tf.col_taps)]
    assert len(close) == 1
    if split:
        torch.manual_seed(0)
        train, val = get_dataloader(dict(config), "cpu", True, str(tmp_path), 0.25)
        assert train.indices.numel() == 12 and val.indices.numel() == 4
        assert close[0] == int(val.indices[0])                                # the validation loader's first image (it is not shuffled)
