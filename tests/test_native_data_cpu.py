"""The native input pipeline without a device: the resize / crop arithmetic and the tap tables of
utils/image_batch.py against the float64 restatement (tests/image_batch_ref.py) and against torch's own antialiased interpolate, the
flip rule against the oracle's Philox, NativeImageLoader on the host path, the validation split, get_dataloader's routing, the new
command-line flags, prepare_dataset.py on inputs written here, and the C ABI of the two new entries."""
import gzip
import os
import pickle
import re
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_batch_ref as R
from conftest import ROOT

from utils import image_batch as IB
from utils.data import NativeImageLoader, SyntheticImages, get_dataloader

CASES = [(hs, ws, s, c) for hs, ws, s in R.SHAPES for c in (1, 3)]


def test_resize_and_crop_arithmetic():
    for (hs, ws, s), shape, off in [((218, 178, 64), (78, 64), 7), ((40, 24, 32), (53, 32), 10), ((33, 47, 16), (16, 22), 3),
                                    ((12, 20, 24), (24, 40), 8)]:
        assert IB.resized_shape(hs, ws, s) == shape
        assert IB.crop_offset(max(shape), s) == off and IB.crop_offset(min(shape), s) == 0
        assert R.geometry(hs, ws, s)[:2] == shape
    assert IB.crop_offset(53, 32) == 10          # (53 - 32) / 2 = 10.5 rounds to even


@pytest.mark.parametrize("hs,ws,s", R.SHAPES)
def test_tables_against_the_float64_matrix(hs, ws, s):
    tf = IB.Transform(hs, ws, s)
    for (start, w, taps, n_in), want in zip(((tf.row_start, tf.row_w, tf.row_taps, hs), (tf.col_start, tf.col_w, tf.col_taps, ws)),
                                           R.matrices(hs, ws, s)):
        assert start.dtype == np.int32 and w.dtype == np.float32 and w.shape == (s, taps) and start.shape == (s,)
        assert 1 <= taps <= 32 and start.min() >= 0 and (start + taps).max() <= n_in
        assert taps == int((want > 0).sum(axis=1).max())
        got = IB.dense(start, w, n_in)
        assert np.array_equal(got, want.astype(np.float32))                   # the float64 rows, rounded to fp32 once
        assert np.abs(got.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -23
    if hs == ws == s:
        assert tf.row_taps == tf.col_taps == 1 and np.all(tf.row_w == 1.0) and np.array_equal(tf.row_start, np.arange(s))


@pytest.mark.parametrize("hs,ws,s,c", CASES)
def test_float64_matrix_against_torch_interpolate(hs, ws, s, c):
    u8 = R.images(3, hs, ws, c, seed=hs * 1000 + ws)
    ho, wo, top, left = R.geometry(hs, ws, s)
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255)
    want = F.interpolate(x, size=(ho, wo), mode="bilinear", antialias=True, align_corners=False)[:, :, top:top + s, left:left + s]
    a_h, a_w = R.matrices(hs, ws, s)
    got = (R.transform(u8, a_h, a_w) + 1.0) / 2.0
    err = float(np.abs(got - want.double().numpy()).max())
    print(f"{hs}x{ws}x{c} -> {s}: float64 matrix against torch interpolate {err:.3e}")
    assert err <= 1e-5
    if hs == ws == s:
        assert torch.equal(want, x)


def test_flip_bits_follow_the_oracles_philox():
    ids = np.concatenate([np.arange(4000), np.arange(96) + (1 << 33)]).astype(np.int64)       # ids above 2^32 use counter word 1
    seen = []
    for seed in (7, 0x1234_5678_9ABC_DEF0):
        for epoch in (0, 3):
            got = IB.flip_bits(ids, seed, epoch)
            assert got.dtype == bool and np.array_equal(got, R.flips(ids, seed, epoch))
            assert 0.45 <= got.mean() <= 0.55                                                 # 6 sigma at n = 4096
            seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
    assert np.array_equal(IB.flip_bits(ids[::-1], 7, 0), seen[0][::-1])                       # a function of the id, not of the position


@pytest.fixture
def small_file(tmp_path):
    u8 = R.images(10, 12, 20, 3, seed=11)
    path = tmp_path / "train.npy"
    np.save(path, u8)
    return str(path), u8


def _epoch(loader):
    batches = [(x, y) for x, y in loader]
    return batches, loader.last_order.clone()


def test_cpu_loader(small_file):
    path, u8 = small_file
    loader = NativeImageLoader(path, 8, 4, "cpu", shuffle=True, flip=True, seed=5)
    assert len(loader) == 2
    (b0, o0), (b1, o1) = _epoch(loader), _epoch(loader)
    assert len(b0) == len(b1) == 2
    for x, y in b0 + b1:
        assert x.shape == (4, 3, 8, 8) and x.dtype == torch.float32 and x.is_contiguous()
        assert y.shape == (4,) and y.dtype == torch.int64 and not y.any()
    assert sorted(o0.tolist()) == list(range(10)) and sorted(o1.tolist()) == list(range(10))
    assert o0.tolist() != o1.tolist()                                                         # two epochs differ
    again = NativeImageLoader(path, 8, 4, "cpu", shuffle=True, flip=True, seed=5)
    (a0, ao0), (a1, ao1) = _epoch(again), _epoch(again)
    assert torch.equal(ao0, o0) and torch.equal(ao1, o1)                                      # the same seed, the same order
    assert all(torch.equal(p[0], q[0]) for p, q in zip(a0 + a1, b0 + b1))
    tf = IB.Transform(12, 20, 8)
    a_h, a_w = tf.matrices()                                                                  # the restatement at the fp32-rounded weights
    assert np.array_equal(a_h, R.matrices(12, 20, 8)[0].astype(np.float32))
    flipped = 0
    for epoch, (batches, order) in enumerate(((b0, o0), (b1, o1))):
        flip = R.flips(order.numpy(), 5, epoch)
        for k, (x, _) in enumerate(batches):
            ids = order[4 * k:4 * k + 4].numpy()
            want = R.transform(u8[ids], a_h, a_w, flip[4 * k:4 * k + 4])
            err = float(np.abs(x.double().numpy() - want).max())
            print(f"epoch {epoch} batch {k}: {err:.3e} against bound {R.bound(tf.row_taps, tf.col_taps):.3e}")
            assert err <= R.bound(tf.row_taps, tf.col_taps)
            flipped += int(flip[4 * k:4 * k + 4].sum())
    assert 0 < flipped < 16
    # a loader without a seed draws one from torch's global generator at its first epoch, as DataLoader does
    torch.manual_seed(3)
    l1 = NativeImageLoader(path, 8, 4, "cpu", shuffle=True)
    o_a = _epoch(l1)[1]
    torch.manual_seed(3)
    o_b = _epoch(NativeImageLoader(path, 8, 4, "cpu", shuffle=True))[1]
    assert torch.equal(o_a, o_b) and l1.base_seed is not None
    with pytest.raises(ValueError, match="make no batch"):
        NativeImageLoader(path, 8, 4, "cpu", indices=[0, 1, 2])                               # cycle() over it would never yield


def test_cpu_loader_identity_is_bit_exact(tmp_path):
    u8 = R.images(6, 16, 16, 3, seed=2)
    u8[0, 0, :, 0] = np.arange(16) * 17                                                       # 0 and 255 among them
    np.save(tmp_path / "test.npy", u8)
    loader = NativeImageLoader(str(tmp_path / "test.npy"), 16, 3, "cpu", shuffle=False, flip=False)
    got = torch.cat([x for x, _ in loader])
    want = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255).mul(2).sub(1)
    assert torch.equal(got, want) and loader.last_order.tolist() == list(range(6))
    from utils.restoration_metrics import to_u8
    back = to_u8(got)
    assert back.dtype == torch.uint8 and np.array_equal(back.numpy(), u8)


def test_gray_file_without_a_channel_axis(tmp_path):
    u8 = R.images(5, 9, 9, 1, seed=4)
    np.save(tmp_path / "g.npy", u8[..., 0])
    x, _ = next(iter(NativeImageLoader(str(tmp_path / "g.npy"), 16, 5, "cpu")))
    a_h, a_w = IB.Transform(9, 9, 16).matrices()
    assert x.shape == (5, 1, 16, 16) and np.abs(x.double().numpy() - R.transform(u8, a_h, a_w)).max() <= R.bound(3, 3)


def test_validation_split_is_the_references(small_file):
    path, _ = small_file
    cfg = dict(dataset="cifar10", image_size=8, batch_size=2, data_file=path, rnd_flip=True)
    torch.manual_seed(9)
    train, val = get_dataloader(cfg, "cpu", True, "/nonexistent", 0.15)
    torch.manual_seed(9)
    perm = torch.randperm(10)
    assert isinstance(train, NativeImageLoader) and isinstance(val, NativeImageLoader)
    assert train.indices.numel() == 8 and val.indices.numel() == 2                            # (10 * [0.85, 0.15]).astype(int) = 8, 1: + 1
    assert torch.equal(train.indices, perm[:8]) and torch.equal(val.indices, perm[8:])
    assert sorted(train.indices.tolist() + val.indices.tolist()) == list(range(10))
    assert train.data is val.data                                                             # one resident array
    assert train.shuffle and not val.shuffle and train.flip and val.flip                      # the training transform on both
    assert _epoch(val)[1].tolist() == perm[8:].tolist()


def test_get_dataloader_routing(small_file, tmp_path, monkeypatch):
    path, u8 = small_file
    monkeypatch.delenv("DDPM_TEST_FILE", raising=False)
    monkeypatch.delenv("DDPM_REAL_DATA", raising=False)
    cfg = dict(dataset="cifar10", image_size=8, batch_size=4)
    # no file: what it always was
    for train in (True, False):
        loader, val = get_dataloader(dict(cfg), "cpu", train, str(tmp_path / "empty"))
        assert isinstance(loader, torch.utils.data.DataLoader) and isinstance(loader.dataset, SyntheticImages) and val is None
    assert isinstance(get_dataloader(dict(cfg), "cpu", True, None)[0].dataset, SyntheticImages)       # callers without a data directory
    # config['data_file']
    loader, val = get_dataloader(dict(cfg, data_file=path), "cpu", True, str(tmp_path / "empty"))
    assert isinstance(loader, NativeImageLoader) and val is None and loader.shuffle and not loader.flip and len(loader) == 2
    assert get_dataloader(dict(cfg, data_file=path, rnd_flip=True), "cpu", True, str(tmp_path / "empty"))[0].flip
    # the convention <data_root>/<dataset>/{train,test}.npy
    root = tmp_path / "data"
    (root / "cifar10").mkdir(parents=True)
    np.save(root / "cifar10" / "train.npy", u8)
    np.save(root / "cifar10" / "test.npy", u8[:5])
    assert isinstance(get_dataloader(dict(cfg), "cpu", True, str(root))[0], NativeImageLoader)
    test = get_dataloader(dict(cfg, rnd_flip=True), "cpu", False, str(root))[0]
    assert isinstance(test, NativeImageLoader) and not test.shuffle and not test.flip and len(test) == 1 and test.data.n == 5
    # DDPM_TEST_FILE, and config['test_file'] in front of it
    other = tmp_path / "other.npy"
    np.save(other, u8[:8])
    monkeypatch.setenv("DDPM_TEST_FILE", str(other))
    assert get_dataloader(dict(cfg), "cpu", False, str(tmp_path / "empty"))[0].data.n == 8
    assert get_dataloader(dict(cfg, test_file=path), "cpu", False, str(tmp_path / "empty"))[0].data.n == 10
    assert isinstance(get_dataloader(dict(cfg), "cpu", True, str(tmp_path / "empty"))[0], torch.utils.data.DataLoader)   # not the train split
    monkeypatch.delenv("DDPM_TEST_FILE")
    # refusals
    with pytest.raises(ValueError, match="channel"):
        get_dataloader(dict(cfg, dataset="mnist", data_file=path), "cpu", True, str(tmp_path / "empty"))
    np.save(tmp_path / "f32.npy", u8.astype(np.float32))
    with pytest.raises(ValueError, match=r"float32.*\(10, 12, 20, 3\)"):
        get_dataloader(dict(cfg, data_file=str(tmp_path / "f32.npy")), "cpu", True, str(tmp_path / "empty"))
    np.save(tmp_path / "flat.npy", u8.reshape(10, -1))
    with pytest.raises(ValueError, match=r"uint8.*\(10, 720\)"):
        get_dataloader(dict(cfg, data_file=str(tmp_path / "flat.npy")), "cpu", True, str(tmp_path / "empty"))
    with pytest.raises(FileNotFoundError):
        get_dataloader(dict(cfg, data_file=str(tmp_path / "missing.npy")), "cpu", True, str(tmp_path / "empty"))
    with pytest.raises(ValueError, match="pack the data set smaller"):
        NativeImageLoader(path, 8, 4, "cpu", resident_gib=1e-6)


def test_get_args_data_flags():
    import models
    from utils import DATASETS, get_args
    cfg, _ = get_args({"lr": 1e-3, "rnd_flip": False}, DATASETS, models.MODEL_NAMES, ["-m", "ddpm"])
    assert cfg["rnd_flip"] is False and not {"data_file", "test_file", "val_split"} & set(cfg)
    cfg, _ = get_args({"rnd_flip": False}, DATASETS, models.MODEL_NAMES,
                      ["--data_file", "a.npy", "--test_file", "b.npy", "--rnd_flip", "--val_split", "0.15"])
    assert cfg["data_file"] == "a.npy" and cfg["test_file"] == "b.npy" and cfg["rnd_flip"] is True and cfg["val_split"] == 0.15
    # the assertions of tests/test_host_logic.py::test_cli_args_surface, unchanged
    cfg, mute = get_args({"lr": 1e-3}, DATASETS, models.MODEL_NAMES,
                         ["-m", "ddpm", "-d", "celeba_hq", "-e", "7", "-bs", "32", "-is", "256", "-downsample", "3", "-mute"])
    assert mute and cfg["dataset"] == "celeba_hq" and cfg["n_steps"] == 7 and cfg["batch_size"] == 32
    assert cfg["image_size"] == 256 and cfg["n_downsamples"] == 3 and cfg["model"] == "ddpm"
    cfg, mute = get_args({}, DATASETS, models.MODEL_NAMES, [])
    assert not mute and cfg["image_size"] == 32 and cfg["batch_size"] == 32 and cfg["n_steps"] == 500
    assert "rnd_flip" not in cfg


# ------------------------------------------------------------------ prepare_dataset.py
def _idx(path, arr, gz):
    raw = struct.pack(">IIII", 0x803, *arr.shape) + arr.tobytes()
    with (gzip.open if gz else open)(path, "wb") as f:
        f.write(raw)


def test_prepare_dataset_mnist(tmp_path):
    import prepare_dataset as P
    tr, te = R.images(5, 28, 28, 1, seed=1)[..., 0], R.images(5, 28, 28, 1, seed=2)[..., 0]
    for gz in (False, True):
        src = tmp_path / f"raw{int(gz)}"
        src.mkdir()
        ext = ".gz" if gz else ""
        _idx(str(src / f"train-images-idx3-ubyte{ext}"), tr, gz)
        _idx(str(src / f"t10k-images-idx3-ubyte{ext}"), te, gz)
        out = tmp_path / f"mnist{int(gz)}"
        assert P.main(["--mnist", str(src), str(out)]) == 0
        got_tr, got_te = np.load(out / "train.npy"), np.load(out / "test.npy")
        assert got_tr.dtype == np.uint8 and np.array_equal(got_tr, tr) and np.array_equal(got_te, te)
    x, _ = next(iter(NativeImageLoader(str(out / "train.npy"), 28, 5, "cpu")))
    assert x.shape == (5, 1, 28, 28)


def test_prepare_dataset_cifar(tmp_path):
    import prepare_dataset as P
    src = tmp_path / "cifar-10-batches-py"
    src.mkdir()
    planes = R.images(4, 3, 32, 32, seed=3)                       # [n, channel, y, x], as the pickles hold them
    planes[0] = 0
    planes[0, 1, 2, 5] = 200                                      # one-hot: green at row 2, column 5
    for name, rows in (("data_batch_1", planes[:2]), ("data_batch_2", planes[2:3]), ("test_batch", planes[3:])):
        with open(src / name, "wb") as f:
            pickle.dump({b"data": rows.reshape(len(rows), 3072), b"labels": [0] * len(rows)}, f)
    assert P.main(["--cifar", str(src), str(tmp_path / "cifar10")]) == 0
    tr, te = np.load(tmp_path / "cifar10" / "train.npy"), np.load(tmp_path / "cifar10" / "test.npy")
    assert tr.shape == (3, 32, 32, 3) and te.shape == (1, 32, 32, 3) and tr.dtype == np.uint8
    assert tr[0, 2, 5].tolist() == [0, 200, 0] and int(tr[0].astype(int).sum()) == 200
    assert np.array_equal(tr, planes[:3].transpose(0, 2, 3, 1)) and np.array_equal(te, planes[3:].transpose(0, 2, 3, 1))


def test_prepare_dataset_folder(tmp_path, capsys):
    Image = pytest.importorskip("PIL.Image")
    import prepare_dataset as P
    src = tmp_path / "imgs"
    src.mkdir()
    u8 = R.images(3, 10, 14, 3, seed=6)
    for i in range(3):
        Image.fromarray(u8[i]).save(src / f"{i:03d}.png")
    assert P.main(["--folder", str(src), str(tmp_path / "out")]) == 0
    tr, te = np.load(tmp_path / "out" / "train.npy"), np.load(tmp_path / "out" / "test.npy")
    assert np.array_equal(tr, u8[:2]) and np.array_equal(te, u8[2:])                          # sorted order, the last is the test split
    assert P.main(["--folder", str(src), "--size", "8", str(tmp_path / "out8")]) == 0
    assert np.load(tmp_path / "out8" / "train.npy").shape == (2, 8, 8, 3)
    Image.fromarray(u8[0, :9]).save(src / "003.png")
    with pytest.raises(SystemExit) as e:
        P.main(["--folder", str(src), str(tmp_path / "out2")])
    assert "003.png" in str(e.value) and "one size" in str(e.value)


# ------------------------------------------------------------------ the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    """the declaration in the issue -- images, n_images, Hs, Ws, C, index, B, two (start, weights, taps) table triples, S, flip, seed,
    epoch, out, stream -- has 19 parameters, the query 6"""
    import ctypes
    from ddk import lib as L
    from ddk import ops
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    for name, n in (("ddk_image_batch", 19), ("ddk_image_batch_rows_per_group", 6)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n == len(L.SIGNATURES[name][1])
        assert L.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(L.load(), name) is not None
    assert L.ABI_VERSION == 400 and L.load().ddk_version() == 400
    assert callable(ops.image_batch)
    with pytest.raises(L.DDKError):                                                           # no CPU fallback
        ops.image_batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64),
                        tuple(torch.from_numpy(t) for t in (lambda tf: (tf.row_start, tf.row_w, tf.col_start, tf.col_w))(IB.Transform(8, 8, 8))), 8)


def test_rows_per_group_query_is_host_arithmetic():
    from ddk import lib as L
    q = L.load().ddk_image_batch_rows_per_group
    tf = IB.Transform(218, 178, 64)
    r = q(218, 178, 3, 64, tf.row_taps, tf.col_taps)
    assert 1 <= r <= 32 and -(-64 // r) >= 2
    assert -(-16 // q(64, 64, 3, 16, 8, 8)) >= 2
    assert q(218, 178, 5, 64, 7, 7) == 0 and q(218, 178, 3, 66, 7, 7) == 0 and q(218, 178, 3, 64, 33, 7) == 0
    assert q(218, 178, 3, 64, 0, 7) == 0 and q(4, 178, 3, 64, 7, 7) == 0                      # more taps than source rows
    assert q(4096, 4096, 4, 1024, 8, 8) == 0                                                  # one output row's source rows exceed 64 KB
