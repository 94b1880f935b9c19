#!/usr/bin/env python3
"""Pack a data set into the two files the native loader reads (utils/data.py):

    python prepare_dataset.py --cifar  ../data/cifar-10-batches-py  ../data/cifar10
    python prepare_dataset.py --mnist  ../data/MNIST/raw            ../data/mnist
    python prepare_dataset.py --folder ../data/celeba/img_align_celeba ../data/celeba [--size 64] [--test_share 0.1]

OUT/train.npy and OUT/test.npy are uint8 [N, H, W, C] ([N, H, W] for MNIST).  Nothing is downloaded: the inputs are the files the
data sets are distributed as -- the python-pickle batches of CIFAR-10 / CIFAR-100, the idx files of MNIST (gz or plain), a folder of
images.  numpy only, plus PIL for --folder.
"""
import argparse
import gzip
import os
import pickle
import struct
import sys

import numpy as np


def _cifar_batch(path):
    with open(path, 'rb') as f:
        d = pickle.load(f, encoding='bytes')
    data = np.asarray(d[b'data'] if b'data' in d else d['data'], dtype=np.uint8)
    if data.ndim != 2 or data.shape[1] != 3072:
        sys.exit(f"{path}: 'data' is {data.shape}, a CIFAR batch holds [n, 3072]")
    return data.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)          # planes R, G, B of 32 x 32 -> [n, 32, 32, 3]


def pack_cifar(src):
    """(train, test) of a CIFAR-10 (data_batch_1..5, test_batch) or CIFAR-100 (train, test) directory"""
    names = sorted(n for n in os.listdir(src) if n.startswith('data_batch_')) or ['train']
    test = 'test_batch' if names != ['train'] else 'test'
    for n in names + [test]:
        if not os.path.isfile(os.path.join(src, n)):
            sys.exit(f"{src}: no file {n} (expected CIFAR-10's data_batch_* + test_batch or CIFAR-100's train + test)")
    return np.concatenate([_cifar_batch(os.path.join(src, n)) for n in names]), _cifar_batch(os.path.join(src, test))


def _idx_images(path):
    opener = gzip.open if path.endswith('.gz') else open
    with opener(path, 'rb') as f:
        raw = f.read()
    magic, n, h, w = struct.unpack('>IIII', raw[:16])
    if magic != 0x00000803 or len(raw) != 16 + n * h * w:
        sys.exit(f"{path}: not an idx3-ubyte image file (magic {magic:#x}, {len(raw)} bytes for {n} x {h} x {w})")
    return np.frombuffer(raw, dtype=np.uint8, offset=16).reshape(n, h, w).copy()


def pack_mnist(src):
    out = []
    for stem in ('train-images-idx3-ubyte', 't10k-images-idx3-ubyte'):
        found = [p for p in (os.path.join(src, stem), os.path.join(src, stem + '.gz')) if os.path.isfile(p)]
        if not found:
            sys.exit(f"{src}: no {stem} or {stem}.gz")
        out.append(_idx_images(found[0]))
    return out[0], out[1]


_EXT = ('.png', '.jpg', '.jpeg', '.bmp', '.webp')


def pack_folder(src, size=None, test_share=0.1):
    """every image under src in sorted order; the last test_share of them (at least one) is the test split"""
    try:
        from PIL import Image
    except ImportError:
        sys.exit("--folder needs PIL to decode images")
    paths = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(src) for f in fs if f.lower().endswith(_EXT))
    if len(paths) < 2:
        sys.exit(f"{src}: {len(paths)} image(s); two make the smallest train / test pair")
    out = None
    for i, p in enumerate(paths):
        with Image.open(p) as im:
            im = im.convert('L' if im.mode in ('1', 'L', 'I;16') else 'RGB')
            if size:
                w, h = im.size
                nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
                im = im.resize((nw, nh), Image.BILINEAR, reducing_gap=None)
                left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
                im = im.crop((left, top, left + size, top + size))
            a = np.asarray(im, dtype=np.uint8)
        a = a[..., None] if a.ndim == 2 else a
        if out is None:
            out = np.empty((len(paths),) + a.shape, dtype=np.uint8)
        elif a.shape != out.shape[1:]:
            sys.exit(f"{p}: {a.shape[0]}x{a.shape[1]}x{a.shape[2]}, the images before it are "
                     f"{out.shape[1]}x{out.shape[2]}x{out.shape[3]}: all images must have one size (--size S resizes and crops)")
        out[i] = a
    n_test = max(1, int(len(paths) * test_share))
    return out[:-n_test], out[-n_test:]


def main(argv=None):
    ap = argparse.ArgumentParser(description="Pack CIFAR, MNIST or an image folder into OUT/train.npy and OUT/test.npy (uint8).")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--cifar', metavar='DIR', help="directory of CIFAR-10 / CIFAR-100 python-pickle batches")
    src.add_argument('--mnist', metavar='DIR', help="directory of the MNIST idx files (gz or plain)")
    src.add_argument('--folder', metavar='DIR', help="directory of images, taken in sorted order")
    ap.add_argument('--size', type=int, default=None, help="--folder: resize the short side to S and centre-crop S x S at packing time")
    ap.add_argument('--test_share', type=float, default=0.1, help="--folder: share of the images (the last in order) that becomes test.npy")
    ap.add_argument('out', metavar='OUT', help="output directory, e.g. ../data/cifar10")
    a = ap.parse_args(argv)
    if a.cifar:
        train, test = pack_cifar(a.cifar)
    elif a.mnist:
        train, test = pack_mnist(a.mnist)
    else:
        train, test = pack_folder(a.folder, a.size, a.test_share)
    os.makedirs(a.out, exist_ok=True)
    for name, arr in (('train.npy', train), ('test.npy', test)):
        np.save(os.path.join(a.out, name), np.ascontiguousarray(arr, dtype=np.uint8))
        print(f"{os.path.join(a.out, name)}: uint8 {tuple(arr.shape)}, {arr.nbytes / 2 ** 20:.1f} MiB")
    return 0


if __name__ == '__main__':
    sys.exit(main())
