"""Input pipeline boundary (reference utils/data.py:12-246).

The reference builds torchvision datasets (ToTensor -> Resize -> CenterCrop -> x*2-1).  Neither torchvision nor
any dataset exists offline, and the input pipeline is outside the accelerated path, so this
module provides the same entry points over a SYNTHETIC dataset of the right shape (uniform in [-1, 1]);
if torchvision and the data are present the real datasets are used.

Real images come in as ONE uint8 array per split, [N, H, W, C] in a .npy file (prepare_dataset.py packs CIFAR, MNIST and image
folders): NativeImageLoader keeps it resident on the device and builds every batch there with one HIP launch.
get_dataloader serves it whenever such a file is configured or lies at the conventional path, and the synthetic set otherwise.
"""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .image_batch import Transform, flip_bits

DATASETS = ['cifar10', 'cifar100', 'mnist', 'omniglot', 'celeba', 'celeba_hq_65', 'celeba_hq_64', 'celeba_hq']
_GRAY = ('mnist', 'omniglot')


def get_color_channels(dataset: str) -> int:
    """data.py: 1 channel for mnist / omniglot, else 3."""
    return 1 if dataset in _GRAY else 3


class SyntheticImages(Dataset):
    """Deterministic uniform [-1,1] images, generated per index (no storage)."""

    def __init__(self, channels, size, length=50000, seed=4321):
        self.shape, self.length, self.seed = (channels, size, size), length, seed

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        return torch.rand(self.shape, generator=g) * 2 - 1, 0


class _Resident:
    """One uint8 image array [N, H, W, C], loaded once and (on a ROCm device) uploaded once, with the tap tables of its transform.
    The loaders of a train / validation split share one."""

    def __init__(self, path_or_array, image_size, device, resident_gib=64):
        if isinstance(path_or_array, (str, os.PathLike)):
            self.name = os.fspath(path_or_array)
            arr = np.load(self.name, mmap_mode='r', allow_pickle=False)
        else:
            self.name = 'array'
            arr = path_or_array.numpy() if torch.is_tensor(path_or_array) else np.asarray(path_or_array)
        if arr.dtype != np.uint8 or arr.ndim not in (3, 4) or 0 in arr.shape:
            raise ValueError(f"{self.name}: an image file is uint8 [N, H, W, C] (or [N, H, W] for one channel), got dtype {arr.dtype} "
                             f"shape {tuple(arr.shape)}")
        if arr.ndim == 3:
            arr = arr[..., None]
        if not 1 <= arr.shape[3] <= 4:
            raise ValueError(f"{self.name}: 1..4 channels, got dtype {arr.dtype} shape {tuple(arr.shape)}")
        if arr.nbytes > resident_gib * 2 ** 30:
            raise ValueError(f"{self.name}: {arr.nbytes / 2 ** 30:.1f} GiB of images do not fit the resident budget of {resident_gib} GiB: "
                             f"pack the data set smaller (prepare_dataset.py --size resizes at packing time)")
        self.device = torch.device(device)
        self.n, self.channels = int(arr.shape[0]), int(arr.shape[3])
        self.transform = tf = Transform(arr.shape[1], arr.shape[2], image_size)
        self.images = torch.from_numpy(np.array(arr, order='C')).to(self.device)     # read (the file is mapped until here), upload once
        if self.device.type == 'cuda':
            self.tables = tuple(torch.from_numpy(t).to(self.device) for t in (tf.row_start, tf.row_w, tf.col_start, tf.col_w))
        else:
            a_h, a_w = tf.matrices()
            self.a_h, self.a_w = torch.from_numpy(a_h).double(), torch.from_numpy(a_w).double()


class NativeImageLoader:
    """Batches of a resident uint8 image array, built on the device: iterating yields (x, labels) with x a
    fresh [B, C, S, S] fp32 tensor in [-1, 1] on `device` -- one launch of ddk.ops.image_batch per batch, no host work, no worker
    processes -- and labels a cached zero int64 [B].  len() is len(indices) // batch_size (drop_last).  Every __iter__ starts an
    epoch: with `shuffle` the order is torch.randperm(len(indices)) of a generator seeded with base_seed + epoch, and with `flip` an
    image is mirrored iff utils.image_batch.flip_bits(id, base_seed, epoch) says so.  base_seed is `seed`, or drawn from torch's global
    generator at the first __iter__, as DataLoader draws its own.  On device "cpu" the same tables are applied with torch on the host.
    `path_or_array`: a .npy path, an array, or the _Resident of another loader (a split shares one upload)."""

    def __init__(self, path_or_array, image_size, batch_size, device='cuda', shuffle=False, flip=False, indices=None, seed=None,
                 resident_gib=64):
        self.data = path_or_array if isinstance(path_or_array, _Resident) else _Resident(path_or_array, image_size, device, resident_gib)
        self.device, self.batch_size, self.shuffle, self.flip = self.data.device, int(batch_size), bool(shuffle), bool(flip)
        idx = torch.arange(self.data.n) if indices is None else torch.as_tensor(indices, dtype=torch.int64).reshape(-1).clone()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.data.n):
            raise ValueError(f"{self.data.name}: indices outside [0, {self.data.n})")
        if self.batch_size < 1 or idx.numel() < self.batch_size:
            raise ValueError(f"{self.data.name}: {idx.numel()} images make no batch of {self.batch_size} (drop_last)")
        self.indices, self.base_seed, self.epoch = idx, seed, -1
        self.last_order = None                       # the epoch's image ids in serving order (host tensor)
        self._labels = torch.zeros(self.batch_size, dtype=torch.int64, device=self.device)

    def __len__(self):
        return self.indices.numel() // self.batch_size

    def __iter__(self):
        if self.base_seed is None:
            self.base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        self.epoch += 1
        epoch, order = self.epoch, self.indices
        if self.shuffle:
            g = torch.Generator().manual_seed((self.base_seed + epoch) & 0x7FFFFFFFFFFFFFFF)
            order = order[torch.randperm(order.numel(), generator=g)]
        self.last_order = order
        on_device = order.to(self.device)            # one upload per epoch; a batch's index is a view into it
        bs = self.batch_size
        for k in range(len(self)):
            index = on_device[k * bs:(k + 1) * bs]
            yield self._batch(index, epoch), self._labels

    def _batch(self, index, epoch):
        d = self.data
        if self.device.type == 'cuda':
            from ddk import ops
            return ops.image_batch(d.images, index, d.tables, d.transform.S, self.flip, self.base_seed, epoch)
        v = d.images[index].float().div(255).double()                        # [B, Hs, Ws, C], the correctly rounded fp32 quotients
        x = torch.einsum('yh,bhwc,xw->bcyx', d.a_h, v, d.a_w).float().mul(2).sub(1)
        if self.flip:
            mirrored = torch.from_numpy(flip_bits(index.numpy(), self.base_seed, epoch))
            x[mirrored] = x[mirrored].flip(-1)
        return x.contiguous()


def _find_file(config, key, env, data_root, name):
    """the first that is set and exists: config[key], the environment variable, <data_root>/<dataset>/<name>; a set one that does
    not exist is an error, not a reason to train on noise"""
    for what, path in ((f"config['{key}']", config.get(key)), (env, os.environ.get(env) if env else None)):
        if path:
            if not os.path.isfile(path):
                raise FileNotFoundError(f"{what} = {path}: no such file")
            return path
    if not data_root:                                # callers without a data directory (bench.py, the tests' workers) pass None
        return None
    path = os.path.join(data_root, config['dataset'], name)
    return path if os.path.isfile(path) else None


def _native_loaders(path, config, device, train, val_split):
    """get_dataloader over an image file: the reference's loaders (data.py:152-201) as NativeImageLoaders over one resident array"""
    size, bs = config['image_size'], config['batch_size']
    data = _Resident(path, size, device, config.get('resident_gib', 64))
    want = get_color_channels(config['dataset'])
    if data.channels != want:
        raise ValueError(f"{path}: {data.channels} channel(s), {config['dataset']} has {want}")
    flip = bool(config.get('rnd_flip')) and train
    if train and val_split and val_split > 0:
        split = (data.n * np.array([1 - val_split, val_split])).astype(int)      # data.py:159-163
        split[1] += data.n - split.sum()
        perm = torch.randperm(data.n)                                            # random_split's draw from the global generator
        return (NativeImageLoader(data, size, bs, device, shuffle=True, flip=flip, indices=perm[:split[0]]),
                NativeImageLoader(data, size, bs, device, shuffle=False, flip=flip, indices=perm[split[0]:]))
    return NativeImageLoader(data, size, bs, device, shuffle=train, flip=flip), None


def get_dataloader(config: dict, device: str = 'cpu', train: bool = True, data_root: str = './data/', val_split: float = 0):
    """Returns (train_loader, val_loader) like data.py:103-140.  With an image file -- config['data_file'] or
    <data_root>/<dataset>/train.npy for training; config['test_file'], $DDPM_TEST_FILE or <data_root>/<dataset>/test.npy for the test
    split -- the loaders are NativeImageLoaders (training: shuffled, mirrored iff config['rnd_flip']; test: file order, never mirrored;
    a validation split is the reference's, unshuffled, with the training transform).  Without one: synthetic unless DDPM_REAL_DATA=1
    and torchvision works."""
    path = (_find_file(config, 'data_file', None, data_root, 'train.npy') if train
            else _find_file(config, 'test_file', 'DDPM_TEST_FILE', data_root, 'test.npy'))
    if path is not None:
        return _native_loaders(path, config, device, train, val_split)
    channels = get_color_channels(config['dataset'])
    size, bs = config['image_size'], config['batch_size']
    ds = None
    if os.environ.get('DDPM_REAL_DATA') == '1':
        ds = _try_real_dataset(config, data_root, train)
    if ds is None:
        ds = SyntheticImages(channels, size)
    kw = dict(num_workers=4, pin_memory=True) if device == 'cuda' else {}
    if val_split and val_split > 0:
        n_val = int(len(ds) * val_split)
        tr, va = torch.utils.data.random_split(ds, [len(ds) - n_val, n_val])
        return (DataLoader(tr, batch_size=bs, shuffle=True, drop_last=True, **kw),
                DataLoader(va, batch_size=bs, shuffle=False, drop_last=True, **kw))
    return DataLoader(ds, batch_size=bs, shuffle=train, drop_last=True, **kw), None


def _try_real_dataset(config, data_root, train):
    try:
        from torchvision import datasets, transforms as T
    except Exception:
        return None
    tf = T.Compose([T.ToTensor(), T.Resize(config['image_size']), T.CenterCrop(config['image_size']),
                    T.Lambda(lambda x: x * 2 - 1)])
    name = config['dataset']
    try:
        if name == 'cifar10':
            return datasets.CIFAR10(data_root, train=train, transform=tf, download=False)
        if name == 'cifar100':
            return datasets.CIFAR100(data_root, train=train, transform=tf, download=False)
        if name == 'mnist':
            return datasets.MNIST(data_root, train=train, transform=tf, download=False)
        folder = {'celeba': 'celeba', 'celeba_hq': 'celeba_hq', 'celeba_hq_64': 'celeba_hq_64',
                  'celeba_hq_65': 'celeba_hq_64'}.get(name)
        if folder:
            return datasets.ImageFolder(os.path.join(data_root, folder), transform=tf)
    except Exception:
        return None
    return None
